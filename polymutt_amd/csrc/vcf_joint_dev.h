// vcf_joint_dev.h -- the joint call plane of the --in_vcf path (pm_engine_set_vcf_joint): for every family F of every written
// row of an autosomal section the most probable joint assignment g* of its members' states (g11, g12, g22 of the record's
// (ref, alt)) under the distribution behind the genotype rows, the posterior plane (vcf_post_dev.h) and the phase plane
// (vcf_phase_dev.h): same founder priors, same single-family prior mode, same family routing, plain transmission.  With
//   J(g) = founder priors x the transmission T[g_fa][g_mo][g_c] of every non-founder x the members' penetrances,
//   L = Sum_g J(g),
// every member of F gets its state in g* (J(g*) = max J) and lp = log10(J(g*) / L), the same value for the whole family.
// It is the max-product counterpart of the sums the other planes take: marginal argmaxes need not fit together, g* does.
// max J = 0 or L = 0 gives g = 255 and lp = 0.  Included by engine.hip after vcf_phase_dev.h.
//
// One extra pass after the phase plane's, on the engine's stream, only with the feature on.  Its kernels write the plane
// (VjArgs::joint, [row][person] of pm_vcf_joint) and nothing else, one kernel per loop of vcf_plane_dev.h:
//   k_vcf_joint_lean  lean_nuc_joint, the argmax over the parental pairs from a family's 12 PL bytes;
//   k_vcf_joint_nuc   the same argmax with the product over any number of kids;
//   k_vcf_joint_es    one thread per (row, peeled family): d_es_joint3, the autosomal three-state peel with max in
//                     place of every sum and a back-pointer word per step, then a backtrack through the steps in reverse.
// Ties go to the first maximum of the fixed enumeration order (a candidate replaces the best only when strictly greater).
// No atomics, no scratch; lp is formed in double and rounded once to float.  Sections that are not autosomal launch
// none of the three: k_vcf_joint_none fills the plane with (g = 255, lp = 0) instead (engine.hip, launch_vcf_joint).
#pragma once

struct VjArgs {
  pm_vcf_joint* joint;   // [max_batch][n_person]
  const int* fams;       // [n_fams] the peeled families of the plan in use
  int n_fams;
  double* ws;            // k_vcf_joint_es<false>: lane-interleaved workspace [ws_per_lane][grid x 256] (else unused)
  int ws_per_lane;       // doubles per thread: max over the peeled families of steps + n * 3 + slots * 9
};

// (one 8-byte store per person: the plane is 8-byte aligned and so is every entry; the pad bytes are written as 0)
__device__ __forceinline__ void d_store_joint(pm_vcf_joint* dst, int g, double lp) {
  uint2 v;
  v.x = __float_as_uint((float)lp); v.y = (uint32_t)g & 255u;
  *reinterpret_cast<uint2*>(dst) = v;
}

// A section that is not autosomal: every entry of the plane is (g = 255, lp = 0)
__global__ void __launch_bounds__(256) k_vcf_joint_none(pm_vcf_joint* joint, size_t cells) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) d_store_joint(joint + i, 255, 0.0);
}

// A founders-only family factorises: every person's own argmax of prior x penetrance (Hardy-Weinberg at the site's
// frequency, CalcPostProb_SinglePerson's), lp = the sum of the persons' log10 shares in person order.  A person whose
// three products are all zero leaves the whole family without an assignment.
__device__ __forceinline__ void d_joint_founders(const double* s_lk, const uint8_t* pl, int np, int p0, int n, int g11, int g12, int g22,
                                                 double freq, pm_vcf_joint* out) {
  const double gq = 1 - freq;
  const double pr0 = freq * freq, pr1 = freq * gq * 2, pr2 = gq * gq;
  double lp = 0.0;
  bool ok = true;
  for (int j = 0; j < n; j++) {
    const int p = p0 + j;
    const double m0 = s_lk[PLB(pl, np, p, g11)] * pr0, m1 = s_lk[PLB(pl, np, p, g12)] * pr1, m2 = s_lk[PLB(pl, np, p, g22)] * pr2;
    double b = m0;
    if (m1 > b) b = m1;
    if (m2 > b) b = m2;
    const double s = m0 + m1 + m2;
    if (!(b > 0.0) || !(s > 0.0)) ok = false;
    else lp += log10(b / s);
  }
  for (int j = 0; j < n; j++) {
    const int p = p0 + j;
    const double m0 = s_lk[PLB(pl, np, p, g11)] * pr0, m1 = s_lk[PLB(pl, np, p, g12)] * pr1, m2 = s_lk[PLB(pl, np, p, g22)] * pr2;
    double b = m0;
    int g = 0;
    if (m1 > b) { b = m1; g = 1; }
    if (m2 > b) { b = m2; g = 2; }
    d_store_joint(out + p, ok ? g : 255, ok ? lp : 0.0);
  }
}

// The three terms T[k][g] * l[g] of one child under the parental pair k = 3a + b (tk: the pair's row of the plain
// transmission table), their sum and their first maximum
__device__ __forceinline__ void d_joint_kid(const double* tk, double l0, double l1, double l2, double& sum, double& mx, int& g) {
  const double t0 = tk[0] * l0, t1 = tk[1] * l1, t2 = tk[2] * l2;
  sum = (t0 + t1) + t2;
  mx = t0; g = 0;
  if (t1 > mx) { mx = t1; g = 1; }
  if (t2 > mx) { mx = t2; g = 2; }
}

// d_joint_kid with the pair's three transmission values known when the code is compiled (lean_nuc_joint's unrolled k): a
// product with 0 is the constant 0 and one with 1 the likelihood itself -- the values d_joint_kid forms, the likelihoods
// being finite, without the table in LDS or the multiplications
__device__ __forceinline__ double d_joint_tmul(double t, double l) { return t == 0.0 ? 0.0 : t == 1.0 ? l : t * l; }
__device__ __forceinline__ void d_joint_kid_c(double ta, double tb, double tc, double l0, double l1, double l2, double& sum, double& mx,
                                              int& g) {
  const double t0 = d_joint_tmul(ta, l0), t1 = d_joint_tmul(tb, l1), t2 = d_joint_tmul(tc, l2);
  sum = (t0 + t1) + t2;
  mx = t0; g = 0;
  if (t1 > mx) { mx = t1; g = 1; }
  if (t2 > mx) { mx = t2; g = 2; }
}

// LEAN nuclear family (autosome, <= 4 persons) from its 12 PL bytes: for each parental pair k = 3a + b in ascending order
//   score_k = (lF[a] * lM[b]) * pp[k] * Prod_kids max_g T[a][b][g] * l_kid[g],
// the first maximum over k, then every kid's first maximum g under that pair; L = Sum_k the same product with the kids'
// sums.  NF as lean_nuc_phase's.
template <int NF>
__device__ __forceinline__ void lean_nuc_joint(const double* s_lk, const uint32_t* by, size_t out, int p0, int n_rt, const double* pp,
                                               pm_vcf_joint* vj) {
  constexpr double kT[27] = {1, 0, 0, .5, .5, 0, 0, 1, 0, .5, .5, 0, .25, .5, .25, 0, .5, .5, 0, 1, 0, 0, .5, .5, 0, 0, 1};   // c_TBA[0]
  const int n = NF ? NF : n_rt;
  double lF[3], lM[3], kl[2][3];
#pragma unroll
  for (int t = 0; t < 3; t++) {
    lF[t] = s_lk[by[t]]; lM[t] = s_lk[by[3 + t]]; kl[0][t] = s_lk[by[6 + t]]; kl[1][t] = s_lk[by[9 + t]];
  }
  const bool two = n == 4;
  double best = 0.0, L = 0.0;
  int kb = -1, gb0 = 0, gb1 = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double w = (lF[k / 3] * lM[k % 3]) * pp[k];
    double s0, m0, s1, m1;
    int g0, g1;
    d_joint_kid_c(kT[3 * k], kT[3 * k + 1], kT[3 * k + 2], kl[0][0], kl[0][1], kl[0][2], s0, m0, g0);
    d_joint_kid_c(kT[3 * k], kT[3 * k + 1], kT[3 * k + 2], kl[1][0], kl[1][1], kl[1][2], s1, m1, g1);
    const double sc = two ? (w * m0) * m1 : w * m0;
    const double sm = two ? (w * s0) * s1 : w * s0;
    L = k == 0 ? sm : L + sm;
    if (sc > best) { best = sc; kb = k; gb0 = g0; gb1 = g1; }
  }
  const bool ok = kb >= 0 && L > 0.0;
  const double lp = ok ? log10(best / L) : 0.0;
  d_store_joint(vj + out + p0, ok ? kb / 3 : 255, lp);
  d_store_joint(vj + out + p0 + 1, ok ? kb % 3 : 255, lp);
  d_store_joint(vj + out + p0 + 2, ok ? gb0 : 255, lp);
  if (two) d_store_joint(vj + out + p0 + 3, ok ? gb1 : 255, lp);
}

// The lean loop around lean_nuc_joint and d_joint_founders, 8 bytes per person at a time.
__global__ void __launch_bounds__(256) k_vcf_joint_lean(DevArgs A, VjArgs P) {
  __shared__ double s_lk[256];
  extern __shared__ uint32_t s_fam[];   // [n_fam]
  stage_lk(s_lk, A);
  lean_fam_table(A, s_fam);
  __syncthreads();
  lean_family_rows(
      A, s_fam,
      [&](auto nf, const LeanRow& cur, const double* pp, int, int p0, int n, const uint32_t* by) {
        lean_nuc_joint<decltype(nf)::value>(s_lk, by, cur.out, p0, n, pp, P.joint);
      },
      [&](const LeanRow& cur, int p0, int n) {
        d_joint_founders(s_lk, cur.pl, A.n_person, p0, n, cur.g11, cur.g12, cur.g22, cur.freq, P.joint + cur.out);
      });
}

// The nuc loop: founders-only families factorise; a nuclear family of any number of children takes lean_nuc_joint's argmax
// with the product over its kids, kid by kid in person order, and a second pass over the kids for their states under the
// best pair.
__global__ void __launch_bounds__(256) k_vcf_joint_nuc(DevArgs A, VjArgs P) {
  __shared__ double s_lk[256];
  __shared__ double s_tba[27];
  stage_lk(s_lk, A);
  stage_tba(s_tba);
  __syncthreads();
  const int np = A.n_person;
  nuc_family_rows(
      A,
      [&](const LeanRow& r, int p0, int n) { d_joint_founders(s_lk, r.pl, np, p0, n, r.g11, r.g12, r.g22, r.freq, P.joint + r.out); },
      [&](const LeanRow& r, int, int, int p0, int n) {
        const uint8_t* pl = r.pl;
        const int g11 = r.g11, g12 = r.g12, g22 = r.g22;
        pm_vcf_joint* out = P.joint + r.out;
        double pp[9];
        d_parent_prior((!A.n_fam_gt1 && !r.mono) ? PR_TRIO : PR_AUTO, r.freq, pp);
        const double F0 = s_lk[PLB(pl, np, p0, g11)], F1 = s_lk[PLB(pl, np, p0, g12)], F2 = s_lk[PLB(pl, np, p0, g22)];
        const double M0 = s_lk[PLB(pl, np, p0 + 1, g11)], M1 = s_lk[PLB(pl, np, p0 + 1, g12)], M2 = s_lk[PLB(pl, np, p0 + 1, g22)];
        double best = 0.0, L = 0.0;
        int kb = -1;
#pragma unroll
        for (int k = 0; k < 9; k++) {
          const double lf = k / 3 == 0 ? F0 : k / 3 == 1 ? F1 : F2, lm = k % 3 == 0 ? M0 : k % 3 == 1 ? M1 : M2;
          const double w = (lf * lm) * pp[k];
          double sc = w, sm = w;
          for (int j = 2; j < n; j++) {
            double s, m;
            int g;
            d_joint_kid(s_tba + 3 * k, s_lk[PLB(pl, np, p0 + j, g11)], s_lk[PLB(pl, np, p0 + j, g12)], s_lk[PLB(pl, np, p0 + j, g22)], s, m, g);
            sc *= m; sm *= s;
          }
          L = k == 0 ? sm : L + sm;
          if (sc > best) { best = sc; kb = k; }
        }
        const bool ok = kb >= 0 && L > 0.0;
        const double lp = ok ? log10(best / L) : 0.0;
        d_store_joint(out + p0, ok ? kb / 3 : 255, lp);
        d_store_joint(out + p0 + 1, ok ? kb % 3 : 255, lp);
        const double* tk = s_tba + 3 * (ok ? kb : 0);
        for (int j = 2; j < n; j++) {
          double s, m;
          int g;
          d_joint_kid(tk, s_lk[PLB(pl, np, p0 + j, g11)], s_lk[PLB(pl, np, p0 + j, g12)], s_lk[PLB(pl, np, p0 + j, g22)], s, m, g);
          d_store_joint(out + p0 + j, ok ? g : 255, lp);
        }
      });
}

// d_es_lk3_vdn's autosomal peel (both tables the plain transmission tt, nobody clamped) with max in place of every sum and a
// back-pointer word per step, kept as a small integer in a double beside the partials:
//   type 1 (offspring -> parents)        per parental pair (i, j) the best child state: 9 x 2 bits, bit 2 (3 i + j);
//   type 2 (spouse -> spouse)            per target state i the best spouse state: 3 x 2 bits, bit 2 i;
//   type 3 (parents -> only offspring)   per child state k the best parental pair 3 i + j: 3 x 4 bits, bit 4 k.
// Then the first maximum over the final person's three partials and a backtrack through the steps in reverse order: a
// step's target is fixed before the step is met (it is peeled later or is the final person), and the children of a
// marriage partial are resolved once the step that consumed the partial has fixed both parents.  A fixed state takes the
// place of the person's first partial.  Workspace: BP [steps], then partials [n][3], then marriage partials [slots][9],
// strided by st.  L: the family's normaliser.  Writes the n members' plane entries.
__device__ __forceinline__ void d_es_joint3(const DevArgs& A, int f, const uint8_t* pl, const double* lk, const int* gidx, double freq,
                                            const double* tt, double* ws, size_t st, double L, pm_vcf_joint* out) {
  const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0, nf = A.fam_founders[f];
  const int s0 = A.peel_start[f], s1 = A.peel_start[f + 1], nst = s1 - s0;
#define BP(s) ws[(size_t)(s) * st]
#define PP(i, j) ws[((size_t)nst + (size_t)(i) * 3 + (j)) * st]
#define MPP(sl, x, y) ws[((size_t)nst + (size_t)n * 3 + (size_t)(sl) * 9 + (x) * 3 + (y)) * st]
  const size_t np = (size_t)A.n_person;
  for (int i = 0; i < n; i++) {
    const bool fo = A.is_founder[p0 + i] != 0;
    const uint8_t* R = pl + p0 + i;   // plane g at R[g * n_person]
    double pr[3] = {0.0, 0.0, 0.0};
    if (i < nf) { pr[0] = freq * freq; pr[1] = 2 * freq * (1 - freq); pr[2] = (1 - freq) * (1 - freq); }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double pen = lk[R[gidx[j] * np]];
      PP(i, j) = fo ? pr[j] * pen : pen;
    }
  }
  for (int s = s0; s < s1; s++) {
    const int2 S = A.steps[s];
    const int type = S.x & 255, from0 = (S.x >> 8) & 255, from1 = (S.x >> 16) & 255, to0 = (S.x >> 24) & 255;
    const int slot = (S.y >> 8) & 255, create = (S.y >> 16) & 1, fa2mo = (S.y >> 17) & 1;
    unsigned bits = 0;
    if (type == 1) {
      if (create)
        for (int x = 0; x < 9; x++) MPP(slot, x / 3, x % 3) = 1.0;
      const double pk0 = PP(from0, 0), pk1 = PP(from0, 1), pk2 = PP(from0, 2);
      for (int x = 0; x < 9; x++) {
        double sum, mx;
        int g;
        d_joint_kid(tt + 3 * x, pk0, pk1, pk2, sum, mx, g);
        MPP(slot, x / 3, x % 3) *= mx;
        bits |= (unsigned)g << (2 * x);
      }
    } else if (type == 2) {
      const double ps0 = PP(from0, 0), ps1 = PP(from0, 1), ps2 = PP(from0, 2);
      for (int i = 0; i < 3; i++) {
        double v0 = ps0, v1 = ps1, v2 = ps2;
        if (slot != 255) {
          if (fa2mo) { v0 *= MPP(slot, 0, i); v1 *= MPP(slot, 1, i); v2 *= MPP(slot, 2, i); }
          else { v0 *= MPP(slot, i, 0); v1 *= MPP(slot, i, 1); v2 *= MPP(slot, i, 2); }
        }
        double mx = v0;
        int g = 0;
        if (v1 > mx) { mx = v1; g = 1; }
        if (v2 > mx) { mx = v2; g = 2; }
        PP(to0, i) *= mx;
        bits |= (unsigned)g << (2 * i);
      }
    } else {
      const double pf0 = PP(from0, 0), pf1 = PP(from0, 1), pf2 = PP(from0, 2);
      const double pm0 = PP(from1, 0), pm1 = PP(from1, 1), pm2 = PP(from1, 2);
      double b0 = 0.0, b1 = 0.0, b2 = 0.0;
      unsigned k0 = 0, k1 = 0, k2 = 0;
      for (int x = 0; x < 9; x++) {
        const int i = x / 3, j = x % 3;
        const double pf = i == 0 ? pf0 : i == 1 ? pf1 : pf2, pm = j == 0 ? pm0 : j == 1 ? pm1 : pm2;
        const double w = (slot == 255) ? pf * pm : pf * MPP(slot, i, j) * pm;
        const double v0 = w * tt[3 * x], v1 = w * tt[3 * x + 1], v2 = w * tt[3 * x + 2];
        if (x == 0 || v0 > b0) { b0 = v0; k0 = x; }
        if (x == 0 || v1 > b1) { b1 = v1; k1 = x; }
        if (x == 0 || v2 > b2) { b2 = v2; k2 = x; }
      }
      PP(to0, 0) *= b0; PP(to0, 1) *= b1; PP(to0, 2) *= b2;
      bits = k0 | k1 << 4 | k2 << 8;
    }
    BP(s - s0) = (double)bits;
  }
  const int fin = (A.steps[s1 - 1].x >> 24) & 255;
  double best = PP(fin, 0);
  int gf = 0;
  { const double v1 = PP(fin, 1), v2 = PP(fin, 2);
    if (v1 > best) { best = v1; gf = 1; }
    if (v2 > best) { best = v2; gf = 2; } }
  const bool ok = best > 0.0 && L > 0.0;
  const double lp = ok ? log10(best / L) : 0.0;
  if (ok) {
    PP(fin, 0) = (double)gf;
    for (int s = s1 - 1; s >= s0; s--) {
      const int2 S = A.steps[s];
      const int type = S.x & 255, from0 = (S.x >> 8) & 255, from1 = (S.x >> 16) & 255, to0 = (S.x >> 24) & 255, to1 = S.y & 255;
      const unsigned bits = (unsigned)BP(s - s0);
      const int gt = (int)PP(to0, 0);
      if (type == 1) PP(from0, 0) = (double)((bits >> (2 * (3 * gt + (int)PP(to1, 0)))) & 3u);
      else if (type == 2) PP(from0, 0) = (double)((bits >> (2 * gt)) & 3u);
      else {
        const unsigned x = (bits >> (4 * gt)) & 15u;
        PP(from0, 0) = (double)(x / 3); PP(from1, 0) = (double)(x % 3);
      }
    }
  }
  for (int i = 0; i < n; i++) d_store_joint(out + p0 + i, ok ? (int)PP(i, 0) : 255, lp);
#undef BP
#undef PP
#undef MPP
}

// The es loop over the peeled families (VjArgs::fams): one unclamped sum peel for the normaliser L (d_es_lk3_vdn<false>,
// both of its tables the plain transmission in LDS, as k_vcf_phase_es takes it), then the max peel and its backtrack over
// the same workspace.  The HBM workspace is VjArgs::ws, this pass's own: the back-pointers need more words than DevArgs::ws
// has per lane.
template <bool LDSWS>
__global__ void __launch_bounds__(256) k_vcf_joint_es(DevArgs A, VjArgs P) {
  __shared__ double s_lk[256];
  __shared__ double s_tba[27];
  stage_lk(s_lk, A);
  stage_tba(s_tba);
  __syncthreads();
  es_rows<LDSWS>(A, P.ws, P.fams, P.n_fams, [&](const LeanRow& r, int f, double* wsl, size_t stride) {
    const int gidx[3] = {r.g11, r.g12, r.g22};
    const double L = d_es_lk3_vdn<false>(A, f, r.pl, s_lk, gidx, r.freq, s_tba, s_tba, wsl, stride);
    d_es_joint3(A, f, r.pl, s_lk, gidx, r.freq, s_tba, wsl, stride, L, P.joint + r.out);
  });
}
