// vcf_phase_dev.h -- the transmission phase plane of the --in_vcf path (pm_engine_set_vcf_phase): for every non-founder c
// of every written row of an autosomal section the two ordered heterozygous posteriors
//   p12 = P(c got a1 from the father and a2 from the mother | data),  p21 = P(a2 from the father, a1 from the mother | data)
// under the distribution behind the genotype rows and the posterior plane (vcf_post_dev.h): same founder priors, same
// single-family prior mode, same family routing.  With J(a, b) = the family likelihood restricted to father = a, mother = b,
// child = het (plain transmission) and L = the family's normaliser,
//   p12 = [J(0,1) + J(0,2) + J(1,2) + J(1,1) / 2] / L,   p21 = [J(1,0) + J(2,0) + J(2,1) + J(1,1) / 2] / L:
// the weights 0, 1/2, 1 are the share of the child's het transmission T[a][b][1] that hands a1 down the paternal side.
// Founders get (0, 0), and so does a person whose normalising sum is zero.  Included by engine.hip after vcf_post_dev.h.
//
// One extra pass after the standard posterior stage (and after the posterior plane's pass), on the engine's stream, only
// with the feature on.  Its kernels write the plane (VphArgs::phase, [row][person] of pm_vcf_phase) and nothing else, one
// kernel per loop of vcf_plane_dev.h:
//   k_vcf_phase_lean  lean_nuc_phase: lean_nuc_post's kid terms with the het ones split by (a, b);
//   k_vcf_phase_nuc   hoist-free, d_parent_prior and d_kid_geno in k_vcf_post_nuc's order with the same split;
//   k_vcf_phase_es    the children of peeled families: seven d_es_lk3_vdn<true> peels with father, mother and child (het)
//                     clamped, both tables the plain transmission, and one unclamped peel for L.
// Fixed summation order, no atomics, no scratch; a value is the double quotient rounded once to float.  Sections that are
// not autosomal launch nothing: the plane is cleared (engine.hip, launch_vcf_phase).
#pragma once

struct VphArgs {
  pm_vcf_phase* phase;   // [max_batch][n_person]
  const int* kids;       // [n_kids] family << 8 | member: the non-founders of the peeled families of the plan in use
  int n_kids;
};

// (one 8-byte store per person: the plane is 8-byte aligned and so is every entry; s: the normalising sum, 0 = no phase)
__device__ __forceinline__ void d_store_phase(pm_vcf_phase* dst, double s, double a, double b) {
  float2 v;
  v.x = s != 0 ? (float)(a / s) : 0.f; v.y = s != 0 ? (float)(b / s) : 0.f;
  *reinterpret_cast<float2*>(dst) = v;
}

// The het terms v[k] = J[k][1] * w[k] of one child over the parental configurations k = 3a + b (a: person p0's state, b:
// person p0 + 1's) into the two ordered sums, in a fixed order: w12 = (0, 1, 1, 0, 1/2, 1, 0, 0, 0), w21 = (0, 0, 0, 1,
// 1/2, 0, 1, 1, 0).  v[0] and v[8] are structurally zero (two homozygous parents of the same kind have no het child).
// sw: the family lists the mother first (person p0 + 1 is the father): the two sums change places.
__device__ __forceinline__ void d_phase_split(const double* v, bool sw, double& n12, double& n21) {
  const double h = 0.5 * v[4];
  const double x = ((v[1] + v[2]) + h) + v[5];
  const double y = ((v[3] + h) + v[6]) + v[7];
  n12 = sw ? y : x; n21 = sw ? x : y;
}

// LEAN nuclear family (autosome, <= 4 persons) from its 12 PL bytes: lean_nuc_post's kid terms (KidJointGenoLikelihood
// :798-835, d_kid_geno's autosomal switch with the structurally zero terms left out), the het ones kept apart by k.  The
// denominator is the child's normaliser g11 + g12 + g22 with g12 summed in lean_nuc_post's order, as the posterior body
// forms it.  NF as lean_nuc_post's.  swm: bit i = kid slot i's father is person p0 + 1.
template <int NF>
__device__ __forceinline__ void lean_nuc_phase(const double* s_lk, const uint32_t* by, size_t out, int p0, int n_rt, const double* pp,
                                               unsigned swm, pm_vcf_phase* vph) {
  const int n = NF ? NF : n_rt;
  double lF[3], lM[3], kl[2][3];
#pragma unroll
  for (int t = 0; t < 3; t++) {
    lF[t] = s_lk[by[t]]; lM[t] = s_lk[by[3 + t]]; kl[0][t] = s_lk[by[6 + t]]; kl[1][t] = s_lk[by[9 + t]];
  }
  double wk[9];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) wk[3 * a + b] = (lF[a] * lM[b]) * pp[3 * a + b];
  d_store_phase(vph + out + p0, 0.0, 0.0, 0.0);       // the parents are founders
  d_store_phase(vph + out + p0 + 1, 0.0, 0.0, 0.0);
#pragma unroll
  for (int j = 2; j < 4; j++) {
    if (j >= n) break;
    const int me = j - 2, other = 1 - me;
    const bool two = n == 4;
    const double m11 = kl[me][0], m12 = kl[me][1], m22 = kl[me][2];
    const double o11 = kl[other][0], o12 = kl[other][1], o22 = kl[other][2];
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, v[9];
    v[0] = v[8] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      double lo, q11 = 0, q12 = 0, q22 = 0;
      bool z11 = true, z12 = true, z22 = true;
      switch (k) {
        case 0: lo = o11; q11 = m11; z11 = false; break;
        case 1: case 3: lo = 0.5 * (o11 + o12); q11 = m11 * 0.5; q12 = m12 * 0.5; z11 = z12 = false; break;
        case 2: case 6: lo = o12; q12 = m12; z12 = false; break;
        case 4: lo = 0.25 * o11 + 0.5 * o12 + 0.25 * o22; q11 = m11 * 0.25; q12 = m12 * 0.5; q22 = m22 * 0.25; z11 = z12 = z22 = false; break;
        case 5: case 7: lo = 0.5 * (o12 + o22); q12 = m12 * 0.5; q22 = m22 * 0.5; z12 = z22 = false; break;
        default: lo = o22; q22 = m22; z22 = false; break;
      }
      const double w = wk[k];
      if (!z11) { const double t = (two ? q11 * lo : q11) * w; g0 = k == 0 ? t : g0 + t; }
      if (!z12) { const double t = (two ? q12 * lo : q12) * w; v[k] = t; g1 = k == 1 ? t : g1 + t; }
      if (!z22) { const double t = (two ? q22 * lo : q22) * w; g2 = k == 4 ? t : g2 + t; }
    }
    double n12, n21;
    d_phase_split(v, (swm >> me) & 1, n12, n21);
    d_store_phase(vph + out + p0 + j, g0 + g1 + g2, n12, n21);
  }
}

// The lean loop around lean_nuc_phase, 8 bytes per person at a time.  Behind the packed family table the dynamic LDS holds
// a byte per family: which of its kid slots have person p0 + 1 as father (n_fam * 5 bytes in all).
__global__ void __launch_bounds__(256) k_vcf_phase_lean(DevArgs A, VphArgs P) {
  __shared__ double s_lk[256];
  extern __shared__ uint32_t s_fam[];   // [n_fam], then uint8_t [n_fam]
  uint8_t* s_sw = reinterpret_cast<uint8_t*>(s_fam + A.n_fam);
  stage_lk(s_lk, A);
  lean_fam_table(A, s_fam, [&](int fi, int, int p0, int n, bool nuc) {
    unsigned m = 0;
    if (nuc)
      for (int j = 2; j < n && j < 4; j++) m |= (A.fa_local[p0 + j] == 1 ? 1u : 0u) << (j - 2);
    s_sw[fi] = (uint8_t)m;
  });
  __syncthreads();
  lean_family_rows(
      A, s_fam,
      [&](auto nf, const LeanRow& cur, const double* pp, int fi, int p0, int n, const uint32_t* by) {
        lean_nuc_phase<decltype(nf)::value>(s_lk, by, cur.out, p0, n, pp, s_sw[fi], P.phase);
      },
      [&](const LeanRow& cur, int p0, int n) {
        for (int j = 0; j < n; j++) d_store_phase(P.phase + cur.out + p0 + j, 0.0, 0.0, 0.0);   // founders only
      });
}

// The nuc loop, k_vcf_post_nuc's arithmetic on an autosome: founders-only families are zeros; a nuclear family's children
// take KidJointGenoLikelihood's nine terms J[k] * (pg[k] * pp[k]) in k order, the het ones split by k.  (The founders of
// the families the section peels are never written: the plane is cleared when it is allocated and on sections that are
// not autosomal.)
__global__ void __launch_bounds__(256) k_vcf_phase_nuc(DevArgs A, VphArgs P) {
  __shared__ double s_lk[256];
  stage_lk(s_lk, A);
  __syncthreads();
  nuc_family_rows(
      A,
      [&](const LeanRow& r, int p0, int n) {
        for (int j = 0; j < n; j++) d_store_phase(P.phase + r.out + p0 + j, 0.0, 0.0, 0.0);
      },
      [&](const LeanRow& r, int, int, int p0, int n) {
        const int np = A.n_person;
        const uint8_t* pl = r.pl;
        const int g11 = r.g11, g12 = r.g12, g22 = r.g22;
        pm_vcf_phase* out = P.phase + r.out;
        double pp[9], wk[9];
        d_parent_prior((!A.n_fam_gt1 && !r.mono) ? PR_TRIO : PR_AUTO, r.freq, pp);
        {
          const double lF[3] = {s_lk[PLB(pl, np, p0, g11)], s_lk[PLB(pl, np, p0, g12)], s_lk[PLB(pl, np, p0, g22)]};
          const double lM[3] = {s_lk[PLB(pl, np, p0 + 1, g11)], s_lk[PLB(pl, np, p0 + 1, g12)], s_lk[PLB(pl, np, p0 + 1, g22)]};
#pragma unroll
          for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) wk[3 * x + y] = (lF[x] * lM[y]) * pp[3 * x + y];   // pg[k] * pp[k]
        }
        d_store_phase(out + p0, 0.0, 0.0, 0.0);
        d_store_phase(out + p0 + 1, 0.0, 0.0, 0.0);
        for (int j = 2; j < n; j++) {
          double q11 = 0.0, q12 = 0.0, q22 = 0.0, v[9];
#pragma unroll
          for (int k = 0; k < 9; k++) {
            double J[3];
            d_kid_geno(PM_CHR_AUTO, pl, np, s_lk, p0, n, A.sex, g11, g12, g22, j, k, J);
            const double w = wk[k];
            J[0] *= w; J[1] *= w; J[2] *= w;
            v[k] = J[1];
            q11 = k == 0 ? J[0] : q11 + J[0]; q12 = k == 0 ? J[1] : q12 + J[1]; q22 = k == 0 ? J[2] : q22 + J[2];
          }
          double n12, n21;
          d_phase_split(v, A.fa_local[p0 + j] == 1, n12, n21);
          d_store_phase(out + p0 + j, q11 + q12 + q22, n12, n21);
        }
      });
}

// The es loop over the non-founders of the peeled families (VphArgs::kids) and DevArgs::ws: the seven (a, b) pairs with
// T[a][b][1] != 0, each one clamped three-state peel in the reference's operation order with father = a, mother = b, child =
// het (d_es_lk3_vdn<true>, both of its tables the plain transmission in LDS: d_es_lk<3>'s autosomal arithmetic), and one
// unclamped peel for the family likelihood.
template <bool LDSWS>
__global__ void __launch_bounds__(256) k_vcf_phase_es(DevArgs A, VphArgs P) {
  __shared__ double s_lk[256];
  __shared__ double s_tba[27];
  stage_lk(s_lk, A);
  stage_tba(s_tba);
  __syncthreads();
  es_rows<LDSWS>(A, A.ws, P.kids, P.n_kids, [&](const LeanRow& r, int e, double* wsl, size_t stride) {
    const int f = e >> 8, jc = e & 255;
    const int p0 = A.fam_start[f], fa = A.fa_local[p0 + jc], mo = A.mo_local[p0 + jc];
    const int gidx[3] = {r.g11, r.g12, r.g22};
    // d_phase_split's sums with a = the father's state, taken as the peels come: k = 1, 2, 4, 5 into n12 and k = 3, 4, 6, 7
    // into n21 are its two orders, the weights 0, 1/2, 1 are exact and so is adding the +0 of a term that is left out
    double n12 = 0.0, n21 = 0.0;
#pragma unroll 1
    for (int k = 1; k < 8; k++) {   // (a, b) = (k / 3, k % 3): all but (0, 0) and (2, 2)
      const double J = d_es_lk3_vdn<true>(A, f, r.pl, s_lk, gidx, r.freq, s_tba, s_tba, wsl, stride, fa, 1 << (k / 3), mo, 1 << (k % 3), jc, 1 << 1);
      const double w12 = (k == 1 || k == 2 || k == 5) ? 1.0 : k == 4 ? 0.5 : 0.0;
      const double w21 = (k == 3 || k == 6 || k == 7) ? 1.0 : k == 4 ? 0.5 : 0.0;
      n12 += w12 * J; n21 += w21 * J;
    }
    const double L = d_es_lk3_vdn<false>(A, f, r.pl, s_lk, gidx, r.freq, s_tba, s_tba, wsl, stride);
    d_store_phase(P.phase + r.out + p0 + jc, L, n12, n21);
  });
}
