// vcf_denovo_dev.h -- de novo calling on the --in_vcf path (pm_engine_set_vcf_denovo): the three-genotype mutation model of
// include/polymutt_engine.h, one more Brent item per called autosomal site -- and, behind pm_engine_set_vcf_denovo_chrx, per
// called chrX site (k_vdn_brent_x, a kernel of its own below).  Included by engine.hip after engine_dev.h.
//
// On a biallelic record only the genotypes g = (g11, g12, g22) of (ref, alt) carry data, so the 10 x 10 genotype
// mutation matrix M collapses to M3[x][y] = M[g[x]][g[y]] and the de novo transmission to
//     Tdn[i][j][k] = Sum_m T[i][j][m] M3[m][k]       (T: the autosomal bi-allelic transmission, c_TBA[0]).
// The objective is the vcf_mode one (FamilyLikelihoodSeq_VCF::CalcAllFamLogLikelihood, Hardy-Weinberg founder priors
// everywhere) with the families routed as k_brent routes them, every transmission followed by M3:
//   founders-only families  the product of single persons: (l11 t^2 + 2 l12 t + l22) g^2 per person, t = f / g, g = 1 - f;
//   nuclear families        (n_fam > 1) the closed form over the 9 parental pairs, each kid's factor d_one_kid_dn of
//                           D = M3 l; a quartic Sum_k c_k t^k g^4 whose five coefficients are hoisted once per item;
//   everything else         the bi-allelic Elston-Stewart peel in the reference's operation order (d_es_lk3_vdn) with Tdn
//                           in type-1 steps and in type-3 steps without a marriage partial, plain T in type-3 steps with
//                           one (FamilyLikelihoodES.cpp:1391, the quirk d_es_lk<10> keeps as well); a lone nuclear
//                           family goes this way through its schedule, as on vcf_mode's plan 1.
// One block per item; the block's threads take the terms (a peeled family, a nuclear family or a founder person each)
// round robin, the per-thread products are combined by vdn_logprod (fixed order, one log10 per evaluation), and the
// item runs OptimizeFrequency + Brent through brent_core.h's state machine like every other item.
//
// The autosomal and the chrX kernels (k_vdn_brent / k_vdn_brent_x, and k_vdn_who / k_vdn_who_x for the families and
// children behind each DQ) differ in their term lists and argument structs and stay apart; what they compute alike is
// written once, with the chrX model behind a template parameter X: the peel (d_es_lk3_vdn), lkSinglePerson
// (vdn_person_lk) and a founders-only family's product of it (vdn_founders_lk), the per-site tables of the two who
// kernels (vdn_tables), stages B and C of their clamped peels (vdn_stage_b, vdn_stage_c) and their sums and rankings
// (vdn_rank_fams, vdn_rank_kids, on engine_dev.h's block_sum_fixed and block_top_k).  The two Brent kernels keep their
// own text of the table set-up, and k_vdn_brent of the nuclear closed form (vdn_nuc_lk holds the other): with either
// behind a shared function the compiler schedules the Brent kernels differently, and they are the ones a run waits for.
#pragma once

enum VdnTerm { VT_PEEL = 0, VT_NUC = 1, VT_PERSON = 2 };

struct VdnArgs {
  const int* terms;   // [n_terms] family (peeled, nuclear) or person index: n_peel peeled families, n_nuc nuclear ones, then persons
  int n_terms, n_peel, n_nuc;
  int co_lds;         // the hoisted coefficients [5][n_terms - n_peel] in dynamic LDS (else co, one slice per block)
  double* co;
  double* ws;         // peel workspace [grid][ws_per_lane][T], lane-interleaved like DevArgs::ws
};

__device__ __forceinline__ int vdn_pick3(const int* g, int s) { return s == 0 ? g[0] : s == 1 ? g[1] : g[2]; }

// d_es_lk<3> with the transmission tables passed in (LDS): tdn where the de novo model mutates, tpl (plain) elsewhere.
// X: the chrX model -- a male founder takes the prior (f, 0, 1 - f) and the tables are picked by the sex of the step's
// child, t[0] to a daughter (or a child of unknown sex), t[27] to a son; without X one autosomal table each.
// CL: three more persons c0, c1, c2 (family-local indices) are clamped to the state sets m0, m1, m2 (bit s = state s of
// (g11, g12, g22) allowed), where the initial partials are filled, as d_es_lk<10, true> does (k_vdn_who, k_vdn_who_x);
// without CL nothing is added.
// ALT (vcf_pedcheck_dev.h): the steps whose child is the family-local person alt.c -- type 1 from it, type 3 to it -- take
// alt's table in place of tdn / tpl; without ALT nothing is added.
struct EsAltNone {};
template <bool CL = false, bool X = false, bool ALT = false, class Alt = EsAltNone>
__device__ __forceinline__ double d_es_lk3_vdn(const DevArgs& A, int f, const uint8_t* pl, const double* lk, const int* gidx, double freq,
                                               const double* tdn, const double* tpl, double* ws, size_t st, int c0 = -1, int m0 = 0,
                                               int c1 = -1, int m1 = 0, int c2 = -1, int m2 = 0, Alt alt = Alt()) {
  const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0, nf = A.fam_founders[f];
#define PP(i, j) ws[((size_t)(i) * 3 + (j)) * st]
#define MPP(sl, x, y) ws[((size_t)n * 3 + (size_t)(sl) * 9 + (x) * 3 + (y)) * st]
  const size_t np = (size_t)A.n_person;
  for (int i = 0; i < n; i++) {
    const bool fo = A.is_founder[p0 + i] != 0;
    const uint8_t* R = pl + p0 + i;   // plane g at R[g * n_person]
    double pr[3] = {0.0, 0.0, 0.0};
    if (i < nf) {
      pr[0] = freq * freq; pr[1] = 2 * freq * (1 - freq); pr[2] = (1 - freq) * (1 - freq);
      if (X && A.sex[p0 + i] == MALE) { pr[0] = freq; pr[1] = 0; pr[2] = 1 - freq; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double pen = lk[R[gidx[j] * np]];
      if (CL)
        if ((i == c0 && !((m0 >> j) & 1)) || (i == c1 && !((m1 >> j) & 1)) || (i == c2 && !((m2 >> j) & 1))) pen = 0.0;
      PP(i, j) = fo ? pr[j] * pen : pen;
    }
  }
  const int s0 = A.peel_start[f], s1 = A.peel_start[f + 1];
  for (int s = s0; s < s1; s++) {
    const int2 S = A.steps[s];
    const int type = S.x & 255, from0 = (S.x >> 8) & 255, from1 = (S.x >> 16) & 255, to0 = (S.x >> 24) & 255;
    const int slot = (S.y >> 8) & 255, create = (S.y >> 16) & 1, fa2mo = (S.y >> 17) & 1;
    if (type == 1) {   // offspring -> parents: transmission_denovo (X: of the child's sex)
      if (create)
        for (int x = 0; x < 9; x++) MPP(slot, x / 3, x % 3) = 1.0;
      const double* tt = tdn + (X && A.sex[p0 + from0] == MALE ? 27 : 0);
      double pk[3];
#pragma unroll
      for (int k = 0; k < 3; k++) pk[k] = PP(from0, k);
      if constexpr (ALT) {
        if (alt.is_child(from0)) {
          const bool first_fa = alt.is_father(to0);   // the partial's first index is the father's state
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
              double sum = 0;
#pragma unroll
              for (int k = 0; k < 3; k++) sum += alt.t(first_fa, i, j, k) * pk[k];
              MPP(slot, i, j) *= sum;
            }
          continue;
        }
      }
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          double sum = 0;
#pragma unroll
          for (int k = 0; k < 3; k++) sum += tt[(i * 3 + j) * 3 + k] * pk[k];
          MPP(slot, i, j) *= sum;
        }
    } else if (type == 2) {   // spouse -> spouse
      double ps[3];
#pragma unroll
      for (int j = 0; j < 3; j++) ps[j] = PP(from0, j);
      for (int i = 0; i < 3; i++) {
        double sum = 0.0;
        if (slot == 255) for (int j = 0; j < 3; j++) sum += ps[j];
        else if (fa2mo) for (int j = 0; j < 3; j++) sum += ps[j] * MPP(slot, j, i);
        else for (int j = 0; j < 3; j++) sum += ps[j] * MPP(slot, i, j);
        PP(to0, i) *= sum;
      }
    } else {   // parents -> only offspring: transmission_denovo without a marriage partial, plain transmission with one
      const double* tt = (slot == 255 ? tdn : tpl) + (X && A.sex[p0 + to0] == MALE ? 27 : 0);
      double pf[3], pm[3], sum[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { pf[k] = PP(from0, k); pm[k] = PP(from1, k); sum[k] = 0.0; }
      if constexpr (ALT) {
        if (alt.is_child(to0)) {
          const bool first_fa = alt.is_father(from0);
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
              const double w = (slot == 255) ? pf[i] * pm[j] : pf[i] * MPP(slot, i, j) * pm[j];
#pragma unroll
              for (int k = 0; k < 3; k++) sum[k] += w * alt.t(first_fa, i, j, k);
            }
#pragma unroll
          for (int k = 0; k < 3; k++) PP(to0, k) *= sum[k];
          continue;
        }
      }
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          const double w = (slot == 255) ? pf[i] * pm[j] : pf[i] * MPP(slot, i, j) * pm[j];
#pragma unroll
          for (int k = 0; k < 3; k++) sum[k] += w * tt[(i * 3 + j) * 3 + k];
        }
#pragma unroll
      for (int k = 0; k < 3; k++) PP(to0, k) *= sum[k];
    }
  }
  const int fin = (A.steps[s1 - 1].x >> 24) & 255;
  double L = 0.0;
  for (int i = 0; i < 3; i++) L += PP(fin, i);
  return L;
#undef PP
#undef MPP
}

// block_logprod with a log10 that keeps its relative accuracy where the product is near 1 (a site without data in a small
// pedigree: L = 1 - 5e-8 under the mutation model, 1 under the standard one).  log10_mant_u adds e log10(2) to the
// table's log10 of the mantissa; for L = 1 = 0.5 x 2^1 the two cancel to 2^-53 instead of 0, and DQ = N - D of ~1e-8 is
// lost in it.  For |e| <= 1 the product is rebuilt exactly (ldexp) and given to log10 whole.
template <int T>
__device__ __forceinline__ double vdn_logprod(double m, int e, double* red, int* rede, int& par) {
  wave_prod(m, e);
  if (T > 64) {
    constexpr int W = T / 64;
    if ((threadIdx.x & 63) == 0) { red[par * 16 + (threadIdx.x >> 6)] = m; rede[par * 16 + (threadIdx.x >> 6)] = e; }
    __syncthreads();
    m = red[par * 16]; e = rede[par * 16];
#pragma unroll
    for (int i = 1; i < W; i++) {
      int ev;
      m = frexp(m * red[par * 16 + i], &ev);
      e += rede[par * 16 + i] + ev;
    }
    par ^= 1;
  }
  if (e >= -1 && e <= 1) return log10(ldexp(m, e));
  return log10_mant_u(m, e);
}

// The per-site tables of a record with the alleles (a1, a2): m3 = M3, on X h3 = H3 (the haploid mutation matrix: the
// 2 x 2 block of the allele mutation matrix a4 on states 0 and 2, row and column 1 zero), and tdn = the plain table(s)
// tpl followed by them -- [0..26] T M3 (on X: to a daughter), on X [27..53] to a son, followed by H3.  Every thread of
// the block calls it (k_vdn_who, k_vdn_who_x); the tables are written when it returns.
template <bool X>
__device__ __forceinline__ void vdn_tables(const int* gidx, int a1, int a2, const double* M, const double* a4, const double* tpl,
                                           double* m3, double* h3, double* tdn) {
  __syncthreads();   // (the previous row no longer reads the tables, the lines or jbuf; tpl is written)
  if (threadIdx.x < 9) {
    const int x = threadIdx.x / 3, y = threadIdx.x % 3;
    m3[threadIdx.x] = M[vdn_pick3(gidx, x) * 10 + vdn_pick3(gidx, y)];
    if (X) h3[threadIdx.x] = (x == 1 || y == 1) ? 0.0 : a4[(((x ? a2 : a1) - 1) & 3) * 4 + (((y ? a2 : a1) - 1) & 3)];   // (bases are 1..4)
  }
  __syncthreads();
  if (threadIdx.x < (X ? 54 : 27)) {
    const int ij = (X ? threadIdx.x % 27 : threadIdx.x) / 3, k = threadIdx.x % 3;
    const double* tp = tpl + (!X || threadIdx.x < 27 ? 0 : 27);
    const double* mm = !X || threadIdx.x < 27 ? m3 : h3;
    double s = 0.0;
    for (int m = 0; m < 3; m++) s += tp[ij * 3 + m] * mm[m * 3 + k];
    tdn[threadIdx.x] = s;
  }
  __syncthreads();
}

// lkSinglePerson at the frequency x (g = 1 - x) of a person with the likelihoods (l11, l12, l22): a male on X is hemizygous
template <bool X>
__device__ __forceinline__ double vdn_person_lk(double l11, double l12, double l22, bool male, double x, double g) {
  return X && male ? l11 * x + l22 * g : l11 * (x * x) + l12 * (2 * x * g) + l22 * (g * g);
}

// The de novo Brent item of every site of list 0 (the called sites of a vcf_mode batch): results to raw / minv / evals
// slot 2 of the site, a stuck Brent to counts[5] / counts[6] like k_brent's.
template <int T>
__global__ void __launch_bounds__(T) k_vdn_brent(DevArgs A, VdnArgs V) {
  __shared__ double s_lk[256];
  __shared__ double s_tba[27], s_tdn[27], s_m3[9];
  __shared__ double s_red[T > 64 ? 96 : 1];
  __shared__ int s_rede[T > 64 ? 32 : 1];
  extern __shared__ double s_vco[];
  for (int i = threadIdx.x; i < 256; i += T) s_lk[i] = A.lktab[i];
  if (threadIdx.x < 27) s_tba[threadIdx.x] = c_TBA[0][threadIdx.x];
  const int nco = V.n_terms - V.n_peel;
  double* co = V.co_lds ? s_vco : V.co + (size_t)blockIdx.x * 5 * nco;
  double* ws = V.ws + (size_t)blockIdx.x * A.ws_per_lane * T + threadIdx.x;
  const int nItems = A.counts[0];
  const int* items = A.items[0];
  const size_t np = (size_t)A.n_person;
  int par = 0;
  unsigned long long ev_acc = 0;
  for (int it = blockIdx.x; it < nItems; it += gridDim.x) {
    const int site = items[it] >> 3;
    const int r = A.ref[site];
    const int a1 = r & 15, a2 = r >> 4;
    const int gidx[3] = {d_gi(a1, a1), d_gi(a1, a2), d_gi(a2, a2)};
    const uint8_t* pl = A.pl + (size_t)site * np * 10;
    __syncthreads();   // (the tables and coefficients of the block's previous item are no longer read)
    if (threadIdx.x < 9) s_m3[threadIdx.x] = A.M[gidx[threadIdx.x / 3] * 10 + gidx[threadIdx.x % 3]];
    __syncthreads();
    if (threadIdx.x < 27) {
      const int ij = threadIdx.x / 3, k = threadIdx.x % 3;
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += s_tba[ij * 3 + m] * s_m3[m * 3 + k];
      s_tdn[threadIdx.x] = s;
    }
    // Two passes over the same code: pass 0 the standard objective (no mutation: M3 = identity, plain T everywhere),
    // evaluated once at the standard item's maximiser for D; pass 1 the de novo objective through Brent for N.
    // (DQ = N - D is taken between two values of this kernel's log10, see vdn_logprod.)
    const double f_std = A.minv[site * 8 + 1];
    double d_std = 0.0;
    PmBrent B;
    for (int pass = 0; pass < 2; pass++) {
    const bool dn = pass != 0;
    const double* tt = dn ? s_tdn : s_tba;
    __syncthreads();   // (s_tdn is written; the previous pass no longer reads the coefficients)
    // hoisting: the frequency-independent coefficients of the nuclear families and the founder persons
    for (int q = threadIdx.x; q < nco; q += T) {
      const int x = V.terms[V.n_peel + q];
      double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // c[k]: the coefficient of f^k g^(D - k)
      if (q < V.n_nuc) {
        const int p0 = A.fam_start[x], n = A.fam_start[x + 1] - p0;
        const uint8_t* P = pl + p0;
        double lF[3], lM[3], kids[9];
#pragma unroll
        for (int j = 0; j < 3; j++) { lF[j] = s_lk[P[gidx[j] * np]]; lM[j] = s_lk[P[gidx[j] * np + 1]]; }
#pragma unroll
        for (int k = 0; k < 9; k++) kids[k] = 1.0;
        for (int j = 2; j < n; j++) {
          const double l0 = s_lk[P[gidx[0] * np + j]], l1 = s_lk[P[gidx[1] * np + j]], l2 = s_lk[P[gidx[2] * np + j]];
          // CalcDenovoMutLk on the three genotypes (pass 0: likelihoodONEKid on l itself)
          const double D11 = dn ? s_m3[0] * l0 + s_m3[1] * l1 + s_m3[2] * l2 : l0;
          const double D12 = dn ? s_m3[3] * l0 + s_m3[4] * l1 + s_m3[5] * l2 : l1;
          const double D22 = dn ? s_m3[6] * l0 + s_m3[7] * l1 + s_m3[8] * l2 : l2;
#pragma unroll
          for (int k = 0; k < 9; k++) kids[k] *= d_one_kid_dn(k, D11, D12, D22);
        }
        double cond[9];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
          for (int b = 0; b < 3; b++) cond[3 * a + b] = kids[3 * a + b] * (lF[a] * lM[b]);
        // SetParentPrior (d_parent_prior PR_AUTO) by powers of f
        c[4] = cond[0];
        c[3] = 2 * (cond[1] + cond[3]);
        c[2] = cond[2] + cond[6] + 4 * cond[4];
        c[1] = 2 * (cond[5] + cond[7]);
        c[0] = cond[8];
      } else {   // lkSinglePerson: f^2 l11 + 2 f g l12 + g^2 l22
        const uint8_t* P = pl + x;
        c[2] = s_lk[P[gidx[0] * np]];
        c[1] = 2 * s_lk[P[gidx[1] * np]];
        c[0] = s_lk[P[gidx[2] * np]];
      }
#pragma unroll
      for (int k = 0; k < 5; k++) co[(size_t)k * nco + q] = c[k];
    }
    __syncthreads();
    pm_brent_init(B, A.precision, A.itmax);
    if (!dn) B.x = f_std;
    for (;;) {
      const double x = B.x, g = 1 - x;   // x in [0.0001, 0.9999]: g > 0
      const double t = pos_div(x, g), g2 = g * g, g4 = g2 * g2;
      double m = 1.0;
      int e = 0;
      for (int q = threadIdx.x; q < V.n_peel; q += T) {
        int e1, e2;
        const double mv = frexp(d_es_lk3_vdn(A, V.terms[q], pl, s_lk, gidx, x, tt, s_tba, ws, T), &e1);
        m = frexp(m * mv, &e2);
        e += e1 + e2;
      }
      for (int q = threadIdx.x; q < nco; q += T) {
        double acc = co[(size_t)4 * nco + q];
#pragma unroll
        for (int k = 3; k >= 0; k--) acc = fma(acc, t, co[(size_t)k * nco + q]);
        int e1, e2;
        const double mv = frexp(acc * (q < V.n_nuc ? g4 : g2), &e1);
        m = frexp(m * mv, &e2);
        e += e1 + e2;
      }
      const double tot = vdn_logprod<T>(m, e, s_red, s_rede, par);
      if (!dn) { d_std = tot; break; }
      if (!pm_brent_feed(B, -tot)) break;
    }
    }
    if (threadIdx.x == 0) {
      A.raw[(size_t)site * 8 + 3] = d_std;
      A.raw[(size_t)site * 8 + 2] = -B.fmin;
      A.minv[site * 8 + 2] = B.mn;
      A.evals[site * 8 + 2] = B.nev;
      ev_acc += B.nev - 1;   // (f(a) and f(c) are counted, not computed; one evaluation for D)
      if (!B.ok) { atomicExch(&A.counts[5], 1); atomicMin(&A.counts[6], site); }
    }
  }
  if (threadIdx.x == 0 && ev_acc) atomicAdd(A.eval_total, ev_acc);
}

// N, its maximiser and evaluation count, and DQ = N - D of every called site (D: k_vdn_brent's value of the standard
// objective at varfreq[1], raw slot 3)
__global__ void __launch_bounds__(256) k_finalize_vdn(DevArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.counts[0]) return;
  const int site = A.items[0][i] >> 3;
  pm_site_result* R = A.res + site;
  const double N = A.raw[(size_t)site * 8 + 2];
  R->varllk[2] = N;
  R->varfreq[2] = A.minv[site * 8 + 2];
  R->evals[2] = A.evals[site * 8 + 2];
  R->denovo_lr = N - A.raw[(size_t)site * 8 + 3];
}

// ------------------------------------------------------------------------------------------------
// chrX (pm_engine_set_vcf_denovo_chrx): the sex-aware three-state model of include/polymutt_engine.h.  A male carries the
// states 0 and 2 only (hemizygous a1, a2), so a son's transmission c_TBA[2] is followed by the haploid mutation matrix
// H3 and a daughter's c_TBA[1] by M3 (vdn_tables<true>); male founders take the prior (f, 0, 1 - f).  There is no closed
// form on X: every family with offspring is peeled on every evaluation (vcf_mode's plan 1 routing), a founders-only
// family is the product of its persons.
struct VdnXArgs {
  const int* terms;   // [n_terms] n_peel peeled families (every family with offspring), then the persons of founders-only families
  int n_terms, n_peel;
  double* ws;         // peel workspace [grid][ws_per_lane][T], lane-interleaved like DevArgs::ws
  double a4[16];      // the allele mutation matrix of denovo_mut_rate / denovo_tstv (the one M is built from)
};

// The chrX de novo Brent item of every site of list 0: k_vdn_brent's outputs (raw / minv / evals slot 2, D to raw slot 3,
// a stuck Brent to counts[5] / counts[6]) for k_finalize_vdn.  One block per item, the terms round robin over its threads.
template <int T>
__global__ void __launch_bounds__(T) k_vdn_brent_x(DevArgs A, VdnXArgs V) {
  __shared__ double s_lk[256];
  __shared__ double s_tpl[54], s_tdn[54], s_m3[9], s_h3[9];   // [0..26] to a daughter, [27..53] to a son
  __shared__ double s_red[T > 64 ? 96 : 1];
  __shared__ int s_rede[T > 64 ? 32 : 1];
  for (int i = threadIdx.x; i < 256; i += T) s_lk[i] = A.lktab[i];
  if (threadIdx.x < 54) s_tpl[threadIdx.x] = c_TBA[1 + threadIdx.x / 27][threadIdx.x % 27];
  double* ws = V.ws + (size_t)blockIdx.x * A.ws_per_lane * T + threadIdx.x;
  const int nItems = A.counts[0];
  const int* items = A.items[0];
  const size_t np = (size_t)A.n_person;
  int par = 0;
  unsigned long long ev_acc = 0;
  for (int it = blockIdx.x; it < nItems; it += gridDim.x) {
    const int site = items[it] >> 3;
    const int r = A.ref[site];
    const int a1 = r & 15, a2 = r >> 4;
    const int gidx[3] = {d_gi(a1, a1), d_gi(a1, a2), d_gi(a2, a2)};
    const uint8_t* pl = A.pl + (size_t)site * np * 10;
    __syncthreads();   // (the tables of the block's previous item are no longer read; s_tpl is written)
    if (threadIdx.x < 9) {
      const int x = threadIdx.x / 3, y = threadIdx.x % 3;
      s_m3[threadIdx.x] = A.M[vdn_pick3(gidx, x) * 10 + vdn_pick3(gidx, y)];
      s_h3[threadIdx.x] = (x == 1 || y == 1) ? 0.0 : V.a4[(((x ? a2 : a1) - 1) & 3) * 4 + (((y ? a2 : a1) - 1) & 3)];   // (bases are 1..4)
    }
    __syncthreads();
    if (threadIdx.x < 54) {
      const int ij = (threadIdx.x % 27) / 3, k = threadIdx.x % 3;
      const double* tp = s_tpl + (threadIdx.x < 27 ? 0 : 27);
      const double* mm = threadIdx.x < 27 ? s_m3 : s_h3;
      double s = 0.0;
      for (int m = 0; m < 3; m++) s += tp[ij * 3 + m] * mm[m * 3 + k];
      s_tdn[threadIdx.x] = s;
    }
    __syncthreads();
    // Two passes over the same code, as in k_vdn_brent: pass 0 the standard chrX objective (plain T everywhere) once at
    // the standard item's maximiser for D; pass 1 the de novo objective through Brent for N.
    const double f_std = A.minv[site * 8 + 1];
    double d_std = 0.0;
    PmBrent B;
    for (int pass = 0; pass < 2; pass++) {
      const bool dn = pass != 0;
      const double* tt = dn ? s_tdn : s_tpl;
      pm_brent_init(B, A.precision, A.itmax);
      if (!dn) B.x = f_std;
      for (;;) {
        const double x = B.x, g = 1 - x;
        double m = 1.0;
        int e = 0;
        for (int q = threadIdx.x; q < V.n_peel; q += T) {
          int e1, e2;
          const double mv = frexp(d_es_lk3_vdn<false, true>(A, V.terms[q], pl, s_lk, gidx, x, tt, s_tpl, ws, T), &e1);
          m = frexp(m * mv, &e2);
          e += e1 + e2;
        }
        for (int q = V.n_peel + threadIdx.x; q < V.n_terms; q += T) {
          const int p = V.terms[q];
          const uint8_t* P = pl + p;
          const double l11 = s_lk[P[gidx[0] * np]], l12 = s_lk[P[gidx[1] * np]], l22 = s_lk[P[gidx[2] * np]];
          const double v = vdn_person_lk<true>(l11, l12, l22, A.sex[p] == MALE, x, g);
          int e1, e2;
          const double mv = frexp(v, &e1);
          m = frexp(m * mv, &e2);
          e += e1 + e2;
        }
        const double tot = vdn_logprod<T>(m, e, s_red, s_rede, par);
        if (!dn) { d_std = tot; break; }
        if (!pm_brent_feed(B, -tot)) break;
      }
    }
    if (threadIdx.x == 0) {
      A.raw[(size_t)site * 8 + 3] = d_std;
      A.raw[(size_t)site * 8 + 2] = -B.fmin;
      A.minv[site * 8 + 2] = B.mn;
      A.evals[site * 8 + 2] = B.nev;
      ev_acc += B.nev - 1;   // (f(a) and f(c) are counted, not computed; one evaluation for D)
      if (!B.ok) { atomicExch(&A.counts[5], 1); atomicMin(&A.counts[6], site); }
    }
  }
  if (threadIdx.x == 0 && ev_acc) atomicAdd(A.eval_total, ev_acc);
}

// ------------------------------------------------------------------------------------------------
// The families and the children behind each DQ (pm_engine_set_vcf_denovo_detail, and on chrX
// pm_engine_set_vcf_denovo_chrx_detail).  A row is a called site with evals[2] > 0 (the de novo item ran) and
// denovo_lr >= pm_params.denovo_min_llr; rows are numbered in site order.
struct VdnWhoArgs {
  int fam_k, car_k;         // 0 (that half is off) or 1..8
  int* row_site;            // [max_batch] row -> site (k_vdn_rows; the row count goes to counts[10])
  pm_fam_lr* fam_top;       // [rows][fam_k]
  double* fam_sum;          // [rows]
  double* fam_all;          // [rows][n_fam], or null
  double* fam_line;         // [gridDim.x][n_fam] when fam_all is null
  const int* pfam;          // [n_person] the person's family
  pm_person_dn* car_top;    // [rows][car_k]
  pm_person_dn* car_all;    // [rows][n_person], or null
  pm_person_dn* car_line;   // [gridDim.x][n_person] when car_all is null
  const int2* kids;         // the non-founders {family, member}: n_nuc of closed-form nuclear families, then n_es of peeled ones
  int n_nuc, n_es;          // (chrX: n_nuc = 0, every child is peeled)
  const int8_t* is_kid;     // [n_person] 1 = listed in kids
  double* jbuf;             // [gridDim.x][n_es * 13] clamped-peel values: 9 pairs, 3 single states, L_f
};

// Rows in site order: one block walks the batch in 1024-site pieces, an exclusive scan per piece, so the table is the same
// on every run.
__global__ void __launch_bounds__(1024) k_vdn_rows(DevArgs A, int* row_site) {
  __shared__ int s_w[16];
  int base = 0;
  for (int s0 = 0; s0 < A.n; s0 += 1024) {   // (block-uniform)
    const int site = s0 + threadIdx.x;
    int e = 0;
    if (site < A.n) {
      const pm_site_result* R = A.res + site;
      e = (R->status == PM_SITE_CALLED && R->evals[2] > 0 && R->denovo_lr >= A.denovo_min_llr) ? 1 : 0;
    }
    int total;
    const int pre = block_excl_scan_1024(e, s_w, total);
    if (e) row_site[base + pre] = site;
    base += total;
    __syncthreads();   // (s_w is rewritten by the next piece)
  }
  if (threadIdx.x == 0) A.counts[10] = base;
}

// log10 of m 2^e taken of the whole double where it is one (vdn_logprod's rule: a family without data gives ~-2e-8)
__device__ __forceinline__ double vdn_log10_me(double m, int e) {
  if (e >= -1 && e <= 1) return log10(ldexp(m, e));
  return log10(m) + e * 0.30102999566398119521;
}

// A nuclear family's closed form at the parental priors pp (d_parent_prior(PR_AUTO)): k_vdn_brent's hoisting, pass DN
template <bool DN>
__device__ __forceinline__ double vdn_nuc_lk(const uint8_t* P, size_t np, int n, const int* gidx, const double* lk, const double* m3,
                                             const double* pp) {
  double lF[3], lM[3], kids[9];
#pragma unroll
  for (int j = 0; j < 3; j++) { lF[j] = lk[P[gidx[j] * np]]; lM[j] = lk[P[gidx[j] * np + 1]]; }
#pragma unroll
  for (int k = 0; k < 9; k++) kids[k] = 1.0;
  for (int j = 2; j < n; j++) {
    const double l0 = lk[P[gidx[0] * np + j]], l1 = lk[P[gidx[1] * np + j]], l2 = lk[P[gidx[2] * np + j]];
    const double D11 = DN ? m3[0] * l0 + m3[1] * l1 + m3[2] * l2 : l0;
    const double D12 = DN ? m3[3] * l0 + m3[4] * l1 + m3[5] * l2 : l1;
    const double D22 = DN ? m3[6] * l0 + m3[7] * l1 + m3[8] * l2 : l2;
#pragma unroll
    for (int k = 0; k < 9; k++) kids[k] *= d_one_kid_dn(k, D11, D12, D22);
  }
  double v = 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) v += (kids[3 * a + b] * (lF[a] * lM[b])) * pp[3 * a + b];
  return v;
}

// the family of term q of a list whose first n_fam_terms terms are families and whose others are founder persons, -1 for
// a founder person that is not its family's first (that person's term carries the whole founders-only family)
__device__ __forceinline__ int vdn_term_fam(const DevArgs& A, const int* terms, int n_fam_terms, const VdnWhoArgs& W, int q) {
  const int x = terms[q];
  if (q < n_fam_terms) return x;
  const int f = W.pfam[x];
  return x == A.fam_start[f] ? f : -1;
}

// A founders-only family at the frequencies xN and xD: the product of lkSinglePerson in person order, the same form in
// both models, as normalised (mantissa, exponent) pairs
template <bool X>
__device__ __forceinline__ void vdn_founders_lk(const DevArgs& A, int f, const uint8_t* pl, const double* lk, const int* gidx, double xN,
                                                double xD, double& mN, int& eN, double& mD, int& eD) {
  const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0;
  const size_t np = (size_t)A.n_person;
  mN = 1.0; mD = 1.0; eN = 0; eD = 0;
  const double gN = 1 - xN, gD = 1 - xD;
  for (int j = 0; j < n; j++) {
    const uint8_t* P = pl + p0 + j;
    const double l11 = lk[P[gidx[0] * np]], l12 = lk[P[gidx[1] * np]], l22 = lk[P[gidx[2] * np]];
    const bool male = X && A.sex[p0 + j] == MALE;
    int e1;
    mN = frexp(mN * vdn_person_lk<X>(l11, l12, l22, male, xN, gN), &e1);
    eN += e1;
    mD = frexp(mD * vdn_person_lk<X>(l11, l12, l22, male, xD, gD), &e1);
    eD += e1;
  }
}

// NonMendX(a, b, sex): the states a child of that sex can carry (a son 0 and 2, anyone else all three) that the plain
// transmission from parents in states (a, b) gives probability 0, as a 3-bit mask.  tpl: [0..26] to a daughter, [27..53]
// to a son.  Empty for a son of a heterozygous mother.
__device__ __forceinline__ int vdnx_nonmend(const double* tpl, int k, bool male) {
  const double* t = tpl + (male ? 27 : 0) + k * 3;
  int m = 0;
#pragma unroll
  for (int s = 0; s < 3; s++)
    if (!(male && s == 1) && t[s] == 0.0) m |= 1 << s;
  return m;
}

// The rest of a row's family half, behind the loop that wrote the terms' D_f to line and summed them to part: the row's
// sum and the top fam_k families.  term_fam(q): vdn_term_fam of the kernel's list.
template <int T, class TermFam>
__device__ __forceinline__ void vdn_rank_fams(const VdnWhoArgs& W, int row, const double* line, double part, int n_terms,
                                              double (*red)[4], int (*redf)[4], int& par, TermFam term_fam) {
  block_sum_fixed<T>(part, red, par, W.fam_sum + row);
  block_top_k<T>(W.fam_k, n_terms, red, redf, par,
    [&](int q, double& d) { const int f = term_fam(q); if (f >= 0) d = line[f]; return f; },   // (written by this thread above)
    [&](int k, double lr, int f) {
      pm_fam_lr o;
      o.fam = f == INT_MAX ? -1 : f; o.pad = 0; o.lr = f == INT_MAX ? 0.0 : lr;
      W.fam_top[(size_t)row * W.fam_k + k] = o;
    });
}

// founders (and anyone without both parents) have no value in a row's line of children
template <int T>
__device__ __forceinline__ void vdn_clear_nonkids(const VdnWhoArgs& W, pm_person_dn* line, int np) {
  for (int p = threadIdx.x; p < np; p += T)
    if (!W.is_kid[p]) {
      pm_person_dn o;
      o.person = p; o.fa_g = o.mo_g = o.kid_g = -1; o.pad = 0; o.pp = 0.0;
      line[p] = o;
    }
}

// Stage B of the clamped peels of the n_es children kids[] (jb: the block's jbuf, [n_es * 9] stage A's pair terms J, then
// [n_es * 4] this stage's): per child the unclamped L_f, and the best pair's peels with the child clamped to each single
// state of the pair's non-Mendelian set (-1 for the others).  X: the chrX peel and NonMendX of the child's sex.
template <int T, bool X>
__device__ __forceinline__ void vdn_stage_b(const DevArgs& A, const int2* kids, int n_es, const uint8_t* pl, const double* lk, const int* gidx,
                                            double xN, const double* tdn, const double* tpl, double* ws, double* jb) {
  double* jb2 = jb + (size_t)n_es * 9;
  for (int it = threadIdx.x; it < n_es * 4; it += T) {
    const int ci = it / 4, slot = it % 4;
    const int2 kd = kids[ci];
    const int p0 = A.fam_start[kd.x], jc = kd.y, fa = A.fa_local[p0 + jc], mo = A.mo_local[p0 + jc];
    double v = -1.0;
    if (slot == 3) v = d_es_lk3_vdn<false, X>(A, kd.x, pl, lk, gidx, xN, tdn, tpl, ws, T);
    else {
      double bj = 0.0;
      int bi = -1;
      for (int q = 0; q < 9; q++) { const double J = jb[ci * 9 + q]; if (J > bj) { bj = J; bi = q; } }
      if (bi >= 0 && (((X ? vdnx_nonmend(tpl, bi, A.sex[p0 + jc] == MALE) : 7 & ~d_mend3(bi)) >> slot) & 1))
        v = d_es_lk3_vdn<true, X>(A, kd.x, pl, lk, gidx, xN, tdn, tpl, ws, T, fa, 1 << (bi / 3), mo, 1 << (bi % 3), jc, 1 << slot);
    }
    jb2[it] = v;
  }
}

// Stage C: one thread per child sums the nine pair terms in (a, b) order and names the event
template <int T>
__device__ __forceinline__ void vdn_stage_c(const DevArgs& A, const int2* kids, int n_es, const int* gidx, const double* jb, pm_person_dn* line) {
  const double* jb2 = jb + (size_t)n_es * 9;
  for (int ci = threadIdx.x; ci < n_es; ci += T) {
    const int2 kd = kids[ci];
    const int p = A.fam_start[kd.x] + kd.y;
    double num = 0.0, bj = 0.0;
    int bi = -1;
    for (int q = 0; q < 9; q++) { const double J = jb[ci * 9 + q]; num += J; if (J > bj) { bj = J; bi = q; } }
    const double L = jb2[ci * 4 + 3];
    double bv = 0.0;
    int bs = -1;
    for (int s = 0; s < 3; s++) { const double v = jb2[ci * 4 + s]; if (v > bv) { bv = v; bs = s; } }
    pm_person_dn o;
    o.person = p; o.pad = 0;
    o.fa_g = (int8_t)(bs < 0 ? -1 : vdn_pick3(gidx, bi / 3)); o.mo_g = (int8_t)(bs < 0 ? -1 : vdn_pick3(gidx, bi % 3));
    o.kid_g = (int8_t)(bs < 0 ? -1 : vdn_pick3(gidx, bs));
    o.pp = L > 0.0 ? fmin(num / L, 1.0) : 0.0;   // (L_f and the terms come from separate peels: rounding may pass 1)
    line[p] = o;
  }
}

// the top car_k of a row's children by pp (line: every child's entry, visible to the block)
template <int T>
__device__ __forceinline__ void vdn_rank_kids(const DevArgs& A, const VdnWhoArgs& W, int row, const pm_person_dn* line, double (*red)[4],
                                              int (*redf)[4], int& par) {
  block_top_k<T>(W.car_k, W.n_nuc + W.n_es, red, redf, par,
    [&](int i, double& d) { const int2 kd = W.kids[i]; const int p = A.fam_start[kd.x] + kd.y; d = line[p].pp; return p; },
    [&](int k, double, int p) {
      pm_person_dn o;
      o.person = -1; o.fa_g = o.mo_g = o.kid_g = -1; o.pad = 0; o.pp = 0.0;
      if (p != INT_MAX) o = line[p];
      W.car_top[(size_t)row * W.car_k + k] = o;
    });
}

// k_vdn_who: per row, in the three states of the record's (ref, alt) and the model of k_vdn_brent,
//   D_f = log10 L_f^dn(varfreq[2]) - log10 L_f^std(varfreq[1]) of every family (k_vdn_brent's factors, pass 1 and pass 0),
//   pp_c = Sum_{a,b} J_c(a, b, NonMend3(a, b)) / L_f^dn and the event of every non-founder c (k_person_dn's definitions),
// and their top-k rankings.  One block of T threads per row at a time, after k_finalize_vdn on the engine's stream (the
// peel workspace is k_vdn_brent's).  Families: the terms round robin over the threads.  Children of closed-form nuclear
// families: one lane per child, registers only.  Children of peeled families: stage A, per (child, a, b) the peel with
// father, mother and child clamped to a, b and NonMend3(a, b) (nothing for 12 x 12: the set is empty); stage B, per child
// the unclamped L_f and the best pair's peels with the child clamped to one state; stage C, one thread per child sums the
// nine terms in (a, b) order.  Barriers between the stages.  Sums and rankings are k_fam_dnlr's fixed trees: no atomics.
template <int T>
__global__ void __launch_bounds__(T) k_vdn_who(DevArgs A, VdnArgs V, VdnWhoArgs W) {
  __shared__ double s_lk[256];
  __shared__ double s_tba[27], s_tdn[27], s_m3[9];
  __shared__ double s_red[2][4];
  __shared__ int s_redf[2][4];
  for (int i = threadIdx.x; i < 256; i += T) s_lk[i] = A.lktab[i];
  if (threadIdx.x < 27) s_tba[threadIdx.x] = c_TBA[0][threadIdx.x];
  const int rows = A.counts[10], nf = A.n_fam;
  const size_t np = (size_t)A.n_person;
  double* ws = V.ws + (size_t)blockIdx.x * A.ws_per_lane * T + threadIdx.x;
  double* jb = W.jbuf + (size_t)blockIdx.x * W.n_es * 13;
  int par = 0;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {   // (block-uniform: every thread reaches the barriers)
    const int site = W.row_site[row];
    const pm_site_result* R = A.res + site;
    const int r = A.ref[site];
    const int a1 = r & 15, a2 = r >> 4;
    const int gidx[3] = {d_gi(a1, a1), d_gi(a1, a2), d_gi(a2, a2)};
    const uint8_t* pl = A.pl + (size_t)site * np * 10;
    const double xN = R->varfreq[2], xD = R->varfreq[1];
    vdn_tables<false>(gidx, a1, a2, A.M, nullptr, s_tba, s_m3, nullptr, s_tdn);
    double ppN[9];
    d_parent_prior(PR_AUTO, xN, ppN);
    if (W.fam_k > 0) {
      double ppD[9];
      d_parent_prior(PR_AUTO, xD, ppD);
      double* line = W.fam_all ? W.fam_all + (size_t)row * nf : W.fam_line + (size_t)blockIdx.x * nf;
      const auto term_fam = [&](int q) { return vdn_term_fam(A, V.terms, V.n_peel + V.n_nuc, W, q); };
      double part = 0.0;
      for (int q = threadIdx.x; q < V.n_terms; q += T) {
        const int f = term_fam(q);
        if (f < 0) continue;
        const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0;
        double l_dn, l_std;
        if (q < V.n_peel) {
          l_dn = log10(d_es_lk3_vdn(A, f, pl, s_lk, gidx, xN, s_tdn, s_tba, ws, T));
          l_std = log10(d_es_lk3_vdn(A, f, pl, s_lk, gidx, xD, s_tba, s_tba, ws, T));
        } else if (q < V.n_peel + V.n_nuc) {
          l_dn = log10(vdn_nuc_lk<true>(pl + p0, np, n, gidx, s_lk, s_m3, ppN));
          l_std = log10(vdn_nuc_lk<false>(pl + p0, np, n, gidx, s_lk, s_m3, ppD));
        } else {
          double mN, mD;
          int eN, eD;
          vdn_founders_lk<false>(A, f, pl, s_lk, gidx, xN, xD, mN, eN, mD, eD);
          l_dn = vdn_log10_me(mN, eN);
          l_std = vdn_log10_me(mD, eD);
        }
        const double D = l_dn - l_std;
        line[f] = D;
        part += D;
      }
      vdn_rank_fams<T>(W, row, line, part, V.n_terms, s_red, s_redf, par, term_fam);
    }
    if (W.car_k > 0) {
      pm_person_dn* line = W.car_all ? W.car_all + (size_t)row * np : W.car_line + (size_t)blockIdx.x * np;
      vdn_clear_nonkids<T>(W, line, (int)np);
      // ---- closed-form nuclear families: one child per lane
      for (int ci = threadIdx.x; ci < W.n_nuc; ci += T) {
        const int2 kd = W.kids[ci];
        const int p0 = A.fam_start[kd.x], n = A.fam_start[kd.x + 1] - p0, jc = kd.y;
        const bool sw = A.fa_local[p0 + jc] == 1;   // (the closed form's first parent is person p0: the father unless the family lists the mother first)
        const uint8_t* P = pl + p0;
        double lF[3], lM[3], w[9];   // w: the family around c -- every other kid's factor, the parents, the prior
#pragma unroll
        for (int j = 0; j < 3; j++) { lF[j] = s_lk[P[gidx[j] * np]]; lM[j] = s_lk[P[gidx[j] * np + 1]]; }
#pragma unroll
        for (int k = 0; k < 9; k++) w[k] = 1.0;
        for (int j = 2; j < n; j++) {
          if (j == jc) continue;
          const double l0 = s_lk[P[gidx[0] * np + j]], l1 = s_lk[P[gidx[1] * np + j]], l2 = s_lk[P[gidx[2] * np + j]];
          const double D11 = s_m3[0] * l0 + s_m3[1] * l1 + s_m3[2] * l2;
          const double D12 = s_m3[3] * l0 + s_m3[4] * l1 + s_m3[5] * l2;
          const double D22 = s_m3[6] * l0 + s_m3[7] * l1 + s_m3[8] * l2;
#pragma unroll
          for (int k = 0; k < 9; k++) w[k] *= d_one_kid_dn(k, D11, D12, D22);
        }
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
          for (int b = 0; b < 3; b++) w[3 * a + b] = (w[3 * a + b] * (lF[a] * lM[b])) * ppN[3 * a + b];
        // c's own factor split by state: e[q][s] = M3[q][s] l_s
        double e[3][3];
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const double ls = s_lk[P[gidx[s] * np + jc]];
#pragma unroll
          for (int q = 0; q < 3; q++) e[q][s] = s_m3[q * 3 + s] * ls;
        }
        double num = 0.0, den = 0.0, bj = 0.0, bw = 0.0;
        int bk = -1, bfa = -1, bmo = -1;
#pragma unroll
        for (int k = 0; k < 9; k++) {
          const int md = d_mend3(k);
          double nm[3], me[3];
#pragma unroll
          for (int q = 0; q < 3; q++) {
            nm[q] = 0.0; me[q] = 0.0;
#pragma unroll
            for (int s = 0; s < 3; s++) {
              if ((md >> s) & 1) me[q] += e[q][s];
              else nm[q] += e[q][s];
            }
          }
          const double fn = d_one_kid_dn(k, nm[0], nm[1], nm[2]), fm = d_one_kid_dn(k, me[0], me[1], me[2]);
          const double Jn = w[k] * fn;
          num += Jn;
          den += w[k] * (fn + fm);   // (term by term >= Jn: num <= den, pp <= 1)
          const int fs = sw ? k % 3 : k / 3, ms = sw ? k / 3 : k % 3;
          if (Jn > bj || (Jn == bj && bk >= 0 && (fs < bfa || (fs == bfa && ms < bmo)))) { bj = Jn; bw = w[k]; bk = k; bfa = fs; bmo = ms; }
        }
        int bs = -1;
        if (bk >= 0) {   // the largest single-state term of the best pair
          const int md = d_mend3(bk);
          double bv = 0.0;
#pragma unroll
          for (int s = 0; s < 3; s++) {
            if ((md >> s) & 1) continue;
            const double v = bw * d_one_kid_dn(bk, e[0][s], e[1][s], e[2][s]);
            if (v > bv) { bv = v; bs = s; }
          }
        }
        pm_person_dn o;
        o.person = p0 + jc; o.pad = 0;
        o.fa_g = (int8_t)(bs < 0 ? -1 : vdn_pick3(gidx, bfa)); o.mo_g = (int8_t)(bs < 0 ? -1 : vdn_pick3(gidx, bmo));
        o.kid_g = (int8_t)(bs < 0 ? -1 : vdn_pick3(gidx, bs));
        o.pp = den > 0.0 ? num / den : 0.0;
        line[p0 + jc] = o;
      }
      // ---- peeled families: clamped peels
      if (W.n_es > 0) {   // (block-uniform)
        const int2* kids = W.kids + W.n_nuc;
        for (int it = threadIdx.x; it < W.n_es * 9; it += T) {   // stage A
          const int ci = it / 9, k = it % 9;
          const int2 kd = kids[ci];
          const int p0 = A.fam_start[kd.x], jc = kd.y, fa = A.fa_local[p0 + jc], mo = A.mo_local[p0 + jc];
          const int nonm = 7 & ~d_mend3(k);
          double J = 0.0;
          if (nonm)
            J = d_es_lk3_vdn<true>(A, kd.x, pl, s_lk, gidx, xN, s_tdn, s_tba, ws, T, fa, 1 << (k / 3), mo, 1 << (k % 3), jc, nonm);
          jb[it] = J;
        }
        __syncthreads();
        vdn_stage_b<T, false>(A, kids, W.n_es, pl, s_lk, gidx, xN, s_tdn, s_tba, ws, jb);
        __syncthreads();
        vdn_stage_c<T>(A, kids, W.n_es, gidx, jb, line);
      }
      __syncthreads();   // the row's entries are visible to the block: the ranking reads what other threads wrote
      vdn_rank_kids<T>(A, W, row, line, s_red, s_redf, par);
    }
  }
}

// k_vdn_who_x: the same per row of a chrX section, in the sex-aware model of k_vdn_brent_x,
//   D_f = log10 L_f^dn(varfreq[2]) - log10 L_f^std(varfreq[1]) of every family (k_vdn_brent_x's factors, pass 1 and pass 0),
//   pp_c = Sum_{a in {0,2}, b} J_c(a, b, NonMendX(a, b, sex_c)) / L_f^dn and the event of every non-founder c,
// and their top-k rankings.  One block of T threads per row at a time, after k_finalize_vdn on the engine's stream (the
// peel workspace is k_vdn_brent_x's).  Families: the terms round robin over the threads.  Children (W.kids: every one is
// peeled, there is no closed form on X; W.n_nuc is 0): k_vdn_who's stages A, B and C with barriers between them.  A father
// has no state 1, so stage A deals out six items per child, not nine, and writes the other three as exact zeros; a son of
// a heterozygous mother has no non-Mendelian state, that pair gives 0 without a peel.
template <int T>
__global__ void __launch_bounds__(T) k_vdn_who_x(DevArgs A, VdnXArgs V, VdnWhoArgs W) {
  __shared__ double s_lk[256];
  __shared__ double s_tpl[54], s_tdn[54], s_m3[9], s_h3[9];   // [0..26] to a daughter, [27..53] to a son
  __shared__ double s_red[2][4];
  __shared__ int s_redf[2][4];
  for (int i = threadIdx.x; i < 256; i += T) s_lk[i] = A.lktab[i];
  if (threadIdx.x < 54) s_tpl[threadIdx.x] = c_TBA[1 + threadIdx.x / 27][threadIdx.x % 27];
  const int rows = A.counts[10], nf = A.n_fam, nk = W.n_es;
  const size_t np = (size_t)A.n_person;
  double* ws = V.ws + (size_t)blockIdx.x * A.ws_per_lane * T + threadIdx.x;
  double* jb = W.jbuf + (size_t)blockIdx.x * nk * 13;
  int par = 0;
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {   // (block-uniform: every thread reaches the barriers)
    const int site = W.row_site[row];
    const pm_site_result* R = A.res + site;
    const int r = A.ref[site];
    const int a1 = r & 15, a2 = r >> 4;
    const int gidx[3] = {d_gi(a1, a1), d_gi(a1, a2), d_gi(a2, a2)};
    const uint8_t* pl = A.pl + (size_t)site * np * 10;
    const double xN = R->varfreq[2], xD = R->varfreq[1];
    vdn_tables<true>(gidx, a1, a2, A.M, V.a4, s_tpl, s_m3, s_h3, s_tdn);
    if (W.fam_k > 0) {
      double* line = W.fam_all ? W.fam_all + (size_t)row * nf : W.fam_line + (size_t)blockIdx.x * nf;
      const auto term_fam = [&](int q) { return vdn_term_fam(A, V.terms, V.n_peel, W, q); };
      double part = 0.0;
      for (int q = threadIdx.x; q < V.n_terms; q += T) {
        const int f = term_fam(q);
        if (f < 0) continue;
        double l_dn, l_std;
        if (q < V.n_peel) {
          l_dn = log10(d_es_lk3_vdn<false, true>(A, f, pl, s_lk, gidx, xN, s_tdn, s_tpl, ws, T));
          l_std = log10(d_es_lk3_vdn<false, true>(A, f, pl, s_lk, gidx, xD, s_tpl, s_tpl, ws, T));
        } else {
          double mN, mD;
          int eN, eD;
          vdn_founders_lk<true>(A, f, pl, s_lk, gidx, xN, xD, mN, eN, mD, eD);
          l_dn = vdn_log10_me(mN, eN);
          l_std = vdn_log10_me(mD, eD);
        }
        const double D = l_dn - l_std;
        line[f] = D;
        part += D;
      }
      vdn_rank_fams<T>(W, row, line, part, V.n_terms, s_red, s_redf, par, term_fam);
    }
    if (W.car_k > 0) {
      pm_person_dn* line = W.car_all ? W.car_all + (size_t)row * np : W.car_line + (size_t)blockIdx.x * np;
      vdn_clear_nonkids<T>(W, line, (int)np);
      if (nk > 0) {   // (block-uniform)
        for (int it = threadIdx.x; it < nk * 6; it += T) {   // stage A: the six pairs of a father in state 0 or 2
          const int ci = it / 6, b = it % 3, k = (it % 6 < 3 ? 0 : 6) + b;
          const int2 kd = W.kids[ci];
          const int p0 = A.fam_start[kd.x], jc = kd.y, fa = A.fa_local[p0 + jc], mo = A.mo_local[p0 + jc];
          const int nonm = vdnx_nonmend(s_tpl, k, A.sex[p0 + jc] == MALE);
          double J = 0.0;
          if (nonm)
            J = d_es_lk3_vdn<true, true>(A, kd.x, pl, s_lk, gidx, xN, s_tdn, s_tpl, ws, T, fa, 1 << (k / 3), mo, 1 << b, jc, nonm);
          jb[ci * 9 + k] = J;
          if (k < 3) jb[ci * 9 + 3 + b] = 0.0;   // a father has no state 1: exactly 0, no peel
        }
        __syncthreads();
        vdn_stage_b<T, true>(A, W.kids, nk, pl, s_lk, gidx, xN, s_tdn, s_tpl, ws, jb);
        __syncthreads();
        vdn_stage_c<T>(A, W.kids, nk, gidx, jb, line);
      }
      __syncthreads();   // the row's entries are visible to the block: the ranking reads what other threads wrote
      vdn_rank_kids<T>(A, W, row, line, s_red, s_redf, par);
    }
  }
}
