// vcf_denovo_dev.h -- de novo calling on the --in_vcf path (pm_engine_set_vcf_denovo): the three-genotype mutation model of
// include/polymutt_engine.h, one more Brent item per called autosomal site.  Included by engine.hip after engine_dev.h.
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
#pragma once

enum VdnTerm { VT_PEEL = 0, VT_NUC = 1, VT_PERSON = 2 };

struct VdnArgs {
  const int* terms;   // [n_terms] family (peeled, nuclear) or person index: n_peel peeled families, n_nuc nuclear ones, then persons
  int n_terms, n_peel, n_nuc;
  int co_lds;         // the hoisted coefficients [5][n_terms - n_peel] in dynamic LDS (else co, one slice per block)
  double* co;
  double* ws;         // peel workspace [grid][ws_per_lane][T], lane-interleaved like DevArgs::ws
};

// d_es_lk<3> on an autosome with the transmission tables passed in (LDS): tdn where the de novo model mutates, tba elsewhere
__device__ __forceinline__ double d_es_lk3_vdn(const DevArgs& A, int f, const uint8_t* pl, const double* lk, const int* gidx, double freq,
                                               const double* tdn, const double* tba, double* ws, size_t st) {
  const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0, nf = A.fam_founders[f];
#define PP(i, j) ws[((size_t)(i) * 3 + (j)) * st]
#define MPP(sl, x, y) ws[((size_t)n * 3 + (size_t)(sl) * 9 + (x) * 3 + (y)) * st]
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
  const int s0 = A.peel_start[f], s1 = A.peel_start[f + 1];
  for (int s = s0; s < s1; s++) {
    const int2 S = A.steps[s];
    const int type = S.x & 255, from0 = (S.x >> 8) & 255, from1 = (S.x >> 16) & 255, to0 = (S.x >> 24) & 255;
    const int slot = (S.y >> 8) & 255, create = (S.y >> 16) & 1, fa2mo = (S.y >> 17) & 1;
    if (type == 1) {   // offspring -> parents: transmission_denovo
      if (create)
        for (int x = 0; x < 9; x++) MPP(slot, x / 3, x % 3) = 1.0;
      double pk[3];
#pragma unroll
      for (int k = 0; k < 3; k++) pk[k] = PP(from0, k);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          double sum = 0;
#pragma unroll
          for (int k = 0; k < 3; k++) sum += tdn[(i * 3 + j) * 3 + k] * pk[k];
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
      const double* tt = slot == 255 ? tdn : tba;
      double pf[3], pm[3], sum[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { pf[k] = PP(from0, k); pm[k] = PP(from1, k); sum[k] = 0.0; }
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
