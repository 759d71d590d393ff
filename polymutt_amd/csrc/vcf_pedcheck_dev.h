// vcf_pedcheck_dev.h -- the pedigree check of the --in_vcf path (pm_engine_set_vcf_pedcheck): for every non-founder c, summed
// over every written row of every autosomal batch, the log10 likelihood ratio of the stated pedigree against one in which
// c's father, c's mother or both are unrelated to c.  With L0 the family's likelihood under the distribution behind the
// genotype rows and the three planes (same founder priors, same single-family prior mode, same family routing, plain
// transmission T) and pi = (f^2, 2 f (1 - f), (1 - f)^2) at the row's frequency f,
//   L_fa    the same with c's transmission T_fa[a][b][k] = Sum_a' pi(a') T[a'][b][k]  (the paternal allele from the population),
//   L_mo    its mirror T_mo[a][b][k] = Sum_b' pi(b') T[a][b'][k],
//   L_both  T_un[a][b][k] = pi(k);
// everybody else, c's own children included, keeps its table.  T is symmetric in the parents, so T_fa[a][b] = U[b] and
// T_mo[a][b] = U[a] with the one 3 x 3 table U[s][k] = Sum_a' pi(a') T[a'][s][k] (d_pc_mix).  A row counts for c when all
// four likelihoods are finite and positive; it then adds 1 to n and q_h = llrint(log10(L0 / L_h) * 2^28) to three int64
// sums.  Integer sums do not depend on the order: any split of the rows into batches, grids, workspaces, engines and shards
// gives the same bits.  Nothing is summed across rows in floating point.  Included by engine.hip after vcf_joint_dev.h.
//
// One extra pass after the joint plane's, on the engine's stream, only with the feature on and only on autosomal sections,
// routed as the planes are but over vcf_plane_dev.h's stripe_items: a thread owns a family or a child over a stripe of rows,
// keeps the sums in registers, the block adds its threads' in LDS and issues at most one 64-bit atomicAdd per accumulator:
//   k_vcf_pedcheck_lean  the nuclear families of <= 4 persons of a lean section from their 12 PL bytes and pp[9];
//   k_vcf_pedcheck_nuc   the children (VpcArgs::kids) of the nuclear families a section without the lean loop does not peel;
//   k_vcf_pedcheck_es    the non-founders of the peeled families: one unaltered d_es_lk3_vdn peel and three with c's table
//                        replaced (its ALT parameter).
// Founders-only families contribute nothing.  No scratch; a row's operations run in a fixed order.
#pragma once

#define PC_SCALE 268435456.0   // 2^28: a row's quantisation error is <= 2^-29, the int64 range 3.4e10 log10 units

// the plain transmission table c_TBA[0], [father][mother][child], for loops whose indices are known when the code is compiled
static __device__ constexpr double kPcT[27] = {1, 0, 0, .5, .5, 0, 0, 1, 0, .5, .5, 0, .25, .5, .25, 0, .5, .5, 0, 1, 0, 0, .5, .5, 0, 0, 1};

struct VpcArgs {
  unsigned long long* acc;   // [non-founders][4]: n, q father, q mother, q both (two's complement sums)
  const int* slot;           // [n_person] a non-founder's index in acc, -1 for a founder
  const int* kids;           // [n_kids] family << 8 | member: the nuc / es kernel's children of the plan in use
  int n_kids;
};

__device__ __forceinline__ void d_pc_prior(double f, double* pi) {   // d_es_lk3_vdn's founder prior
  pi[0] = f * f; pi[1] = 2 * f * (1 - f); pi[2] = (1 - f) * (1 - f);
}

// U[s][k] = Sum_a' pi(a') T[a'][s][k] in a' order
__device__ __forceinline__ void d_pc_mix(const double* pi, double* u) {
#pragma unroll
  for (int s = 0; s < 3; s++)
#pragma unroll
    for (int k = 0; k < 3; k++)
      u[3 * s + k] = (d_joint_tmul(kPcT[s * 3 + k], pi[0]) + d_joint_tmul(kPcT[(3 + s) * 3 + k], pi[1])) + d_joint_tmul(kPcT[(6 + s) * 3 + k], pi[2]);
}

// (t0, t1, t2) . (l0, l1, l2), the table's values known when the code is compiled
__device__ __forceinline__ double d_pc_dot_c(double t0, double t1, double t2, const double* l) {
  return (d_joint_tmul(t0, l[0]) + d_joint_tmul(t1, l[1])) + d_joint_tmul(t2, l[2]);
}
__device__ __forceinline__ double d_pc_dot(const double* t, const double* l) { return (t[0] * l[0] + t[1] * l[1]) + t[2] * l[2]; }

// One row's share of c's four accumulators
__device__ __forceinline__ void d_pc_add(long long* acc, double L0, double Lfa, double Lmo, double Lun) {
  const double big = __builtin_huge_val();
  if (!(L0 > 0.0 && L0 < big && Lfa > 0.0 && Lfa < big && Lmo > 0.0 && Lmo < big && Lun > 0.0 && Lun < big)) return;
  acc[0] += 1;
  acc[1] += llrint(log10(L0 / Lfa) * PC_SCALE);
  acc[2] += llrint(log10(L0 / Lmo) * PC_SCALE);
  acc[3] += llrint(log10(L0 / Lun) * PC_SCALE);
}

// A nuclear family's child c at one row: w[k] = the parental pair's likelihoods and prior, k = 3 a + b (a: person p0's
// state, b: person p0 + 1's), rest[k] = w[k] times the other children's factors Sum_g T[k][g] l[g], lc = c's three
// likelihoods.  sw: the family lists the mother first (person p0 + 1 is c's father), as d_phase_split's sw.
__device__ __forceinline__ void d_pc_nuc_child(const double* rest, const double* lc, const double* pi, const double* u, bool sw,
                                               long long* acc) {
  double su[3];
#pragma unroll
  for (int s = 0; s < 3; s++) su[s] = d_pc_dot(u + 3 * s, lc);
  const double sn = d_pc_dot(pi, lc);
  double L0 = 0.0, L1st = 0.0, L2nd = 0.0, R = 0.0;   // L1st: person p0 unrelated to c (the table keeps b), L2nd: person p0 + 1
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double r = rest[k];
    const double t0 = r * d_pc_dot_c(kPcT[3 * k], kPcT[3 * k + 1], kPcT[3 * k + 2], lc), t1 = r * su[k % 3], t2 = r * su[k / 3];
    L0 = k == 0 ? t0 : L0 + t0; L1st = k == 0 ? t1 : L1st + t1; L2nd = k == 0 ? t2 : L2nd + t2; R = k == 0 ? r : R + r;
  }
  d_pc_add(acc, L0, sw ? L2nd : L1st, sw ? L1st : L2nd, R * sn);
}

// The lean loop's families, a thread per family and stripe of rows: accumulators 0..3 the first child's, 4..7 the second's.
__global__ void __launch_bounds__(256) k_vcf_pedcheck_lean(DevArgs A, VpcArgs P) {
  __shared__ double s_lk[256];
  __shared__ unsigned long long s_acc[256 * 8];
  stage_lk(s_lk, A);
  __syncthreads();
  const int rows = A.counts[3], np = A.n_person;
  stripe_items<8>(
      rows, A.n_fam, s_acc,
      [&](int fi, int row0, int row_step, long long* acc) {
        const int f = A.fam_perm[fi];
        if (A.fam_kind[f] != PM_FAM_NUCLEAR) return;
        const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0;   // 3 or 4 on a lean section
        const bool two = n == 4;
        const bool sw0 = A.fa_local[p0 + 2] == 1, sw1 = two && A.fa_local[p0 + 3] == 1;
        for (int row = row0; row < rows; row += row_step) {
          LeanRow r;
          lean_row(A, row, r);
          double pp[9], pi[3], u[9];
          d_parent_prior((!A.n_fam_gt1 && !r.mono) ? PR_TRIO : PR_AUTO, r.freq, pp);
          d_pc_prior(r.freq, pi);
          d_pc_mix(pi, u);
          uint32_t by[12];
          lean_fam_bytes(r.pl, np, p0, n, r.g11, r.g12, r.g22, by);
          double lF[3], lM[3], kl[2][3];
#pragma unroll
          for (int t = 0; t < 3; t++) {
            lF[t] = s_lk[by[t]]; lM[t] = s_lk[by[3 + t]]; kl[0][t] = s_lk[by[6 + t]]; kl[1][t] = s_lk[by[9 + t]];
          }
          double w[9], r0[9], r1[9];   // r0: what the first child's factor multiplies, r1: the second's
#pragma unroll
          for (int k = 0; k < 9; k++) {
            w[k] = (lF[k / 3] * lM[k % 3]) * pp[k];
            r0[k] = two ? w[k] * d_pc_dot_c(kPcT[3 * k], kPcT[3 * k + 1], kPcT[3 * k + 2], kl[1]) : w[k];
            r1[k] = w[k] * d_pc_dot_c(kPcT[3 * k], kPcT[3 * k + 1], kPcT[3 * k + 2], kl[0]);
          }
          d_pc_nuc_child(r0, kl[0], pi, u, sw0, acc);
          if (two) d_pc_nuc_child(r1, kl[1], pi, u, sw1, acc + 4);
        }
      },
      [&](int fi, int a, unsigned long long v) {
        const int sl = P.slot[A.fam_start[A.fam_perm[fi]] + 2 + a / 4];   // (v is non-zero: a nuclear family's child)
        if (sl >= 0) atomicAdd(P.acc + (size_t)sl * 4 + a % 4, v);
      });
}

// The nuc loop's children, a thread per child and stripe of rows: d_parent_prior as k_vcf_post_nuc takes it, the children's
// factors in person order.
__global__ void __launch_bounds__(256) k_vcf_pedcheck_nuc(DevArgs A, VpcArgs P) {
  __shared__ double s_lk[256];
  __shared__ unsigned long long s_acc[256 * 4];
  stage_lk(s_lk, A);
  __syncthreads();
  const int rows = A.counts[3], np = A.n_person;
  stripe_items<4>(
      rows, P.n_kids, s_acc,
      [&](int it, int row0, int row_step, long long* acc) {
        const int e = P.kids[it], f = e >> 8, jc = e & 255;
        const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0;
        const bool sw = A.fa_local[p0 + jc] == 1;
        for (int row = row0; row < rows; row += row_step) {
          LeanRow r;
          lean_row(A, row, r);
          const uint8_t* pl = r.pl;
          const int g11 = r.g11, g12 = r.g12, g22 = r.g22;
          double pp[9], pi[3], u[9];
          d_parent_prior((!A.n_fam_gt1 && !r.mono) ? PR_TRIO : PR_AUTO, r.freq, pp);
          d_pc_prior(r.freq, pi);
          d_pc_mix(pi, u);
          const double lF[3] = {s_lk[PLB(pl, np, p0, g11)], s_lk[PLB(pl, np, p0, g12)], s_lk[PLB(pl, np, p0, g22)]};
          const double lM[3] = {s_lk[PLB(pl, np, p0 + 1, g11)], s_lk[PLB(pl, np, p0 + 1, g12)], s_lk[PLB(pl, np, p0 + 1, g22)]};
          double rest[9], lc[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int k = 0; k < 9; k++) rest[k] = (lF[k / 3] * lM[k % 3]) * pp[k];
          for (int j = 2; j < n; j++) {
            const double l[3] = {s_lk[PLB(pl, np, p0 + j, g11)], s_lk[PLB(pl, np, p0 + j, g12)], s_lk[PLB(pl, np, p0 + j, g22)]};
            if (j == jc) { lc[0] = l[0]; lc[1] = l[1]; lc[2] = l[2]; continue; }
#pragma unroll
            for (int k = 0; k < 9; k++) rest[k] *= d_pc_dot_c(kPcT[3 * k], kPcT[3 * k + 1], kPcT[3 * k + 2], l);
          }
          d_pc_nuc_child(rest, lc, pi, u, sw, acc);
        }
      },
      [&](int it, int a, unsigned long long v) {
        const int e = P.kids[it], sl = P.slot[A.fam_start[e >> 8] + (e & 255)];
        if (sl >= 0) atomicAdd(P.acc + (size_t)sl * 4 + a, v);
      });
}

// What d_es_lk3_vdn's ALT parameter asks of c's alternative table: mode 0 the father, 1 the mother, 2 both unrelated to c.
// A step's partial is indexed (i, j) by its two parents; first_fa says that i is the father's state.  The values sit in
// registers: the step's loops are unrolled, so every index here is known when the code is compiled.
struct PcAlt {
  int c, fa, mode;
  double u0, u1, u2, u3, u4, u5, u6, u7, u8, q0, q1, q2;   // U and pi, a field each: every read below is of a named field
  __device__ __forceinline__ void set(const double* pi, const double* u) {
    u0 = u[0]; u1 = u[1]; u2 = u[2]; u3 = u[3]; u4 = u[4]; u5 = u[5]; u6 = u[6]; u7 = u[7]; u8 = u[8];
    q0 = pi[0]; q1 = pi[1]; q2 = pi[2];
  }
  __device__ __forceinline__ double uu(int x) const {
    return x == 0 ? u0 : x == 1 ? u1 : x == 2 ? u2 : x == 3 ? u3 : x == 4 ? u4 : x == 5 ? u5 : x == 6 ? u6 : x == 7 ? u7 : u8;
  }
  __device__ __forceinline__ bool is_child(int i) const { return i == c; }
  __device__ __forceinline__ bool is_father(int i) const { return i == fa; }
  __device__ __forceinline__ double t(bool first_fa, int i, int j, int k) const {
    const bool by_j = (mode == 0) == first_fa;   // the parent that stays related holds the second index
    const double a = uu(3 * j + k), b = uu(3 * i + k), p = k == 0 ? q0 : k == 1 ? q1 : q2;
    return mode == 2 ? p : by_j ? a : b;
  }
};

// The es loop's children (the phase plane's list), a thread per child and stripe of rows: four peels per row, both tables
// of each the plain transmission in LDS.  The block's sums follow the LDS workspace (A.ws_per_lane doubles per thread) in
// dynamic LDS; with the HBM workspace (DevArgs::ws, one lane per thread of the grid) they are static.
template <bool LDSWS>
__global__ void __launch_bounds__(256) k_vcf_pedcheck_es(DevArgs A, VpcArgs P) {
  extern __shared__ double s_wsp[];
  __shared__ double s_lk[256];
  __shared__ double s_tba[27];
  __shared__ unsigned long long s_acc_hbm[LDSWS ? 1 : 256 * 4];
  unsigned long long* s_acc = LDSWS ? reinterpret_cast<unsigned long long*>(s_wsp + (size_t)A.ws_per_lane * blockDim.x) : s_acc_hbm;
  stage_lk(s_lk, A);
  stage_tba(s_tba);
  __syncthreads();
  const int rows = A.counts[3];
  const size_t stride = LDSWS ? (size_t)blockDim.x : (size_t)gridDim.x * blockDim.x;
  double* wsl = LDSWS ? s_wsp + threadIdx.x : A.ws + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  stripe_items<4>(
      rows, P.n_kids, s_acc,
      [&](int it, int row0, int row_step, long long* acc) {
        const int e = P.kids[it], f = e >> 8;
        PcAlt alt;
        alt.c = e & 255;
        alt.fa = A.fa_local[A.fam_start[f] + alt.c];
        for (int row = row0; row < rows; row += row_step) {
          LeanRow r;
          lean_row(A, row, r);
          const int gidx[3] = {r.g11, r.g12, r.g22};
          double pi[3], u[9];
          d_pc_prior(r.freq, pi);
          d_pc_mix(pi, u);
          alt.set(pi, u);
          const double L0 = d_es_lk3_vdn<false>(A, f, r.pl, s_lk, gidx, r.freq, s_tba, s_tba, wsl, stride);
          double Lfa = 0.0, Lmo = 0.0, Lun = 0.0;
#pragma unroll 1
          for (int m = 0; m < 3; m++) {
            alt.mode = m;
            const double v = d_es_lk3_vdn<false, false, true, PcAlt>(A, f, r.pl, s_lk, gidx, r.freq, s_tba, s_tba, wsl, stride, -1, 0, -1, 0,
                                                                      -1, 0, alt);
            if (m == 0) Lfa = v; else if (m == 1) Lmo = v; else Lun = v;
          }
          d_pc_add(acc, L0, Lfa, Lmo, Lun);
        }
      },
      [&](int it, int a, unsigned long long v) {
        const int e = P.kids[it], sl = P.slot[A.fam_start[e >> 8] + (e & 255)];
        if (sl >= 0) atomicAdd(P.acc + (size_t)sl * 4 + a, v);
      });
}
