// vcf_plane_dev.h -- the loops every output plane of the --in_vcf path runs (vcf_post_dev.h, vcf_phase_dev.h,
// vcf_joint_dev.h), written once.  A plane is one value per (written row, person), filled by one extra pass behind the
// standard posterior stage with that stage's routing of a section's families:
//   lean  (lean_fam_table + lean_family_rows)  autosomal sections whose families are nuclear ones of <= 4 persons or
//         founders only: k_posterior_lean's row-blocked loop;
//   nuc   (nuc_family_rows)  every other nuclear or founders-only family, one thread per (row, family);
//   es    (es_rows)  the peeled families, one thread per (row, item of the plane's own list), over a peel workspace.
// A plane's kernel stages its tables, calls one of the loops and hands it the plane's arithmetic per family (or item) as a
// lambda, which the compiler inlines: no function pointer, nothing captured that is not a register or a kernel argument.
// Included by engine.hip after engine_dev.h.
#pragma once
#include <type_traits>

__device__ __forceinline__ void stage_lk(double* s_lk, const DevArgs& A) {
  for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lk[i] = A.lktab[i];
}
__device__ __forceinline__ void stage_tba(double* s_tba) {   // the plain transmission table
  if (threadIdx.x < 27) s_tba[threadIdx.x] = c_TBA[0][threadIdx.x];
}

// The family table of the lean loop in LDS, in fam_perm order: first person | persons << 24 | nuclear << 31.
// extra(fi, f, p0, n, nuc): what else a plane keeps per family.  The block's barrier is the caller's.
template <class Extra>
__device__ __forceinline__ void lean_fam_table(const DevArgs& A, uint32_t* s_fam, Extra extra) {
  for (int fi = threadIdx.x; fi < A.n_fam; fi += blockDim.x) {
    const int f = A.fam_perm[fi];
    const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0;
    const bool nuc = A.fam_kind[f] == PM_FAM_NUCLEAR;
    s_fam[fi] = (uint32_t)p0 | (uint32_t)n << 24 | (nuc ? 1u << 31 : 0u);
    extra(fi, f, p0, n, nuc);
  }
}
__device__ __forceinline__ void lean_fam_table(const DevArgs& A, uint32_t* s_fam) {
  lean_fam_table(A, s_fam, [](int, int, int, int, bool) {});
}

// Row-blocked: a block per emitted row at a time, its threads striding over the families of s_fam, the next row's set-up
// loaded under this row's arithmetic.  A lane owns a family: its persons are contiguous and adjacent lanes hold adjacent
// families, so a wave writes one contiguous stretch of the plane.
//   nuc_body(integral_constant<int, NF>, cur, pp, fi, p0, n, by)  a nuclear family from its 12 PL bytes (lean_fam_bytes)
//       and the row's parent prior pp[9]; NF = 4 or 3 where the whole wave has that many persons, else 0 (fam_perm groups
//       families by size, so a wave's families almost always share one);
//   founders_body(cur, p0, n)  a founders-only family.
template <class Nuc, class Founders>
__device__ __forceinline__ void lean_family_rows(const DevArgs& A, const uint32_t* s_fam, Nuc nuc_body, Founders founders_body) {
  const int rows = A.counts[3], np = A.n_person, nf = A.n_fam;
  int row = blockIdx.x;
  if (row >= rows || (int)threadIdx.x >= nf) return;
  LeanRow cur, nxt;
  lean_row(A, row, cur);
  for (; row < rows; row += gridDim.x) {
    if (row + (int)gridDim.x < rows) lean_row(A, row + gridDim.x, nxt);
    double pp[9];
    d_parent_prior((!A.n_fam_gt1 && !cur.mono) ? PR_TRIO : PR_AUTO, cur.freq, pp);
    for (int fi = threadIdx.x; fi < nf; fi += blockDim.x) {
      const uint32_t d = s_fam[fi];
      const int p0 = d & 0xFFFFFF, n = (d >> 24) & 127;
      if (d >> 31) {
        uint32_t by[12];
        lean_fam_bytes(cur.pl, np, p0, n, cur.g11, cur.g12, cur.g22, by);
        const int n0 = __builtin_amdgcn_readfirstlane(n);
        const bool uni = __builtin_amdgcn_ballot_w64(n != n0) == 0;
        if (uni && n0 == 4) nuc_body(std::integral_constant<int, 4>{}, cur, pp, fi, p0, n, by);
        else if (uni && n0 == 3) nuc_body(std::integral_constant<int, 3>{}, cur, pp, fi, p0, n, by);
        else nuc_body(std::integral_constant<int, 0>{}, cur, pp, fi, p0, n, by);
      } else {
        founders_body(cur, p0, n);
      }
    }
    cur = nxt;
  }
}

// One thread per (row, family) in fam_perm order: founders_body(r, p0, n) for a founders-only family,
// nuc_body(r, row, f, p0, n) for a nuclear one the section does not peel.  Peeled families are the es kernel's.
template <class Founders, class Nuc>
__device__ __forceinline__ void nuc_family_rows(const DevArgs& A, Founders founders_body, Nuc nuc_body) {
  const long long work = (long long)A.counts[3] * A.n_fam;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < work; gid += stride) {
    const int row = (int)(gid / A.n_fam), f = A.fam_perm[(int)(gid % A.n_fam)];
    LeanRow r;
    lean_row(A, row, r);
    const int p0 = A.fam_start[f], n = A.fam_start[f + 1] - p0, kind = A.fam_kind[f];
    if (kind == PM_FAM_FOUNDERS) { founders_body(r, p0, n); continue; }
    if (kind != PM_FAM_NUCLEAR || A.nuc_es) continue;
    nuc_body(r, row, f, p0, n);
  }
}

// A reduction over rows (vcf_pedcheck_dev.h) turns the loops above inside out: a work item -- a family, or a child of one --
// is owned by a thread over a stripe of rows, and the thread keeps the item's NA integer accumulators in registers.  With
// IT = min(n_items, block) items side by side, thread t takes item base + t % IT on row lane t / IT of block / IT: adjacent
// lanes hold adjacent items at the same row, so the PL reads stay coalesced, and block b's row lane rl takes the rows
// b * RL + rl, + grid * RL, ...  body(item, row0, row_step, acc) runs the thread's rows and adds to acc[NA].  The block then
// sums its row lanes' accumulators in s_acc [block * NA] (LDS integer adds: any order gives the same bits) and hands every
// non-zero sum to flush(item, a, sum) once: at most one global atomic per (block, accumulator) and launch.  Blocks without
// a row leave at once.
template <int NA, class Body, class Flush>
__device__ __forceinline__ void stripe_items(int rows, int n_items, unsigned long long* s_acc, Body body, Flush flush) {
  const int bt = blockDim.x;
  const int IT = n_items < bt ? n_items : bt;
  if (IT <= 0) return;
  const int RL = bt / IT;
  if ((long long)blockIdx.x * RL >= rows) return;
  const int il = threadIdx.x % IT, rl = threadIdx.x / IT;
  for (int base = 0; base < n_items; base += IT) {
    for (int i = threadIdx.x; i < IT * NA; i += bt) s_acc[i] = 0;
    __syncthreads();
    if (base + il < n_items && rl < RL) {
      long long acc[NA];
#pragma unroll
      for (int a = 0; a < NA; a++) acc[a] = 0;
      body(base + il, (int)blockIdx.x * RL + rl, (int)gridDim.x * RL, acc);
#pragma unroll
      for (int a = 0; a < NA; a++)
        if (acc[a]) atomicAdd(&s_acc[il * NA + a], (unsigned long long)acc[a]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < IT * NA; i += bt) {
      const unsigned long long v = s_acc[i];
      if (v && base + i / NA < n_items) flush(base + i / NA, i % NA, v);
    }
    __syncthreads();
  }
}

// One thread per (row, item of items[n_items]): body(r, item, wsl, stride) with the thread's peel workspace wsl, strided
// by stride.  LDSWS: the workspace in dynamic LDS, interleaved across the block's threads, instead of the lane-interleaved
// HBM one (hbm_ws, sized for the grid; DevArgs::ws is idle once the standard stage's kernels are done on the stream).
template <bool LDSWS, class Body>
__device__ __forceinline__ void es_rows(const DevArgs& A, double* hbm_ws, const int* items, int n_items, Body body) {
  extern __shared__ double s_wsp[];
  const long long work = (long long)A.counts[3] * n_items;
  const size_t gid_base = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = LDSWS ? (size_t)blockDim.x : (size_t)gridDim.x * blockDim.x;
  double* wsl = LDSWS ? s_wsp + threadIdx.x : hbm_ws + gid_base;
  for (long long gid = (long long)gid_base; gid < work; gid += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(gid / n_items), item = items[gid % n_items];
    LeanRow r;
    lean_row(A, row, r);
    body(r, item, wsl, stride);
  }
}
