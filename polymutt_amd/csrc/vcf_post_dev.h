// vcf_post_dev.h -- the genotype posterior plane of the --in_vcf path (pm_engine_set_vcf_posteriors): for every person of
// every written row the vector post[] = (P(g11), P(g12), P(g22)) given the pedigree, from which the standard posterior
// stage takes the person's best genotype and GQ and which it then drops (d_emit_call keeps 4 bytes).  Included by
// engine.hip after vcf_plane_dev.h, whose three loops its kernels run.
//
// One extra pass after that stage, on the engine's stream, and only with the feature on.  Its kernels write the plane
// (VpArgs::post, [row][person] of pm_vcf_post) and nothing else, so the site results and the genotype rows cannot move.
// Their bodies call the standard stage's device functions:
//   k_vcf_post_lean  lean_nuc_post's own body (its POST instantiation);
//   k_vcf_post_nuc   (more than two children, chrX / chrY / MT sections) hoist_nuc, d_parent_prior and d_kid_geno in
//                    k_posterior<false, false>'s order;
//   k_vcf_post_es    three d_es_lk<3> peels per person as k_posterior_es<false> runs them.  It runs with and without the
//                    schedule compiler, whose generated posterior kernel keeps no vector.
// A value is the double quotient rounded once to float; a zero normalising sum gives three zeros (d_store_post), and so
// does a chrY female (the rows label her PM_LBL_DOT).
#pragma once

struct VpArgs {
  pm_vcf_post* post;   // [max_batch][n_person]
};

// The lean loop: a nuclear family's 3 or 4 persons through lean_nuc_post, a founders-only family's through
// CalcPostProb_SinglePerson's HWE prior (:754-795); 12 bytes per person at a time.
__global__ void __launch_bounds__(256) k_vcf_post_lean(DevArgs A, VpArgs P) {
  __shared__ double s_lk[256];
  extern __shared__ uint32_t s_fam[];   // [n_fam]
  stage_lk(s_lk, A);
  lean_fam_table(A, s_fam);
  __syncthreads();
  lean_family_rows(
      A, s_fam,
      [&](auto nf, const LeanRow& cur, const double* pp, int, int p0, int n, const uint32_t* by) {
        lean_nuc_post<false, decltype(nf)::value, true>(A, s_lk, nullptr, by, cur.out, p0, n, pp, P.post);
      },
      [&](const LeanRow& cur, int p0, int n) {
        const int np = A.n_person;
        const double fq = cur.freq, gq = 1 - cur.freq;
        const double pr0 = fq * fq, pr1 = fq * gq * 2, pr2 = gq * gq;
        for (int j = 0; j < n; j++) {
          const int p = p0 + j;
          const double l11 = s_lk[PLB(cur.pl, np, p, cur.g11)], l12 = s_lk[PLB(cur.pl, np, p, cur.g12)], l22 = s_lk[PLB(cur.pl, np, p, cur.g22)];
          const double m11 = l11 * pr0, m12 = l12 * pr1, m22 = l22 * pr2;
          d_store_post(P.post + cur.out + p, m11 + m12 + m22, m11, m12, m22);
        }
      });
}

// The nuc loop, k_posterior<false, false>'s arithmetic: CalcPostProb_SinglePerson for founders-only families,
// CalcParentMarginal + KidJointGenoLikelihood for nuclear ones (every chromosome class, any number of children; the first
// family's member sex on chrX / chrY is d_member_sex_before's).
__global__ void __launch_bounds__(256) k_vcf_post_nuc(DevArgs A, VpArgs P) {
  __shared__ double s_lk[256];
  stage_lk(s_lk, A);
  __syncthreads();
  const int np = A.n_person, chrom = A.chrom;
  nuc_family_rows(
      A,
      [&](const LeanRow& r, int p0, int n) {
        for (int j = 0; j < n; j++) {   // CalcPostProb_SinglePerson :754-795
          const int p = p0 + j, sx = A.sex[p];
          const double l11 = s_lk[PLB(r.pl, np, p, r.g11)], l12 = s_lk[PLB(r.pl, np, p, r.g12)], l22 = s_lk[PLB(r.pl, np, p, r.g22)];
          const double fq = r.freq, gq = 1 - r.freq;
          double pr0 = fq * fq, pr1 = fq * gq * 2, pr2 = gq * gq;
          if (chrom == PM_CHR_X) { if (sx == MALE) { pr0 = fq; pr1 = 0.; pr2 = 1 - fq; } else { pr0 = fq * fq; pr1 = 2 * fq * gq; pr2 = gq * gq; } }
          if (chrom == PM_CHR_Y) { if (sx == MALE) { pr0 = fq; pr1 = 0.; pr2 = 1 - fq; } else { pr0 = pr1 = pr2 = 1.0; } }
          if (chrom == PM_CHR_MT) { pr0 = fq; pr1 = 0; pr2 = 1 - fq; }
          const double m11 = l11 * pr0, m12 = l12 * pr1, m22 = l22 * pr2;
          const bool yf = chrom == PM_CHR_Y && sx == FEMALE;
          d_store_post(P.post + r.out + p, yf ? 0.0 : m11 + m12 + m22, m11, m12, m22);
        }
      },
      [&](const LeanRow& r, int row, int f, int p0, int n) {
        const uint8_t* pl = r.pl;
        const int g11 = r.g11, g12 = r.g12, g22 = r.g22;
        pm_vcf_post* out = P.post + r.out;
        ItemCtx I;
        I.a1 = 0; I.a2 = 0; I.g11 = g11; I.g12 = g12; I.g22 = g22; I.denovo = 0; I.chrom = chrom;
        I.sex = f == 0 ? d_member_sex_before(A, A.row_site[row]) : A.sex[p0 - 1];   // member sex when family f's CalcParentMarginal runs
        double cond[9], pp[9], wk[9];
        hoist_nuc<true, false>(A, I, pl, s_lk, nullptr, p0, n, cond);
        int pmode;
        if (!A.n_fam_gt1 && !r.mono) pmode = PR_TRIO;
        else pmode = chrom == PM_CHR_X ? PR_X : chrom == PM_CHR_Y ? PR_Y : chrom == PM_CHR_MT ? PR_MT : PR_AUTO;
        d_parent_prior(pmode, r.freq, pp);
        {
          double F11 = s_lk[PLB(pl, np, p0, g11)], F12 = s_lk[PLB(pl, np, p0, g12)], F22 = s_lk[PLB(pl, np, p0, g22)];
          double M11 = s_lk[PLB(pl, np, p0 + 1, g11)], M12 = s_lk[PLB(pl, np, p0 + 1, g12)], M22 = s_lk[PLB(pl, np, p0 + 1, g22)];
          if (chrom == PM_CHR_X) F12 = 0.0;
          if (chrom == PM_CHR_Y) { M11 = M12 = M22 = 1.0; F12 = 0.0; }
          if (chrom == PM_CHR_MT) F12 = M12 = 0.0;
          const double lF[3] = {F11, F12, F22}, lM[3] = {M11, M12, M22};
#pragma unroll
          for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) wk[3 * x + y] = (lF[x] * lM[y]) * pp[3 * x + y];   // pg[k] * pp[k]
        }
        double m[9];
#pragma unroll
        for (int k = 0; k < 9; k++) m[k] = cond[k] * pp[k];
        for (int j = 0; j < n; j++) {
          const int p = p0 + j;
          const bool yf = chrom == PM_CHR_Y && A.sex[p] == FEMALE;
          double q11, q12, q22;
          if (j == 0) { q11 = m[0] + m[1] + m[2]; q12 = m[3] + m[4] + m[5]; q22 = m[6] + m[7] + m[8]; }
          else if (j == 1) { q11 = m[0] + m[3] + m[6]; q12 = m[1] + m[4] + m[7]; q22 = m[2] + m[5] + m[8]; }
          else {   // KidJointGenoLikelihood :798-835: J[0] + J[1] + ... + J[8]
            q11 = q12 = q22 = 0.0;
#pragma unroll
            for (int k = 0; k < 9; k++) {
              double J[3];
              d_kid_geno(chrom, pl, np, s_lk, p0, n, A.sex, g11, g12, g22, j, k, J);
              const double w = wk[k];
              J[0] *= w; J[1] *= w; J[2] *= w;
              q11 = k == 0 ? J[0] : q11 + J[0]; q12 = k == 0 ? J[1] : q12 + J[1]; q22 = k == 0 ? J[2] : q22 + J[2];
            }
          }
          d_store_post(out + p, yf ? 0.0 : q11 + q12 + q22, q11, q12, q22);
        }
      });
}

// The es loop over the persons of the peeled families (DevArgs::es_pers, family << 8 | member):
// k_posterior_es<false>'s three peels with the person clamped to each of its genotypes, in the reference's operation order
// (d_es_lk<3>), over DevArgs::ws where the workspace is not in LDS.
template <bool LDSWS>
__global__ void __launch_bounds__(256) k_vcf_post_es(DevArgs A, VpArgs P) {
  __shared__ double s_lk[256];
  stage_lk(s_lk, A);
  __syncthreads();
  es_rows<LDSWS>(A, A.ws, A.es_pers, A.n_es_pers, [&](const LeanRow& r, int e, double* wsl, size_t stride) {
    const int f = e >> 8, j = e & 255;
    const int chrom = A.chrom;
    const int p = A.fam_start[f] + j;
    pm_vcf_post* out = P.post + r.out + p;
    if (chrom == PM_CHR_Y && A.sex[p] == FEMALE) { d_store_post(out, 0.0, 0.0, 0.0, 0.0); return; }
    const double l11 = d_es_lk<3>(A, f, r.pl, s_lk, r.g11, r.g12, r.g22, chrom, r.freq, j, r.g11, wsl, stride);
    const double l12 = d_es_lk<3>(A, f, r.pl, s_lk, r.g11, r.g12, r.g22, chrom, r.freq, j, r.g12, wsl, stride);
    const double l22 = d_es_lk<3>(A, f, r.pl, s_lk, r.g11, r.g12, r.g22, chrom, r.freq, j, r.g22, wsl, stride);
    d_store_post(out, l11 + l12 + l22, l11, l12, l22);
  });
}
