/*
 * polymutt_engine.h -- C ABI of the MI355X-native polyMutt per-site family-likelihood engine.
 *
 * The reference (genome-vendor/polymutt v0.13) has no plugin/FFI boundary; its hot path is the C++
 * class surface FamilyLikelihoodSeq (-> NucFamGenotypeLikelihood -> ScalarMinimizer) driven once per
 * site by the OpenMP site loop of src/main.cpp:325-594.  This header is the drop-in replacement for
 * that loop body: the host driver (polymutt_amd/host, or any FFI caller) packs a batch of sites into a
 * dense block and one call evaluates, per site, everything main.cpp:327-589 computes:
 *
 *   CalcReadStats + depth/PS/MQ filters ........ src/NucFamGenotypeLikelihood.cpp:520-546, main.cpp:343-348
 *   MonomorphismLogLikelihood(_denovo) ......... NucFamGenotypeLikelihood.cpp:502-517, FamilyLikelihoodSeq.cpp:68-72
 *   PolymorphismLogLikelihood x3 (+x3) ......... FamilyLikelihoodSeq.cpp:91-104 -> OptimizeFrequency
 *                                                 NucFamGenotypeLikelihood.cpp:432-444 -> Brent core/MathGold.cpp:81-177
 *   CalcVarPosterior(4 | 7) .................... NucFamGenotypeLikelihood.cpp:1693-1749
 *   allele switch / counters / de-novo LR ...... main.cpp:539-574
 *   CalcPostProb (genotype posteriors, GQ, DS) . FamilyLikelihoodSeq.cpp:74-89, NucFamGenotypeLikelihood.cpp:590-868
 *   CalculateAB ................................ NucFamGenotypeLikelihood.cpp:1006-1039
 *
 * VCF text formatting (OutputVCF, NucFamGenotypeLikelihood.cpp:1751-1915) stays on the host.
 *
 * Conventions: plain C types, caller-owned buffers, no global state except the thread-local last-error
 * string.  Every entry point returns 0 on success and a negative pm_status on failure; the message is
 * available from pm_last_error().  All computation is FP64 on the GPU; there is no CPU fallback -- a
 * missing/failed HIP device makes pm_engine_create fail loudly.
 */
#ifndef POLYMUTT_ENGINE_H
#define POLYMUTT_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_ABI_VERSION 8   /* 8: per-family de novo evidence (pm_engine_set_denovo_families / pm_engine_denovo_families);
                               7: pm_engine_stuck_site, partial batches on PM_EBRENT; 6: pm_engine_run_vcf; 5: submit / collect */
#define PM_NCFG 7           /* varllk slots: 0 mono, 1 ref/ts, 2 ref/tv1, 3 ref/tv2, 4 ts/tv1, 5 ts/tv2, 6 tv1/tv2 */

typedef enum { PM_OK = 0, PM_EINVAL = -1, PM_EHIP = -2, PM_ENOMEM = -3, PM_EBRENT = -4, PM_EPED = -5 } pm_status;

/* chromosome class of the current GLF section (main.cpp:312-315) */
typedef enum { PM_CHR_AUTO = 0, PM_CHR_X = 1, PM_CHR_Y = 2, PM_CHR_MT = 3 } pm_chrom;

/* How FamilyLikelihoodSeq::CalcAllFamLogLikelihood treats a family (FamilyLikelihoodSeq.cpp:228-234):
 * all-founder families -> product of single-person likelihoods (NucFamGenotypeLikelihood.cpp:943-949),
 * isNuclear() families -> closed form over 9 parental genotype pairs (:1041-1084),
 * everything else       -> Elston-Stewart peeling (FamilyLikelihoodES.cpp:1013-1057). */
typedef enum { PM_FAM_NUCLEAR = 0, PM_FAM_FOUNDERS = 1, PM_FAM_EXTENDED = 2 } pm_fam_kind;

/* One Elston-Stewart peeling step (ES_Peeling::from/to/peelingType, FamilyLikelihoodES.h:29-31).
 * Indices are family-local positions in Family::path (founders first). */
typedef struct {
  int32_t type;           /* 1 offspring->parents, 2 spouse->spouse, 3 parents->only offspring */
  int32_t from0, from1;   /* from1 = -1 unless type 3 (father, mother)            */
  int32_t to0, to1;       /* to1   = -1 unless type 1 (father, mother)            */
} pm_peel_step;

/* Flattened pedigree.  Persons are numbered in VCF column order: families in Pedigree order, members
 * in Family::path order (core/PedigreeFamily.cpp:11-85) -- i.e. exactly pedGLF->glf[i][j]. */
typedef struct {
  int32_t n_fam;
  int32_t n_person;
  const int32_t *fam_start;    /* [n_fam+1] first person of each family                         */
  const int32_t *fam_founders; /* [n_fam]  Family::founders                                      */
  const int32_t *fam_kind;     /* [n_fam]  pm_fam_kind                                           */
  const int8_t  *sex;          /* [n_person] 0 unknown, 1 male, 2 female (PedigreeGLF::sexes)    */
  const int8_t  *is_founder;   /* [n_person] Person::isFounder()                                 */
  const int32_t *father;       /* [n_person] person index of the father, -1 for founders          */
  const int32_t *mother;       /* [n_person] person index of the mother, -1 for founders          */
  const int32_t *peel_start;   /* [n_fam+1] offsets into steps (empty range for founders-only)    */
  const pm_peel_step *steps;   /* ES_Peeling::BuildPeelingOrder output for every family with
                                  offspring (FamilyLikelihoodSeq.cpp:14-35); nuclear families need
                                  theirs only in vcf_mode (chrX/Y/MT or a single family)          */
  int32_t n_founders;          /* PedigreeGLF::nFounders   (sum of Family::founders)             */
  int32_t male_founders;       /* PedigreeGLF::maleFounders                                      */
  int32_t female_founders;     /* PedigreeGLF::femaleFounders                                    */
} pm_pedigree;

/* Command-line parameters that reach the model (CmdLinePar, src/CmdLinePar.h; defaults main.cpp:59-85). */
typedef struct {
  double  theta;               /* --theta 1e-3 */
  double  poly_tstv;           /* --poly_tstv 2 */
  double  precision;           /* --prec 1e-4 (Brent tol) */
  double  posterior;           /* -c 0.5 */
  int32_t min_total_depth;     /* --minDepth */
  int32_t max_total_depth;     /* --maxDepth (0 = off) */
  double  min_ps;              /* --minPercSampleWithData */
  int32_t min_map_quality;     /* --minMapQuality */
  int32_t denovo;              /* --denovo */
  double  denovo_mut_rate;     /* --rate_denovo 1.5e-8 */
  double  denovo_tstv;         /* --tstv_denovo 2 */
  double  denovo_min_llr;      /* --minLLR_denovo 0.01 */
  int32_t force_call;          /* set by --pos */
  int32_t all_sites;           /* --all_sites */
  int32_t quick_call;          /* --quick_call */
  int32_t numerics;            /* pm_numerics: how the engine evaluates the Brent objective */
  int32_t vcf_mode;            /* --in_vcf: FamilyLikelihoodSeq_VCF semantics (PedVCF.cpp:43-164) -- one (ref, alt)
                                  Brent per site, ref[i] = refAllele | altAllele << 4, PL->lk table pow(10,-i/10),
                                  no filters; res.varllk[0] = mono, varllk[1] = poly (no priors), af = minimiser */
} pm_params;

/* Diagnostic environment variables (tests and tools only; results never depend on them beyond the documented
 * bit-identical alternatives).  The engine reads every one of its switches once, at pm_engine_create, and keeps the
 * values for the engine's life (EngineSwitches in polymutt_amd/csrc/brent_plan.h lists them all; INTEGRATION.md
 * describes them); setting or clearing one afterwards does not affect a live engine.  Among them:
 *   PM_NO_PREFETCH=1  the lean kernels hoist from direct HBM loads instead of LDS-staged PL bytes (tests
 *                     compare the two paths bit for bit);
 *   PM_BRENT_TS=T,S   force the Brent lane plan to T threads x S slots when it holds the pedigree (silently ignored
 *                     when it does not: check pm_engine_plan).  tools/brent_sweep.py sweeps geometries with it, and
 *                     tests/test_gpu_brent_variants.py launches every k_brent instantiation through it and compares
 *                     each with the oracle; 31 instantiations are reached by no other means. */

/* Objective-evaluation numerics.  All three compute CalcAllFamLogLikelihood; they differ in rounding only.
 *   PM_NUM_PRODUCT: each family's likelihood exactly as the reference forms it (same operations, same order),
 *                   families combined as a normalised product, one log10 per evaluation;
 *   PM_NUM_EXACT:   one log10 per family, summed (the reference's form; ~2x slower);
 *   PM_NUM_POLY:    (default) nuclear families as a 4-FMA Horner quartic in min(f,1-f)/max(f,1-f) on the lean
 *                   autosomal kernel (>1 family); every other kernel flavour uses PRODUCT.  Objective values
 *                   differ from the reference by ~1e-14 relative, so on objectives flat to rounding noise Brent
 *                   may stop at another point of equal likelihood (never visible in the VCF). */
typedef enum { PM_NUM_PRODUCT = 0, PM_NUM_EXACT = 1, PM_NUM_POLY = 2 } pm_numerics;

/* Site status codes (which `continue` of main.cpp:300-594 was taken). */
typedef enum {
  PM_SITE_CALLED = 0,          /* evaluated; see emit */
  PM_SITE_MIN_DEPTH = 1, PM_SITE_MAX_DEPTH = 2, PM_SITE_MIN_PS = 3, PM_SITE_MIN_MAPQ = 4,
  PM_SITE_BAD_REF = 5,         /* refBase not in 1..4 (main.cpp:340) */
  PM_SITE_QUICK_SKIP = 7       /* rejected by the --quick_call pre-filter (main.cpp:432-433) */
} pm_site_status;

/* Genotype-label flavour of a person in an emitted record (the four labellers of
 * NucFamGenotypeLikelihood.cpp:1573-1608 plus the chrY-female "."). */
typedef enum { PM_LBL_VCF_DIPLOID = 0, PM_LBL_VCF_HAPLOID = 1, PM_LBL_ALLELES = 2, PM_LBL_GENO10 = 3, PM_LBL_DOT = 4 } pm_label_kind;

/* Per-site result (240 bytes, naturally aligned, no implicit padding). */
typedef struct {
  int32_t status;              /* pm_site_status */
  int32_t n_cfg;               /* 4 or 7 configurations evaluated */
  int32_t maxidx;              /* CalcVarPosterior argmax */
  int32_t emit;                /* 1: a VCF record is written; 2: OutputVCF_denovo called but record suppressed */
  int32_t total_depth;
  int32_t num_samp_with_data;
  double  avg_map_qual;
  double  perc_samp_with_data;
  double  var_post_prob;
  double  poly_qual;
  double  varllk[PM_NCFG];
  double  varfreq[PM_NCFG];    /* Brent minimiser per configuration (1.0 for mono) */
  double  af;                  /* GetMinimizer() printed as AF */
  double  ab;                  /* CalculateAB */
  double  denovo_lr;           /* DQ */
  int32_t evals[PM_NCFG];      /* objective evaluations per configuration */
  int32_t allele1, allele2;    /* famlk[0] alleles at output time (1..4) */
  int32_t is_mono;             /* famlk[0].isMono for the record (BA= tag) */
  int32_t denovo_mono;         /* OutputVCF_denovo prints ALT=allele1 */
  int32_t call_row;            /* row of pm_geno_call output for this site, -1 if none */
} pm_site_result;

/* Per-person genotype call of an emitted record (16 bytes). */
typedef struct {
  double  dosage;              /* DS */
  int16_t best;                /* bestGenoIdx (0..2, or 0..9 for de-novo kids) */
  int16_t gq;                  /* GQ */
  int8_t  label;               /* pm_label_kind */
  int8_t  _pad[3];
} pm_geno_call;

/* vcf_mode genotype row entry (FamilyLikelihoodSeq_VCF::OutputVCF prints GT/GQ only): the device rows of a
 * vcf_mode engine (pm_engine_run_device's d_calls) use this 4-byte layout; pm_engine_run expands them into
 * pm_geno_call rows with dosage 0. */
typedef struct {
  int8_t best;
  int8_t gq;
  int8_t label;                /* pm_label_kind */
  int8_t pad;
} pm_vcf_call;

/* Summary counters of one section (main.cpp:264-282, printed :596-619); summed over shards/GPUs. */
typedef struct {
  int64_t ref_base_counts[5];
  int64_t min_total_depth_filter, max_total_depth_filter, min_ps_filter, min_map_qual_filter;
  int64_t homo_ref, transitions, transversions, tstvs1, tstvs2, tvs1tvs2, nocall;
} pm_counters;

typedef struct pm_engine pm_engine;

/* Create an engine on HIP device `device` (one engine per GPU; engines are independent and thread-safe
 * with respect to each other).  max_batch bounds the sites per pm_engine_run call. */
int pm_engine_create(const pm_pedigree *ped, const pm_params *par, int device, int max_batch, pm_engine **out);
void pm_engine_destroy(pm_engine *eng);

/* The lane plan pm_engine_create chose for the Brent kernel: threads per item (one wave = 64) and
 * family slots per lane.  Diagnostics and tests only (no reference counterpart). */
int pm_engine_plan(pm_engine *eng, int32_t *threads, int32_t *slots);

/* The distinct k_brent instantiations this engine has enqueued since pm_engine_create, in first-launch order: 11
 * int32 each, k_brent's template arguments in order (T, S, NUM, GEN, ES, DN, PF, EP, QD, NF, PD; brent_variants.h).
 * At most `cap` of them are written to keys; *n receives their number even when it exceeds cap.  The fused
 * hoisting + Brent kernel of all-peeled bi-allelic engines is no k_brent instantiation and is not listed.  Host
 * bookkeeping only.  Diagnostics and tests only (no reference counterpart). */
int pm_engine_brent_variants(pm_engine *eng, int32_t *keys, int32_t cap, int32_t *n);

/* famlk[0]'s stale state across sites: whether CalcPostProb has already run earlier in the run (any
 * earlier site reached OutputVCF).  The reference's likelihoodONEKid reads the object's member `sex`
 * (NucFamGenotypeLikelihood.cpp:1193, 1202-1264), which CalcPostProb leaves at the last person's sex; it
 * changes the first family's chrX/Y genotype posteriors.  The engine tracks it itself across
 * pm_engine_run calls; a driver that splits a run over several engines (site shards) sets it at each
 * shard's start.  0 at creation. */
int pm_engine_set_posterior_carry(pm_engine *eng, int32_t seen);

/* Start a GLF section: sets the chromosome class, recomputes the polymorphism prior
 * (GetPolyPrior, NucFamGenotypeLikelihood.cpp:295-304) and zeroes the section counters. */
int pm_engine_begin_section(pm_engine *eng, int32_t chrom);

/* Evaluate n sites.  Inputs are the dense per-site block, persons in pm_pedigree order:
 *   pl  [n][n_person][10]  phred genotype likelihoods AA,AC,AG,AT,CC,CG,CT,GG,GT,TT (0 when absent)
 *   dm  [n][n_person]      depth (bits 0-23) | mapQ << 24   (0 when absent; not read in vcf_mode -- the VCF path has no
 *                          depth -- where it may be NULL)
 *   ref [n]                refBase 1..4 (anything else -> PM_SITE_BAD_REF)
 * inputs_on_device != 0: pl/dm/ref are device pointers on this engine's GPU, else host pointers.
 * Outputs are host pointers: res[n]; calls[n_rows * n_person] receives one row per written record
 * (emit == 1; row index = res[i].call_row, rows numbered in site order, -1 for every other site: a
 * suppressed de novo record, emit == 2, prints nothing and gets no row); *n_rows is set to the row count.
 * Counters accumulate into the section totals.  Synchronous.
 * PM_EBRENT: some site's Brent maximisation hit ITMAX (ScalarMinimizer::Brent's numerror, core/MathGold.cpp:98,175,
 * where the reference's site loop ends the run).  res[] is still written for the whole batch, and the sites before the
 * first stuck one -- pm_engine_stuck_site -- are complete: their genotype rows are the first *n_rows rows (*n_rows
 * counts only their rows), as the reference had written their records (NucFamGenotypeLikelihood.cpp:1829, fflush per
 * record) before exiting at the stuck site.  The section counters then include the whole batch. */
int pm_engine_run(pm_engine *eng, int32_t n, const uint8_t *pl, const uint32_t *dm, const uint8_t *ref,
                  int32_t inputs_on_device, pm_site_result *res, pm_geno_call *calls, int32_t *n_rows);

/* vcf_mode engines only: pm_engine_run on host inputs (no depth plane) with the genotype rows returned in the
 * compact pm_vcf_call form the device writes -- best / GQ / label, all FamilyLikelihoodSeq_VCF::OutputVCF
 * (src/FamilyLikelihoodSeq_VCF.cpp:412-521) prints -- instead of widened into pm_geno_call rows: a quarter of
 * the bytes, copied straight into `calls` (one synchronous device-to-host copy; page-locked `calls` from
 * pm_host_alloc copy at full PCIe rate).  Replaces, for the --in_vcf path, the per-record
 * FamilyLikelihoodSeq_VCF::FillPenetrance -> CalcLikelihood -> OutputVCF calls of PedVCF::VarCallFromVCF
 * (src/PedVCF.cpp:103-160).  PM_EINVAL on an engine created without vcf_mode, or while a pm_engine_submit batch
 * has not been collected (that batch stays pending).  PM_EBRENT as for pm_engine_run. */
int pm_engine_run_vcf(pm_engine *eng, int32_t n, const uint8_t *pl, const uint8_t *ref, pm_site_result *res,
                      pm_vcf_call *calls, int32_t *n_rows);

/* pm_engine_run split in two, so a driver keeps several batches in flight (one per engine; each engine has its
 * own HIP stream): pm_engine_submit queues the batch's host-to-device copies (asynchronous when pl/dm/ref are
 * page-locked, pm_host_alloc), the pipeline and the copy-back of the per-site results on the engine's stream and
 * returns; pm_engine_collect waits for that batch and writes res[n], the genotype rows and *n_rows exactly as
 * pm_engine_run does.  One batch per engine between the two calls.  The input buffers must stay untouched until
 * the collect.  (The reference's site loop body, main.cpp:327-589, per batch; no reference counterpart for the
 * asynchrony itself.) */
int pm_engine_submit(pm_engine *eng, int32_t n, const uint8_t *pl, const uint32_t *dm, const uint8_t *ref);
int pm_engine_collect(pm_engine *eng, pm_site_result *res, pm_geno_call *calls, int32_t *n_rows);

/* After a batch returned PM_EBRENT (pm_engine_run, _run_vcf, _collect or _sync): *site = the batch index of the first
 * site whose Brent hit ITMAX, i.e. the number of leading sites whose results and rows are complete; -1 when the last
 * finished batch had none.  (core/MathGold.cpp:98,175: the reference exits at that site, its earlier records
 * written.)  The environment variable PM_TEST_ITMAX, read at pm_engine_create, lowers ITMAX (200) for tests. */
int pm_engine_stuck_site(pm_engine *eng, int32_t *site);

/* Per-family de novo evidence (--denovo engines, not vcf_mode; no reference counterpart: v0.13 prints only the
 * site-level DQ).  pm_site_result.denovo_lr is a sum over families: for every written record (emit == 1) and family f
 *   maxidx >= 1:  D_f = log10 L_f^dn(allele1, allele2; varfreq[maxidx]) - log10 L_f^std(allele1, allele2; x_std),
 *                 x_std = the minimiser of the no-mutation re-optimisation (main.cpp:567-573);
 *   maxidx == 0:  D_f = log10 L_f^dn(ref, ref == 4 ? 3 : ref + 1; 1.0) - Sum_{persons of f} (-PL[homoRef] / 10)
 *                 (MonomorphismLogLikelihood_denovo - MonomorphismLogLikelihood, main.cpp:458, :557-565),
 * L_f being the family's term of CalcAllFamLogLikelihood in the reference's operation order, so Sum_f D_f = denovo_lr
 * up to summation rounding.  One extra kernel per batch (k_fam_dnlr) over the written rows only; results are
 * deterministic (fixed reduction trees, no floating-point atomics). */
typedef struct { int32_t fam; int32_t pad; double lr; } pm_fam_lr;   /* 16 bytes; fam = family index in pm_pedigree order */

/* top_k = 0 switches the feature off (the default: nothing is allocated or launched, every output is bit-identical);
 * 1..8 keeps, per written record, the top_k families ranked by D_f descending, ties by lower family index.
 * want_all != 0 also keeps the full [max_batch][n_fam] matrix on the device (PM_EINVAL above 1 GiB).
 * PM_EINVAL: top_k out of range, an engine without denovo, a vcf_mode engine, or a submitted batch not yet collected. */
int pm_engine_set_denovo_families(pm_engine *eng, int32_t top_k, int32_t want_all);

/* The rows of the last finished batch (after pm_engine_run, pm_engine_collect, or pm_engine_run_device + pm_engine_sync),
 * indexed by pm_site_result.call_row: top[n_rows][top_k] (entries past n_fam are {fam = -1, lr = 0}), sum[n_rows]
 * (Sum_f D_f; may be NULL) and all[n_rows][n_fam] (D_f by family; may be NULL, PM_EINVAL when asked for without
 * want_all).  After PM_EBRENT only the rows before the stuck site are valid, as for the genotype rows. */
int pm_engine_denovo_families(pm_engine *eng, pm_fam_lr *top, double *sum, double *all);

/* *n_rows = the rows pm_engine_denovo_families and pm_engine_denovo_carriers write (0 with both features off): the
 * row count the last pm_engine_run / pm_engine_collect returned (after PM_EBRENT: the rows before the stuck site), or
 * after pm_engine_run_device + pm_engine_sync the batch's written records (the results with call_row >= 0). */
int pm_engine_denovo_rows(pm_engine *eng, int32_t *n_rows);

/* Per-person de novo posteriors (--denovo engines, not vcf_mode; additive to ABI 8: callers detect the feature by
 * these symbols).  For every written record (emit == 1) and every non-founder c with father fa and mother mo, in the
 * alleles and frequency of pm_engine_denovo_families' numerator (maxidx >= 1: allele1, allele2 at varfreq[maxidx];
 * maxidx == 0: ref, ref == 4 ? 3 : ref + 1 at 1.0), with L_f the de novo-model likelihood of c's family (a sum over
 * the joint genotypes of its members) and J_c(a, b, S) the same sum restricted to G_fa = a, G_mo = b, G_c in S:
 *   pp    = Sum_{a,b} J_c(a, b, NonMend(a, b)) / L_f, NonMend(a, b) = the genotypes that cannot take one allele from a
 *           and one from b (the autosomal rule on every chromosome class, as the de novo model's transmission);
 *   event = (fa_g, mo_g) maximising J_c(a, b, NonMend(a, b)) (ties: the first pair in (a, b) order), then kid_g
 *           maximising J_c(fa_g, mo_g, {g}) over NonMend(fa_g, mo_g) (ties: the lowest g); (-1, -1, -1) when every
 *           term is 0.
 * Genotypes are indices 0..9 in GLF order (AA, AC, AG, AT, CC, CG, CT, GG, GT, TT).  One extra kernel per batch
 * (k_person_dn) over the written rows only; results are deterministic (fixed reduction trees, no atomics). */
typedef struct { int32_t person; int8_t fa_g, mo_g, kid_g, pad; double pp; } pm_person_dn;   /* 16 bytes; person = index in pm_pedigree order */

/* top_k = 0 switches the feature off (the default: nothing is allocated or launched, every output is bit-identical);
 * 1..8 keeps, per written record, the top_k non-founders ranked by pp descending, ties by lower person index.
 * want_all != 0 also keeps the full [max_batch][n_person] matrix on the device (PM_EINVAL above 1 GiB).
 * PM_EINVAL: top_k out of range, an engine without denovo, a vcf_mode engine, or a submitted batch not yet collected.
 * Independent of pm_engine_set_denovo_families: either, both or neither may be on. */
int pm_engine_set_denovo_carriers(pm_engine *eng, int32_t top_k, int32_t want_all);

/* The rows of the last finished batch, indexed by pm_site_result.call_row (pm_engine_denovo_rows tells how many, with
 * either feature on): top[n_rows][top_k] (entries past the non-founder count are {-1, -1, -1, -1, 0, 0.0}) and
 * all[n_rows][n_person] (person = p; founders have genotypes -1 and pp 0; may be NULL, PM_EINVAL when asked for
 * without want_all).  After PM_EBRENT only the rows before the stuck site are valid. */
int pm_engine_denovo_carriers(pm_engine *eng, pm_person_dn *top, pm_person_dn *all);

/* De novo calling from VCF input (vcf_mode engines; additive to ABI 8: callers detect the feature by this symbol; no
 * reference counterpart -- PedVCF::VarCallFromVCF never calls its _denovo members).  A vcf_mode block carries data in the
 * three genotypes of (ref, alt) only, so the de novo model collapses to three states.  For a called site of an autosomal
 * section with alleles (a1, a2) = (ref, alt):
 *   g            = (g11, g12, g22), the GLF genotype indices of a1a1, a1a2, a2a2;
 *   M3[x][y]     = M[g[x]][g[y]], M the 10 x 10 genotype mutation matrix (GenotypeMutationModel::SetGenoMutMatrix) of
 *                  pm_params.denovo_mut_rate / denovo_tstv;
 *   T            = the autosomal bi-allelic transmission (SetTransmissionMatrix_BA);
 *   Tdn[i][j][k] = Sum_m T[i][j][m] M3[m][k].
 * L^dn(f) is the vcf_mode objective (FamilyLikelihoodSeq_VCF::CalcAllFamLogLikelihood, Hardy-Weinberg founder priors in f
 * everywhere) with the families routed as for varllk[1] -- all-founder families the product of single persons; nuclear
 * families in closed form when n_fam > 1; everything else, a single nuclear family included, by the bi-allelic peel --
 * and these differences:
 *   closed form: each child's factor for the parental pair (i, j) is Sum_k Tdn[i][j][k] l_k (likelihoodONEKid_denovo applied
 *                to D = M3 l);
 *   peel:        type-1 steps (offspring -> parents) use Tdn; type-3 steps (parents -> only offspring) use Tdn when the
 *                couple has no marriage partial yet and plain T when it has one (the reference's 10-state quirk,
 *                FamilyLikelihoodES.cpp:1391, kept so that the 10-state oracle pins the values); type-2 steps are unchanged.
 * Outputs per called site: N = max_f log10 L^dn(f) by the same OptimizeFrequency + Brent as every other item, D =
 * the standard maximum varllk[1], DQ = N - D:  denovo_lr = DQ, varllk[2] = N, varfreq[2] = its maximiser, evals[2] = its
 * evaluation count.  (The D subtracted is the standard objective at varfreq[1] formed by the de novo kernel with the
 * log10 it uses for N: varllk[1] up to the rounding of its log10, ~1e-16 absolute, which matters only where both
 * likelihoods are within 1e-7 of 1.)
 * n_cfg, maxidx, every other field and the genotype rows are those of the feature-off run, byte for byte.  Only the three
 * planes g11, g12, g22 of the block are read.  A de novo Brent that hits ITMAX is a stuck site like the standard one:
 * PM_EBRENT, pm_engine_stuck_site = the first site at which either stuck.
 * Not in the model: chrY/MT sections, and chrX sections unless pm_engine_set_vcf_denovo_chrx below is on (the autosomal
 * transmission is wrong there: no DQ is computed, the results are those of the feature-off run); indel records (the engine cannot tell them from SNVs: the host prints no tag for them);
 * the fixed single-trio prior of the GLF path (it gives two homozygous-reference parents weight 0, hiding exactly the
 * event looked for).
 * on = 0 (the default): nothing is allocated or launched, every output byte is that of an engine without the feature.
 * PM_EINVAL: an engine without vcf_mode, or a submitted batch not yet collected.  pm_engine_set_denovo_families and
 * pm_engine_set_denovo_carriers keep refusing vcf_mode engines. */
int pm_engine_set_vcf_denovo(pm_engine *eng, int32_t on);

/* De novo calling on the chrX sections of a pm_engine_set_vcf_denovo engine: a sex-aware three-state model (additive to
 * ABI 8: callers detect the feature by this symbol; no reference counterpart).  It takes effect on batches run while the
 * current section is PM_CHR_X.  Alleles (a1, a2) = (ref, alt); states s = 0, 1, 2 = a1a1, a1a2, a2a2 with GLF indices
 * g = (g11, g12, g22).  A male uses states 0 and 2 only, as hemizygous a1 and a2; sex 0 (unknown) is treated as female, as
 * the standard chrX model does.
 *   M3[x][y]       = M[g[x]][g[y]], M the 10 x 10 genotype mutation matrix above;
 *   A4             = the 4 x 4 allele mutation matrix M is built from (GenotypeMutationModel: diagonal 1 - mu, a transition
 *                    mu r / (1 + r), each transversion mu 0.5 / (1 + r); mu = denovo_mut_rate, r = denovo_tstv);
 *   H3             = the haploid mutation matrix on the three states: H3[0][0] = A4[a1][a1], H3[0][2] = A4[a1][a2],
 *                    H3[2][0] = A4[a2][a1], H3[2][2] = A4[a2][a2], row 1 and column 1 zero;
 *   T_F, T_M       = the chrX bi-allelic transmissions to a daughter and to a son (SetTransmissionMatrix_BA_CHRX_2Female,
 *                    _2Male), [father][mother][child];
 *   Tdn_F[i][j][k] = Sum_m T_F[i][j][m] M3[m][k],   Tdn_M[i][j][k] = Sum_m T_M[i][j][m] H3[m][k].
 * Founder priors in the frequency f: a male (f, 0, 1 - f), everyone else (f^2, 2 f (1 - f), (1 - f)^2) -- those of the
 * standard chrX objective.
 * L^dn_X(f) routes the families as vcf_mode does on chrX: a founders-only family is the product of its persons (a male
 * f l11 + (1 - f) l22, everyone else the Hardy-Weinberg quadratic); every family with offspring, nuclear ones included,
 * goes through the bi-allelic peel (there is no closed form on X).  Type-1 steps use Tdn of the child's sex; type-3 steps
 * use Tdn of the child's sex without a marriage partial and plain T of the child's sex with one (the
 * FamilyLikelihoodES.cpp:1391 quirk the autosomal feature keeps); type-2 steps are unchanged.
 * Outputs per called site of a chrX section, in the autosomal feature's fields: varllk[2] = N = max_f log10 L^dn_X(f) by
 * the same OptimizeFrequency + Brent, varfreq[2] its maximiser, evals[2] its evaluation count, denovo_lr = N - D with D
 * the standard chrX objective (M3 = H3 = identity, plain T) evaluated once at varfreq[1] by the same kernel with the same
 * log10.  Every other result field and the genotype rows are those of the feature-off run, byte for byte; only the three
 * planes g11, g12, g22 are read.  A de novo Brent that hits ITMAX is a stuck site like any other.  FP64, a fixed
 * reduction order and no floating-point atomics: the same input gives the same bytes.
 * Not in the model: chrY and MT sections (no DQ, as before); pseudo-autosomal regions (ignored, as in the standard chrX
 * model); the per-family and per-child detail, which stays autosomal only by default -- pm_engine_vcf_denovo_rows keeps
 * returning 0 rows on chrX sections unless pm_engine_set_vcf_denovo_chrx_detail below is on.
 * on = 0 (the default): nothing is allocated or launched, every output byte is that of an engine without the feature.
 * It may be set at any point between batches.  PM_EINVAL: an engine without vcf_mode, pm_engine_set_vcf_denovo not on, or a
 * submitted batch not yet collected.  pm_engine_set_vcf_denovo(eng, 0) switches this off too (and so does a repeated
 * pm_engine_set_vcf_denovo(eng, 1), which rebuilds that feature: set this switch after it). */
int pm_engine_set_vcf_denovo_chrx(pm_engine *eng, int32_t on);

/* The families and the children behind each DQ of pm_engine_set_vcf_denovo (vcf_mode engines; additive to ABI 8: callers
 * detect the feature by these symbols; no reference counterpart).  A row is a called site (status == 0) of an autosomal
 * section with evals[2] > 0 and denovo_lr >= pm_params.denovo_min_llr; rows are numbered in ascending site order within
 * the batch.  Everything is in the three states g = (g11, g12, g22) and the tables M3, T, Tdn above, the families routed
 * and the founders given Hardy-Weinberg priors as for N.
 *   Per family f:  D_f = log10 L_f^dn(x_N) - log10 L_f^std(x_D), x_N = varfreq[2], x_D = varfreq[1].  L_f^dn is the
 *     family's factor of the de novo objective (a peeled family by the peel with Tdn, the FamilyLikelihoodES.cpp:1391
 *     quirk included; a nuclear family by the closed form on D = M3 l; a founders-only family the product of its persons);
 *     L_f^std is the same code with M3 = identity and plain T.  Sum_f D_f = denovo_lr up to summation rounding.  Each
 *     log10 is taken of the whole double, so a family without data gives about -2e-8.
 *   Per non-founder c (father fa, mother mo), at x_N in the de novo model:
 *     pp    = Sum_{a,b in the 3 states} J_c(a, b, NonMend3(a, b)) / L_f^dn, J_c(a, b, S) = L_f^dn restricted to G_fa = a,
 *             G_mo = b, G_c in S, NonMend3(a, b) = the states among the three that cannot take one allele from each
 *             parent (empty for 12 x 12);
 *     event = the pair (a, b) of the largest term, then the state of NonMend3(a, b) with the largest J_c(a, b, {s}); ties
 *             go to the first in state order (a1a1, a1a2, a2a2); (-1, -1, -1) when every term is 0.
 *     Genotypes are reported as GLF indices 0..9 (the values g[s]) in pm_person_dn; founders get (-1, -1, -1) and 0.0.  A
 *     child reached only through a type-3 step with a marriage partial has pp = 0 (plain T there: the reference's model).
 * Rankings: pm_fam_lr by D_f descending, ties by lower family index; persons by pp descending, ties by lower person
 * index; padding entries as in the GLF features.  One block per row at a time (k_vdn_rows + k_vdn_who after the de novo
 * item); fixed reduction trees and no floating-point atomics, so the same input gives the same bytes.  The site results
 * and the genotype rows are those of pm_engine_set_vcf_denovo alone, byte for byte.
 *
 * fam_k, car_k: 0 (that half off) or 1..8 entries kept per row; both 0 switches the feature off and frees its buffers
 * (the default: nothing is allocated or launched).  want_all != 0 also keeps the full [max_batch][n_fam] and
 * [max_batch][n_person] matrices of the halves that are on (PM_EINVAL above 1 GiB each).
 * PM_EINVAL: an engine without vcf_mode, pm_engine_set_vcf_denovo not on, k out of range, or a submitted batch not yet
 * collected.  pm_engine_set_vcf_denovo(eng, 0) also switches this off.  pm_engine_set_denovo_families and
 * pm_engine_set_denovo_carriers still refuse vcf_mode engines. */
int pm_engine_set_vcf_denovo_detail(pm_engine *eng, int32_t fam_k, int32_t car_k, int32_t want_all);

/* The rows of the last finished batch (after pm_engine_run, _run_vcf, _collect, or _run_device + _sync): *n_rows, and
 * their batch indices in site[n_rows] (may be NULL).  0 rows with the feature off and on chrX/Y/MT sections (on chrX:
 * unless pm_engine_set_vcf_denovo_chrx_detail is on).  After
 * PM_EBRENT only the rows before the stuck site are counted and valid.  Like the two readers below, PM_EINVAL while a
 * submitted batch has not been collected. */
int pm_engine_vcf_denovo_rows(pm_engine *eng, int32_t *n_rows, int32_t *site);

/* top[n_rows][fam_k] (entries past n_fam are {fam = -1, lr = 0}), sum[n_rows] (Sum_f D_f; may be NULL) and
 * all[n_rows][n_fam] (may be NULL; PM_EINVAL when asked for without want_all).  PM_EINVAL with fam_k == 0. */
int pm_engine_vcf_denovo_families(pm_engine *eng, pm_fam_lr *top, double *sum, double *all);

/* top[n_rows][car_k] (entries past the non-founder count are {-1, -1, -1, -1, 0, 0.0}) and all[n_rows][n_person]
 * (person = p; may be NULL; PM_EINVAL when asked for without want_all).  PM_EINVAL with car_k == 0. */
int pm_engine_vcf_denovo_carriers(pm_engine *eng, pm_person_dn *top, pm_person_dn *all);

/* The families and the children behind each DQ of a chrX section: pm_engine_set_vcf_denovo_detail's outputs in the
 * sex-aware model of pm_engine_set_vcf_denovo_chrx (additive to ABI 8: callers detect the feature by this symbol; no
 * reference counterpart).  An opt-in of its own: with pm_engine_set_vcf_denovo_chrx and pm_engine_set_vcf_denovo_detail
 * both on and this switch off, chrX sections keep giving 0 rows.  Everything is in the three states and the four tables
 * T_F, T_M, Tdn_F = T_F M3, Tdn_M = T_M H3 of pm_engine_set_vcf_denovo_chrx, with its founder priors ((f, 0, 1 - f) for a
 * male, Hardy-Weinberg for everyone else) and its routing (every family with offspring is peeled).  x_N = varfreq[2],
 * x_D = varfreq[1].
 *   Rows: the called sites (status == 0) of a PM_CHR_X section with evals[2] > 0 and denovo_lr >= pm_params.denovo_min_llr,
 *     in ascending site order within the batch.
 *   Per family f:  D_f = log10 L_f^dn(x_N) - log10 L_f^std(x_D), L_f the family's factor of the chrX de novo objective and
 *     of the standard chrX objective: a family with offspring by the peel (Tdn of the child's sex at x_N, the
 *     FamilyLikelihoodES.cpp:1391 quirk included; plain T of the child's sex everywhere at x_D); a founders-only family
 *     the product of its persons in person order, a male l11 x + l22 (1 - x), everyone else the Hardy-Weinberg quadratic.
 *     Each log10 is taken of the whole double.  Sum_f D_f = denovo_lr up to summation rounding.
 *   Per non-founder c with both parents in its family (father fa, mother mo), at x_N in the de novo model:
 *     pp    = Sum_{a in {0, 2}, b in {0, 1, 2}} J_c(a, b, NonMendX(a, b, sex_c)) / L_f^dn, capped at 1, the sum in (a, b)
 *             order.  J_c(a, b, S) = L_f^dn restricted to G_fa = a, G_mo = b, G_c in S.  NonMendX(a, b, sex) = the states s
 *             allowed for that sex -- 0, 1, 2 for a daughter or a child of unknown sex, 0 and 2 for a son -- with
 *             T_sex[a][b][s] = 0.  A father has no state 1: those three pairs contribute exactly 0.  A son of a
 *             heterozygous mother has an empty set: that pair contributes 0 too.
 *     event = the pair (a, b) of the largest term, then the state of its set with the largest J_c(a, b, {s}); ties go to
 *             the first pair in (a, b) order, then to the first state; (-1, -1, -1) when every term is 0.
 *     Genotypes are reported as the GLF indices g[s] in pm_person_dn: a hemizygous male's state 0 or 2 is reported as g11
 *     or g22.  Founders get (-1, -1, -1) and 0.0.  A child reached only through a type-3 step with a marriage partial
 *     has pp = 0 (plain T there), as on autosomes.
 * Rankings, padding entries and determinism are those of pm_engine_set_vcf_denovo_detail (k_vdn_rows as it is, then
 * k_vdn_who_x, one block per row at a time; fixed reduction trees, no floating-point atomics: the same input gives the
 * same bytes).  The outputs go to that feature's buffers with its fam_k, car_k and want_all, so pm_engine_vcf_denovo_rows,
 * _families and _carriers read them unchanged.  The site results and the genotype rows of chrX sections are those of
 * pm_engine_set_vcf_denovo_chrx alone, byte for byte; autosomal sections, chrY and MT are untouched.
 * on = 0 (the default) frees what this switch allocated: nothing is allocated or launched.
 * PM_EINVAL: an engine without vcf_mode, a submitted batch not yet collected, pm_engine_set_vcf_denovo_chrx not on, or
 * pm_engine_set_vcf_denovo_detail off (fam_k = car_k = 0).  Any later call of pm_engine_set_vcf_denovo,
 * pm_engine_set_vcf_denovo_chrx or pm_engine_set_vcf_denovo_detail switches this off, because each rebuilds what it rests
 * on: set this switch last. */
int pm_engine_set_vcf_denovo_chrx_detail(pm_engine *eng, int32_t on);

/* Genotype posteriors of every person of every written record of a vcf_mode batch (additive to ABI 8: callers detect
 * the feature by this symbol; FamilyLikelihoodSeq_VCF::OutputVCF prints GT and GQ only, so there is no reference
 * counterpart for the output, only for the values).  One row entry is the vector post[] from which the engine takes
 * a person's best genotype and GQ -- P(g11), P(g12), P(g22) given the whole pedigree at the site's frequency
 * (pm_site_result.af), with the founder priors and the single-family prior mode of the genotype rows -- each value
 * rounded once from double to float.  The chromosome class keeps its rules: hemizygous persons (chrX / chrY males,
 * everyone on MT) have p[1] = 0, chrY females are all zero, and a person whose normalising sum is zero is all zero.
 * DS = p[1] + 2 p[2]. */
typedef struct {
  float p[3];                  /* P(g11), P(g12), P(g22) given the pedigree */
} pm_vcf_post;

/* Switch the posterior plane on or off (off at creation).  With it on, every batch runs one extra pass after the
 * standard posterior stage (k_vcf_post_lean / k_vcf_post_nuc / k_vcf_post_es, chosen as that stage's kernels are),
 * which writes only the plane: the site results and the genotype rows are those of the engine without it, byte for
 * byte.  The device buffer is max_batch x n_person x 12 bytes, allocated on the first `on` and freed on `off` or
 * pm_engine_destroy; off = nothing allocated, nothing launched.  Independent of the pm_engine_set_vcf_denovo family:
 * either may be on without the other and neither switches the other off.  It may be set at any point between
 * batches.  PM_EINVAL: an engine without vcf_mode, or a submitted batch not yet collected. */
int pm_engine_set_vcf_posteriors(pm_engine *eng, int32_t on);

/* The plane of the last finished batch (pm_engine_run, pm_engine_run_vcf or pm_engine_submit / pm_engine_collect):
 * *n_rows = the batch's row count, out[row * n_person + person] with the rows of pm_site_result.call_row and the
 * persons in pm_pedigree order.  out may be NULL (the count alone).  After PM_EBRENT: the same prefix of rows the
 * batch returned.  PM_EINVAL: the feature is off, or a submitted batch has not been collected. */
int pm_engine_vcf_posteriors(pm_engine *eng, int32_t *n_rows, pm_vcf_post *out);

/* Transmission phase of every non-founder of every written record of a vcf_mode batch (additive to ABI 8: callers
 * detect the feature by this symbol; the reference has no counterpart).  With (a1, a2) = (ref, alt) and the states
 * 0, 1, 2 = a1a1, a1a2, a2a2, for a non-founder c whose father and mother are in its family
 *   p12 = P(c got a1 from the father and a2 from the mother | data)
 *       = [J(0,1,1) + J(0,2,1) + J(1,2,1) + J(1,1,1) / 2] / L
 *   p21 = P(c got a2 from the father and a1 from the mother | data)
 *       = [J(1,0,1) + J(2,0,1) + J(2,1,1) + J(1,1,1) / 2] / L
 * where J(a, b, s) is the family likelihood restricted to father = a, mother = b, child = s under the plain transmission
 * and L the unrestricted one, at the site's frequency (pm_site_result.af) with the founder priors, the single-family
 * prior mode and the family routing of the genotype rows and of pm_vcf_post: p12 + p21 is that plane's p[1] up to the
 * order of the sums.  Each value is the double quotient rounded once to float.  Founders, persons whose normalising sum
 * is zero and every person of a chrX / chrY / MT section are (0, 0): sex-aware phase is not computed. */
typedef struct {
  float p12, p21;              /* P(paternal a1 | maternal a2), P(paternal a2 | maternal a1) given the pedigree */
} pm_vcf_phase;

/* Switch the phase plane on or off (off at creation).  With it on, every batch runs one extra pass after the standard
 * posterior stage and the posterior plane's (k_vcf_phase_lean / k_vcf_phase_nuc / k_vcf_phase_es, chosen as that
 * stage's kernels are), which writes only the plane: the site results, the genotype rows, the posterior plane and the
 * de novo outputs are those of the engine without it, byte for byte.  The device buffer is max_batch x n_person x 8
 * bytes, allocated on the first `on` and freed on `off` or pm_engine_destroy; off = nothing allocated, nothing
 * launched.  Independent of pm_engine_set_vcf_posteriors and of the pm_engine_set_vcf_denovo family: either may be on
 * without the other and neither switches the other off.  It may be set at any point between batches.  PM_EINVAL: an
 * engine without vcf_mode, or a submitted batch not yet collected. */
int pm_engine_set_vcf_phase(pm_engine *eng, int32_t on);

/* The plane of the last finished batch (pm_engine_run, pm_engine_run_vcf or pm_engine_submit / pm_engine_collect):
 * *n_rows = the batch's row count, out[row * n_person + person] with the rows of pm_site_result.call_row and the
 * persons in pm_pedigree order.  out may be NULL (the count alone).  After PM_EBRENT: the same prefix of rows the
 * batch returned.  PM_EINVAL: the feature is off, or a submitted batch has not been collected. */
int pm_engine_vcf_phase(pm_engine *eng, int32_t *n_rows, pm_vcf_phase *out);

/* The most probable joint genotype assignment of every family of every written record of a vcf_mode batch (additive to
 * ABI 8: callers detect the feature by this symbol; the reference has no counterpart).  With (a1, a2) = (ref, alt) and
 * the states 0, 1, 2 = a1a1, a1a2, a2a2, an assignment g of a family's members has the joint weight
 *   J(g) = founder priors x the plain transmission T[g_fa][g_mo][g_c] of every non-founder x the members' penetrances
 * at the site's frequency (pm_site_result.af) with the founder priors, the single-family prior mode and the family
 * routing of the genotype rows, of pm_vcf_post and of pm_vcf_phase.  Every member of the family gets
 *   g  = its state in an assignment g* with J(g*) = max J (ties: the first maximum of the kernel's fixed enumeration),
 *   lp = log10(J(g*) / L),  L = the sum of J over all assignments: the same value for every member of the family,
 * formed in double and rounded once to float.  A founders-only family factorises: each person's own best state, lp =
 * the sum of the persons' log10 shares.  The rows' `best` is each person's marginal argmax, and marginal argmaxes need
 * not be Mendelian-consistent; g* always is.  max J = 0 or L = 0: g = 255 and lp = 0 for the whole family, and so for
 * every person of a chrX / chrY / MT section: sex-aware joint calls are not computed.  pad is written as 0. */
typedef struct {
  float lp;                    /* log10 posterior probability of the family's most probable joint assignment */
  uint8_t g;                   /* this person's state in it: 0, 1, 2 = a1a1, a1a2, a2a2; 255 = none */
  uint8_t pad[3];
} pm_vcf_joint;

/* Switch the joint call plane on or off (off at creation).  With it on, every batch runs one extra pass after the
 * phase plane's (k_vcf_joint_lean / k_vcf_joint_nuc / k_vcf_joint_es, chosen as that pass's kernels are), which writes
 * only the plane: the site results, the genotype rows, the posterior plane, the phase plane and the de novo outputs are
 * those of the engine without it, byte for byte.  The device buffer is max_batch x n_person x 8 bytes, allocated on the
 * first `on` and freed on `off` or pm_engine_destroy; off = nothing allocated, nothing launched.  Independent of
 * pm_engine_set_vcf_posteriors, pm_engine_set_vcf_phase and the pm_engine_set_vcf_denovo family: any may be on without
 * the others and none switches another off.  It may be set at any point between batches.  PM_EINVAL: an engine without
 * vcf_mode, or a submitted batch not yet collected. */
int pm_engine_set_vcf_joint(pm_engine *eng, int32_t on);

/* The plane of the last finished batch (pm_engine_run, pm_engine_run_vcf or pm_engine_submit / pm_engine_collect):
 * *n_rows = the batch's row count, out[row * n_person + person] with the rows of pm_site_result.call_row and the
 * persons in pm_pedigree order.  out may be NULL (the count alone).  After PM_EBRENT: the same prefix of rows the
 * batch returned.  PM_EINVAL: the feature is off, or a submitted batch has not been collected. */
int pm_engine_vcf_joint(pm_engine *eng, int32_t *n_rows, pm_vcf_joint *out);

/* The pedigree check of a vcf_mode engine (pm_engine_set_vcf_pedcheck / pm_engine_vcf_pedcheck; additive to ABI 8: callers
 * detect the feature by these symbols; the reference has no counterpart).  Unlike the planes it is one value per person
 * summed over every written row of every autosomal batch.  For a non-founder c (both parents stated inside its family) and
 * a row with the frequency f (pm_site_result.af; 1 - theta on a monomorphic row),
 *   L0      = the family's likelihood under the stated pedigree: the founder priors, the single-family prior mode, the plain
 *             transmission T and the family routing of the genotype rows and the three planes;
 *   L_fa    = the same with only c's transmission replaced by T_fa[a][b][k] = Sum_a' pi(a') T[a'][b][k], the paternal
 *             allele drawn from the population: pi = (f^2, 2 f (1 - f), (1 - f)^2);
 *   L_mo    = its mirror;   L_both = the same with T_un[a][b][k] = pi(k).
 * Everybody else, c's own children included, keeps its table.  A row counts for c when all four are finite and positive;
 * it then adds 1 to n and llrint(log10(L0 / L_h) * 2^28) to q[h], h = father, mother, both.  The sums are int64, so they
 * do not depend on how the rows were split into batches, on the launch shape or on the order of the additions: value =
 * q * 2^-28 log10 units, a row's quantisation error at most 2^-29.  A positive sum supports the stated link.  chrX / chrY
 * / MT sections add nothing, and neither do the children of a family of more than 255 persons (the kernels' work lists pack
 * a member's index into 8 bits, as the phase plane's do): they are listed with n = 0. */
typedef struct {
  int32_t person, pad;         /* pm_pedigree index of the non-founder; pad is written as 0 */
  int64_t n;                   /* rows counted */
  int64_t q[3];                /* father, mother, both: Sum llrint(log10(L0 / L_h) * 2^28) */
} pm_vcf_pedcheck;

/* Switch the pedigree check on or off (off at creation).  on: the sums are allocated and zeroed; with it on every
 * autosomal batch runs one extra pass after the joint plane's (k_vcf_pedcheck_lean / k_vcf_pedcheck_nuc /
 * k_vcf_pedcheck_es, routed as the planes' kernels are) that adds to the sums and writes nothing else: every other output
 * of the engine is that of the engine without it, byte for byte.  on while on keeps the sums.  off frees them; off =
 * nothing allocated, nothing launched.  A failed on frees what it allocated.  PM_EINVAL: an engine without vcf_mode, or a
 * submitted batch not yet collected. */
int pm_engine_set_vcf_pedcheck(pm_engine *eng, int32_t on);

/* Zero the sums.  PM_EINVAL as above, or with the feature off. */
int pm_engine_reset_vcf_pedcheck(pm_engine *eng);

/* *n_kids = the pedigree's non-founders; out[i], by ascending person index, holds the sums over every batch finished
 * since on / reset.  out may be NULL (the count alone).  PM_EINVAL: the feature is off, or a submitted batch has not been
 * collected. */
int pm_engine_vcf_pedcheck(pm_engine *eng, int32_t *n_kids, pm_vcf_pedcheck *out);

/* Page-locked host memory for pm_engine_submit's inputs and the result rows (H2D/D2H at full PCIe rate). */
int pm_host_alloc(uint64_t bytes, void **h_ptr);
int pm_host_free(void *h_ptr);

/* Device-resident variant for benchmarking / multi-GPU sharding: all pointers are device pointers,
 * results stay on the device (d_res[n], d_calls[n * n_person] indexed by site), launched on the
 * engine's stream; returns immediately.  pm_engine_sync waits.
 * d_pl is in the engine's GENOTYPE-PLANAR layout: [n][10][n_person] (site block of 10 planes, plane g
 * holding every person's phred for genotype g), so the engine's wavefronts read consecutive persons as
 * consecutive bytes.  pm_engine_synth writes this layout; pm_engine_to_planar converts person-major
 * GLF-record blocks (the layout of pm_engine_run). */
int pm_engine_run_device(pm_engine *eng, int32_t n, const uint8_t *d_pl, const uint32_t *d_dm, const uint8_t *d_ref,
                         pm_site_result *d_res, pm_geno_call *d_calls);
int pm_engine_sync(pm_engine *eng);

/* Person-major device block [n][n_person][10] -> genotype-planar [n][10][n_person] (distinct buffers),
 * on the engine's stream (asynchronous, like pm_engine_run_device). */
int pm_engine_to_planar(pm_engine *eng, int32_t n, const uint8_t *d_src, uint8_t *d_dst);

/* Section counters accumulated so far (device -> host copy). */
int pm_engine_counters(pm_engine *eng, pm_counters *out);

/* Deterministic synthetic GLF block generator on the device (SURVEY.md section 8(d) recipe):
 * families shaped by the engine's pedigree, 10% polymorphic sites, depth U{8..29}, error 1%.
 * Writes d_pl in the genotype-planar layout of pm_engine_run_device. */
int pm_engine_synth(pm_engine *eng, int32_t n, uint64_t seed, uint64_t site_offset,
                    uint8_t *d_pl, uint32_t *d_dm, uint8_t *d_ref);

/* Device allocation helpers (so FFI callers need no HIP runtime of their own). */
int pm_device_alloc(pm_engine *eng, uint64_t bytes, void **d_ptr);
int pm_device_free(pm_engine *eng, void *d_ptr);
int pm_copy_to_host(pm_engine *eng, void *h_dst, const void *d_src, uint64_t bytes);
int pm_copy_to_device(pm_engine *eng, void *d_dst, const void *h_src, uint64_t bytes);

/* Timing of the dominant (Brent) kernel over the last run: launches, summed kernel ms (HIP events on the
 * engine stream), total objective evaluations and family-evaluations (for roofline accounting). */
typedef struct {
  int64_t launches;      /* k_brent launches */
  double  kernel_ms;     /* summed k_brent time (HIP events on the engine stream) */
  int64_t evals;         /* objective evaluations computed by Brent items (OptimizeFrequency's f(a) and f(c),
                            which Brent never reads, are counted in pm_site_result.evals but not computed) */
  int64_t fam_evals;     /* evals x families */
  int64_t items;         /* (site, configuration) work items evaluated */
  int64_t sites;         /* sites processed */
  int64_t site_visits;   /* sum over k_brent launches of the distinct sites each launch touched (each visit
                            reads that site's PL block once: the launch's algorithmic HBM bytes) */
  int64_t hoist_wave_ns; /* with PM_PHASE_TIMING set at engine creation (else 0): k_brent wave time spent hoisting
                            the frequency-independent family terms, summed over the items' blocks (lane 0's clock) */
  int64_t eval_wave_ns;  /* ... and in the Brent loop (objective evaluations + updates) */
  int64_t timed_items;   /* items the two fields above cover */
  /* extended families in polynomial form (EP): the coefficient hoisting that precedes each Brent chunk, timed apart
     from the Brent launches (kernel_ms / launches above exclude it) */
  int64_t es_hoist_launches;
  double  es_hoist_ms;
  double  es_hoist_ops;  /* its FP64 operations (each mul, add or fma one), counted by the schedule compiler per family
                            shape and variant; 0 when the generic kernel ran (PM_NO_JIT) */
} pm_kernel_stats;
int pm_engine_kernel_stats(pm_engine *eng, pm_kernel_stats *out, int32_t reset);

const char *pm_last_error(void);
int pm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* POLYMUTT_ENGINE_H */
