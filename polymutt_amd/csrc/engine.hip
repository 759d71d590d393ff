// engine.hip -- host side of the MI355X (gfx950) engine (pm_engine_*, the C ABI of include/polymutt_engine.h) and the
// non-Brent kernels' instantiations.  The device code is in engine_dev.h; the k_brent instantiations are compiled in
// separate units (brent_inst.hip, one object per PM_BRENT_PART) and declared extern here (brent_variants.h).  Which of
// them a launch takes is decided in brent_plan.h (host-only) and resolved through kBrentTable.
#include "engine_dev.h"
#include "brent_plan.h"
#include "brent_variants.h"
#include "vcf_denovo_dev.h"
#include "vcf_plane_dev.h"
#include "vcf_post_dev.h"
#include "vcf_phase_dev.h"
#include "vcf_joint_dev.h"
#include "vcf_pedcheck_dev.h"

#define PM_BRENT_X(part, ...) extern template __global__ void k_brent<__VA_ARGS__>(DevArgs, int);
PM_BRENT_VARIANTS
#undef PM_BRENT_X
// every instantiation by its template arguments: one list produces key and kernel, so a key cannot name another kernel
typedef void (*BrentFn)(DevArgs, int);
#define PM_BRENT_X(part, ...) {{__VA_ARGS__}, k_brent<__VA_ARGS__>},
static const struct { pmplan::BrentKey key; BrentFn fn; } kBrentTable[] = {PM_BRENT_VARIANTS};
#undef PM_BRENT_X
static_assert(pmplan::kPdLo == PM_PD_LO && pmplan::kPdHi == PM_PD_HI && pmplan::kEpe == PM_EPE && pmplan::kDnPfC == DN_PF_C &&
              pmplan::kDnPfBuf == DN_PF_BUF && pmplan::kQWave == QWAVE, "brent_plan.h restates engine_dev.h's constants");

// ------------------------------------------------------------------------------------------------
// error reporting (thread-local, C ABI)
static thread_local std::string g_last_error;
extern "C" void pm_set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }
extern "C" const char* pm_last_error(void) { return g_last_error.c_str(); }
extern "C" int pm_abi_version(void) { return PM_ABI_VERSION; }
// ================================================================================================
// host side
// One output plane of vcf_mode batches, [max_batch][n_person] cells: off = no buffer, no launch
struct Plane {
  size_t cell;                      // bytes per (row, person)
  void* d = nullptr;
  bool on = false, valid = false;   // valid: the last finished batch filled the plane
};
// An index list per lane plan (0 / 1) that a plane's peel kernel walks: built with the engine, on the device while the plane is on
struct PlanList {
  std::vector<int> h[2];
  int* d[2] = {nullptr, nullptr};
  int users = 0;   // the features that hold the device copy (acquire / release)
  int upload();
  void free();
  int acquire() { if (users == 0) { if (int rc = upload()) { free(); return rc; } } users++; return 0; }
  void release() { if (users > 0 && --users == 0) free(); }
};

struct pm_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  pm_params par;
  pmplan::EngineSwitches sw;   // the PM_* environment switches as pm_engine_create found them
  int n_fam = 0, n_person = 0, max_batch = 0;
  int chrom = PM_CHR_AUTO;
  int T = 64, S = 1;
  int grid_brent = 1024;
  bool has_fp = false;
  bool quad = false;       // QUAD lane plan (hoist_quad): every unit a 4-person nuclear family at a multiple-of-4 person
  int quad_full = 0;       // slot rows below this have no empty lane
  int last_n = 0;
  int n_cu = 256;
  bool carry_postprob = false;
  std::vector<int> fam_start_h;
  std::vector<int8_t> sex_h;
  int single_nuclear = 0, max_nuc = 0;
  int max_fam = 0;            // largest family (persons)
  double prior = 0;
  int n_founders = 0, male_founders = 0, female_founders = 0;
  // device buffers
  int *d_fam_start = nullptr, *d_fam_kind = nullptr, *d_fa = nullptr, *d_mo = nullptr;
  int8_t* d_sex = nullptr;
  int4* d_units = nullptr;
  double *d_lktab = nullptr, *d_M = nullptr;
  pm_synth_tables* d_syn = nullptr;
  uint8_t *d_pl = nullptr, *d_ref = nullptr;
  uint8_t* d_stage = nullptr;   // person-major staging block of pm_engine_run (transposed into d_pl)
  // pm_engine_submit / pm_engine_collect: the batch in flight, its results and counts landing in page-locked memory
  pm_site_result* h_res = nullptr;
  int* h_counts = nullptr;
  int pending_n = -1;
  uint32_t* d_dm = nullptr;
  pm_site_result* d_res = nullptr;
  pm_geno_call* d_calls = nullptr;
  double *d_raw = nullptr, *d_minv = nullptr, *d_mono = nullptr;
  int* d_evals = nullptr;
  // extended families (Elston-Stewart)
  int n_ext = 0, max_ext = 0, ws_per_lane = 0, grid_post = 0;
  int *d_fam_founders = nullptr, *d_peel_start = nullptr, *d_ext_count = nullptr, *d_ext_fam = nullptr;
  int8_t* d_is_founder = nullptr;
  int2* d_steps = nullptr;
  double *d_T10 = nullptr, *d_T10dn = nullptr, *d_ws = nullptr, *d_tba = nullptr;
  // ES polynomial form (PM_NUM_POLY): per-family layouts and per-step degrees (poly_layout)
  bool es_poly = false;
  int poly_ws = 0, poly_coef = 0, poly_dcap = 0;
  int ep_dmax[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  int itmax = 200;          // ScalarMinimizer::Brent's ITMAX (core/MathGold.cpp:98); PM_TEST_ITMAX lowers it (tests)
  int stuck_site = -1;      // the last finished batch's first site whose Brent hit ITMAX (pm_engine_stuck_site)   // [plan][class]: the largest polynomial degree of a peeled family
  int hoist_tmp = 0, hoist_waves = 4, es_chunk = 0;   // k_es_hoist: step temporaries per wave, waves per block, items per launch
  double* d_es_coef = nullptr;                        // [es_chunk][max_ext][poly_dcap][T] hoisted coefficients
  unsigned long long* d_es_prof = nullptr;            // PM_ES_PROF: es_hoist_wave cycles by part
  // the schedule compiler (es_jit.h): per plan (0, 1) and chromosome class, built on first use (0 untried, 1 ok, -1 failed)
  std::vector<int> ext_fam_h, ext_fam1_h, peel_start_h;
  std::vector<int2> steps_h;
  std::vector<int8_t> founder_h;
  std::vector<int> fam_founders_h;
  pmjit::Kernel jit[2][4];
  int jit_state[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  int* d_jit_slots[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};   // e | sig | p0
  // the fused hoisting + Brent kernel (es_jit.h ep_brent_jit) per plan and class: 0 not tried, 1 built, -1 unavailable
  pmjit::FusedKernel fused[2][4];
  int fused_state[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  int* d_fused_tab[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
  int *d_poly_start = nullptr, *d_poly_lay = nullptr, *d_poly_deg = nullptr;
  int *d_es_pers = nullptr, *d_es_pers1 = nullptr;   // (family << 8 | member) of peeled families: plan 0 / plan 1
  int* d_fam_perm = nullptr;   // families by (kind, size) for k_posterior
  int n_es_pers = 0, n_es_pers1 = 0;
  // vcf_mode on chrX/Y/MT or with a single family: nuclear families go through ES peeling as well
  // (FamilyLikelihoodSeq_VCF.cpp:97-103), so a second lane plan with them in the per-lane ES lists
  bool vcf = false, plan1_ok = false, use_plan1 = false;
  int T1 = 0, S1 = 0, grid1 = 0, n_ext1 = 0, max_ext1 = 0, has_fp1 = 0;
  int4* d_units1 = nullptr;
  int *d_ext_count1 = nullptr, *d_ext_fam1 = nullptr;
  // --quick_call: the MakeUnrelated() plan (every family an all-founder product) with its own geometry
  int Tq = 0, Sq = 0, grid_q = 0;
  bool units_empty = false, units1_empty = false;   // a lane plan with no nuclear or founder unit (every family peeled)
  std::vector<std::pair<const void*, int>> bpc;   // QUAD / EP one-wave k_brent blocks resident per CU, per instantiation
  std::vector<int> brent_launched;   // kBrentTable indices of the instantiations enqueued so far (pm_engine_brent_variants)
  bool all_trio = false;   // every unit of the lane plan is a 3-person nuclear family (or empty): k_brent's NF = 3
  bool split34 = false;    // plan_split34: quads in the first half of the slot rows, trios in the second (NF = 34)
  int4* d_units_q = nullptr;
  int* d_items[N_LISTS] = {nullptr, nullptr, nullptr};
  int* d_counts = nullptr;
  int* d_qctr = nullptr;     // QUAD dynamic item order: 8 per-XCD claim counters (k_brent DevArgs::qd_ctr)
  unsigned long long* d_eval_total = nullptr;
  unsigned long long* d_phase = nullptr;   // PM_PHASE_TIMING set at engine creation: k_brent hoisting / evaluation wave time
  int wall_khz = 100000;                   // wall_clock64() rate (hipDeviceAttributeWallClockRate)
  int* d_row_site = nullptr;
  int* d_row_blk = nullptr;   // k_rows_count: written records per 1024-site block
  // per-family de novo evidence (pm_engine_set_denovo_families): off (top_k 0) = no buffer, no launch
  int fam_top_k = 0, fam_grid = 0;
  int last_rows = 0;          // written rows of the last finished batch (pm_engine_denovo_families / _carriers)
  pm_fam_lr* d_fam_top = nullptr;                                      // [max_batch][top_k]
  double *d_fam_sum = nullptr, *d_fam_all = nullptr, *d_fam_line = nullptr;   // [max_batch], [max_batch][n_fam] | [fam_grid][n_fam]
  // per-person de novo posteriors (pm_engine_set_denovo_carriers): off (top_k 0) = no buffer, no launch
  int pdn_top_k = 0, pdn_grid = 0, pdn_n_nuc = 0, pdn_n_es = 0;
  pm_person_dn *d_pdn_top = nullptr, *d_pdn_all = nullptr, *d_pdn_line = nullptr;   // [max_batch][top_k], [max_batch][n_person] | [pdn_grid][n_person]
  int2* d_pdn_kids = nullptr;       // the non-founders {family, member}: nuclear families' in fam_perm order, then extended families'
  int8_t* d_pdn_is_kid = nullptr;   // [n_person]
  double* d_pdn_jbuf = nullptr;     // [pdn_grid][pdn_n_es * 111] clamped-peel values of k_person_dn<true>
  // de novo calling from VCF input (pm_engine_set_vcf_denovo): off = no buffer, no launch
  bool vdn_on = false;
  int vdn_T = 0, vdn_grid = 0, vdn_terms = 0, vdn_peel = 0, vdn_nuc = 0;
  size_t vdn_lds = 0;        // dynamic LDS of k_vdn_brent (the hoisted coefficients), 0: they live in d_vdn_co
  int* d_vdn_terms = nullptr;
  double *d_vdn_co = nullptr, *d_vdn_ws = nullptr;
  // its chrX model (pm_engine_set_vcf_denovo_chrx): off = no buffer, no launch
  bool vdnx_on = false;
  int vdnx_T = 0, vdnx_grid = 0, vdnx_terms = 0, vdnx_peel = 0;
  int* d_vdnx_terms = nullptr;
  double* d_vdnx_ws = nullptr;
  // the families and children behind each DQ (pm_engine_set_vcf_denovo_detail): off (both k 0) = no buffer, no launch
  int vw_fam_k = 0, vw_car_k = 0, vw_grid = 0, vw_n_nuc = 0, vw_n_es = 0;
  int vw_rows = 0;            // rows of the last finished batch (after PM_EBRENT: those before the stuck site)
  int* d_vw_row_site = nullptr;                                         // [max_batch]
  int* d_vw_pfam = nullptr;                                             // [n_person]
  pm_fam_lr* d_vw_fam_top = nullptr;                                    // [max_batch][fam_k]
  double *d_vw_fam_sum = nullptr, *d_vw_fam_all = nullptr, *d_vw_fam_line = nullptr;   // [max_batch], [max_batch][n_fam] | [vw_grid][n_fam]
  pm_person_dn *d_vw_car_top = nullptr, *d_vw_car_all = nullptr, *d_vw_car_line = nullptr;   // [max_batch][car_k], [max_batch][n_person] | [vw_grid][n_person]
  int2* d_vw_kids = nullptr;
  int8_t* d_vw_is_kid = nullptr;
  double* d_vw_jbuf = nullptr;                                          // [vw_grid][vw_n_es * 13]
  // the same on chrX (pm_engine_set_vcf_denovo_chrx_detail): off = no buffer, no launch; the outputs are the detail's own
  bool vwx_on = false;
  int vwx_grid = 0, vwx_n_kids = 0;
  int2* d_vwx_kids = nullptr;                                           // every person with both parents in the family
  int8_t* d_vwx_is_kid = nullptr;
  double* d_vwx_jbuf = nullptr;                                         // [vwx_grid][vwx_n_kids * 13]
  // the output planes of vcf_mode batches: genotype posteriors (pm_engine_set_vcf_posteriors), transmission phase
  // (pm_engine_set_vcf_phase), joint calls (pm_engine_set_vcf_joint)
  Plane vp{sizeof(pm_vcf_post)}, vph{sizeof(pm_vcf_phase)}, vj{sizeof(pm_vcf_joint)};
  PlanList vph_kids;                        // (family << 8 | member) of the non-founders of peeled families
  PlanList vj_fams;                         // the peeled families
  double* d_vj_ws = nullptr;                // k_vcf_joint_es<false>'s workspace (only where the LDS one does not fit)
  int vj_ws_per_lane = 0, vj_grid = 0;      // doubles per thread; HBM grid
  // the pedigree check (pm_engine_set_vcf_pedcheck): sums over every autosomal batch; off = no buffer, no launch
  bool pc_on = false;
  std::vector<int> pc_person;               // the non-founders by ascending person index
  unsigned long long* d_pc_acc = nullptr;   // [non-founders][4]: n, q father, q mother, q both
  int* d_pc_slot = nullptr;                 // [n_person] index into pc_person, -1 for a founder
  bool vph_holds_kids = false, pc_holds_kids = false;               // the phase plane / the check holds vph_kids' device copy
  PlanList pc_nuc_kids;                     // the children of the nuclear families plan 0 does not peel
  std::vector<int> fam_kind_h, fam_perm_h;
  std::vector<int32_t> fa_h, mo_h;  // family-local parent indices (-1: none)
  unsigned long long* d_counters = nullptr;
  double M_h[100], A4_h[16];   // the genotype mutation matrix and the allele one it is built from
  // stats
  pm_kernel_stats stats{};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> brent_events;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> es_events;   // the EP hoisting launches (schedule compiler or k_es_hoist)
  double es_item_ops[6] = {0, 0, 0, 0, 0, 0};   // FP64 ops of one item's hoisting over the lane plan's extended families, by variant
  bool es_grouped = false;             // es_hoist_wave tasks are a site's de novo items (the leaf steps taken once)
  bool es_ops_known = false;           // (the compiled kernels report them; the generic k_es_hoist does not)
};

static void geno_mut_matrix(double mu, double tstv, double* out, double* a4) {   // src/MutationModel.cpp:15-90
  double A[4][4];
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) A[i][j] = (i == j) ? 1 - mu : (1 - mu) / 3;
  if (tstv != 0.0) {
    A[0][2] = A[2][0] = A[1][3] = A[3][1] = mu / 3 * (3 - 3 / (1 + tstv));
    A[0][1] = A[0][3] = A[1][0] = A[1][2] = A[2][1] = A[2][3] = A[3][0] = A[3][2] = mu / 3 * (0.5 / (1 + tstv) * 3);
  }
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) a4[i * 4 + j] = A[i][j];
  double R[16][16];
  int from = -1;
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) {
    from++; int to = -1;
    for (int ii = 0; ii < 4; ii++) for (int jj = 0; jj < 4; jj++) { to++; R[from][to] = A[i][ii] * A[j][jj]; }
  }
  static const int h1[6] = {2, 3, 4, 7, 8, 12}, h2[6] = {5, 9, 13, 10, 14, 15};
  for (int i = 0; i < 6; i++) for (int j = 0; j < 16; j++) R[j][h1[i] - 1] += R[j][h2[i] - 1];
  static const int un[10] = {1, 2, 3, 4, 6, 7, 8, 11, 12, 16};
  for (int i = 0; i < 10; i++) for (int j = 0; j < 10; j++) out[i * 10 + j] = R[un[i] - 1][un[j] - 1];
}

template <typename X>
static int dalloc(X** p, size_t count) {
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void**)p, count * sizeof(X));
  if (e != hipSuccess) {
    char b[256]; snprintf(b, sizeof(b), "hipMalloc(%zu bytes) failed: %s", count * sizeof(X), hipGetErrorString(e));
    pm_set_last_error(b);
    return PM_ENOMEM;
  }
  return PM_OK;
}
static void dfree(void** p) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
}
int PlanList::upload() {
  for (int plan = 0; plan < 2; plan++) {
    if (int rc = dalloc(&d[plan], std::max<size_t>(1, h[plan].size()))) return rc;
    if (!h[plan].empty()) HIP_TRY(hipMemcpy(d[plan], h[plan].data(), sizeof(int) * h[plan].size(), hipMemcpyHostToDevice));
  }
  return PM_OK;
}
void PlanList::free() {
  for (int plan = 0; plan < 2; plan++) dfree((void**)&d[plan]);
  users = 0;
}
// a persistent grid rounded down to whole rounds of the 8 XCDs (the kernels' XCD-aware item order needs gridDim % 8 == 0;
// they fall back to plain order otherwise), never below one block
static int xcd_grid(int g) { return g >= 8 ? g - g % 8 : std::max(g, 1); }
#define DALLOC(p, n) do { int _r = dalloc(&(p), (n)); if (_r) { pm_engine_destroy(E); return _r; } } while (0)

// What brent_plan.h's functions read from the engine (pm_engine_create calls it with the fields it has set so far).
static pmplan::Facts facts_of(const pm_engine* E) {
  pmplan::Facts f;
  f.n_person = E->n_person; f.n_fam = E->n_fam; f.chrom = E->chrom; f.numerics = E->par.numerics; f.max_nuc = E->max_nuc;
  f.denovo = E->par.denovo != 0; f.quick_call = E->par.quick_call != 0; f.vcf = E->vcf; f.use_plan1 = E->use_plan1;
  f.has_fp = E->has_fp; f.es_poly = E->es_poly; f.quad = E->quad; f.all_trio = E->all_trio; f.split34 = E->split34;
  f.plan[0] = {E->T, E->S, E->n_ext, E->units_empty, E->ep_dmax[0][E->chrom]};
  f.plan[1] = {E->T1, E->S1, E->n_ext1, E->units1_empty, E->ep_dmax[1][E->chrom]};
  f.quick = {E->Tq, E->Sq};
  return f;
}

// Deal families to lanes: family-major round robin; founders-only families are split into <=3-person chunks
// kept on one lane.  Returns false if the plan does not fit T x S.
// Extended families are not units: they go to per-lane lists (plan_ext).  unrelated = the --quick_call
// MakeUnrelated() view (FamilyLikelihoodSeq.cpp:54-59): every family is an all-founder product.
static bool plan_units(const pm_pedigree* ped, int T, int S, std::vector<int4>& units, bool unrelated = false,
                       bool nuc_es = false) {
  units.assign((size_t)T * S, make_int4(U_NONE, -1, 0, 0));
  std::vector<int> used(T, 0);
  int lane = 0;
  for (int f = 0; f < ped->n_fam; f++) {
    const int p0 = ped->fam_start[f], n = ped->fam_start[f + 1] - p0, kind = unrelated ? PM_FAM_FOUNDERS : ped->fam_kind[f];
    std::vector<int4> us;
    if (kind == PM_FAM_EXTENDED || (nuc_es && kind == PM_FAM_NUCLEAR)) continue;
    if (kind == PM_FAM_NUCLEAR) us.push_back(make_int4(U_NUC, f, p0, n));
    else if (kind == PM_FAM_FOUNDERS) {
      for (int j = 0; j < n; j += 3) {
        int c = std::min(3, n - j), fl = c;
        if (j == 0) fl |= UF_FIRST;
        if (j + 3 >= n) fl |= UF_LAST;
        us.push_back(make_int4(U_FP, f, p0 + j, fl));
      }
    }
    // choose the lane: next in round-robin order with enough room
    int tries = 0;
    while (used[lane] + (int)us.size() > S && tries < T) { lane = (lane + 1) % T; tries++; }
    if (tries >= T) return false;
    for (auto& u : us) units[(size_t)used[lane]++ * T + lane] = u;
    lane = (lane + 1) % T;
  }
  return true;
}

// Split plan for pedigrees of trios and quads only (config 5's 2000 mixed families): quads dealt round-robin over the lanes
// of slot rows [0, S/2), trios over rows [S/2, S), so the lean PF kernel hoists each half with its family size known
// (k_brent NF = 34).  false when either kind does not fit its half.
static bool plan_split34(const pm_pedigree* ped, int T, int S, std::vector<int4>& units) {
  if (S < 2 || S % 2) return false;
  units.assign((size_t)T * S, make_int4(U_NONE, -1, 0, 0));
  int nq = 0, nt = 0;
  for (int f = 0; f < ped->n_fam; f++) {
    const int p0 = ped->fam_start[f], n = ped->fam_start[f + 1] - p0;
    if (ped->fam_kind[f] != PM_FAM_NUCLEAR || (n != 3 && n != 4)) return false;
    int& c = n == 4 ? nq : nt;
    const int row = (n == 4 ? 0 : S / 2) + c / T;
    if (c / T >= S / 2) return false;
    units[(size_t)row * T + c % T] = make_int4(U_NUC, f, p0, n);
    c++;
  }
  return nq > 0 && nt > 0;
}

// pack_steps: es_jit.cpp (pmjit::pack_steps), shared with the schedule compiler.
using pmjit::pack_steps;

// Layout of one family's peel in polynomial form (k_es_hoist / wave_poly_peel): for every chromosome class the degree each
// step combines (founders: 2; 1 for chrX/Y males and chrMT; 0 for chrY females), per slot the coefficient
// capacity (largest degree + 1 over the classes), a temp region, and the likelihood's degree D.  Appends the
// family's layout ints to lay and its steps' degree words to deg; returns the workspace doubles, -1 if a degree
// exceeds the packing (the exact peel is used then).
static int poly_layout(const pm_pedigree* ped, int f, int ns, const int2* st, int nst, std::vector<int>& lay, std::vector<int>& deg) {
  const int p0 = ped->fam_start[f], n = ped->fam_start[f + 1] - p0, nf = ped->fam_founders[f];
  int nkeys = 0;
  for (int s = 0; s < nst; s++)
    if ((st[s].x & 255) == 1) nkeys = std::max(nkeys, ((st[s].y >> 8) & 255) + 1);
  std::vector<int> capP(n, 1), capM(nkeys, 1), Dc(4, 0);
  std::vector<int> dg((size_t)nst * 4, 0);
  int tmp = 1;
  for (int cls = 0; cls < 4; cls++) {
    const bool X = cls == PM_CHR_X, Y = cls == PM_CHR_Y, MT = cls == PM_CHR_MT;
    std::vector<int> dP(n), dM(nkeys, 0);
    for (int i = 0; i < n; i++) {
      const bool fo = ped->is_founder[p0 + i] && i < nf;
      const int sx = ped->sex[p0 + i];
      dP[i] = !fo ? 0 : (Y && sx == FEMALE) ? 0 : (((X || Y) && sx == MALE) || MT) ? 1 : 2;
      capP[i] = std::max(capP[i], dP[i] + 1);
    }
    for (int s = 0; s < nst; s++) {
      const int type = st[s].x & 255, from0 = (st[s].x >> 8) & 255, from1 = (st[s].x >> 16) & 255, to0 = (st[s].x >> 24) & 255;
      const int slot = (st[s].y >> 8) & 255, create = (st[s].y >> 16) & 1;
      int a = 0, b = 0, c = 0, e = 0;
      if (type == 1) {
        a = dP[from0]; b = create ? 0 : dM[slot];
        dM[slot] = a + b;
        capM[slot] = std::max(capM[slot], dM[slot] + 1);
        tmp = std::max(tmp, a + 1);
      } else if (type == 2) {
        a = dP[from0]; b = slot == 255 ? 0 : dM[slot]; c = dP[to0];
        dP[to0] = a + b + c;
        capP[to0] = std::max(capP[to0], dP[to0] + 1);
        tmp = std::max(tmp, a + b + 1);
      } else {
        a = dP[from0]; b = slot == 255 ? 0 : dM[slot]; c = dP[from1]; e = dP[to0];
        dP[to0] = a + b + c + e;
        capP[to0] = std::max(capP[to0], dP[to0] + 1);
        tmp = std::max(tmp, (ns + 1) * (a + b + c + 1));
      }
      if (std::max({a, b, c, e, a + b + c + e}) > 120) return -1;
      dg[(size_t)s * 4 + cls] = a | (b << 7) | (c << 14) | (e << 21);
    }
    Dc[cls] = dP[(st[nst - 1].x >> 24) & 255];
  }
  const size_t base = lay.size();
  lay.push_back(nkeys);
  lay.push_back(0);   // temp offset, below
  for (int c = 0; c < 4; c++) lay.push_back(Dc[c]);
  int off = 0;
  for (int i = 0; i < n; i++) { if (capP[i] > 127) return -1; lay.push_back(off | (capP[i] << 24)); off += ns * capP[i]; }
  for (int m = 0; m < nkeys; m++) { if (capM[m] > 127) return -1; lay.push_back(off | (capM[m] << 24)); off += ns * ns * capM[m]; }
  lay[base + 1] = off;
  off += tmp;
  if (off >= (1 << 24)) return -1;
  deg.insert(deg.end(), dg.begin(), dg.end());
  return off;
}

static int gi_h(int b1, int b2) { return b1 < b2 ? (b1 - 1) * (10 - b1) / 2 + (b2 - b1) : (b2 - 1) * (10 - b2) / 2 + (b1 - b2); }

// FamilyLikelihoodES::SetTransmissionMatrix (:752-785) and SetTransmissionMatrix_denovo (:787-810)
static void transmission_tables(const double* M, std::vector<double>& T10, std::vector<double>& T10dn) {
  T10.assign(1000, 0.0);
  T10dn.assign(1000, 0.0);
  for (int i = 1; i <= 4; i++)
    for (int j = i; j <= 4; j++) {
      const int x = gi_h(i, j);
      for (int k = 1; k <= 4; k++)
        for (int m = k; m <= 4; m++) {
          const int y = gi_h(k, m), g[4] = {gi_h(i, k), gi_h(i, m), gi_h(j, k), gi_h(j, m)};
          for (int t = 0; t < 4; t++) T10[(x * 10 + y) * 10 + g[t]] += 0.25;
        }
    }
  for (int i = 0; i < 10; i++)
    for (int j = 0; j < 10; j++)
      for (int k = 0; k < 10; k++) {
        double s = .0;
        for (int m = 0; m < 10; m++) s += T10[(i * 10 + j) * 10 + m] * M[m * 10 + k];
        T10dn[(i * 10 + j) * 10 + k] = s;
      }
}

// SetTransmissionMatrix_BA, _CHRX_2Female, _CHRX_2Male, _CHRY, _MITO (:812-924), [parent1][parent2][child]
static const double kTBA[5][27] = PM_TBA_VALUES;

extern "C" {

void pm_engine_destroy(pm_engine* E) {
  if (!E) return;
  hipSetDevice(E->device);
  if (E->d_es_prof) {
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    if (hipMemcpy(h, E->d_es_prof, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess && (h[0] | h[1] | h[2] | h[3] | h[4]))
      fprintf(stderr, "PM_ES_PROF wave-cycles pen %llu toprest %llu leaf %llu rest %llu whole %llu\n", h[0], h[1], h[2], h[3], h[4]);
    (void)hipFree(E->d_es_prof);
  }
  void* bufs[] = {E->d_units1, E->d_ext_count1, E->d_ext_fam1, E->d_fam_founders, E->d_peel_start, E->d_ext_count, E->d_ext_fam, E->d_is_founder, E->d_steps, E->d_T10,
                  E->d_T10dn, E->d_ws, E->d_tba, E->d_units_q, E->d_poly_start, E->d_poly_lay, E->d_poly_deg, E->d_es_coef, E->d_es_pers, E->d_es_pers1, E->d_fam_perm,
                  E->d_fam_start, E->d_fam_kind, E->d_fa, E->d_mo, E->d_sex, E->d_units, E->d_lktab, E->d_M, E->d_syn,
                  E->d_pl, E->d_stage, E->d_ref, E->d_dm, E->d_res, E->d_calls, E->d_raw, E->d_minv, E->d_mono, E->d_evals,
                  E->d_items[0], E->d_items[1], E->d_items[2], E->d_counts, E->d_eval_total, E->d_row_site,
                  E->d_counters, E->d_row_blk, E->d_qctr, E->d_fam_top, E->d_fam_sum, E->d_fam_all, E->d_fam_line,
                  E->d_pdn_top, E->d_pdn_all, E->d_pdn_line, E->d_pdn_kids, E->d_pdn_is_kid, E->d_pdn_jbuf,
                  E->d_vdn_terms, E->d_vdn_co, E->d_vdn_ws, E->d_vdnx_terms, E->d_vdnx_ws, E->d_vw_row_site, E->d_vw_pfam, E->d_vw_fam_top, E->d_vw_fam_sum,
                  E->d_vw_fam_all, E->d_vw_fam_line, E->d_vw_car_top, E->d_vw_car_all, E->d_vw_car_line, E->d_vw_kids, E->d_vw_is_kid,
                  E->d_vw_jbuf, E->d_vwx_kids, E->d_vwx_is_kid, E->d_vwx_jbuf, E->vp.d, E->vph.d, E->vj.d, E->d_vj_ws, E->d_pc_acc, E->d_pc_slot};
  for (void* b : bufs) if (b) hipFree(b);
  E->vph_kids.free();
  E->vj_fams.free();
  E->pc_nuc_kids.free();
  for (auto& pl : E->d_jit_slots)
    for (int* b : pl) if (b) hipFree(b);
  for (auto& pl : E->d_fused_tab)
    for (int* b : pl) if (b) hipFree(b);
  for (auto& pr : E->brent_events) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
  for (auto& pr : E->es_events) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
  if (E->h_res) hipHostFree(E->h_res);
  if (E->h_counts) hipHostFree(E->h_counts);
  if (E->ev0) hipEventDestroy(E->ev0);
  if (E->ev1) hipEventDestroy(E->ev1);
  if (E->stream) hipStreamDestroy(E->stream);
  delete E;
}

int pm_engine_create(const pm_pedigree* ped, const pm_params* par, int device, int max_batch, pm_engine** out) {
  if (!ped || !par || !out || ped->n_fam <= 0 || ped->n_person <= 0 || max_batch <= 0) {
    pm_set_last_error("pm_engine_create: invalid arguments");
    return PM_EINVAL;
  }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    pm_set_last_error("pm_engine_create: no HIP device available (the engine has no CPU fallback)");
    return PM_EHIP;
  }
  if (device < 0 || device >= ndev) { pm_set_last_error("pm_engine_create: device index out of range"); return PM_EINVAL; }
  if (par->numerics < PM_NUM_PRODUCT || par->numerics > PM_NUM_POLY) {
    pm_set_last_error("pm_engine_create: unknown numerics mode");
    return PM_EINVAL;
  }
  pm_engine* E = new pm_engine;
  E->device = device;
  E->par = *par;
  E->vcf = par->vcf_mode != 0;
  if (E->vcf) { E->par.denovo = 0; E->par.quick_call = 0; }   // the VCF path has neither (PedVCF.cpp)
  par = &E->par;
  E->sw = pmplan::EngineSwitches::from_env();   // every engine switch is read here, once
  const pmplan::EngineSwitches& sw = E->sw;
  if (sw.test_itmax > 0) E->itmax = std::min(200, sw.test_itmax);
  E->n_fam = ped->n_fam;
  E->n_person = ped->n_person;
  E->max_batch = max_batch;
  E->n_founders = ped->n_founders; E->male_founders = ped->male_founders; E->female_founders = ped->female_founders;
  // a lone nuclear family is evaluated once at 0.5 (FamilyLikelihoodSeq.cpp:91-104); the VCF path always runs Brent
  E->single_nuclear = (!E->vcf && ped->n_fam == 1 && ped->fam_kind[0] == PM_FAM_NUCLEAR) ? 1 : 0;
  for (int f = 0; f < ped->n_fam; f++) {
    if (ped->fam_kind[f] == PM_FAM_NUCLEAR) E->max_nuc = std::max(E->max_nuc, ped->fam_start[f + 1] - ped->fam_start[f]);
    E->max_fam = std::max(E->max_fam, ped->fam_start[f + 1] - ped->fam_start[f]);
  }
  for (int f = 0; f < ped->n_fam; f++) {
    if (ped->fam_kind[f] != PM_FAM_NUCLEAR) E->has_fp = true;
    if (ped->fam_kind[f] == PM_FAM_EXTENDED) E->n_ext++;
  }
  E->fam_start_h.assign(ped->fam_start, ped->fam_start + ped->n_fam + 1);
  E->sex_h.assign(ped->sex, ped->sex + ped->n_person);
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&E->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreate(&E->ev0));
  HIP_TRY(hipEventCreate(&E->ev1));
  // --- Elston-Stewart schedules and their polynomial-form layouts first: whether the polynomial form is usable
  // (es_poly) decides how many extended families a lane of the plan may hold
  const int ns = par->denovo ? 10 : 3;
  std::vector<int> peel_start(ped->n_fam + 1, 0);
  std::vector<int2> steps;
  std::vector<int> founders(ped->fam_founders, ped->fam_founders + ped->n_fam);
  int wsmax = 0;
  E->plan1_ok = E->vcf;
  for (int f = 0; f < ped->n_fam; f++) {
    peel_start[f] = (int)steps.size();
    const int kind = ped->fam_kind[f];
    if (kind == PM_FAM_FOUNDERS || (kind == PM_FAM_NUCLEAR && !E->vcf)) continue;
    const size_t mark = steps.size();
    const int w = pack_steps(ped, f, ns, steps);
    if (w < 0 && kind == PM_FAM_EXTENDED) {
      pm_engine_destroy(E);
      pm_set_last_error("pm_engine_create: extended family without a usable peeling schedule (or > 255 members)");
      return PM_EPED;
    }
    if (w < 0) { steps.resize(mark); E->plan1_ok = false; continue; }   // nuclear without a schedule: no plan 1
    wsmax = std::max(wsmax, w);
  }
  peel_start[ped->n_fam] = (int)steps.size();
  E->ws_per_lane = wsmax;
  // polynomial-form layouts (PM_NUM_POLY): every family with a schedule.  Under --denovo the 10-state layout
  // also serves the BA (cfg-7) items: the degrees do not depend on the state count, the slots are larger.
  std::vector<int> poly_start(ped->n_fam + 1, 0), poly_lay, poly_deg((size_t)steps.size() * 4, 0);
  int poly_w = 0, poly_d = 0;
  E->es_poly = par->numerics == PM_NUM_POLY && !steps.empty();
  for (int f = 0; f < ped->n_fam && E->es_poly; f++) {
    poly_start[f] = (int)poly_lay.size();
    const int ns0 = peel_start[f], ns1 = peel_start[f + 1];
    if (ns1 == ns0) continue;
    std::vector<int> dg;
    const int w = poly_layout(ped, f, par->denovo ? 10 : 3, steps.data() + ns0, ns1 - ns0, poly_lay, dg);
    if (w < 0) { E->es_poly = false; break; }
    std::copy(dg.begin(), dg.end(), poly_deg.begin() + (size_t)ns0 * 4);
    poly_w = std::max(poly_w, w);
    for (int c = 0; c < 4; c++) poly_d = std::max(poly_d, poly_lay[poly_start[f] + 2 + c]);
  }
  poly_start[ped->n_fam] = (int)poly_lay.size();
  auto fam_deg = [&](int f, int c) {   // the polynomial degree of family f in chromosome class c (0: no layout)
    return poly_start[f + 1] > poly_start[f] ? poly_lay[poly_start[f] + 2 + c] : 0;
  };
  if (E->es_poly) {   // k_es_hoist temporaries: the largest step's out-of-place phases (wave_poly_peel)
    const int ns = par->denovo ? 10 : 3;
    for (size_t s = 0; s < steps.size(); s++)
      for (int cls = 0; cls < 4; cls++) {
        const int dg = poly_deg[s * 4 + cls], type = steps[s].x & 255;
        const int a = dg & 127, b = (dg >> 7) & 127, c = (dg >> 14) & 127, e = (dg >> 21) & 127;
        int need;
        if (type == 1) need = ns * ns * (a + 1) + ns * ns * (a + b + 1);
        else if (type == 2) need = ns * (a + b + 1) + ns * (a + b + c + 1);
        else need = ns * ns * (a + b + c + 1) + ns * (a + b + c + 1) + ns * (a + b + c + e + 1);
        E->hoist_tmp = std::max(E->hoist_tmp, need);
      }
    // 4 waves per block when their LDS slices fit, else fewer; none: the reference-order peel per evaluation
    const size_t stat = (256 + 5 * 27 + (par->denovo ? 2000 : 2)) * sizeof(double);
    const size_t per_wave = (size_t)(poly_w + E->hoist_tmp) * sizeof(double);
    E->hoist_waves = 0;
    for (int w = 4; w >= 1 && !E->hoist_waves; w--)
      if (stat + per_wave * w <= 150 * 1024) E->hoist_waves = w;
    if (!E->hoist_waves) E->es_poly = false;
  }
  // plan 0: PM_BRENT_TS="T,S" (geometry experiments), else the first geometry in preference order that holds every family
  std::vector<int4> units;
  const pmplan::Geometry g0 = pmplan::choose_geometry(facts_of(E), sw, [&](int t, int s) { return plan_units(ped, t, s, units); });
  E->T = g0.T; E->S = g0.S;
  if (!g0.T) { pm_engine_destroy(E); pm_set_last_error("pm_engine_create: pedigree too large for the lane plan"); return PM_EPED; }
  // mixed trio / quad pedigrees on the lean one- or two-wave 16-slot plans: the split layout (PM_NO_SPLIT34=1: off)
  if (!par->denovo && par->numerics == PM_NUM_POLY && !E->has_fp && E->n_ext == 0 && E->S == 16 && (E->T == 64 || E->T == 128) &&
      !sw.no_split34) {
    std::vector<int4> u2;
    if (plan_split34(ped, E->T, E->S, u2)) { units.swap(u2); E->split34 = true; }
  }
  {   // QUAD plan: each nuclear family's four PL bytes of a genotype plane form one aligned dword
    bool q = E->n_person % 16 == 0 && !E->has_fp && E->T == 64;
    int full = E->S;
    for (int sl = 0; sl < E->S && q; sl++)
      for (int l = 0; l < E->T; l++) {
        const int4 u = units[(size_t)sl * E->T + l];
        if (u.x == U_NONE) { full = std::min(full, sl); continue; }
        if (u.x != U_NUC || u.w != 4 || u.z != 4 * (sl * E->T + l)) { q = false; break; }
      }
    E->quad = q && !sw.no_quad;
    E->quad_full = full;
  }
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  const int blocksPerCU = std::max(1, 1024 / E->T);   // ~16 waves per CU
  E->n_cu = prop.multiProcessorCount;
  E->grid_brent = prop.multiProcessorCount * blocksPerCU;
  // tables
  double lk[256];
  for (int i = 0; i <= 255; i++) lk[i] = pow(0.1, i * 0.1);   // core/BaseQualityHelper.cpp:13 (host glibc)
  if (E->vcf)   // FamilyLikelihoodSeq_VCF::PL2LK_table (src/FamilyLikelihoodSeq_VCF.cpp:21-22)
    for (int i = 0; i <= 255; i++) lk[i] = pow(10, -double(i) / 10.0);
  geno_mut_matrix(par->denovo_mut_rate, par->denovo_tstv, E->M_h, E->A4_h);
  static pm_synth_tables syn;
  pm_synth_build_tables(&syn);
  std::vector<int32_t> fa(ped->n_person, -1), mo(ped->n_person, -1);
  if (ped->father && ped->mother)
    for (int f = 0; f < ped->n_fam; f++)
      for (int j = ped->fam_start[f]; j < ped->fam_start[f + 1]; j++) {
        fa[j] = ped->father[j] < 0 ? -1 : ped->father[j] - ped->fam_start[f];
        mo[j] = ped->mother[j] < 0 ? -1 : ped->mother[j] - ped->fam_start[f];
      }
  E->fa_h = fa; E->mo_h = mo;
  E->fam_kind_h.assign(ped->fam_kind, ped->fam_kind + ped->n_fam);
  DALLOC(E->d_fam_start, ped->n_fam + 1);
  DALLOC(E->d_fam_kind, ped->n_fam);
  DALLOC(E->d_fa, ped->n_person);
  DALLOC(E->d_mo, ped->n_person);
  DALLOC(E->d_sex, ped->n_person);
  DALLOC(E->d_units, units.size());
  DALLOC(E->d_lktab, 256);
  DALLOC(E->d_M, 100);
  DALLOC(E->d_syn, 1);
  HIP_TRY(hipMemcpy(E->d_fam_start, ped->fam_start, sizeof(int) * (ped->n_fam + 1), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_fam_kind, ped->fam_kind, sizeof(int) * ped->n_fam, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_fa, fa.data(), sizeof(int) * ped->n_person, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_mo, mo.data(), sizeof(int) * ped->n_person, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_sex, ped->sex, ped->n_person, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_units, units.data(), sizeof(int4) * units.size(), hipMemcpyHostToDevice));
  E->units_empty = std::all_of(units.begin(), units.end(), [](const int4& u) { return u.x == U_NONE; });
  E->all_trio = !E->units_empty &&
                std::all_of(units.begin(), units.end(), [](const int4& u) { return u.x == U_NONE || (u.x == U_NUC && (u.w & 0xFF) == 3); });
  {   // k_posterior's family order: by kind, then size (mixed trio / quad pedigrees: no divergent family-size paths)
    std::vector<int> perm(ped->n_fam);
    for (int f = 0; f < ped->n_fam; f++) perm[f] = f;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) {
      const int na = ped->fam_start[a + 1] - ped->fam_start[a], nb = ped->fam_start[b + 1] - ped->fam_start[b];
      return ped->fam_kind[a] != ped->fam_kind[b] ? ped->fam_kind[a] < ped->fam_kind[b] : na < nb;
    });
    E->fam_perm_h = perm;
    DALLOC(E->d_fam_perm, ped->n_fam);
    HIP_TRY(hipMemcpy(E->d_fam_perm, perm.data(), sizeof(int) * ped->n_fam, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(E->d_lktab, lk, sizeof(lk), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_M, E->M_h, sizeof(E->M_h), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_syn, &syn, sizeof(syn), hipMemcpyHostToDevice));
  // --- Elston-Stewart data: packed schedules, per-lane family lists, transmission tables, workspace
  {
    if (E->es_poly)
      for (int f = 0; f < ped->n_fam; f++)
        for (int c = 0; c < 4; c++) {
          if (ped->fam_kind[f] == PM_FAM_EXTENDED) E->ep_dmax[0][c] = std::max(E->ep_dmax[0][c], fam_deg(f, c));
          if (ped->fam_kind[f] != PM_FAM_FOUNDERS) E->ep_dmax[1][c] = std::max(E->ep_dmax[1][c], fam_deg(f, c));
        }
    const int T = E->T;
    E->max_ext = (E->n_ext + T - 1) / T;
    std::vector<int> ext_count(T, 0), ext_fam((size_t)std::max(1, E->max_ext) * T, -1);
    int q = 0;
    for (int f = 0; f < ped->n_fam; f++)
      if (ped->fam_kind[f] == PM_FAM_EXTENDED) { const int lane = q % T; ext_fam[(size_t)ext_count[lane]++ * T + lane] = f; q++; }
    {   // persons of the peeled families, for k_posterior_es: plan 0 (extended) and plan 1 (every family with offspring)
      std::vector<int> e0, e1;
      for (int f = 0; f < ped->n_fam; f++) {
        const int n = ped->fam_start[f + 1] - ped->fam_start[f];
        for (int j = 0; j < n && n <= 255; j++) {
          if (ped->fam_kind[f] == PM_FAM_EXTENDED) e0.push_back(f << 8 | j);
          if (ped->fam_kind[f] != PM_FAM_FOUNDERS) e1.push_back(f << 8 | j);
        }
      }
      // ... and their non-founders, both parents in the family (k_vcf_phase_es; uploaded by pm_engine_set_vcf_phase)
      for (int plan = 0; plan < 2; plan++)
        for (int e : plan ? e1 : e0) {
          const int p = ped->fam_start[e >> 8] + (e & 255), n = ped->fam_start[(e >> 8) + 1] - ped->fam_start[e >> 8];
          if (!ped->is_founder[p] && fa[p] >= 0 && mo[p] >= 0 && fa[p] < n && mo[p] < n && fa[p] != mo[p]) E->vph_kids.h[plan].push_back(e);
        }
      // ... and the families themselves (k_vcf_joint_es; uploaded by pm_engine_set_vcf_joint)
      for (int f = 0; f < ped->n_fam; f++) {
        if (ped->fam_start[f + 1] - ped->fam_start[f] > 255) continue;
        if (ped->fam_kind[f] == PM_FAM_EXTENDED) E->vj_fams.h[0].push_back(f);
        if (ped->fam_kind[f] != PM_FAM_FOUNDERS) E->vj_fams.h[1].push_back(f);
      }
      E->n_es_pers = (int)e0.size();
      E->n_es_pers1 = (int)e1.size();
      DALLOC(E->d_es_pers, std::max<size_t>(1, e0.size()));
      DALLOC(E->d_es_pers1, std::max<size_t>(1, e1.size()));
      if (!e0.empty()) HIP_TRY(hipMemcpy(E->d_es_pers, e0.data(), sizeof(int) * e0.size(), hipMemcpyHostToDevice));
      if (!e1.empty()) HIP_TRY(hipMemcpy(E->d_es_pers1, e1.data(), sizeof(int) * e1.size(), hipMemcpyHostToDevice));
    }
    std::vector<double> T10, T10dn;
    transmission_tables(E->M_h, T10, T10dn);
    DALLOC(E->d_fam_founders, ped->n_fam);
    DALLOC(E->d_is_founder, ped->n_person);
    DALLOC(E->d_peel_start, ped->n_fam + 1);
    DALLOC(E->d_steps, std::max<size_t>(1, steps.size()));
    E->ext_fam_h = ext_fam;
    E->peel_start_h = peel_start;
    E->steps_h = steps;
    E->founder_h.assign(ped->is_founder, ped->is_founder + ped->n_person);
    E->fam_founders_h = founders;
    DALLOC(E->d_ext_count, T);
    DALLOC(E->d_ext_fam, ext_fam.size());
    DALLOC(E->d_T10, 1000);
    DALLOC(E->d_T10dn, 1000);
    HIP_TRY(hipMemcpy(E->d_fam_founders, founders.data(), sizeof(int) * ped->n_fam, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_is_founder, ped->is_founder, ped->n_person, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_peel_start, peel_start.data(), sizeof(int) * peel_start.size(), hipMemcpyHostToDevice));
    if (!steps.empty()) HIP_TRY(hipMemcpy(E->d_steps, steps.data(), sizeof(int2) * steps.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_ext_count, ext_count.data(), sizeof(int) * T, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_ext_fam, ext_fam.data(), sizeof(int) * ext_fam.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_T10, T10.data(), sizeof(double) * 1000, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(E->d_T10dn, T10dn.data(), sizeof(double) * 1000, hipMemcpyHostToDevice));
    DALLOC(E->d_tba, 5 * 27);
    HIP_TRY(hipMemcpy(E->d_tba, kTBA, sizeof(kTBA), hipMemcpyHostToDevice));
    {   // GQ thresholds (d_gq): smallest double q in (0, 1] with int(-10 log10(q) + 0.5) <= k, by bisection on the
        // bit patterns of positive doubles (ordered like their values), with the host's glibc log10
      double thr[101];
      auto gq_of = [](double q) { return (int)(-10. * log10(q) + 0.5); };
      for (int k = 0; k <= 100; k++) {
        uint64_t lo = 1, hi = 0x3FF0000000000000ull;   // gq_of(hi = 1.0) = 0 <= k; search the first bit pattern with gq <= k
        while (lo < hi) {
          const uint64_t mid = lo + (hi - lo) / 2;
          double q;
          memcpy(&q, &mid, 8);
          if (gq_of(q) <= k) hi = mid; else lo = mid + 1;
        }
        memcpy(&thr[k], &lo, 8);
      }
      HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_gq_thr), thr, sizeof(thr)));
    }
    // vcf_mode plan 1: nuclear families peeled too (chrX/Y/MT sections, or a single family)
    if (E->plan1_ok) {
      int n1 = 0;
      for (int f = 0; f < ped->n_fam; f++) {
        if (ped->fam_kind[f] != PM_FAM_FOUNDERS) n1++;
        else E->has_fp1 = 1;
      }
      int tmin = 1;
      while (tmin < std::min(std::max(n1, 1), 256)) tmin *= 2;
      std::vector<int4> u1;
      for (const pmplan::Geometry* g = pmplan::kPeeled; g->T && !E->T1; g++)
        if (g->T >= tmin && plan_units(ped, g->T, g->S, u1, false, true)) { E->T1 = g->T; E->S1 = g->S; }
      if (!E->T1) E->plan1_ok = false;
      else {
        E->n_ext1 = n1;
        E->max_ext1 = (n1 + E->T1 - 1) / E->T1;
        std::vector<int> c1(E->T1, 0), e1((size_t)std::max(1, E->max_ext1) * E->T1, -1);
        int q1 = 0;
        for (int f = 0; f < ped->n_fam; f++)
          if (ped->fam_kind[f] != PM_FAM_FOUNDERS) { const int lane = q1 % E->T1; e1[(size_t)c1[lane]++ * E->T1 + lane] = f; q1++; }
        E->ext_fam1_h = e1;
        DALLOC(E->d_units1, u1.size());
        DALLOC(E->d_ext_count1, E->T1);
        DALLOC(E->d_ext_fam1, e1.size());
        HIP_TRY(hipMemcpy(E->d_units1, u1.data(), sizeof(int4) * u1.size(), hipMemcpyHostToDevice));
        E->units1_empty = std::all_of(u1.begin(), u1.end(), [](const int4& u) { return u.x == U_NONE; });
        HIP_TRY(hipMemcpy(E->d_ext_count1, c1.data(), sizeof(int) * E->T1, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(E->d_ext_fam1, e1.data(), sizeof(int) * e1.size(), hipMemcpyHostToDevice));
        E->grid1 = E->n_cu * std::max(1, 1024 / E->T1);
      }
    }
    // polynomial form: per lane the peel workspace (reused family by family) and each ES family's D + 1
    // coefficients + D, kept for the item's evaluations
    if (E->es_poly) {
      E->poly_dcap = poly_d + 2;
      E->poly_coef = poly_w;
      E->poly_ws = poly_w + std::max({E->max_ext, E->max_ext1, 1}) * E->poly_dcap;
      DALLOC(E->d_poly_start, poly_start.size());
      DALLOC(E->d_poly_lay, std::max<size_t>(1, poly_lay.size()));
      DALLOC(E->d_poly_deg, std::max<size_t>(1, poly_deg.size()));
      HIP_TRY(hipMemcpy(E->d_poly_start, poly_start.data(), sizeof(int) * poly_start.size(), hipMemcpyHostToDevice));
      if (!poly_lay.empty()) HIP_TRY(hipMemcpy(E->d_poly_lay, poly_lay.data(), sizeof(int) * poly_lay.size(), hipMemcpyHostToDevice));
      if (!poly_deg.empty()) HIP_TRY(hipMemcpy(E->d_poly_deg, poly_deg.data(), sizeof(int) * poly_deg.size(), hipMemcpyHostToDevice));
      // hoisted coefficients of a chunk of items: every item a batch can enqueue in one list (4 per site, rounded up
      // to whole 12-item groups), <= 4 GiB.  launch_brent runs hoisting + Brent once per chunk of the list's largest
      // possible item count (4 per site), so a chunk even 4 items short of it costs an extra pair of launches per
      // list over items that do not exist (config 4's 16 384-site batches: 65 532-item chunks for 65 536, two empty
      // pairs per step).  PM_ES_CHUNK = items per chunk caps it (experiments).
      const size_t per_item = (size_t)std::max({E->max_ext * E->T, E->max_ext1 * std::max(1, E->T1), 1}) * E->poly_dcap * sizeof(double);
      const size_t want = ((size_t)4 * std::max(1, max_batch) + 11) / 12 * 12;
      E->es_chunk = (int)std::max<size_t>(1, std::min<size_t>(want, ((size_t)1 << 32) / per_item));
      if (sw.es_chunk > 0) E->es_chunk = std::min(E->es_chunk, sw.es_chunk);
      if (E->es_chunk >= 12) E->es_chunk -= E->es_chunk % 12;   // whole sites of lists 0 and 1 per chunk (grouped tasks)
      // (a full-batch chunk that does not fit -- several engines per GPU, a smaller device -- falls back to the 1 GiB
      // chunk: launch_brent loops over chunks)
      if (dalloc(&E->d_es_coef, (size_t)E->es_chunk * per_item / sizeof(double)) != PM_OK) {
        (void)hipGetLastError();
        E->es_chunk = (int)std::max<size_t>(1, std::min<size_t>(E->es_chunk, ((size_t)1 << 30) / per_item));
        if (E->es_chunk >= 12) E->es_chunk -= E->es_chunk % 12;
        DALLOC(E->d_es_coef, (size_t)E->es_chunk * per_item / sizeof(double));
      }
    }
    // workspace: the Brent grids and the posterior grid are capped so each needs <= 1 GiB
    E->grid_post = E->n_cu * 8;
    if (wsmax > 0) {
      const size_t cap = (size_t)1 << 30, per_lane = (size_t)wsmax * sizeof(double);
      const size_t per_lane_b = (size_t)wsmax * sizeof(double);   // Brent grids (EP kernels use no workspace: k_es_hoist)
      E->grid_brent = (int)std::max<size_t>(E->n_cu, std::min<size_t>(E->grid_brent, cap / (per_lane_b * T)));
      E->grid_brent = xcd_grid(E->grid_brent);   // keep the XCD-aware item order exact
      if (E->T1) {
        E->grid1 = (int)std::max<size_t>(E->n_cu, std::min<size_t>(E->grid1, cap / (per_lane_b * E->T1)));
        E->grid1 = xcd_grid(E->grid1);
      }
      E->grid_post = (int)std::max<size_t>(E->n_cu, std::min<size_t>(E->grid_post, cap / (per_lane * 256)));
      const size_t words = std::max({(size_t)E->grid_brent * T * (per_lane_b / sizeof(double)),
                                     (size_t)E->grid1 * E->T1 * (per_lane_b / sizeof(double)), (size_t)E->grid_post * 256 * wsmax});
      DALLOC(E->d_ws, words);
    }
  }
  // --- --quick_call: the unrelated plan (all persons in <=3-person founder chunks)
  if (par->quick_call) {
    std::vector<int4> uq;
    for (const pmplan::Geometry* g = pmplan::kPeeled; g->T && !E->Tq; g++)
      if (plan_units(ped, g->T, g->S, uq, true)) { E->Tq = g->T; E->Sq = g->S; }
    if (!E->Tq) { pm_engine_destroy(E); pm_set_last_error("pm_engine_create: pedigree too large for the --quick_call lane plan"); return PM_EPED; }
    E->grid_q = E->n_cu * std::max(1, 1024 / E->Tq);
    DALLOC(E->d_units_q, uq.size());
    HIP_TRY(hipMemcpy(E->d_units_q, uq.data(), sizeof(int4) * uq.size(), hipMemcpyHostToDevice));
  }
  // batch buffers
  const size_t nb = (size_t)max_batch, np = (size_t)ped->n_person;
  DALLOC(E->d_pl, nb * np * 10);
  DALLOC(E->d_stage, nb * np * 10);
  DALLOC(E->d_dm, nb * np);
  DALLOC(E->d_ref, nb);
  DALLOC(E->d_res, nb);
  DALLOC(E->d_calls, nb * np);
  DALLOC(E->d_raw, nb * 8);
  DALLOC(E->d_minv, nb * 8);
  DALLOC(E->d_evals, nb * 8);
  DALLOC(E->d_mono, nb);
  for (int l = 0; l < N_LISTS; l++) DALLOC(E->d_items[l], nb * 4);
  DALLOC(E->d_counts, 16);
  DALLOC(E->d_qctr, 8);
  DALLOC(E->d_eval_total, 1);
  DALLOC(E->d_row_site, nb);
  DALLOC(E->d_row_blk, nb / 1024 + 2);
  DALLOC(E->d_counters, 16);
  HIP_TRY(hipMemset(E->d_counters, 0, 16 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(E->d_eval_total, 0, sizeof(unsigned long long)));
  if (sw.phase_timing) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) E->wall_khz = khz;
    DALLOC(E->d_phase, 3);
    HIP_TRY(hipMemset(E->d_phase, 0, 3 * sizeof(unsigned long long)));
  }
  int rc = pm_engine_begin_section(E, PM_CHR_AUTO);
  if (rc) { pm_engine_destroy(E); return rc; }
  *out = E;
  return PM_OK;
}

int pm_engine_plan(pm_engine* E, int32_t* threads, int32_t* slots) {
  if (!E || !threads || !slots) { pm_set_last_error("pm_engine_plan: invalid arguments"); return PM_EINVAL; }
  *threads = E->T;
  *slots = E->S;
  return PM_OK;
}

int pm_engine_brent_variants(pm_engine* E, int32_t* keys, int32_t cap, int32_t* n) {
  if (!E || !n || cap < 0 || (cap > 0 && !keys)) { pm_set_last_error("pm_engine_brent_variants: invalid arguments"); return PM_EINVAL; }
  *n = (int32_t)E->brent_launched.size();
  for (int i = 0; i < std::min<int>(cap, *n); i++) {
    const pmplan::BrentKey& k = kBrentTable[E->brent_launched[i]].key;
    const int32_t v[11] = {k.T, k.S, k.NUM, k.GEN, k.ES, k.DN, k.PF, k.EP, k.QD, k.NF, k.PD};
    std::copy(v, v + 11, keys + (size_t)i * 11);
  }
  return PM_OK;
}

int pm_engine_set_posterior_carry(pm_engine* E, int32_t seen) {
  if (!E) { pm_set_last_error("pm_engine_set_posterior_carry: invalid arguments"); return PM_EINVAL; }
  E->carry_postprob = seen != 0;
  return PM_OK;
}

int pm_engine_begin_section(pm_engine* E, int32_t chrom) {
  if (!E || chrom < 0 || chrom > 3) { pm_set_last_error("pm_engine_begin_section: invalid arguments"); return PM_EINVAL; }
  E->chrom = chrom;
  E->use_plan1 = E->vcf && (chrom != PM_CHR_AUTO || E->n_fam == 1);
  if (E->use_plan1 && !E->plan1_ok) {
    pm_set_last_error("pm_engine_begin_section: vcf_mode on chrX/Y/MT (or with a single family) needs a peeling schedule "
                      "for every nuclear family (pm_pedigree.steps)");
    return PM_EPED;
  }
  // GetPolyPrior (NucFamGenotypeLikelihood.cpp:231-304)
  int n;
  if (chrom == PM_CHR_X) n = E->female_founders * 2 + E->male_founders;
  else if (chrom == PM_CHR_Y) n = E->male_founders;
  else if (chrom == PM_CHR_MT) n = E->n_founders;
  else n = 2 * E->n_founders;
  double p = 0;
  for (int i = 1; i <= n; i++) p += 1.0 / i;
  E->prior = p * E->par.theta;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipMemsetAsync(E->d_counters, 0, 16 * sizeof(unsigned long long), E->stream));
  HIP_TRY(hipStreamSynchronize(E->stream));
  return PM_OK;
}

static DevArgs make_args(pm_engine* E, int n, const uint8_t* pl, const uint32_t* dm, const uint8_t* ref, pm_site_result* res,
                         pm_geno_call* calls) {
  DevArgs A;
  memset(&A, 0, sizeof(A));
  A.n_fam = E->n_fam; A.n_person = E->n_person; A.n_fam_gt1 = E->n_fam > 1; A.single_nuclear = E->single_nuclear;
  A.max_nuc = E->max_nuc;
  A.chrom = E->chrom; A.denovo = E->par.denovo;
  A.fam_start = E->d_fam_start; A.fam_kind = E->d_fam_kind; A.sex = E->d_sex; A.fa_local = E->d_fa; A.mo_local = E->d_mo;
  A.units = E->d_units; A.T = E->T; A.S = E->S;
  A.fam_founders = E->d_fam_founders; A.is_founder = E->d_is_founder; A.peel_start = E->d_peel_start; A.steps = E->d_steps;
  A.ext_count = E->n_ext ? E->d_ext_count : nullptr; A.ext_fam = E->d_ext_fam;
  A.T10 = E->d_T10; A.T10dn = E->d_T10dn; A.ws = E->d_ws; A.ws_per_lane = E->ws_per_lane;
  A.es_poly = 0;   // set per Brent launch (launch_brent)
  A.poly_start = E->d_poly_start; A.poly_lay = E->d_poly_lay; A.poly_deg = E->d_poly_deg;
  A.poly_coef = E->poly_coef; A.poly_dcap = E->poly_dcap;
  A.es_coef = E->d_es_coef; A.es_it0 = 0; A.es_it1 = INT_MAX; A.max_ext = E->use_plan1 ? E->max_ext1 : E->max_ext;
  A.hoist_ws = E->poly_coef; A.hoist_tmp = E->hoist_tmp;
  A.es_pers = E->use_plan1 ? E->d_es_pers1 : E->d_es_pers;
  A.fam_perm = E->d_fam_perm;
  A.n_es_pers = E->use_plan1 ? E->n_es_pers1 : E->n_es_pers;
  A.theta_one = 1.0;
  A.unrelated = E->par.quick_call ? 1 : 0;   // k_prep: route sites through the quick pre-filter first
  A.vcf = E->vcf ? 1 : 0;
  if (E->use_plan1) {
    A.units = E->d_units1; A.T = E->T1; A.S = E->S1;
    A.ext_count = E->n_ext1 ? E->d_ext_count1 : nullptr; A.ext_fam = E->d_ext_fam1; A.nuc_es = 1;
  }
  A.lktab = E->d_lktab; A.M = E->d_M; A.syn = E->d_syn;
  memcpy(A.Mk, E->M_h, sizeof(A.Mk));
  A.precision = E->par.precision; A.posterior = E->par.posterior; A.theta = E->par.theta;
  A.min_total_depth = E->par.min_total_depth; A.max_total_depth = E->par.max_total_depth; A.min_map_quality = E->par.min_map_quality;
  A.min_ps = E->par.min_ps; A.denovo_min_llr = E->par.denovo_min_llr; A.log10_denovo_min_llr = log10(E->par.denovo_min_llr);
  A.force_call = E->par.force_call; A.all_sites = E->par.all_sites;
  const double pts = E->par.poly_tstv / (E->par.poly_tstv + 1), ptv = (1 - pts) / 2, prior = E->prior;
  A.lp_mono = log10(1 - prior);                  // main.cpp:450
  A.lp_ts = log10(prior * pts);                  // :469
  A.lp_tv = log10(prior * ptv);                  // :479, :489
  A.lp_other = log10(prior * 0.001);             // :509-529
  A.np_ts = log10(prior * 2. / 3.);              // :472
  A.np_tv = log10(prior * 1. / 6.);              // :482, :492
  A.n = n; A.pl = pl; A.dm = dm; A.ref = ref; A.res = res; A.calls = calls;
  A.raw = E->d_raw; A.minv = E->d_minv; A.evals = E->d_evals; A.mono_plain = E->d_mono;
  for (int l = 0; l < N_LISTS; l++) A.items[l] = E->d_items[l];
  A.counts = E->d_counts; A.eval_total = E->d_eval_total; A.phase = E->d_phase; A.row_site = E->d_row_site; A.row_blk = E->d_row_blk; A.counters = E->d_counters;
  A.carry_postprob = E->carry_postprob ? 1 : 0;
  A.itmax = E->itmax;
  A.qd_ctr = nullptr;
  A.mono_dn = pmplan::mono_dn(facts_of(E), E->sw);
  return A;
}

// The extended families of the current plan as the schedule compiler sees them (slot order e = q * T + lane).
static std::vector<pmjit::Family> jit_families(const pm_engine* E, int plan) {
  const std::vector<int>& ef = plan ? E->ext_fam1_h : E->ext_fam_h;
  std::vector<pmjit::Family> fams;
  for (size_t e = 0; e < ef.size(); e++) {
    const int f = ef[e];
    if (f < 0) continue;
    pmjit::Family F;
    F.e = (int)e;
    F.p0 = E->fam_start_h[f];
    F.n = E->fam_start_h[f + 1] - F.p0;
    F.nf = E->fam_founders_h[f];
    F.sex.assign(E->sex_h.begin() + F.p0, E->sex_h.begin() + F.p0 + F.n);
    F.founder.assign(E->founder_h.begin() + F.p0, E->founder_h.begin() + F.p0 + F.n);
    F.steps.assign(E->steps_h.begin() + E->peel_start_h[f], E->steps_h.begin() + E->peel_start_h[f + 1]);
    fams.push_back(F);
  }
  return fams;
}

// The schedule compiler's kernels for the current plan and chromosome class (es_jit.h), built on first use; nullptr
// when it is off (PM_NO_JIT) or failed to build (then the generic k_es_hoist / k_posterior_es run).
static const pmjit::Kernel* jit_kernel(pm_engine* E) {
  const int plan = E->use_plan1 ? 1 : 0, cls = E->chrom;
  if (!E->es_poly || E->sw.no_jit) return nullptr;
  int& st = E->jit_state[plan][cls];
  if (st == 0) {
    st = -1;
    const std::vector<pmjit::Family> fams = jit_families(E, plan);
    std::string err;
    pmjit::Kernel& K = E->jit[plan][cls];
    // (--denovo outside vcf_mode: every de novo item is hoisted in a grouped task, launch_brent)
    const int dmode = !E->par.denovo ? 0 : (!E->vcf && !E->sw.es_nogroup) ? 2 : 1;
    if (!fams.empty() && pmjit::build(E->device, cls, fams, kTBA, dmode, &K, &err)) {
      const size_t ns = K.slot_e.size();
      std::vector<int> tab(3 * ns + K.pair_k.size());   // slot_e | slot_sig | slot_p0 | pair_k (es_hoist_wave)
      for (size_t i = 0; i < ns; i++) { tab[i] = K.slot_e[i]; tab[ns + i] = K.slot_sig[i]; tab[2 * ns + i] = K.slot_p0[i]; }
      std::copy(K.pair_k.begin(), K.pair_k.end(), tab.begin() + 3 * ns);
      if (dalloc(&E->d_jit_slots[plan][cls], tab.size()) == PM_OK &&
          hipMemcpy(E->d_jit_slots[plan][cls], tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice) == hipSuccess)
        st = 1;
    } else if (!fams.empty())
      fprintf(stderr, "polymutt: peeling-schedule compiler unavailable (%s); using the generic hoisting kernel\n", err.c_str());
  }
  return st == 1 ? &E->jit[plan][cls] : nullptr;
}

// The fused hoisting + Brent kernel for the current plan and class (bi-allelic engines, every family peeled), built on
// first use; nullptr when off (PM_NO_FUSED, PM_NO_JIT) or unavailable (then es_hoist_jit + k_brent run).
static const pmjit::FusedKernel* fused_kernel(pm_engine* E) {
  const int plan = E->use_plan1 ? 1 : 0, cls = E->chrom;
  if (!E->es_poly || E->sw.no_jit || E->sw.no_fused) return nullptr;
  int& st = E->fused_state[plan][cls];
  if (st == 0) {
    st = -1;
    const std::vector<pmjit::Family> fams = jit_families(E, plan);
    std::string err;
    pmjit::FusedKernel& F = E->fused[plan][cls];
    if (!fams.empty() && pmjit::build_fused(E->device, cls, fams, kTBA, &F, &err) && F.blocks_per_cu > 0) {
      if (dalloc(&E->d_fused_tab[plan][cls], F.lane_tab.size()) == PM_OK &&
          hipMemcpy(E->d_fused_tab[plan][cls], F.lane_tab.data(), sizeof(int) * F.lane_tab.size(), hipMemcpyHostToDevice) == hipSuccess)
        st = 1;
    } else if (!fams.empty() && E->sw.jit_layout)
      fprintf(stderr, "polymutt: fused Brent kernel unavailable (%s); hoisting + k_brent\n", err.c_str());
  }
  return st == 1 ? &E->fused[plan][cls] : nullptr;
}

// HIP events around a launch (pm_kernel_stats reports Brent and EP hoisting launches apart): begin pushes a fresh pair
// and records its first event, end records the last pair's second
static int mark(pm_engine* E, std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, bool begin) {
  if (begin) {
    v.push_back({nullptr, nullptr});
    HIP_TRY(hipEventCreate(&v.back().first));
    HIP_TRY(hipEventCreate(&v.back().second));
  }
  HIP_TRY(hipEventRecord(begin ? v.back().first : v.back().second, E->stream));
  return PM_OK;
}

// Blocks of a one-wave k_brent instantiation resident per CU (occupancy query on first use).
static int resident_blocks(pm_engine* E, BrentFn fn, int T, size_t lds) {
  for (auto& c : E->bpc)
    if (c.first == (const void*)fn) return c.second;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)fn, T, lds) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    n = 1024 / T;
  }
  E->bpc.push_back({(const void*)fn, n});
  return n;
}

// One k_brent launch between its pair of events; the instantiation is noted for pm_engine_brent_variants.
static int launch_plain(pm_engine* E, BrentFn fn, int grid, int T, size_t lds, const DevArgs& A, int list) {
  for (int i = 0; i < (int)(sizeof(kBrentTable) / sizeof(kBrentTable[0])); i++)
    if (kBrentTable[i].fn == fn && std::find(E->brent_launched.begin(), E->brent_launched.end(), i) == E->brent_launched.end())
      E->brent_launched.push_back(i);
  if (int rc = mark(E, E->brent_events, true)) return rc;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(T), lds, E->stream, A, list);
  HIP_TRY(hipGetLastError());
  return mark(E, E->brent_events, false);
}

// Bi-allelic engines whose every family is peeled (config 4): one fused launch per list -- each lane hoists its
// families' polynomials into registers and the wave runs the item's Brent (es_jit.h ep_brent_jit)
static int launch_fused(pm_engine* E, const pmjit::FusedKernel* FK, const DevArgs& A, int list) {
  E->es_ops_known = true;   // (finish_batch: every item is bi-allelic, o[0] = one item's hoisting over every family)
  for (int v = 0; v < 6; v++) E->es_item_ops[v] = v == 0 ? FK->item_ops : 0.0;
  pmjit::FusedArgs F;
  F.items = A.items[list]; F.counts = A.counts; F.ref = A.ref; F.res = (const int*)A.res; F.pl = A.pl; F.lktab = A.lktab;
  F.lane_tab = E->d_fused_tab[E->use_plan1 ? 1 : 0][E->chrom];
  F.raw = A.raw; F.minv = A.minv; F.evals = A.evals; F.eval_total = A.eval_total; F.precision = A.precision;
  F.list = list; F.it0 = 0; F.it1 = INT_MAX; F.np = A.n_person; F.vcf = A.vcf; F.res_words = sizeof(pm_site_result) / 4;
  F.res_a1 = offsetof(pm_site_result, allele1) / 4; F.res_a2 = offsetof(pm_site_result, allele2) / 4;
  F.itmax = A.itmax; F.pad = 0;
  void* params[] = {&F};
  if (int rc = mark(E, E->brent_events, true)) return rc;
  // (PM_FUSED_ROUNDS rounds of the resident blocks: measured)
  HIP_TRY(hipModuleLaunchKernel(FK->fn, xcd_grid(E->n_cu * FK->blocks_per_cu * E->sw.fused_rounds), 1, 1, 64, 1, 1, 0, E->stream, params,
                                nullptr));
  return mark(E, E->brent_events, false);
}

// Extended families in polynomial form, in chunks of the list (the coefficient buffer holds es_chunk items): the hoisting
// (the schedule compiler's kernel, else k_es_hoist), then the chunk's Brent items
static int launch_ep_chunks(pm_engine* E, BrentFn fn, int grid, int T, size_t lds, DevArgs A, int list) {
  void (*hoist)(DevArgs, int) = A.denovo ? k_es_hoist<true> : k_es_hoist<false>;
  const size_t hlds = (size_t)E->hoist_waves * (E->poly_coef + E->hoist_tmp) * sizeof(double);
  if (hlds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)hoist, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hlds));
  const size_t stat = (256 + 5 * 27 + (A.denovo ? 2000 : 2)) * sizeof(double);
  const int hgrid = E->n_cu * std::max(1, std::min(8, (int)((160 * 1024) / (hlds + stat))));
  const int max_items = 4 * E->last_n;
  const pmjit::Kernel* K = jit_kernel(E);
  E->es_ops_known = K != nullptr;
  for (int v = 0; v < 6 && K; v++) {   // one item's hoisting ops over the plan's extended families (slot shapes), by variant
    E->es_item_ops[v] = 0;
    for (int sg : K->slot_sig) E->es_item_ops[v] += K->shape_ops[v].empty() ? 0.0 : K->shape_ops[v][sg];
  }
  for (int it0 = 0; it0 < max_items; it0 += E->es_chunk) {
    A.es_it0 = it0;
    A.es_it1 = (int)std::min<long long>((long long)it0 + E->es_chunk, INT_MAX);
    if (int rc = mark(E, E->es_events, true)) return rc;
    if (K) {   // compiled schedule: one thread (--denovo: one wave) per (item, family)
      const int plan = E->use_plan1 ? 1 : 0, ns = (int)K->slot_e.size();
      const int* tab = E->d_jit_slots[plan][E->chrom];
      pmjit::Args J;
      J.items = A.items[list]; J.counts = A.counts; J.ref = A.ref; J.res = (const int*)A.res; J.pl = A.pl; J.lktab = A.lktab;
      J.coef = A.es_coef; J.slot_e = tab; J.slot_sig = tab + ns; J.slot_p0 = tab + 2 * ns;
      J.pair_k = tab + 3 * ns; J.npairs = (int)K->pair_k.size() / 2;
      J.T10 = E->d_T10; J.T10dn = E->d_T10dn; J.tba = E->d_tba;
      J.list = list; J.it0 = A.es_it0; J.it1 = A.es_it1; J.nslots = ns; J.np = A.n_person; J.T = A.T; J.max_ext = A.max_ext;
      J.dcap = A.poly_dcap; J.vcf = A.vcf; J.res_words = sizeof(pm_site_result) / 4;
      J.res_a1 = offsetof(pm_site_result, allele1) / 4; J.res_a2 = offsetof(pm_site_result, allele2) / 4;
      J.denovo = A.denovo;
      J.prof = nullptr;
      if (E->sw.es_prof) {
        if (!E->d_es_prof) {
          if (int r = dalloc(&E->d_es_prof, 5)) return r;
          HIP_TRY(hipMemset(E->d_es_prof, 0, 5 * sizeof(unsigned long long)));
        }
        J.prof = E->d_es_prof;
      }
      // a site's de novo items are consecutive in lists 0 (cfgs 0-3, or 1-3 when k_prep / the QUAD item takes the
      // monomorphism) and 1 (cfgs 4-6): one task takes them together, the 10-state leaf steps once
      J.group = 0;
      if (K->wave && A.denovo && !A.vcf && !E->sw.es_nogroup) {
        if (list == 0) J.group = A.mono_dn ? 3 : 4;
        else if (list == 1) J.group = 3;
      }
      if (list == 0) E->es_grouped = J.group > 1;   // (finish_batch's op count: lists 0 and 1 group alike)
      void* params[] = {&J};
      if (K->wave)
        HIP_TRY(hipModuleLaunchKernel(K->fn, E->n_cu * (K->blocks_per_cu > 0 ? K->blocks_per_cu : std::max(1, 16 / K->wpb)), 1, 1,
                                      64 * K->wpb, 1, 1, 0, E->stream, params, nullptr));
      else
        HIP_TRY(hipModuleLaunchKernel(K->fn, E->n_cu * 8, 1, 1, 256, 1, 1, 0, E->stream, params, nullptr));
    } else hipLaunchKernelGGL(hoist, dim3(hgrid), dim3(64 * E->hoist_waves), hlds, E->stream, A, list);
    HIP_TRY(hipGetLastError());
    if (int rc = mark(E, E->es_events, false)) return rc;
    if (int rc = launch_plain(E, fn, grid, T, lds, A, list)) return rc;
  }
  return PM_OK;
}

// One list's Brent items: select the kernel (brent_plan.h), resolve it, adjust launch to the device, launch.
static int launch_brent(pm_engine* E, const DevArgs& A0, int list, bool unrelated = false) {
  DevArgs A = A0;
  const pmplan::EngineSwitches& sw = E->sw;
  const int align = ((uintptr_t)A.pl & 15) == 0 ? 16 : ((uintptr_t)A.pl & 3) == 0 ? 4 : 1;
  const pmplan::BrentChoice c = pmplan::brent_select(facts_of(E), sw, list, unrelated, align);
  const int T = c.key.T, S = c.key.S;
  int grid = unrelated ? E->grid_q : E->use_plan1 ? E->grid1 : E->grid_brent;
  size_t shmem = c.lds;
  if (unrelated) { A.units = E->d_units_q; A.T = T; A.S = S; A.ext_count = nullptr; A.denovo = 0; }
  A.unrelated = unrelated ? 1 : 0;
  A.pf_npad = c.pf_npad; A.pf_stride = c.pf_stride; A.pf_dw = c.pf_dw; A.dn_pf = c.dn_pf; A.qd_group = c.qd_group; A.quad_full = E->quad_full;
  BrentFn fn = nullptr;
  for (const auto& v : kBrentTable)
    if (v.key == c.key) fn = v.fn;
  if (!fn) { pm_set_last_error("launch_brent: no kernel variant for the lane plan"); return PM_EINVAL; }
  if (c.quad) {   // persistent grid = the blocks that are resident at once (PM_QD_WAVES per SIMD): no partial second round
    const int bpc = sw.qd_bpc ? sw.qd_bpc : resident_blocks(E, fn, 64, shmem);
    // PM_QD_ROUNDS = R rounds of them keep a site's three items closer in one XCD's L2 (less traffic, a faster launch)
    // but cost the three-engine wall rate 1.5%, so R = 1; PM_QD_DYN=1, the per-XCD claimed item order (k_brent qd_ctr),
    // is slower ("Headline traffic explained": profiles/r06l_*, r06n_*, r06o_*)
    if (sw.qd_dyn && A.qd_group == 1) {
      HIP_TRY(hipMemsetAsync(E->d_qctr, 0, 8 * sizeof(int), E->stream));
      A.qd_ctr = E->d_qctr;
    }
    grid = xcd_grid(E->n_cu * bpc * (sw.qd_bpc ? 1 : sw.qd_rounds));   // (the XCD-aware item order)
  }
  // multi-wave de novo plans (T = 512 / 1024: more than 1024 families) stage 2 buffers per wave: above the
  // default 64 KB dynamic-LDS limit the kernel must opt in, and the block (plus its static LDS: lane plan,
  // tables) must fit one CU's 160 KB; otherwise the same kernel hoists from direct loads
  if (A.dn_pf && !(T == 64 && S == 16)) {
    const size_t stat = (size_t)S * T * 4 + 256 * 8 + 100 * 8 + 96 * 8 + 32 * 4;
    bool ok = shmem + stat <= 160 * 1024;
    if (ok && shmem > 64 * 1024)
      ok = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); A.dn_pf = 0; shmem = 0; }
  }
  // Elston-Stewart workspace in LDS: every partial / marriage-partial access of the peel becomes an LDS round
  // trip instead of an L2 one.  Blocks per CU follow from the LDS budget (160 KB per CU).
  A.ws_lds = 0;
  if (c.ep) {   // polynomial-form peels: coefficients from k_es_hoist, no workspace in k_brent
    A.es_poly = 1;
    A.ep_only = c.ep_only;
  } else if (c.key.ES && !E->par.denovo) {   // BA peels (the 10-state one is too big)
    const size_t need = (size_t)E->ws_per_lane * T * sizeof(double);
    if (need > 0 && need <= 150 * 1024) {
      if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need) == hipSuccess) {
        A.ws_lds = 1;
        shmem = need;
        grid = E->n_cu * std::max(1, std::min(1024 / T, (int)((160 * 1024) / (need + 8 * 1024))));
      } else (void)hipGetLastError();
    }
  }
  // EP one-wave plans: a persistent grid of exactly the resident blocks (no partial second round)
  if (c.ep && T == 64) grid = xcd_grid(std::min(grid, E->n_cu * resident_blocks(E, fn, T, shmem)));
  // lean PF kernels: PM_PF_ROUNDS x the default grid (2 rounds of the resident blocks).  One-wave quad plans take 4:
  // their planes are re-read from L2 (+1.5-3.7%, profiles/r06m_*); trio plans lost 2% with it (r06p_*) and the two-wave
  // 128 x 16 plans gained nothing: 1 (same paragraph)
  if (A.pf_npad > 0 && !c.ep) grid = xcd_grid(grid * (sw.pf_rounds ? sw.pf_rounds : (T == 64 && !E->all_trio) ? 4 : 1));
  const pmjit::FusedKernel* FK = (c.ep_only && !A.denovo && T == 64) ? fused_kernel(E) : nullptr;
  if (FK) return launch_fused(E, FK, A, list);
  if (c.ep) return launch_ep_chunks(E, fn, grid, T, shmem, A, list);
  return launch_plain(E, fn, grid, T, shmem, A, list);
}

// The de novo Brent item of every called site of a vcf_mode batch (three-genotype mutation model, vcf_denovo_dev.h) and the
// four result fields it fills; timed with the Brent launches (pm_kernel_stats).  brent: k_vdn_brent or k_vdn_brent_x of
// T threads on the term list V.  (Templates over the kernel and its term list: C++ linkage inside this file's extern "C".)
extern "C++" template <class K, class VA>
static int launch_vdn_brent(pm_engine* E, const DevArgs& A, K brent, int max_grid, int T, size_t lds, const VA& V) {
  const int grid = std::max(1, std::min(max_grid, A.n));
  if (int rc = mark(E, E->brent_events, true)) return rc;
  hipLaunchKernelGGL(brent, dim3(grid), dim3(T), lds, E->stream, A, V);
  HIP_TRY(hipGetLastError());
  if (int rc = mark(E, E->brent_events, false)) return rc;
  hipLaunchKernelGGL(k_finalize_vdn, dim3((A.n + 255) / 256), dim3(256), 0, E->stream, A);
  HIP_TRY(hipGetLastError());
  return PM_OK;
}

// pm_engine_set_vcf_denovo_detail's buffers and the autosomal children (chrX: launch_vcf_denovo_x puts its own in)
static VdnWhoArgs vdn_who_args(const pm_engine* E) {
  VdnWhoArgs W;
  W.fam_k = E->vw_fam_k; W.car_k = E->vw_car_k; W.row_site = E->d_vw_row_site;
  W.fam_top = E->d_vw_fam_top; W.fam_sum = E->d_vw_fam_sum; W.fam_all = E->d_vw_fam_all; W.fam_line = E->d_vw_fam_line;
  W.pfam = E->d_vw_pfam; W.car_top = E->d_vw_car_top; W.car_all = E->d_vw_car_all; W.car_line = E->d_vw_car_line;
  W.kids = E->d_vw_kids; W.n_nuc = E->vw_n_nuc; W.n_es = E->vw_n_es; W.is_kid = E->d_vw_is_kid; W.jbuf = E->d_vw_jbuf;
  return W;
}

// The rows (DQ at or above the threshold), then their families and children.  who: k_vdn_who or k_vdn_who_x of T threads;
// blocks beyond the row count leave at once.
extern "C++" template <class K, class VA>
static int launch_vdn_who(pm_engine* E, const DevArgs& A, K who, int max_grid, int T, const VA& V, const VdnWhoArgs& W) {
  hipLaunchKernelGGL(k_vdn_rows, dim3(1), dim3(1024), 0, E->stream, A, E->d_vw_row_site);
  HIP_TRY(hipGetLastError());
  const int wgrid = std::max(1, std::min(max_grid, A.n));
  hipLaunchKernelGGL(who, dim3(wgrid), dim3(T), 0, E->stream, A, V, W);
  HIP_TRY(hipGetLastError());
  return PM_OK;
}

// An autosomal section (pm_engine_set_vcf_denovo), and with pm_engine_set_vcf_denovo_detail on the rows and k_vdn_who.
static int launch_vcf_denovo(pm_engine* E, const DevArgs& A) {
  VdnArgs V;
  V.terms = E->d_vdn_terms; V.n_terms = E->vdn_terms; V.n_peel = E->vdn_peel; V.n_nuc = E->vdn_nuc;
  V.co_lds = E->vdn_lds > 0; V.co = E->d_vdn_co; V.ws = E->d_vdn_ws;
  if (int rc = launch_vdn_brent(E, A, E->vdn_T == 64 ? k_vdn_brent<64> : k_vdn_brent<256>, E->vdn_grid, E->vdn_T, E->vdn_lds, V)) return rc;
  if (E->vw_fam_k <= 0 && E->vw_car_k <= 0) return PM_OK;
  // (the peel workspace is k_vdn_brent's, sized for vdn_grid >= vw_grid blocks)
  return launch_vdn_who(E, A, E->vdn_T == 64 ? k_vdn_who<64> : k_vdn_who<256>, E->vw_grid, E->vdn_T, V, vdn_who_args(E));
}

// The same on a chrX section (pm_engine_set_vcf_denovo_chrx): k_vdn_brent_x on its own terms and workspace, then
// k_finalize_vdn as it is.  No detail rows on X (counts[10] stays 0) unless pm_engine_set_vcf_denovo_chrx_detail is on:
// then k_vdn_rows as it is and k_vdn_who_x into the detail's buffers.
static int launch_vcf_denovo_x(pm_engine* E, const DevArgs& A) {
  VdnXArgs V;
  V.terms = E->d_vdnx_terms; V.n_terms = E->vdnx_terms; V.n_peel = E->vdnx_peel; V.ws = E->d_vdnx_ws;
  for (int i = 0; i < 16; i++) V.a4[i] = E->A4_h[i];
  if (int rc = launch_vdn_brent(E, A, E->vdnx_T == 64 ? k_vdn_brent_x<64> : k_vdn_brent_x<256>, E->vdnx_grid, E->vdnx_T, 0, V)) return rc;
  if (!E->vwx_on) return PM_OK;
  VdnWhoArgs W = vdn_who_args(E);
  W.kids = E->d_vwx_kids; W.n_nuc = 0; W.n_es = E->vwx_n_kids; W.is_kid = E->d_vwx_is_kid; W.jbuf = E->d_vwx_jbuf;
  // (vwx_grid <= vdnx_grid, the blocks of k_vdn_brent_x's workspace, and <= vw_grid, the blocks of the detail's lines)
  return launch_vdn_who(E, A, E->vdnx_T == 64 ? k_vdn_who_x<64> : k_vdn_who_x<256>, E->vwx_grid, E->vdnx_T, V, W);
}

// The launch shape of a peel kernel that needs ws_per_lane doubles of workspace per thread.  The workspace goes to dynamic
// LDS when a block's share fits the 64 KB default dynamic-LDS limit: bt is the largest of 256 / 128 / 64 threads that does,
// the grid twice the blocks that 160 KB of LDS per CU hold (3 KB of static LDS and padding per block).  bt = 0 (nothing
// fits, or PM_ES_POST_HBM): the kernel's HBM-workspace form at grid_post x 256.
struct EsShape { int bt, grid; size_t lds_bytes; };
static EsShape es_block_shape(const pm_engine* E, int ws_per_lane) {
  const size_t per = (size_t)ws_per_lane * sizeof(double);
  for (int t : {256, 128, 64})
    if (per * t <= 64 * 1024 && !E->sw.es_post_hbm) {
      const int per_cu = std::max(1, (int)((160 * 1024) / (per * t + 3 * 1024)));
      return {t, E->n_cu * per_cu * 2, per * t};
    }
  return {0, E->grid_post, 0};
}

// One plane's pass over a vcf_mode batch's rows, behind the standard posterior stage and with that stage's routing: the
// lean kernel (lean_lds bytes of family table) where k_posterior_lean ran, else the nuc kernel, both at the stage's grid;
// then, where the section has peeled families (es) and the plane's list n_items entries, the plane's peel kernel at shape
// sh, its HBM form at hbm_grid blocks.  (A template over the plane's args: C++ linkage inside this file's extern "C".)
extern "C++" template <class PA>
static int launch_plane_pass(pm_engine* E, const DevArgs& A, const PA& P, bool lean, void (*k_lean)(DevArgs, PA), size_t lean_lds,
                             void (*k_nuc)(DevArgs, PA), bool es, int n_items, void (*k_es_lds)(DevArgs, PA),
                             void (*k_es_hbm)(DevArgs, PA), const EsShape& sh, int hbm_grid) {
  if (lean) hipLaunchKernelGGL(k_lean, dim3(E->grid_post), dim3(256), lean_lds, E->stream, A, P);
  else hipLaunchKernelGGL(k_nuc, dim3(E->grid_post), dim3(256), 0, E->stream, A, P);
  HIP_TRY(hipGetLastError());
  if (es && n_items > 0) {
    if (sh.bt) hipLaunchKernelGGL(k_es_lds, dim3(sh.grid), dim3(sh.bt), sh.lds_bytes, E->stream, A, P);
    else hipLaunchKernelGGL(k_es_hbm, dim3(hbm_grid), dim3(256), 0, E->stream, A, P);
    HIP_TRY(hipGetLastError());
  }
  return PM_OK;
}

// The posterior plane (vcf_post_dev.h), on every chromosome class.
static int launch_vcf_posteriors(pm_engine* E, const DevArgs& A, bool lean, bool es) {
  VpArgs P;
  P.post = (pm_vcf_post*)E->vp.d;
  if (int rc = launch_plane_pass(E, A, P, lean, k_vcf_post_lean, (size_t)E->n_fam * 4, k_vcf_post_nuc, es, A.n_es_pers, k_vcf_post_es<true>,
                                 k_vcf_post_es<false>, es_block_shape(E, E->ws_per_lane), E->grid_post))
    return rc;
  E->vp.valid = true;
  return PM_OK;
}

// The transmission phase plane (vcf_phase_dev.h).  Sections that are not autosomal have no phase: their plane is cleared.
static int launch_vcf_phase(pm_engine* E, const DevArgs& A, bool lean, bool es) {
  E->vph.valid = true;
  if (E->chrom != PM_CHR_AUTO) {
    HIP_TRY(hipMemsetAsync(E->vph.d, 0, sizeof(pm_vcf_phase) * (size_t)E->max_batch * E->n_person, E->stream));
    return PM_OK;
  }
  const int plan = E->use_plan1 ? 1 : 0;
  VphArgs P;
  P.phase = (pm_vcf_phase*)E->vph.d; P.kids = E->vph_kids.d[plan]; P.n_kids = (int)E->vph_kids.h[plan].size();
  return launch_plane_pass(E, A, P, lean, k_vcf_phase_lean, (size_t)E->n_fam * 5, k_vcf_phase_nuc, es, P.n_kids, k_vcf_phase_es<true>,
                           k_vcf_phase_es<false>, es_block_shape(E, E->ws_per_lane), E->grid_post);
}

// The joint call plane (vcf_joint_dev.h), its peel at this pass's own workspace size and HBM grid.  Sections that are not
// autosomal have no joint calls: their plane is filled with (g = 255, lp = 0).
static int launch_vcf_joint(pm_engine* E, const DevArgs& A, bool lean, bool es) {
  E->vj.valid = true;
  if (E->chrom != PM_CHR_AUTO) {
    hipLaunchKernelGGL(k_vcf_joint_none, dim3(E->grid_post), dim3(256), 0, E->stream, (pm_vcf_joint*)E->vj.d, (size_t)E->max_batch * E->n_person);
    HIP_TRY(hipGetLastError());
    return PM_OK;
  }
  const int plan = E->use_plan1 ? 1 : 0;
  VjArgs P;
  P.joint = (pm_vcf_joint*)E->vj.d; P.fams = E->vj_fams.d[plan]; P.n_fams = (int)E->vj_fams.h[plan].size();
  P.ws = E->d_vj_ws; P.ws_per_lane = E->vj_ws_per_lane;
  return launch_plane_pass(E, A, P, lean, k_vcf_joint_lean, (size_t)E->n_fam * 4, k_vcf_joint_nuc, es, P.n_fams, k_vcf_joint_es<true>,
                           k_vcf_joint_es<false>, es_block_shape(E, E->vj_ws_per_lane), E->vj_grid);
}

// The pedigree check's pass (vcf_pedcheck_dev.h) over an autosomal batch's rows, routed as the planes' passes are.  Every
// kernel's threads own a family or child over a stripe of rows: blocks enough for eight rows per thread when every site of
// the batch is written, within the stage's grid (the peel's HBM workspace holds that many blocks' lanes).
static int launch_vcf_pedcheck(pm_engine* E, const DevArgs& A, int n, bool lean, bool es) {
  const int plan = E->use_plan1 ? 1 : 0;
  VpcArgs P;
  P.acc = E->d_pc_acc; P.slot = E->d_pc_slot; P.kids = nullptr; P.n_kids = 0;
  auto grid_for = [&](int items, int bt, int cap) {
    const int row_lanes = std::max(1, bt / std::max(1, std::min(items, bt)));
    return std::max(1, std::min(cap, (n + row_lanes * 8 - 1) / (row_lanes * 8)));
  };
  if (lean) {
    hipLaunchKernelGGL(k_vcf_pedcheck_lean, dim3(grid_for(E->n_fam, 256, E->grid_post)), dim3(256), 0, E->stream, A, P);
    HIP_TRY(hipGetLastError());
  } else if (!E->pc_nuc_kids.h[plan].empty()) {
    P.kids = E->pc_nuc_kids.d[plan]; P.n_kids = (int)E->pc_nuc_kids.h[plan].size();
    hipLaunchKernelGGL(k_vcf_pedcheck_nuc, dim3(grid_for(P.n_kids, 256, E->grid_post)), dim3(256), 0, E->stream, A, P);
    HIP_TRY(hipGetLastError());
  }
  if (es && !E->vph_kids.h[plan].empty()) {
    P.kids = E->vph_kids.d[plan]; P.n_kids = (int)E->vph_kids.h[plan].size();
    const EsShape sh = es_block_shape(E, E->ws_per_lane + 4);   // (+ 4: the block's sums behind the workspace)
    if (sh.bt) hipLaunchKernelGGL(k_vcf_pedcheck_es<true>, dim3(grid_for(P.n_kids, sh.bt, sh.grid)), dim3(sh.bt), sh.lds_bytes, E->stream, A, P);
    else hipLaunchKernelGGL(k_vcf_pedcheck_es<false>, dim3(grid_for(P.n_kids, 256, E->grid_post)), dim3(256), 0, E->stream, A, P);
    HIP_TRY(hipGetLastError());
  }
  return PM_OK;
}

static int run_pipeline(pm_engine* E, int n, const uint8_t* pl, const uint32_t* dm, const uint8_t* ref, pm_site_result* res,
                        pm_geno_call* calls) {
  DevArgs A = make_args(E, n, pl, dm, ref, res, calls);
  E->last_n = n;
  HIP_TRY(hipMemsetAsync(E->d_counts, 0, 16 * sizeof(int), E->stream));
  {
    // counts[4] = first emitted site, counts[6] = first stuck site (both atomicMin); counts[5] = any stuck
    static const int init[3] = {0x7fffffff, 0, 0x7fffffff};
    HIP_TRY(hipMemcpyAsync(E->d_counts + 4, init, sizeof(init), hipMemcpyHostToDevice, E->stream));
  }
  {   // persons per lane of k_prep: vector loads when n_person allows; the reference's serial mono order in EXACT
    const int np = E->n_person;
    int vmax = 8;   // measured best on 1000 quads (16 and 4 within 1%)
    // (the de novo monomorphism path compiled in only for engines that form it here: mono_dn == 1; vcf_mode never does)
    const bool mdn = A.mono_dn == 1 && !E->vcf;
    void (*prep)(DevArgs, int) = E->par.numerics == PM_NUM_EXACT ? (E->vcf ? k_prep<1, true, true, false> : mdn ? k_prep<1, true> : k_prep<1, true, false, false>)
                          : E->vcf ? ((np % 16 == 0 && vmax >= 16) ? k_prep<16, false, true, false> : (np % 8 == 0 && vmax >= 8) ? k_prep<8, false, true, false>
                                      : (np % 4 == 0 && vmax >= 4) ? k_prep<4, false, true, false> : k_prep<1, false, true, false>)
                          : mdn ? ((np % 16 == 0 && vmax >= 16) ? k_prep<16, false> : (np % 8 == 0 && vmax >= 8) ? k_prep<8, false>
                                   : (np % 4 == 0 && vmax >= 4) ? k_prep<4, false> : k_prep<1, false>)
                          : (np % 16 == 0 && vmax >= 16) ? k_prep<16, false, false, false> : (np % 8 == 0 && vmax >= 8) ? k_prep<8, false, false, false>
                          : (np % 4 == 0 && vmax >= 4) ? k_prep<4, false, false, false> : k_prep<1, false, false, false>;
    // sites per wave: PREP_SPW (PM_PREP_SPW = 1..8 overrides it; fewer sites per wave on config 4's 16 384-site
    // batches measured slower: 20.3 -> 19.7 M sites/s at 1, config 5 within noise, profiles/r05sp_ab_prep_spw.txt)
    int spw = PREP_SPW;
    if (E->sw.prep_spw) spw = std::min(PREP_SPW, E->sw.prep_spw);
    hipLaunchKernelGGL(prep, dim3((n + 4 * spw - 1) / (4 * spw)), dim3(256), 0, E->stream, A, spw);
  }
  HIP_TRY(hipGetLastError());
  int rc;
  const int tb = 256, gb = (n + tb - 1) / tb;
  if (E->par.quick_call) {   // main.cpp:354-437 on lists 1 and 2, survivors -> list 0
    if ((rc = launch_brent(E, A, 1, true))) return rc;
    hipLaunchKernelGGL(k_quick_select, dim3(gb), dim3(tb), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_brent(E, A, 2, true))) return rc;
    hipLaunchKernelGGL(k_quick_final, dim3(gb), dim3(tb), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_quick_stats, dim3(1), dim3(1), 0, E->stream, A);
    HIP_TRY(hipMemsetAsync(E->d_counts + 1, 0, 2 * sizeof(int), E->stream));
  }
  if ((rc = launch_brent(E, A, 0))) return rc;
  if (E->vcf) {
    hipLaunchKernelGGL(k_finalize_vcf, dim3(gb), dim3(tb), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
    if (E->vdn_on && E->chrom == PM_CHR_AUTO && (rc = launch_vcf_denovo(E, A))) return rc;
    if (E->vdnx_on && E->chrom == PM_CHR_X && (rc = launch_vcf_denovo_x(E, A))) return rc;
  } else {
    hipLaunchKernelGGL(k_select, dim3(gb), dim3(tb), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_brent(E, A, 1))) return rc;
    hipLaunchKernelGGL(k_finalize, dim3(gb), dim3(tb), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
  }
  if (E->par.denovo) {
    if ((rc = launch_brent(E, A, 2))) return rc;
    hipLaunchKernelGGL(k_final_dn, dim3(gb), dim3(tb), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
  }
  {
    const int nb = std::max(1, (n + 1023) / 1024);
    hipLaunchKernelGGL(k_rows_count, dim3(nb), dim3(1024), 0, E->stream, A);
    hipLaunchKernelGGL(k_rows, dim3(nb), dim3(1024), 0, E->stream, A);
  }
  HIP_TRY(hipGetLastError());
  {
    const bool es = (E->use_plan1 ? E->n_ext1 : E->n_ext) > 0;
    // k_posterior_lean: its LDS family table packs first person (24 bits) and persons (7 bits), <= 48 KB
    const bool lean = !E->par.denovo && !es && E->chrom == PM_CHR_AUTO && E->max_nuc <= 4 && !E->use_plan1 &&
                      E->n_fam <= 12288 && E->max_fam <= 127 && E->n_person < (1 << 24);
    void (*post)(DevArgs) = E->par.denovo ? (es ? k_posterior<true, true> : k_posterior<true, false>)
                          : es ? k_posterior<false, true> : lean ? (E->vcf ? k_posterior_lean<true> : k_posterior_lean<false>)
                                                                 : k_posterior<false, false>;
    hipLaunchKernelGGL(post, dim3(E->grid_post), dim3(256), lean ? (size_t)E->n_fam * 4 : 0, E->stream, A);
    const pmjit::Kernel* K = es && A.n_es_pers > 0 ? jit_kernel(E) : nullptr;
    if (K && K->fn_post) {   // compiled schedule: one thread per (row, peeled family), all its persons' 3 peels in registers
      HIP_TRY(hipGetLastError());
      const int plan = E->use_plan1 ? 1 : 0, ns = (int)K->slot_e.size();
      const int* tab = E->d_jit_slots[plan][E->chrom];
      void* thr = nullptr;
      HIP_TRY(hipGetSymbolAddress(&thr, HIP_SYMBOL(c_gq_thr)));
      pmjit::PostArgs P;
      P.counts = A.counts; P.row_site = A.row_site; P.res = (const char*)A.res; P.pl = A.pl; P.lktab = A.lktab;
      P.gq_thr = (const double*)thr; P.calls = (void*)A.calls; P.fam_p0 = tab + 2 * ns; P.fam_sig = tab + ns;
      P.nfams = ns; P.np = A.n_person; P.vcf = A.vcf; P.res_bytes = sizeof(pm_site_result);
      P.off_a1 = offsetof(pm_site_result, allele1); P.off_a2 = offsetof(pm_site_result, allele2);
      P.off_maxidx = offsetof(pm_site_result, maxidx); P.off_af = offsetof(pm_site_result, af);
      P.theta = A.theta;
      void* params[] = {&P};
      HIP_TRY(hipModuleLaunchKernel(K->fn_post, E->n_cu * 8, 1, 1, 256, 1, 1, 0, E->stream, params, nullptr));
    } else if (es && A.n_es_pers > 0) {
      HIP_TRY(hipGetLastError());
      const EsShape sh = es_block_shape(E, E->ws_per_lane);
      if (sh.bt) {
        void (*pe)(DevArgs) = E->par.denovo ? k_posterior_es<true, true> : k_posterior_es<false, true>;
        hipLaunchKernelGGL(pe, dim3(sh.grid), dim3(sh.bt), sh.lds_bytes, E->stream, A);
      } else
        hipLaunchKernelGGL(E->par.denovo ? k_posterior_es<true> : k_posterior_es<false>, dim3(sh.grid), dim3(256), 0, E->stream, A);
    }
    if (E->vp.on) {
      HIP_TRY(hipGetLastError());
      if ((rc = launch_vcf_posteriors(E, A, lean, es))) return rc;
    }
    if (E->vph.on) {
      HIP_TRY(hipGetLastError());
      if ((rc = launch_vcf_phase(E, A, lean, es))) return rc;
    }
    if (E->vj.on) {
      HIP_TRY(hipGetLastError());
      if ((rc = launch_vcf_joint(E, A, lean, es))) return rc;
    }
    if (E->pc_on && E->chrom == PM_CHR_AUTO) {
      HIP_TRY(hipGetLastError());
      if ((rc = launch_vcf_pedcheck(E, A, n, lean, es))) return rc;
    }
  }
  HIP_TRY(hipGetLastError());
  if (!E->par.denovo && E->chrom == PM_CHR_AUTO && !E->vcf) {
    hipLaunchKernelGGL(k_ab, dim3(E->n_cu * 8), dim3(256), 0, E->stream, A);
    HIP_TRY(hipGetLastError());
  }
  if (E->fam_top_k > 0) {   // per-family de novo evidence of the written rows (after k_final_dn and k_rows)
    FamLrArgs F;
    F.top_k = E->fam_top_k; F.sum = E->d_fam_sum; F.top = E->d_fam_top; F.all = E->d_fam_all; F.line = E->d_fam_line;
    // (blocks beyond the row count leave at once; the ES instantiation's peel workspace is d_ws, sized for grid_post blocks)
    const int grid = std::max(1, std::min(E->fam_grid, n));
    hipLaunchKernelGGL(E->n_ext > 0 ? k_fam_dnlr<true> : k_fam_dnlr<false>, dim3(grid), dim3(256), 0, E->stream, A, F);
    HIP_TRY(hipGetLastError());
  }
  if (E->pdn_top_k > 0) {   // per-person de novo posteriors of the written rows (the same workspace, after k_fam_dnlr on the stream)
    PersonDnArgs P;
    P.top_k = E->pdn_top_k; P.top = E->d_pdn_top; P.all = E->d_pdn_all; P.line = E->d_pdn_line; P.kids = E->d_pdn_kids;
    P.n_nuc = E->pdn_n_nuc; P.n_es = E->pdn_n_es; P.is_kid = E->d_pdn_is_kid; P.jbuf = E->d_pdn_jbuf;
    const int grid = std::max(1, std::min(E->pdn_grid, n));
    hipLaunchKernelGGL(E->pdn_n_es > 0 ? k_person_dn<true> : k_person_dn<false>, dim3(grid), dim3(256), 0, E->stream, A, P);
    HIP_TRY(hipGetLastError());
  }
  return PM_OK;
}

static int collect_stats(pm_engine* E) {
  auto drain = [](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, auto& ms_sum, auto& launches) -> int {
    for (auto& pr : v) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
      ms_sum += ms;
      launches++;
      hipEventDestroy(pr.first); hipEventDestroy(pr.second);
    }
    v.clear();
    return PM_OK;
  };
  if (int rc = drain(E->brent_events, E->stats.kernel_ms, E->stats.launches)) return rc;
  return drain(E->es_events, E->stats.es_hoist_ms, E->stats.es_hoist_launches);
}

int pm_engine_run_device(pm_engine* E, int32_t n, const uint8_t* d_pl, const uint32_t* d_dm, const uint8_t* d_ref, pm_site_result* d_res,
                         pm_geno_call* d_calls) {
  if (!E || n < 0 || n > E->max_batch) { pm_set_last_error("pm_engine_run_device: invalid arguments (n > max_batch?)"); return PM_EINVAL; }
  if (n == 0) return PM_OK;
  HIP_TRY(hipSetDevice(E->device));
  return run_pipeline(E, n, d_pl, d_dm, d_ref, d_res ? d_res : E->d_res, d_calls ? d_calls : E->d_calls);
}

// Bookkeeping after a batch's stream work has completed (counts = the batch's d_counts, already on the host).
static int finish_batch(pm_engine* E, const int* counts) {
  if (counts[4] != 0x7fffffff) E->carry_postprob = true;
  E->stats.items += (int64_t)counts[0] + counts[1] + counts[2] + counts[8];
  E->stats.site_visits += (int64_t)counts[0] / (E->vcf ? 1 : (E->par.denovo && !pmplan::mono_dn(facts_of(E), E->sw)) ? 4 : 3) + counts[1] / 3 +
                          counts[2] + counts[9];
  E->stats.sites += E->last_n;
  if (E->es_ops_known && (E->use_plan1 ? E->n_ext1 : E->n_ext) > 0) {
    // hoisted items by variant: under --denovo list 0 holds cfg 0 (the top variant) and cfgs 1-3 (10-state) per site,
    // list 1 cfgs 4-6 (10-state), list 2 the cfg-7 re-optimisation (bi-allelic); otherwise every item is bi-allelic
    const double* o = E->es_item_ops;
    if (E->par.denovo && !E->vcf && E->es_grouped)   // a task: one leaf prefix, then the rest per 10-state item
      E->stats.es_hoist_ops += counts[0] / 4 * (o[3] + o[5] + 3 * o[4]) + counts[1] / 3 * (o[3] + 3 * o[4]) + counts[2] * o[0];
    else if (E->par.denovo && !E->vcf)
      E->stats.es_hoist_ops += counts[0] / 4 * o[2] + (counts[0] - counts[0] / 4) * o[1] + counts[1] * o[1] + counts[2] * o[0];
    else E->stats.es_hoist_ops += ((double)counts[0] + counts[1] + counts[2]) * o[0];
  }
  int rc = collect_stats(E);
  if (rc) return rc;
  E->stuck_site = counts[5] ? counts[6] : -1;
  E->last_rows = counts[3];
  E->vw_rows = 0;
  if (E->vw_fam_k > 0 || E->vw_car_k > 0) {
    E->vw_rows = counts[10];
    if (counts[5] && E->vw_rows > 0) {   // a stuck site: only the rows before it are valid (rows are in site order)
      std::vector<int> rs((size_t)E->vw_rows);
      HIP_TRY(hipMemcpy(rs.data(), E->d_vw_row_site, sizeof(int) * rs.size(), hipMemcpyDeviceToHost));
      E->vw_rows = (int)(std::lower_bound(rs.begin(), rs.end(), counts[6]) - rs.begin());
    }
  }
  if (counts[5]) { pm_set_last_error("ScalarMinimizer::Brent got stuck"); return PM_EBRENT; }
  return PM_OK;
}

int pm_engine_set_denovo_families(pm_engine* E, int32_t top_k, int32_t want_all) {
  if (!E || top_k < 0 || top_k > 8) { pm_set_last_error("pm_engine_set_denovo_families: top_k must be 0 (off) or 1..8"); return PM_EINVAL; }
  if (E->vcf) { pm_set_last_error("pm_engine_set_denovo_families: not available on a vcf_mode engine"); return PM_EINVAL; }
  if (!E->par.denovo) { pm_set_last_error("pm_engine_set_denovo_families: the engine was created without denovo"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_set_denovo_families: a submitted batch has not been collected"); return PM_EINVAL; }
  const size_t nb = (size_t)E->max_batch, nf = (size_t)E->n_fam;
  if (top_k > 0 && want_all && nb * nf * sizeof(double) > ((size_t)1 << 30)) {
    char b[256];
    snprintf(b, sizeof(b), "pm_engine_set_denovo_families: want_all needs max_batch x n_fam x 8 = %zu bytes on the device (limit 1 GiB)",
             nb * nf * sizeof(double));
    pm_set_last_error(b);
    return PM_EINVAL;
  }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  E->fam_top_k = 0;
  E->last_rows = 0;
  void** bufs[] = {(void**)&E->d_fam_top, (void**)&E->d_fam_sum, (void**)&E->d_fam_all, (void**)&E->d_fam_line};
  for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
  if (top_k == 0) return PM_OK;
  E->fam_grid = E->grid_post;
  int rc;
  if ((rc = dalloc(&E->d_fam_top, nb * top_k)) || (rc = dalloc(&E->d_fam_sum, nb))) return rc;
  if (want_all) rc = dalloc(&E->d_fam_all, nb * nf);
  else rc = dalloc(&E->d_fam_line, (size_t)E->fam_grid * nf);
  if (rc) return rc;
  E->fam_top_k = top_k;
  return PM_OK;
}

// pm_engine_set_vcf_denovo_detail's buffers (the stream is idle)
static void vw_free(pm_engine* E) {
  E->vw_fam_k = E->vw_car_k = 0;
  E->vw_rows = 0;
  void** bufs[] = {(void**)&E->d_vw_row_site, (void**)&E->d_vw_pfam, (void**)&E->d_vw_fam_top, (void**)&E->d_vw_fam_sum, (void**)&E->d_vw_fam_all,
                   (void**)&E->d_vw_fam_line, (void**)&E->d_vw_car_top, (void**)&E->d_vw_car_all, (void**)&E->d_vw_car_line,
                   (void**)&E->d_vw_kids, (void**)&E->d_vw_is_kid, (void**)&E->d_vw_jbuf};
  for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
}

// pm_engine_set_vcf_denovo_chrx_detail's buffers (the stream is idle)
static void vwx_free(pm_engine* E) {
  E->vwx_on = false;
  E->vwx_grid = E->vwx_n_kids = 0;
  void** bufs[] = {(void**)&E->d_vwx_kids, (void**)&E->d_vwx_is_kid, (void**)&E->d_vwx_jbuf};
  for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
}

// pm_engine_set_vcf_denovo_chrx's buffers (the stream is idle), and the chrX detail that rests on them
static void vdnx_free(pm_engine* E) {
  vwx_free(E);
  E->vdnx_on = false;
  if (E->d_vdnx_terms) (void)hipFree(E->d_vdnx_terms);
  if (E->d_vdnx_ws) (void)hipFree(E->d_vdnx_ws);
  E->d_vdnx_terms = nullptr; E->d_vdnx_ws = nullptr;
}

int pm_engine_set_vcf_denovo(pm_engine* E, int32_t on) {
  if (!E) { pm_set_last_error("pm_engine_set_vcf_denovo: invalid arguments"); return PM_EINVAL; }
  if (!E->vcf) { pm_set_last_error("pm_engine_set_vcf_denovo: the engine was created without vcf_mode"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_set_vcf_denovo: a submitted batch has not been collected"); return PM_EINVAL; }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  E->vdn_on = false;
  vdnx_free(E);
  void** bufs[] = {(void**)&E->d_vdn_terms, (void**)&E->d_vdn_co, (void**)&E->d_vdn_ws};
  for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
  if (!on) { vw_free(E); return PM_OK; }
  // the objective's terms, routed like the vcf_mode objective: peeled families (every family with offspring when the
  // pedigree is one family, the extended ones otherwise), nuclear families in closed form, founder persons
  std::vector<int> peel, nuc, pers;
  for (int f = 0; f < E->n_fam; f++) {
    const int kind = E->fam_kind_h[f];
    if (kind == PM_FAM_FOUNDERS) for (int p = E->fam_start_h[f]; p < E->fam_start_h[f + 1]; p++) pers.push_back(p);
    else if (kind == PM_FAM_NUCLEAR && E->n_fam > 1) nuc.push_back(f);
    else {
      if (E->peel_start_h[f + 1] == E->peel_start_h[f]) {
        pm_set_last_error("pm_engine_set_vcf_denovo: a family with offspring has no peeling schedule (pm_pedigree.steps)");
        return PM_EPED;
      }
      peel.push_back(f);
    }
  }
  E->vdn_peel = (int)peel.size(); E->vdn_nuc = (int)nuc.size();
  std::vector<int> terms(peel);
  terms.insert(terms.end(), nuc.begin(), nuc.end());
  terms.insert(terms.end(), pers.begin(), pers.end());
  E->vdn_terms = (int)terms.size();
  E->vdn_T = E->vdn_terms <= 128 ? 64 : 256;
  // coefficients in LDS when a block's fit (<= 96 KB); blocks per CU from the LDS budget, at most 16 waves per CU
  const size_t co_bytes = (size_t)5 * (terms.size() - peel.size()) * sizeof(double);
  E->vdn_lds = co_bytes <= 96 * 1024 ? std::max<size_t>(co_bytes, 8) : 0;
  const void* fn = E->vdn_T == 64 ? (const void*)k_vdn_brent<64> : (const void*)k_vdn_brent<256>;
  if (E->vdn_lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)E->vdn_lds));
  int bpc = std::max(1, std::min(1024 / E->vdn_T, (int)((160 * 1024) / (E->vdn_lds + 4 * 1024))));
  E->vdn_grid = E->n_cu * bpc;
  const size_t ws_block = (size_t)E->ws_per_lane * E->vdn_T * sizeof(double), co_block = E->vdn_lds ? 0 : co_bytes;
  if (ws_block + co_block > 0)   // workspace and spilled coefficients: <= 1 GiB, never below one block
    E->vdn_grid = (int)std::max<size_t>(1, std::min<size_t>(E->vdn_grid, ((size_t)1 << 30) / (ws_block + co_block)));
  E->vdn_grid = std::min(E->vdn_grid, E->max_batch);
  int rc;
  if ((rc = dalloc(&E->d_vdn_terms, terms.size())) || (rc = dalloc(&E->d_vdn_ws, (size_t)E->vdn_grid * E->ws_per_lane * E->vdn_T)) ||
      (rc = dalloc(&E->d_vdn_co, (size_t)E->vdn_grid * co_block / sizeof(double))))
    return rc;
  HIP_TRY(hipMemcpy(E->d_vdn_terms, terms.data(), sizeof(int) * terms.size(), hipMemcpyHostToDevice));
  E->vdn_on = true;
  return PM_OK;
}

// The output planes' setters and getters.  name: "vcf_phase" for pm_engine_set_vcf_phase / pm_engine_vcf_phase.
static int plane_refuse(const char* fn_prefix, const char* name, const char* why, const char* why_arg = "") {
  char b[192];
  const int k = snprintf(b, sizeof(b), "%s%s: ", fn_prefix, name);
  snprintf(b + k, sizeof(b) - k, why, why_arg);
  pm_set_last_error(b);
  return PM_EINVAL;
}
// A setter's guards, then the device selected and the stream idle
static int plane_guard(pm_engine* E, const char* name) {
  if (!E) return plane_refuse("pm_engine_set_", name, "invalid arguments");
  if (!E->vcf) return plane_refuse("pm_engine_set_", name, "the engine was created without vcf_mode");
  if (E->pending_n >= 0) return plane_refuse("pm_engine_set_", name, "a submitted batch has not been collected");
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  return PM_OK;
}
static void plane_free(Plane& pl) {
  pl.on = pl.valid = false;
  dfree(&pl.d);
}
// max_batch x n_person cells, cleared; on, and no batch has filled it yet
static int plane_alloc_clear(pm_engine* E, Plane& pl) {
  const size_t bytes = (size_t)E->max_batch * E->n_person * pl.cell;
  if (int rc = dalloc((char**)&pl.d, bytes)) return rc;
  HIP_TRY(hipMemset(pl.d, 0, bytes));
  pl.on = true;
  pl.valid = false;
  return PM_OK;
}
// The rows of the last finished batch (0 when it did not fill the plane) and, with out, their cells
static int plane_fetch(pm_engine* E, Plane pm_engine::*which, const char* name, int32_t* n_rows, void* out) {
  if (!E || !n_rows) return plane_refuse("pm_engine_", name, "invalid arguments");
  const Plane& pl = E->*which;
  if (!pl.on) return plane_refuse("pm_engine_", name, "the feature is off (pm_engine_set_%s)", name);
  if (E->pending_n >= 0) return plane_refuse("pm_engine_", name, "a submitted batch has not been collected");
  *n_rows = pl.valid ? E->last_rows : 0;
  if (out && *n_rows > 0) {
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipMemcpy(out, pl.d, pl.cell * (size_t)*n_rows * E->n_person, hipMemcpyDeviceToHost));
  }
  return PM_OK;
}

int pm_engine_set_vcf_posteriors(pm_engine* E, int32_t on) {
  if (int rc = plane_guard(E, "vcf_posteriors")) return rc;
  if (!on) { plane_free(E->vp); return PM_OK; }
  if (E->vp.on) return PM_OK;   // (already on: the last batch's plane stays)
  return plane_alloc_clear(E, E->vp);
}

int pm_engine_vcf_posteriors(pm_engine* E, int32_t* n_rows, pm_vcf_post* out) {
  return plane_fetch(E, &pm_engine::vp, "vcf_posteriors", n_rows, out);
}

static void vph_off(pm_engine* E) {
  plane_free(E->vph);
  if (E->vph_holds_kids) E->vph_kids.release();
  E->vph_holds_kids = false;
}

int pm_engine_set_vcf_phase(pm_engine* E, int32_t on) {
  if (int rc = plane_guard(E, "vcf_phase")) return rc;
  if (!on) { vph_off(E); return PM_OK; }
  if (E->vph.on) return PM_OK;   // (already on: the last batch's plane stays)
  int rc = plane_alloc_clear(E, E->vph);   // (cleared: the founders of peeled families are never written)
  if (!rc && !(rc = E->vph_kids.acquire())) E->vph_holds_kids = true;
  if (rc) vph_off(E);
  return rc;
}

int pm_engine_vcf_phase(pm_engine* E, int32_t* n_rows, pm_vcf_phase* out) {
  return plane_fetch(E, &pm_engine::vph, "vcf_phase", n_rows, out);
}

static void vj_off(pm_engine* E) {
  plane_free(E->vj);
  E->vj_fams.free();
  dfree((void**)&E->d_vj_ws);
}

int pm_engine_set_vcf_joint(pm_engine* E, int32_t on) {
  if (int rc = plane_guard(E, "vcf_joint")) return rc;
  if (!on) { vj_off(E); return PM_OK; }
  if (E->vj.on) return PM_OK;   // (already on: the last batch's plane stays)
  // the max peel's workspace per thread: a back-pointer word per step on top of the partials [n][3] and the marriage
  // partials [slots][9] that ws_per_lane covers (the sum peel for L runs in the same words)
  int ws_need = E->ws_per_lane;
  for (int f = 0; f < E->n_fam; f++) {
    const int s0 = E->peel_start_h[f], s1 = E->peel_start_h[f + 1];
    if (s1 == s0) continue;
    int slots = 0;
    for (int s = s0; s < s1; s++) {
      const int slot = (E->steps_h[s].y >> 8) & 255;
      if (slot != 255) slots = std::max(slots, slot + 1);
    }
    ws_need = std::max(ws_need, (E->fam_start_h[f + 1] - E->fam_start_h[f]) * 3 + slots * 9 + (s1 - s0));
  }
  E->vj_ws_per_lane = ws_need;
  // its HBM form's grid: grid_post blocks, fewer where their workspace would pass 1 GiB, never below one
  const size_t per = (size_t)ws_need * sizeof(double);
  E->vj_grid = per ? (int)std::max<size_t>(1, std::min<size_t>(E->grid_post, ((size_t)1 << 30) / (per * 256))) : E->grid_post;
  const bool peels = !E->vj_fams.h[0].empty() || !E->vj_fams.h[1].empty();
  int rc = plane_alloc_clear(E, E->vj);
  if (!rc && peels && !es_block_shape(E, ws_need).bt) rc = dalloc(&E->d_vj_ws, (size_t)E->vj_grid * 256 * ws_need);
  if (!rc) rc = E->vj_fams.upload();
  if (rc) vj_off(E);
  return rc;
}

int pm_engine_vcf_joint(pm_engine* E, int32_t* n_rows, pm_vcf_joint* out) {
  return plane_fetch(E, &pm_engine::vj, "vcf_joint", n_rows, out);
}

static void pc_off(pm_engine* E) {
  E->pc_on = false;
  dfree((void**)&E->d_pc_acc);
  dfree((void**)&E->d_pc_slot);
  if (E->pc_holds_kids) E->vph_kids.release();
  E->pc_holds_kids = false;
  E->pc_nuc_kids.free();
}

int pm_engine_set_vcf_pedcheck(pm_engine* E, int32_t on) {
  if (int rc = plane_guard(E, "vcf_pedcheck")) return rc;
  if (!on) { pc_off(E); return PM_OK; }
  if (E->pc_on) return PM_OK;   // (already on: the sums stay)
  // the non-founders: both parents stated inside the family
  std::vector<int> slot(E->n_person, -1);
  E->pc_person.clear();
  for (int plan = 0; plan < 2; plan++) E->pc_nuc_kids.h[plan].clear();
  for (int f = 0; f < E->n_fam; f++) {
    const int p0 = E->fam_start_h[f], n = E->fam_start_h[f + 1] - p0;
    if (E->fam_kind_h[f] == PM_FAM_FOUNDERS) continue;
    for (int j = 0; j < n; j++) {
      const int fa = E->fa_h[p0 + j], mo = E->mo_h[p0 + j];
      if (fa < 0 || mo < 0 || fa >= n || mo >= n || fa == mo) continue;
      slot[p0 + j] = (int)E->pc_person.size();
      E->pc_person.push_back(p0 + j);
      // (family << 8 | member, as vph_kids packs its entries: the children of a family of more than 255 persons are on no
      // list, here as there, and keep n = 0 unless the section runs the lean loop)
      if (E->fam_kind_h[f] == PM_FAM_NUCLEAR && n <= 255 && j >= 2) E->pc_nuc_kids.h[0].push_back(f << 8 | j);
    }
  }
  const size_t cells = std::max<size_t>(1, E->pc_person.size() * 4);
  int rc = dalloc(&E->d_pc_acc, cells);
  if (!rc) rc = dalloc(&E->d_pc_slot, (size_t)E->n_person);
  if (!rc && !(rc = E->vph_kids.acquire())) E->pc_holds_kids = true;   // (the phase plane's list, one device copy for both)
  if (!rc) rc = E->pc_nuc_kids.upload();
  if (!rc && hipMemset(E->d_pc_acc, 0, cells * sizeof(unsigned long long)) != hipSuccess) rc = PM_EHIP;
  if (!rc && hipMemcpy(E->d_pc_slot, slot.data(), sizeof(int) * slot.size(), hipMemcpyHostToDevice) != hipSuccess) rc = PM_EHIP;
  if (rc) { pc_off(E); return rc; }
  E->pc_on = true;
  return PM_OK;
}

int pm_engine_reset_vcf_pedcheck(pm_engine* E) {
  if (int rc = plane_guard(E, "vcf_pedcheck")) return rc;
  if (!E->pc_on) return plane_refuse("pm_engine_reset_", "vcf_pedcheck", "the feature is off (pm_engine_set_vcf_pedcheck)");
  HIP_TRY(hipMemset(E->d_pc_acc, 0, std::max<size_t>(1, E->pc_person.size() * 4) * sizeof(unsigned long long)));
  return PM_OK;
}

int pm_engine_vcf_pedcheck(pm_engine* E, int32_t* n_kids, pm_vcf_pedcheck* out) {
  if (!E || !n_kids) return plane_refuse("pm_engine_", "vcf_pedcheck", "invalid arguments");
  if (!E->pc_on) return plane_refuse("pm_engine_", "vcf_pedcheck", "the feature is off (pm_engine_set_vcf_pedcheck)");
  if (E->pending_n >= 0) return plane_refuse("pm_engine_", "vcf_pedcheck", "a submitted batch has not been collected");
  *n_kids = (int32_t)E->pc_person.size();
  if (out && *n_kids > 0) {
    std::vector<long long> acc((size_t)*n_kids * 4);
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipMemcpy(acc.data(), E->d_pc_acc, sizeof(long long) * acc.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < *n_kids; i++) {
      out[i].person = E->pc_person[i]; out[i].pad = 0; out[i].n = acc[4 * (size_t)i];
      for (int h = 0; h < 3; h++) out[i].q[h] = acc[4 * (size_t)i + 1 + h];
    }
  }
  return PM_OK;
}

int pm_engine_set_vcf_denovo_chrx(pm_engine* E, int32_t on) {
  if (!E) { pm_set_last_error("pm_engine_set_vcf_denovo_chrx: invalid arguments"); return PM_EINVAL; }
  if (!E->vcf) { pm_set_last_error("pm_engine_set_vcf_denovo_chrx: the engine was created without vcf_mode"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_set_vcf_denovo_chrx: a submitted batch has not been collected"); return PM_EINVAL; }
  if (!E->vdn_on) {
    pm_set_last_error("pm_engine_set_vcf_denovo_chrx: needs pm_engine_set_vcf_denovo(engine, 1) first (vcf_denovo is off)");
    return PM_EINVAL;
  }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  vdnx_free(E);
  if (!on) return PM_OK;
  // the objective's terms, routed like vcf_mode's plan 1 on chrX: every family with offspring is peeled (nuclear ones
  // included: no closed form), founders-only families give their persons
  std::vector<int> terms, pers;
  int ws_need = 0;   // doubles per lane of the largest peel: partials [n][3] + marriage partials [slots][9]
  for (int f = 0; f < E->n_fam; f++) {
    if (E->fam_kind_h[f] == PM_FAM_FOUNDERS) { for (int p = E->fam_start_h[f]; p < E->fam_start_h[f + 1]; p++) pers.push_back(p); continue; }
    if (E->peel_start_h[f + 1] == E->peel_start_h[f]) {
      pm_set_last_error("pm_engine_set_vcf_denovo_chrx: a family with offspring has no peeling schedule (pm_pedigree.steps)");
      return PM_EPED;
    }
    int slots = 0;
    for (int s = E->peel_start_h[f]; s < E->peel_start_h[f + 1]; s++) {
      const int slot = (E->steps_h[s].y >> 8) & 255;
      if (slot != 255) slots = std::max(slots, slot + 1);
    }
    ws_need = std::max(ws_need, (E->fam_start_h[f + 1] - E->fam_start_h[f]) * 3 + slots * 9);
    terms.push_back(f);
  }
  if (ws_need > E->ws_per_lane) {   // (a vcf_mode engine packs every family's schedule, nuclear ones included)
    pm_set_last_error("pm_engine_set_vcf_denovo_chrx: the peel workspace per lane does not cover a family's peel");
    return PM_EPED;
  }
  E->vdnx_peel = (int)terms.size();
  terms.insert(terms.end(), pers.begin(), pers.end());
  E->vdnx_terms = (int)terms.size();
  E->vdnx_T = E->vdnx_terms <= 128 ? 64 : 256;
  // k_vdn_brent's grid rule (its static LDS only) and 1 GiB workspace cap
  E->vdnx_grid = E->n_cu * std::max(1, std::min(1024 / E->vdnx_T, (160 * 1024) / (4 * 1024)));
  const size_t ws_block = (size_t)E->ws_per_lane * E->vdnx_T * sizeof(double);
  if (ws_block > 0) E->vdnx_grid = (int)std::max<size_t>(1, std::min<size_t>(E->vdnx_grid, ((size_t)1 << 30) / ws_block));
  E->vdnx_grid = std::min(E->vdnx_grid, E->max_batch);
  int rc;
  if ((rc = dalloc(&E->d_vdnx_terms, terms.size())) || (rc = dalloc(&E->d_vdnx_ws, (size_t)E->vdnx_grid * E->ws_per_lane * E->vdnx_T))) {
    vdnx_free(E);
    return rc;
  }
  HIP_TRY(hipMemcpy(E->d_vdnx_terms, terms.data(), sizeof(int) * terms.size(), hipMemcpyHostToDevice));
  E->vdnx_on = true;
  return PM_OK;
}

// The children {family, member} of every family with offspring: every person with both parents in the family; is_kid[p]
// = 1 for the persons listed.  nuc_first: the nuclear families take the closed form, so their children come first (the
// count is returned), then the peeled families'; else one list in family order.
static int vdn_list_children(const pm_engine* E, bool nuc_first, std::vector<int2>& kids, std::vector<int8_t>& is_kid) {
  std::vector<int2> kids_es;
  kids.clear();
  is_kid.assign((size_t)E->n_person, 0);
  for (int f = 0; f < E->n_fam; f++) {
    const int kind = E->fam_kind_h[f], p0 = E->fam_start_h[f], n = E->fam_start_h[f + 1] - p0;
    if (kind == PM_FAM_FOUNDERS) continue;
    const bool closed = nuc_first && kind == PM_FAM_NUCLEAR;
    for (int j = 0; j < n; j++) {
      const int fa = E->fa_h[p0 + j], mo = E->mo_h[p0 + j];
      if (fa < 0 || mo < 0 || fa >= n || mo >= n || fa == mo) continue;
      if (closed && (j < 2 || fa > 1 || mo > 1)) continue;   // (a nuclear family is father, mother, kids)
      (closed ? kids : kids_es).push_back(make_int2(f, j));
      is_kid[p0 + j] = 1;
    }
  }
  const int n_closed = (int)kids.size();
  kids.insert(kids.end(), kids_es.begin(), kids_es.end());
  return n_closed;
}

int pm_engine_set_vcf_denovo_detail(pm_engine* E, int32_t fam_k, int32_t car_k, int32_t want_all) {
  if (!E) { pm_set_last_error("pm_engine_set_vcf_denovo_detail: invalid arguments"); return PM_EINVAL; }
  if (!E->vcf) { pm_set_last_error("pm_engine_set_vcf_denovo_detail: the engine was created without vcf_mode"); return PM_EINVAL; }
  if (fam_k < 0 || fam_k > 8 || car_k < 0 || car_k > 8) {
    pm_set_last_error("pm_engine_set_vcf_denovo_detail: fam_k and car_k must each be 0 (off) or 1..8");
    return PM_EINVAL;
  }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_set_vcf_denovo_detail: a submitted batch has not been collected"); return PM_EINVAL; }
  if ((fam_k > 0 || car_k > 0) && !E->vdn_on) {
    pm_set_last_error("pm_engine_set_vcf_denovo_detail: needs pm_engine_set_vcf_denovo(engine, 1) first (vcf_denovo is off)");
    return PM_EINVAL;
  }
  const size_t nb = (size_t)E->max_batch, nf = (size_t)E->n_fam, np = (size_t)E->n_person;
  if (want_all && ((fam_k > 0 && nb * nf * sizeof(double) > ((size_t)1 << 30)) || (car_k > 0 && nb * np * sizeof(pm_person_dn) > ((size_t)1 << 30)))) {
    char b[320];
    snprintf(b, sizeof(b), "pm_engine_set_vcf_denovo_detail: want_all needs max_batch x n_fam x 8 = %zu and max_batch x n_person x 16 = %zu bytes "
             "on the device (limit 1 GiB each)", nb * nf * sizeof(double), nb * np * sizeof(pm_person_dn));
    pm_set_last_error(b);
    return PM_EINVAL;
  }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  vwx_free(E);   // (it writes into the buffers rebuilt here)
  vw_free(E);
  if (fam_k == 0 && car_k == 0) return PM_OK;
  // the children of the closed-form nuclear families (k_vdn_brent's routing: n_fam > 1), then of the peeled ones
  std::vector<int2> kids;
  std::vector<int8_t> is_kid;
  const int n_nuc = vdn_list_children(E, E->n_fam > 1, kids, is_kid), n_es = (int)kids.size() - n_nuc;
  std::vector<int> pfam(np, 0);
  for (int f = 0; f < E->n_fam; f++)
    for (int p = E->fam_start_h[f]; p < E->fam_start_h[f + 1]; p++) pfam[p] = f;
  // one block per row at a time, on k_vdn_brent's workspace (vdn_grid blocks); the peeled children's term buffer caps the
  // grid at 256 MiB
  int grid = E->vdn_grid;
  const size_t per_block = (size_t)n_es * 13 * sizeof(double);
  if (per_block) grid = (int)std::max<size_t>(1, std::min<size_t>(grid, ((size_t)1 << 28) / per_block));
  int rc;
  if ((rc = dalloc(&E->d_vw_row_site, nb)) || (rc = dalloc(&E->d_vw_pfam, np)) || (rc = dalloc(&E->d_vw_kids, kids.size())) ||
      (rc = dalloc(&E->d_vw_is_kid, np)))
    { vw_free(E); return rc; }
  if (fam_k > 0) {
    if ((rc = dalloc(&E->d_vw_fam_top, nb * fam_k)) || (rc = dalloc(&E->d_vw_fam_sum, nb)) ||
        (rc = want_all ? dalloc(&E->d_vw_fam_all, nb * nf) : dalloc(&E->d_vw_fam_line, (size_t)grid * nf)))
      { vw_free(E); return rc; }
  }
  if (car_k > 0) {
    if ((rc = dalloc(&E->d_vw_car_top, nb * car_k)) ||
        (rc = want_all ? dalloc(&E->d_vw_car_all, nb * np) : dalloc(&E->d_vw_car_line, (size_t)grid * np)) ||
        (per_block && (rc = dalloc(&E->d_vw_jbuf, (size_t)grid * n_es * 13))))
      { vw_free(E); return rc; }
  }
  HIP_TRY(hipMemcpy(E->d_vw_pfam, pfam.data(), sizeof(int) * np, hipMemcpyHostToDevice));
  if (!kids.empty()) HIP_TRY(hipMemcpy(E->d_vw_kids, kids.data(), sizeof(int2) * kids.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_vw_is_kid, is_kid.data(), np, hipMemcpyHostToDevice));
  E->vw_grid = grid; E->vw_n_nuc = n_nuc; E->vw_n_es = n_es;
  E->vw_fam_k = fam_k; E->vw_car_k = car_k;
  return PM_OK;
}

int pm_engine_set_vcf_denovo_chrx_detail(pm_engine* E, int32_t on) {
  if (!E) { pm_set_last_error("pm_engine_set_vcf_denovo_chrx_detail: invalid arguments"); return PM_EINVAL; }
  if (!E->vcf) { pm_set_last_error("pm_engine_set_vcf_denovo_chrx_detail: the engine was created without vcf_mode"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_set_vcf_denovo_chrx_detail: a submitted batch has not been collected"); return PM_EINVAL; }
  if (!E->vdnx_on) {
    pm_set_last_error("pm_engine_set_vcf_denovo_chrx_detail: needs pm_engine_set_vcf_denovo_chrx(engine, 1) first (vcf_denovo_chrx is off)");
    return PM_EINVAL;
  }
  if (E->vw_fam_k == 0 && E->vw_car_k == 0) {
    pm_set_last_error("pm_engine_set_vcf_denovo_chrx_detail: needs pm_engine_set_vcf_denovo_detail first (vcf_denovo_detail is off)");
    return PM_EINVAL;
  }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  vwx_free(E);
  if (!on) return PM_OK;
  // the children of every family with offspring (all peeled on X: k_vdn_brent_x's routing, so the autosomal list's
  // closed-form group does not apply)
  const size_t np = (size_t)E->n_person;
  std::vector<int2> kids;
  std::vector<int8_t> is_kid;
  vdn_list_children(E, false, kids, is_kid);
  // one block per row at a time on k_vdn_brent_x's workspace (vdnx_grid blocks) and the detail's per-block lines (vw_grid
  // blocks); the children's term buffer caps the grid at 256 MiB
  int grid = std::min(E->vdnx_grid, E->vw_grid);
  const size_t per_block = kids.size() * 13 * sizeof(double);
  if (per_block) grid = (int)std::max<size_t>(1, std::min<size_t>(grid, ((size_t)1 << 28) / per_block));
  int rc;
  if ((rc = dalloc(&E->d_vwx_kids, kids.size())) || (rc = dalloc(&E->d_vwx_is_kid, np)) ||
      (per_block && E->vw_car_k > 0 && (rc = dalloc(&E->d_vwx_jbuf, (size_t)grid * kids.size() * 13))))
    { vwx_free(E); return rc; }
  if (!kids.empty()) HIP_TRY(hipMemcpy(E->d_vwx_kids, kids.data(), sizeof(int2) * kids.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_vwx_is_kid, is_kid.data(), np, hipMemcpyHostToDevice));
  E->vwx_grid = grid; E->vwx_n_kids = (int)kids.size();
  E->vwx_on = true;
  return PM_OK;
}

int pm_engine_vcf_denovo_rows(pm_engine* E, int32_t* n_rows, int32_t* site) {
  if (!E || !n_rows) { pm_set_last_error("pm_engine_vcf_denovo_rows: invalid arguments"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_vcf_denovo_rows: a submitted batch has not been collected"); return PM_EINVAL; }
  *n_rows = (E->vw_fam_k > 0 || E->vw_car_k > 0) ? E->vw_rows : 0;
  if (site && *n_rows > 0) {
    HIP_TRY(hipSetDevice(E->device));
    HIP_TRY(hipStreamSynchronize(E->stream));
    HIP_TRY(hipMemcpy(site, E->d_vw_row_site, sizeof(int32_t) * (size_t)*n_rows, hipMemcpyDeviceToHost));
  }
  return PM_OK;
}

int pm_engine_vcf_denovo_families(pm_engine* E, pm_fam_lr* top, double* sum, double* all) {
  if (!E || !top) { pm_set_last_error("pm_engine_vcf_denovo_families: invalid arguments"); return PM_EINVAL; }
  if (E->vw_fam_k <= 0) { pm_set_last_error("pm_engine_vcf_denovo_families: the feature is off (pm_engine_set_vcf_denovo_detail fam_k)"); return PM_EINVAL; }
  if (all && !E->d_vw_fam_all) { pm_set_last_error("pm_engine_vcf_denovo_families: the full matrix needs want_all"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_vcf_denovo_families: a submitted batch has not been collected"); return PM_EINVAL; }
  const size_t rows = (size_t)E->vw_rows;
  if (rows == 0) return PM_OK;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(top, E->d_vw_fam_top, sizeof(pm_fam_lr) * rows * E->vw_fam_k, hipMemcpyDeviceToHost));
  if (sum) HIP_TRY(hipMemcpy(sum, E->d_vw_fam_sum, sizeof(double) * rows, hipMemcpyDeviceToHost));
  if (all) HIP_TRY(hipMemcpy(all, E->d_vw_fam_all, sizeof(double) * rows * E->n_fam, hipMemcpyDeviceToHost));
  return PM_OK;
}

int pm_engine_vcf_denovo_carriers(pm_engine* E, pm_person_dn* top, pm_person_dn* all) {
  if (!E || !top) { pm_set_last_error("pm_engine_vcf_denovo_carriers: invalid arguments"); return PM_EINVAL; }
  if (E->vw_car_k <= 0) { pm_set_last_error("pm_engine_vcf_denovo_carriers: the feature is off (pm_engine_set_vcf_denovo_detail car_k)"); return PM_EINVAL; }
  if (all && !E->d_vw_car_all) { pm_set_last_error("pm_engine_vcf_denovo_carriers: the full matrix needs want_all"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_vcf_denovo_carriers: a submitted batch has not been collected"); return PM_EINVAL; }
  const size_t rows = (size_t)E->vw_rows;
  if (rows == 0) return PM_OK;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(top, E->d_vw_car_top, sizeof(pm_person_dn) * rows * E->vw_car_k, hipMemcpyDeviceToHost));
  if (all) HIP_TRY(hipMemcpy(all, E->d_vw_car_all, sizeof(pm_person_dn) * rows * E->n_person, hipMemcpyDeviceToHost));
  return PM_OK;
}

int pm_engine_denovo_rows(pm_engine* E, int32_t* n_rows) {
  if (!E || !n_rows) { pm_set_last_error("pm_engine_denovo_rows: invalid arguments"); return PM_EINVAL; }
  *n_rows = (E->fam_top_k > 0 || E->pdn_top_k > 0) ? E->last_rows : 0;
  return PM_OK;
}

int pm_engine_set_denovo_carriers(pm_engine* E, int32_t top_k, int32_t want_all) {
  if (!E || top_k < 0 || top_k > 8) { pm_set_last_error("pm_engine_set_denovo_carriers: top_k must be 0 (off) or 1..8"); return PM_EINVAL; }
  if (E->vcf) { pm_set_last_error("pm_engine_set_denovo_carriers: not available on a vcf_mode engine"); return PM_EINVAL; }
  if (!E->par.denovo) { pm_set_last_error("pm_engine_set_denovo_carriers: the engine was created without denovo"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_set_denovo_carriers: a submitted batch has not been collected"); return PM_EINVAL; }
  const size_t nb = (size_t)E->max_batch, np = (size_t)E->n_person;
  if (top_k > 0 && want_all && nb * np * sizeof(pm_person_dn) > ((size_t)1 << 30)) {
    char b[256];
    snprintf(b, sizeof(b), "pm_engine_set_denovo_carriers: want_all needs max_batch x n_person x 16 = %zu bytes on the device (limit 1 GiB)",
             nb * np * sizeof(pm_person_dn));
    pm_set_last_error(b);
    return PM_EINVAL;
  }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  E->pdn_top_k = 0;
  E->last_rows = 0;   // (either setter forgets the last batch's rows: the buffers it fills are new)
  void** bufs[] = {(void**)&E->d_pdn_top, (void**)&E->d_pdn_all, (void**)&E->d_pdn_line, (void**)&E->d_pdn_kids, (void**)&E->d_pdn_is_kid,
                   (void**)&E->d_pdn_jbuf};
  for (void** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
  if (top_k == 0) return PM_OK;
  // the work list: every person with both parents in a nuclear or an extended family
  std::vector<int2> kids, kids_es;
  std::vector<int8_t> is_kid(np, 0);
  for (int f : E->fam_perm_h) {
    const int kind = E->fam_kind_h[f], p0 = E->fam_start_h[f], n = E->fam_start_h[f + 1] - p0;
    if (kind == PM_FAM_FOUNDERS) continue;
    for (int j = 0; j < n; j++) {
      const int fa = E->fa_h[p0 + j], mo = E->mo_h[p0 + j];
      if (fa < 0 || mo < 0 || fa >= n || mo >= n) continue;
      if (kind == PM_FAM_NUCLEAR && (j < 2 || fa > 1 || mo > 1 || fa == mo)) continue;   // (a nuclear family is father, mother, kids)
      (kind == PM_FAM_NUCLEAR ? kids : kids_es).push_back(make_int2(f, j));
      is_kid[p0 + j] = 1;
    }
  }
  E->pdn_n_nuc = (int)kids.size();
  E->pdn_n_es = (int)kids_es.size();
  kids.insert(kids.end(), kids_es.begin(), kids_es.end());
  // one block per row at a time; the extended families' term buffer caps the grid at 256 MiB
  E->pdn_grid = E->grid_post;
  const size_t per_block = (size_t)E->pdn_n_es * 111 * sizeof(double);
  if (per_block) E->pdn_grid = (int)std::max<size_t>(1, std::min<size_t>(E->pdn_grid, ((size_t)1 << 28) / per_block));
  int rc;
  if ((rc = dalloc(&E->d_pdn_top, nb * top_k)) || (rc = dalloc(&E->d_pdn_kids, std::max<size_t>(1, kids.size()))) ||
      (rc = dalloc(&E->d_pdn_is_kid, np)))
    return rc;
  if (want_all) rc = dalloc(&E->d_pdn_all, nb * np);
  else rc = dalloc(&E->d_pdn_line, (size_t)E->pdn_grid * np);
  if (rc) return rc;
  if (per_block && (rc = dalloc(&E->d_pdn_jbuf, (size_t)E->pdn_grid * E->pdn_n_es * 111))) return rc;
  if (!kids.empty()) HIP_TRY(hipMemcpy(E->d_pdn_kids, kids.data(), sizeof(int2) * kids.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(E->d_pdn_is_kid, is_kid.data(), np, hipMemcpyHostToDevice));
  E->pdn_top_k = top_k;
  return PM_OK;
}

int pm_engine_denovo_carriers(pm_engine* E, pm_person_dn* top, pm_person_dn* all) {
  if (!E || !top) { pm_set_last_error("pm_engine_denovo_carriers: invalid arguments"); return PM_EINVAL; }
  if (E->pdn_top_k <= 0) { pm_set_last_error("pm_engine_denovo_carriers: the feature is off (pm_engine_set_denovo_carriers)"); return PM_EINVAL; }
  if (all && !E->d_pdn_all) { pm_set_last_error("pm_engine_denovo_carriers: the full matrix needs want_all"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_denovo_carriers: a submitted batch has not been collected"); return PM_EINVAL; }
  const size_t rows = (size_t)E->last_rows;
  if (rows == 0) return PM_OK;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(top, E->d_pdn_top, sizeof(pm_person_dn) * rows * E->pdn_top_k, hipMemcpyDeviceToHost));
  if (all) HIP_TRY(hipMemcpy(all, E->d_pdn_all, sizeof(pm_person_dn) * rows * E->n_person, hipMemcpyDeviceToHost));
  return PM_OK;
}

int pm_engine_denovo_families(pm_engine* E, pm_fam_lr* top, double* sum, double* all) {
  if (!E || !top) { pm_set_last_error("pm_engine_denovo_families: invalid arguments"); return PM_EINVAL; }
  if (E->fam_top_k <= 0) { pm_set_last_error("pm_engine_denovo_families: the feature is off (pm_engine_set_denovo_families)"); return PM_EINVAL; }
  if (all && !E->d_fam_all) { pm_set_last_error("pm_engine_denovo_families: the full matrix needs want_all"); return PM_EINVAL; }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_denovo_families: a submitted batch has not been collected"); return PM_EINVAL; }
  const size_t rows = (size_t)E->last_rows;
  if (rows == 0) return PM_OK;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(top, E->d_fam_top, sizeof(pm_fam_lr) * rows * E->fam_top_k, hipMemcpyDeviceToHost));
  if (sum) HIP_TRY(hipMemcpy(sum, E->d_fam_sum, sizeof(double) * rows, hipMemcpyDeviceToHost));
  if (all) HIP_TRY(hipMemcpy(all, E->d_fam_all, sizeof(double) * rows * E->n_fam, hipMemcpyDeviceToHost));
  return PM_OK;
}

int pm_engine_stuck_site(pm_engine* E, int32_t* site) {
  if (!E || !site) { pm_set_last_error("pm_engine_stuck_site: invalid arguments"); return PM_EINVAL; }
  *site = E->stuck_site;
  return PM_OK;
}

// rows written for the sites before the first stuck one (rows are numbered in site order)
static int rows_before(const pm_site_result* res, int k) {
  int r = 0;
  for (int i = 0; i < k; i++) r += res[i].call_row >= 0;
  return r;
}

int pm_engine_sync(pm_engine* E) {
  if (!E) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  int counts[16];
  HIP_TRY(hipMemcpy(counts, E->d_counts, sizeof(counts), hipMemcpyDeviceToHost));
  return finish_batch(E, counts);
}

// Host batch -> the engine's stream, without waiting: H2D of the person-major block (asynchronous when the host
// buffers are page-locked, pm_host_alloc), transpose, the pipeline, and D2H of the per-site results and the
// batch counters into the engine's page-locked buffers.  pm_engine_collect waits and hands them out.
int pm_engine_submit(pm_engine* E, int32_t n, const uint8_t* pl, const uint32_t* dm, const uint8_t* ref) {
  if (!E || n < 0 || n > E->max_batch || (n > 0 && (!pl || !ref || (!dm && !E->vcf)))) {
    pm_set_last_error("pm_engine_submit: invalid arguments");
    return PM_EINVAL;
  }
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_submit: the previous batch has not been collected"); return PM_EINVAL; }
  HIP_TRY(hipSetDevice(E->device));
  if (!E->h_res) {
    HIP_TRY(hipHostMalloc((void**)&E->h_res, sizeof(pm_site_result) * (size_t)E->max_batch, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&E->h_counts, 16 * sizeof(int), hipHostMallocDefault));
  }
  E->pending_n = n;
  if (n == 0) return PM_OK;
  const size_t np = E->n_person;
  HIP_TRY(hipMemcpyAsync(E->d_stage, pl, (size_t)n * np * 10, hipMemcpyHostToDevice, E->stream));
  if (!E->vcf)   // (vcf_mode reads no depth: dm is neither copied nor needed, and may be NULL)
    HIP_TRY(hipMemcpyAsync(E->d_dm, dm, (size_t)n * np * 4, hipMemcpyHostToDevice, E->stream));
  HIP_TRY(hipMemcpyAsync(E->d_ref, ref, (size_t)n, hipMemcpyHostToDevice, E->stream));
  int rc = pm_engine_to_planar(E, n, E->d_stage, E->d_pl);   // the engine's genotype-planar layout
  if (rc) return rc;
  rc = run_pipeline(E, n, E->d_pl, E->d_dm, E->d_ref, E->d_res, E->d_calls);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(E->h_res, E->d_res, sizeof(pm_site_result) * n, hipMemcpyDeviceToHost, E->stream));
  HIP_TRY(hipMemcpyAsync(E->h_counts, E->d_counts, 16 * sizeof(int), hipMemcpyDeviceToHost, E->stream));
  return PM_OK;
}

int pm_engine_collect(pm_engine* E, pm_site_result* res, pm_geno_call* calls, int32_t* n_rows) {
  if (!E || !n_rows || E->pending_n < 0 || (E->pending_n > 0 && !res)) {
    pm_set_last_error("pm_engine_collect: invalid arguments (no batch submitted?)");
    return PM_EINVAL;
  }
  const int n = E->pending_n;
  E->pending_n = -1;
  *n_rows = 0;
  if (n == 0) { E->last_rows = 0; E->vw_rows = 0; return PM_OK; }
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  int counts[16];
  memcpy(counts, E->h_counts, sizeof(counts));
  const int rc = finish_batch(E, counts);
  if (rc && rc != PM_EBRENT) return rc;
  memcpy(res, E->h_res, sizeof(pm_site_result) * n);
  *n_rows = rc ? rows_before(res, E->stuck_site) : counts[3];   // PM_EBRENT: the complete sites' rows only
  E->last_rows = *n_rows;
  const size_t np = E->n_person;
  if (calls && counts[3] > 0) {
    if (E->vcf) {   // 4-B rows on the device (pm_vcf_call), expanded into the caller's pm_geno_call rows
      const size_t nr = np * (size_t)counts[3];
      std::vector<pm_vcf_call> v(nr);
      HIP_TRY(hipMemcpy(v.data(), E->d_calls, sizeof(pm_vcf_call) * nr, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < nr; i++) {
        pm_geno_call c;
        c.dosage = 0.0; c.best = v[i].best; c.gq = v[i].gq; c.label = v[i].label;
        c._pad[0] = c._pad[1] = c._pad[2] = 0;
        calls[i] = c;
      }
    } else HIP_TRY(hipMemcpy(calls, E->d_calls, sizeof(pm_geno_call) * np * counts[3], hipMemcpyDeviceToHost));
  }
  return rc;
}

int pm_engine_run_vcf(pm_engine* E, int32_t n, const uint8_t* pl, const uint8_t* ref, pm_site_result* res, pm_vcf_call* calls,
                      int32_t* n_rows) {
  if (!E || !E->vcf || n < 0 || n > E->max_batch || !res || !n_rows) { pm_set_last_error("pm_engine_run_vcf: invalid arguments"); return PM_EINVAL; }
  *n_rows = 0;
  if (n == 0) return PM_OK;
  // (a pm_engine_submit batch still to be collected stays pending: the caller collects it)
  if (E->pending_n >= 0) { pm_set_last_error("pm_engine_run_vcf: a submitted batch has not been collected"); return PM_EINVAL; }
  int rc = pm_engine_submit(E, n, pl, nullptr, ref);
  E->pending_n = -1;   // (this call's own batch: collected below, or abandoned with submit's error)
  if (rc) return rc;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  int counts[16];
  memcpy(counts, E->h_counts, sizeof(counts));
  rc = finish_batch(E, counts);
  if (rc && rc != PM_EBRENT) return rc;
  memcpy(res, E->h_res, sizeof(pm_site_result) * n);
  *n_rows = rc ? rows_before(res, E->stuck_site) : counts[3];   // PM_EBRENT: the complete sites' rows only
  E->last_rows = *n_rows;
  if (calls && counts[3] > 0)   // the device rows as they are (4 B per person)
    HIP_TRY(hipMemcpy(calls, E->d_calls, sizeof(pm_vcf_call) * E->n_person * (size_t)counts[3], hipMemcpyDeviceToHost));
  return rc;
}

int pm_engine_run(pm_engine* E, int32_t n, const uint8_t* pl, const uint32_t* dm, const uint8_t* ref, int32_t on_device,
                  pm_site_result* res, pm_geno_call* calls, int32_t* n_rows) {
  if (!E || n < 0 || n > E->max_batch || !res || !n_rows) { pm_set_last_error("pm_engine_run: invalid arguments"); return PM_EINVAL; }
  *n_rows = 0;
  if (n == 0) { E->last_rows = 0; E->vw_rows = 0; return PM_OK; }
  if (!on_device) {   // host inputs: submit + collect
    int rc = pm_engine_submit(E, n, pl, dm, ref);
    if (rc) { E->pending_n = -1; return rc; }
    return pm_engine_collect(E, res, calls, n_rows);
  }
  HIP_TRY(hipSetDevice(E->device));
  const size_t np = E->n_person;
  int rc = pm_engine_to_planar(E, n, pl, E->d_pl);   // the engine's genotype-planar layout
  if (rc) return rc;
  rc = run_pipeline(E, n, E->d_pl, dm, ref, E->d_res, E->d_calls);
  if (rc) return rc;
  rc = pm_engine_sync(E);
  if (rc && rc != PM_EBRENT) return rc;
  HIP_TRY(hipMemcpy(res, E->d_res, sizeof(pm_site_result) * n, hipMemcpyDeviceToHost));
  int counts[16];
  HIP_TRY(hipMemcpy(counts, E->d_counts, sizeof(counts), hipMemcpyDeviceToHost));
  *n_rows = rc ? rows_before(res, E->stuck_site) : counts[3];   // PM_EBRENT: the complete sites' rows only
  E->last_rows = *n_rows;
  if (calls && counts[3] > 0) {
    if (E->vcf) {
      const size_t nr = np * (size_t)counts[3];
      std::vector<pm_vcf_call> v(nr);
      HIP_TRY(hipMemcpy(v.data(), E->d_calls, sizeof(pm_vcf_call) * nr, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < nr; i++) {
        pm_geno_call c;
        c.dosage = 0.0; c.best = v[i].best; c.gq = v[i].gq; c.label = v[i].label;
        c._pad[0] = c._pad[1] = c._pad[2] = 0;
        calls[i] = c;
      }
    } else HIP_TRY(hipMemcpy(calls, E->d_calls, sizeof(pm_geno_call) * np * counts[3], hipMemcpyDeviceToHost));
  }
  return rc;
}

int pm_engine_to_planar(pm_engine* E, int32_t n, const uint8_t* d_src, uint8_t* d_dst) {
  if (!E || n < 0 || !d_src || !d_dst || d_src == d_dst) { pm_set_last_error("pm_engine_to_planar: invalid arguments"); return PM_EINVAL; }
  if (n == 0) return PM_OK;
  HIP_TRY(hipSetDevice(E->device));
  const long long total = (long long)n * E->n_person;
  const int tb = 256;
  hipLaunchKernelGGL(k_to_planar, dim3((unsigned)((total + tb - 1) / tb)), dim3(tb), 0, E->stream, n, E->n_person, d_src, d_dst);
  HIP_TRY(hipGetLastError());
  return PM_OK;
}

int pm_engine_counters(pm_engine* E, pm_counters* out) {
  if (!E || !out) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  unsigned long long c[16];
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(c, E->d_counters, sizeof(c), hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < 5; k++) out->ref_base_counts[k] = (int64_t)c[k];
  out->min_total_depth_filter = (int64_t)c[5];
  out->max_total_depth_filter = (int64_t)c[6];
  out->min_ps_filter = (int64_t)c[7];
  out->min_map_qual_filter = (int64_t)c[8];
  out->homo_ref = (int64_t)c[9];
  out->transitions = (int64_t)c[10];
  out->transversions = (int64_t)c[11];
  out->tstvs1 = (int64_t)c[12];
  out->tstvs2 = (int64_t)c[13];
  out->tvs1tvs2 = (int64_t)c[14];
  out->nocall = (int64_t)c[15];
  return PM_OK;
}

int pm_engine_synth(pm_engine* E, int32_t n, uint64_t seed, uint64_t off, uint8_t* d_pl, uint32_t* d_dm, uint8_t* d_ref) {
  if (!E || n <= 0) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  DevArgs A = make_args(E, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  const long long total = (long long)n * E->n_fam;
  const int tb = 256;
  hipLaunchKernelGGL(k_synth, dim3((unsigned)((total + tb - 1) / tb)), dim3(tb), 0, E->stream, A, n, seed, off, d_pl, d_dm, d_ref);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(E->stream));
  return PM_OK;
}

int pm_host_alloc(uint64_t bytes, void** p) {
  if (!p) return PM_EINVAL;
  *p = nullptr;
  if (bytes == 0) return PM_OK;
  HIP_TRY(hipHostMalloc(p, bytes, hipHostMallocDefault));
  return PM_OK;
}

int pm_host_free(void* p) {
  if (p) HIP_TRY(hipHostFree(p));
  return PM_OK;
}

int pm_device_alloc(pm_engine* E, uint64_t bytes, void** p) {
  if (!E || !p) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
  return PM_OK;
}
int pm_device_free(pm_engine* E, void* p) {
  if (!E) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipFree(p));
  return PM_OK;
}
int pm_copy_to_host(pm_engine* E, void* dst, const void* src, uint64_t bytes) {
  if (!E) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return PM_OK;
}

int pm_copy_to_device(pm_engine* E, void* dst, const void* src, uint64_t bytes) {
  if (!E) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  HIP_TRY(hipStreamSynchronize(E->stream));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return PM_OK;
}

int pm_engine_kernel_stats(pm_engine* E, pm_kernel_stats* out, int32_t reset) {
  if (!E || !out) return PM_EINVAL;
  HIP_TRY(hipSetDevice(E->device));
  unsigned long long ev = 0;
  HIP_TRY(hipStreamSynchronize(E->stream));
  int rc = collect_stats(E);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(&ev, E->d_eval_total, sizeof(ev), hipMemcpyDeviceToHost));
  *out = E->stats;
  out->evals = (int64_t)ev;
  out->fam_evals = (int64_t)ev * E->n_fam;
  if (E->d_phase) {
    unsigned long long ph[3];
    HIP_TRY(hipMemcpy(ph, E->d_phase, sizeof(ph), hipMemcpyDeviceToHost));
    out->hoist_wave_ns = (int64_t)((double)ph[0] * 1e6 / E->wall_khz);   // wall_clock64 ticks at wall_khz
    out->eval_wave_ns = (int64_t)((double)ph[1] * 1e6 / E->wall_khz);
    out->timed_items = (int64_t)ph[2];
  }
  if (reset) {
    E->stats = pm_kernel_stats{};
    HIP_TRY(hipMemset(E->d_eval_total, 0, sizeof(ev)));
    if (E->d_phase) HIP_TRY(hipMemset(E->d_phase, 0, 3 * sizeof(unsigned long long)));
  }
  return PM_OK;
}

}  // extern "C"
