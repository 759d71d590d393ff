#pragma once
// brent_plan.h -- which k_brent instantiation a batch runs and with what launch flavour, as pure host functions: the
// engine's environment switches (read once, at pm_engine_create), the lane-plan geometry (choose_geometry) and the
// kernel selection (brent_select).  Plain C++17, no HIP: engine.hip calls it, tests/native/plan_check.cpp enumerates it
// against brent_variants.h on a CPU.  A variant is added in tools/gen_brent_variants.py and nowhere else.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include "../../include/polymutt_engine.h"

namespace pmplan {

// engine_dev.h's constants the selection reads (engine.hip static_asserts that the two agree)
constexpr int kPdLo = 8, kPdHi = 12, kEpe = 4, kDnPfC = 1, kDnPfBuf = 3072, kQWave = 9216;

// k_brent's template arguments, in order (engine_dev.h)
struct BrentKey {
  int T, S, NUM;
  bool GEN, ES, DN, PF, EP, QD;
  int NF, PD;
};
inline auto key_tie(const BrentKey& k) { return std::tie(k.T, k.S, k.NUM, k.GEN, k.ES, k.DN, k.PF, k.EP, k.QD, k.NF, k.PD); }
inline bool operator==(const BrentKey& a, const BrentKey& b) { return key_tie(a) == key_tie(b); }

// One field per PM_* environment switch of engine.hip (tests and tools only; include/polymutt_engine.h).
struct EngineSwitches {
  int test_itmax = 0;         // PM_TEST_ITMAX=k > 0: Brent's ITMAX lowered to min(200, k)
  int ts_t = 0, ts_s = 0;     // PM_BRENT_TS=T,S: force the lane plan's geometry when it holds the pedigree
  bool no_prefetch = false;   // PM_NO_PREFETCH: the lean kernels hoist from direct loads, no LDS staging
  bool ep_dn_one = false;     // PM_EP_DN_ONE: one extended family per lane under --denovo
  bool no_split34 = false, no_quad = false;   // PM_NO_SPLIT34 / PM_NO_QUAD: no split trio / quad plan; no QUAD plan
  int es_chunk = 0;           // PM_ES_CHUNK=N > 0: at most N items per coefficient chunk
  bool phase_timing = false;  // PM_PHASE_TIMING: k_brent's in-kernel hoisting / evaluation split
  bool mono_dn_prep = false;  // PM_MONO_DN_PREP: QUAD plans form the de novo monomorphism item in k_prep
  bool no_jit = false, no_fused = false;   // PM_NO_JIT: the generic k_es_hoist; PM_NO_FUSED: hoisting + k_brent apart
  bool es_nogroup = false, es_prof = false;   // PM_ES_NOGROUP: one de novo item per hoisting task; PM_ES_PROF: its cycles by part
  bool jit_layout = false;    // PM_JIT_LAYOUT: say why the fused kernel is unavailable
  bool es_post_hbm = false;   // PM_ES_POST_HBM: k_posterior_es's workspace in HBM
  int qd_group = 1;           // PM_QD_GROUP=1|3: QUAD items a wave takes per step (anything else: 3)
  int qd_bpc = 0;             // PM_QD_BPC=N: QUAD blocks per CU instead of the occupancy query's (and one round)
  bool qd_dyn = false;        // PM_QD_DYN=1: the QUAD kernel's per-XCD claimed item order
  int qd_rounds = 1, fused_rounds = 1;     // PM_QD_ROUNDS / PM_FUSED_ROUNDS=R: rounds of the resident blocks
  int pf_rounds = 0;          // PM_PF_ROUNDS=R: the lean PF kernels' rounds (0: by plan, launch_brent)
  bool no_ep_only = false, no_epo = false;   // PM_NO_EP_ONLY / PM_NO_EPO: no ep_only plan / no NF = 1 kernel for it
  bool no_trio = false, no_pd_hi = false;   // PM_NO_TRIO: trio plans on the any-size PF kernel; PM_NO_PD_HI: PD stays PM_PD_LO
  int prep_spw = 0;           // PM_PREP_SPW=1..8: k_prep's sites per wave (0: PREP_SPW)

  static EngineSwitches from_env() {
    EngineSwitches w;
    auto on = [](const char* k) { return getenv(k) != nullptr; };
    auto pos = [](const char* k) { const char* s = getenv(k); return s && atoi(s) > 0 ? atoi(s) : 0; };
    auto atl1 = [](const char* k, int unset) { const char* s = getenv(k); return s ? std::max(1, atoi(s)) : unset; };
    w.test_itmax = pos("PM_TEST_ITMAX");
    if (const char* s = getenv("PM_BRENT_TS"); !s || sscanf(s, "%d,%d", &w.ts_t, &w.ts_s) != 2) w.ts_t = w.ts_s = 0;
    w.no_prefetch = on("PM_NO_PREFETCH"); w.ep_dn_one = on("PM_EP_DN_ONE"); w.no_split34 = on("PM_NO_SPLIT34");
    w.no_quad = on("PM_NO_QUAD"); w.es_chunk = pos("PM_ES_CHUNK"); w.phase_timing = on("PM_PHASE_TIMING");
    w.mono_dn_prep = on("PM_MONO_DN_PREP"); w.no_jit = on("PM_NO_JIT"); w.no_fused = on("PM_NO_FUSED");
    w.es_nogroup = on("PM_ES_NOGROUP"); w.jit_layout = on("PM_JIT_LAYOUT"); w.es_prof = on("PM_ES_PROF");
    w.es_post_hbm = on("PM_ES_POST_HBM");
    w.qd_group = atl1("PM_QD_GROUP", 1) == 1 ? 1 : 3;
    w.qd_bpc = atl1("PM_QD_BPC", 0);
    if (const char* s = getenv("PM_QD_DYN")) w.qd_dyn = atoi(s) != 0;
    w.qd_rounds = atl1("PM_QD_ROUNDS", 1); w.fused_rounds = atl1("PM_FUSED_ROUNDS", 1); w.pf_rounds = atl1("PM_PF_ROUNDS", 0);
    w.no_ep_only = on("PM_NO_EP_ONLY"); w.no_epo = on("PM_NO_EPO"); w.no_trio = on("PM_NO_TRIO"); w.no_pd_hi = on("PM_NO_PD_HI");
    if (const char* s = getenv("PM_PREP_SPW"); s && *s) w.prep_spw = std::max(1, atoi(s));
    return w;
  }
};

struct Geometry { int T, S; };   // threads per item x family slots per lane

// What the selection reads from an engine: the pedigree's shape, the parameters, the section's chromosome class and the
// lane plans (0: nuclear and founder units, extended families peeled; 1: vcf_mode's plan with every family peeled).
struct LanePlan {
  int T = 0, S = 0, n_ext = 0;
  bool units_empty = false;   // no nuclear or founder unit: every family peeled
  int ep_dmax = 0;            // the largest polynomial degree of a peeled family in the section's chromosome class
};
struct Facts {
  int n_person = 0, n_fam = 0, chrom = PM_CHR_AUTO, numerics = PM_NUM_POLY, max_nuc = 0;
  bool denovo = false, quick_call = false, vcf = false, use_plan1 = false, has_fp = false, es_poly = false;
  bool quad = false, all_trio = false, split34 = false;   // of plan 0's units (pm_engine)
  LanePlan plan[2];
  Geometry quick = {0, 0};    // --quick_call: the MakeUnrelated() plan
};

// The generic kernel on every chromosome class: the reference-order de novo model, founders-only or extended families,
// a lone family.  (The lean kernel: autosome, nuclear families only; with POLY numerics it takes --denovo too.)
inline bool generic_plan(const Facts& f) { return (f.denovo && f.numerics != PM_NUM_POLY) || f.has_fp || f.n_fam == 1; }
// Lean --denovo: the PL windows can be staged through LDS (16-B aligned planes, families of <= 4)
inline bool dn_staging(const Facts& f, const EngineSwitches& w) {
  return f.denovo && f.numerics == PM_NUM_POLY && f.max_nuc <= 4 && f.n_person % 16 == 0 && f.n_person >= 16 && !w.no_prefetch;
}
// Lean autosomal --denovo (POLY numerics, nuclear families only, no quick pre-filter): the cfg-0 de novo monomorphism
// item is not enqueued for k_brent.  DevArgs::mono_dn = 1: k_prep evaluates it; 2: the QUAD kernel's cfg-1 items form it
// from their hoisting (brent_select takes the QUAD kernel for list 0 exactly then).
inline bool quad_plan(const Facts& f) { return f.quad && f.plan[0].T == 64 && (f.plan[0].S == 8 || f.plan[0].S == 16); }
inline int mono_dn(const Facts& f, const EngineSwitches& w) {
  const bool in_prep = f.denovo && f.numerics == PM_NUM_POLY && !f.quick_call && !f.vcf && f.chrom == PM_CHR_AUTO && !f.has_fp &&
                       f.plan[0].n_ext == 0 && f.n_fam > 1;
  return !in_prep ? 0 : (quad_plan(f) && !w.mono_dn_prep) ? 2 : 1;
}

// PM_BRENT_TS accepts these geometries
constexpr Geometry kForced[] = {{64, 1}, {64, 2}, {64, 4}, {128, 4}, {128, 16}, {256, 1}, {256, 4}, {512, 2}, {512, 4},
                                {1024, 1}, {1024, 2}, {1024, 4}, {1024, 8}, {128, 8}, {64, 8}, {64, 16}};
// Preference orders, {0, 0}-terminated.  One wave per item (T = 64, no barrier) wins while its slots fit the register
// file without scratch: up to S = 16 for the lean autosomal kernel, S = 8 for the generic one (de novo / founders-only
// units); beyond that the item is spread over 2-8 waves (one barrier per evaluation).  Sections on chrX/Y/MT run the
// generic kernel on the same plan.  (1025-2048 families: 2 waves x 16 slots, one two-wave exchange per evaluation,
// before 8 waves x 4.)
constexpr Geometry kLean[] = {{64, 1}, {64, 2}, {64, 4}, {64, 8}, {64, 16}, {128, 16}, {1024, 4}, {1024, 8}, {0, 0}};
constexpr Geometry kGeneric[] = {{64, 1}, {64, 2}, {64, 4}, {64, 8}, {256, 1}, {256, 4}, {512, 4}, {1024, 4}, {1024, 8}, {0, 0}};
// lean --denovo: the de novo hoisting state does not fit 16 slots per lane without spilling; 8 slots on 2 waves per
// item is faster (measured: 6.6 vs 6.1 M sites/s, 1000 quads) ...
constexpr Geometry kLeanDn[] = {{64, 1}, {64, 2}, {64, 4}, {64, 8}, {128, 8}, {512, 4}, {1024, 4}, {1024, 8}, {0, 0}};
// ... unless the PL bytes can be staged through LDS (dn_staging): then the 64 x 16 kernel with LDS-staged hoisting only
// has no spills and beats 2 waves x 8 slots (11.9 vs 9.8 M sites/s, 1000 quads)
constexpr Geometry kLeanDnPf[] = {{64, 1}, {64, 2}, {64, 4}, {64, 8}, {64, 16}, {512, 4}, {1024, 4}, {1024, 8}, {0, 0}};
// plans whose families are all peeled or all founder products (vcf_mode plan 1, --quick_call)
constexpr Geometry kPeeled[] = {{64, 1}, {64, 2}, {64, 4}, {64, 8}, {256, 4}, {512, 4}, {1024, 4}, {1024, 8}, {0, 0}};

inline const Geometry* preference(const Facts& f, const EngineSwitches& w) {
  return generic_plan(f) ? kGeneric : !f.denovo ? kLean : dn_staging(f, w) ? kLeanDnPf : kLeanDn;
}

// Plan 0's geometry: PM_BRENT_TS when it names a geometry that holds the pedigree, else the first of the preference
// order that does; {0, 0} when none does.  fits(T, S): does the pedigree fit T lanes x S slots (plan_units).
template <class Fits>
Geometry choose_geometry(const Facts& f, const EngineSwitches& w, Fits fits) {
  for (const Geometry g : kForced)
    if (g.T == w.ts_t && g.S == w.ts_s && fits(g.T, g.S)) return g;
  // extended families are the expensive terms: spread them one per lane up to 256 lanes (polynomial form: up to PM_EPE
  // per lane, their coefficients in registers, one wave per item; --denovo too: the 10-state peels are hoisted by the
  // schedule compiler's es_hoist_wave and k_brent only evaluates their coefficients; the reference-order 10-state peel
  // of PRODUCT / EXACT numerics keeps one per lane)
  const int per_lane = (f.es_poly && !(f.denovo && w.ep_dn_one)) ? kEpe : 1;
  int tmin = 1;
  while (tmin < std::min((f.plan[0].n_ext + per_lane - 1) / per_lane, 256)) tmin *= 2;
  for (const Geometry* g = preference(f, w); g->T; g++)
    if (g->T >= tmin && fits(g->T, g->S)) return *g;
  return {0, 0};
}

// The kernel of one Brent launch and the launch flavour that follows from it, before any device query.
struct BrentChoice {
  BrentKey key;
  bool quad = false, ep = false, ep_only = false;   // QUAD plan (hoist_quad); extended families in polynomial form; and no other unit
  int dn_pf = 0;                  // lean --denovo: PL windows staged through LDS (double buffer per wave)
  int pf_npad = 0, pf_stride = 0, pf_dw = 0;   // lean plain kernel: the item's 3 planes prefetched into LDS (4-B pieces: pf_dw)
  int qd_group = 1;               // QUAD: items of a site one wave takes in turn
  size_t lds = 0;                 // dynamic LDS the flavour asks for
};

// list: the item list (0-2); unrelated: the --quick_call plan's launches; plane_align: 16, 4 or 1, the batch's PL block's
// address alignment.
inline BrentChoice brent_select(const Facts& f, const EngineSwitches& w, int list, bool unrelated, int plane_align) {
  const LanePlan& p = f.plan[f.use_plan1 ? 1 : 0];
  const int T = unrelated ? f.quick.T : p.T, S = unrelated ? f.quick.S : p.S;
  // MakeUnrelated(): all-founder products, no ES, no de novo model; plan 1 and chrX/Y/MT: the generic kernel
  const bool gen = unrelated || f.use_plan1 || f.chrom != PM_CHR_AUTO || generic_plan(f);
  const bool dn = f.denovo && !unrelated, poly = f.numerics == PM_NUM_POLY, es = !unrelated && p.n_ext > 0;
  const bool lean = !gen && p.n_ext == 0;
  BrentChoice c;
  // lean plain kernel at one wave per item (or 128 x 16, one buffer for its two waves): LDS-DMA plane prefetch, in 16-B
  // pieces when the planes are 16-B aligned (n_person % 16 == 0 and the block), else 4-B
  const bool al16 = f.n_person % 16 == 0 && plane_align >= 16, al4 = f.n_person % 4 == 0 && plane_align >= 4;
  const int npad = (f.n_person + 1023) / 1024 * 1024;
  if (lean && !dn && (T == 64 || (T == 128 && S == 16)) && poly && f.max_nuc <= 4 && (al16 || al4) && f.n_person >= 16 &&
      npad * 3 <= 60 * 1024 && !w.no_prefetch) {
    c.pf_npad = npad;
    c.pf_stride = npad + 16;
    c.pf_dw = al16 ? 0 : 1;
    c.lds = (size_t)3 * c.pf_stride;
  }
  // lean --denovo kernel: QUAD plans take their own kernel (list 0 holds cfgs 1-3 of each called site and list 1 cfgs
  // 4-6, consecutive and site-aligned: PM_QD_GROUP=3 lets one wave take a site's three in turn); other plans stage
  c.quad = lean && dn && poly && quad_plan(f);
  if (c.quad) c.lds = kQWave;
  if (c.quad && mono_dn(f, w) == 2 && list <= 1) c.qd_group = w.qd_group;
  if (!c.quad && lean && dn_staging(f, w) && S % kDnPfC == 0) {
    c.dn_pf = 1;
    c.lds = (size_t)(T / 64) * 2 * kDnPfBuf;
  }
  c.ep = es && f.es_poly && poly;
  c.ep_only = c.ep && p.units_empty && !w.no_ep_only;
  // numerics: PRODUCT / EXACT for every flavour, POLY only for the lean kernels (the generic and ES ones take PRODUCT)
  const int num = f.numerics == PM_NUM_EXACT ? PM_NUM_EXACT : PM_NUM_PRODUCT;
  if (c.quad) c.key = {64, S, PM_NUM_POLY, false, false, true, false, false, true, 0, kPdLo};
  else if (c.ep)   // one-wave plans: NF = 1 compiles the nuclear machinery out of ep_only ones; PD = PM_PD_HI keeps degrees
                   // above PM_PD_LO in the register tile (higher degrees: the coefficient buffer)
    c.key = {T, S, PM_NUM_PRODUCT, true, true, dn, false, true, false, (c.ep_only && !w.no_epo && T == 64 && (S == 1 || S == 2 || S == 4)) ? 1 : 0,
             (p.ep_dmax > kPdLo && !w.no_pd_hi && T == 64) ? kPdHi : kPdLo};
  else if (lean && dn && poly)   // PF: the 64 x 16 kernel hoists from staged windows only; the others choose at run time
    c.key = {T, S, PM_NUM_POLY, false, false, true, c.dn_pf && T == 64 && S == 16, false, false, 0, kPdLo};
  else if (c.pf_npad > 0)   // NF: split trio / quad plans 34, trio plans 3
    c.key = {T, S, PM_NUM_POLY, false, false, false, true, false, false, (f.split34 && S == 16) ? 34 : (f.all_trio && !w.no_trio) ? 3 : 0, kPdLo};
  else if (es) c.key = {T, S, num, true, true, false, false, false, false, 0, kPdLo};   // reference-order peels
  else c.key = {T, S, gen ? num : f.numerics, gen, false, false, false, false, false, 0, kPdLo};
  return c;
}

}   // namespace pmplan
