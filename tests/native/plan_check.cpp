// plan_check.cpp -- the k_brent selection (polymutt_amd/csrc/brent_plan.h) enumerated against the variant list
// (brent_variants.h) without a device (tests/test_cpu_brent_plan.py):
//   plan_check cases NUMERICS DENOVO CHROM    one line per case of the slice: the case, then the kernel's template
//                                             arguments and launch flavour, or `none` (no such instantiation)
//   plan_check summary                        over all slices: the case count, the instantiations asked for but missing
//                                             (exit 1 if a default geometry asks for one), the variants never selected
//   plan_check geometry N_FAM N_PERSON MAX_NUC DENOVO NUMERICS    choose_geometry for a pedigree of nuclear families
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "brent_plan.h"
#include "brent_variants.h"

using namespace pmplan;

#define PM_BRENT_X(part, ...) BrentKey{__VA_ARGS__},
static const std::vector<BrentKey> kTable = {PM_BRENT_VARIANTS};
#undef PM_BRENT_X

static int table_index(const BrentKey& k) {
  for (size_t i = 0; i < kTable.size(); i++)
    if (kTable[i] == k) return (int)i;
  return -1;
}
static std::string key_text(const BrentKey& k) {
  char b[96];
  snprintf(b, sizeof(b), "%d,%d,%d,%d%d%d%d%d%d,%d,%d", k.T, k.S, k.NUM, k.GEN, k.ES, k.DN, k.PF, k.EP, k.QD, k.NF, k.PD);
  return b;
}

struct Case {
  Facts f;
  EngineSwitches w;
  bool unrelated = false, forced = false;   // forced: plan 0's geometry comes from PM_BRENT_TS
  int list = 0, align = 16, mode = 0, shape = 0;
  const char* sw = "-";
};

// The selection of one case as text.
static std::string select_text(const Case& c) {
  const BrentChoice r = brent_select(c.f, c.w, c.list, c.unrelated, c.align);
  if (table_index(r.key) < 0) return "none";
  char b[200];
  snprintf(b, sizeof(b), "%s pf %d/%d/%d dnpf %d quad %d ep %d%d grp %d lds %zu", key_text(r.key).c_str(), r.pf_npad, r.pf_stride, r.pf_dw,
           r.dn_pf, r.quad, r.ep, r.ep_only, r.qd_group, r.lds);
  return b;
}

// modes: 0 plain, 1 --quick_call's launches on the family plan, 2 its launches on the unrelated plan, 3 vcf_mode on plan 0
// (autosome, several families), 4 vcf_mode on plan 1 (chrX/Y/MT or a single family: every family with offspring peeled)
// shape bits, then the combinations no pedigree has (plan_units, plan_split34, the QUAD test and es_poly of pm_engine_create)
enum { HAS_FP = 1, NFAM1 = 2, EXT = 4, ES_POLY = 8, EMPTY = 16, TRIO = 32, SPLIT34 = 64, QUAD = 128, DMAX12 = 256, NUC5 = 512, SHAPES = 1024 };
static bool shape_exists(int s, int mode, int numerics, int denovo) {
  auto has = [&](int b) { return (s & b) != 0; };
  if (has(EXT) && !has(HAS_FP) && mode != 4) return false;              // an extended family is not nuclear (plan 1 peels those too)
  if (has(EMPTY) && (!has(EXT) || has(TRIO | SPLIT34 | QUAD | NUC5))) return false;   // every family peeled: no nuclear unit
  if (has(TRIO) && has(SPLIT34 | QUAD | NUC5)) return false;
  if (has(HAS_FP) && has(SPLIT34 | QUAD)) return false;
  if (has(SPLIT34) && (has(QUAD | NFAM1 | NUC5) || denovo || numerics != PM_NUM_POLY)) return false;
  if (has(QUAD) && has(NFAM1 | NUC5)) return false;
  if (has(ES_POLY) && (numerics != PM_NUM_POLY || !(has(EXT) || mode >= 3))) return false;
  if (has(DMAX12) && !has(ES_POLY)) return false;
  if (has(NFAM1) && ((has(EXT) && !has(EMPTY) && mode != 4) || (has(HAS_FP) && has(TRIO)))) return false;
  return true;
}

// A preference order reaches *g only when no earlier geometry of at least tmin lanes holds as many families (tmin: 1
// without peeled families, else any power of two up to 256)
static bool reachable(const Geometry* order, const Geometry* g, bool ext) {
  for (int tmin = 1; tmin <= (ext ? 256 : 1); tmin *= 2) {
    bool ok = g->T >= tmin;
    for (const Geometry* e = order; e != g && ok; e++) ok = !(e->T >= tmin && e->T * e->S >= g->T * g->S);
    if (ok) return true;
  }
  return false;
}

struct Switch { const char* name; void (*set)(EngineSwitches&); };
static const Switch kSwitches[] = {   // each selection-relevant switch on its own
    {"-", [](EngineSwitches&) {}},
    {"NO_PREFETCH", [](EngineSwitches& w) { w.no_prefetch = true; }},
    {"MONO_DN_PREP", [](EngineSwitches& w) { w.mono_dn_prep = true; }},
    {"QD_GROUP=3", [](EngineSwitches& w) { w.qd_group = 3; }},
    {"NO_EP_ONLY", [](EngineSwitches& w) { w.no_ep_only = true; }},
    {"NO_EPO", [](EngineSwitches& w) { w.no_epo = true; }},
    {"NO_TRIO", [](EngineSwitches& w) { w.no_trio = true; }},
    {"NO_PD_HI", [](EngineSwitches& w) { w.no_pd_hi = true; }}};

template <class Visit>
static void for_each_case(int numerics, int denovo, int chrom, Visit visit) {
  for (int mode = 0; mode < 5; mode++)
    for (int s = 0; s < SHAPES; s++) {
      const bool vcf = mode >= 3, nfam1 = (s & NFAM1) != 0;
      if (vcf && denovo) continue;   // vcf_mode has no de novo model
      if ((mode == 3 && (chrom != PM_CHR_AUTO || nfam1)) || (mode == 4 && chrom == PM_CHR_AUTO && !nfam1)) continue;
      if (!shape_exists(s, mode, numerics, denovo)) continue;
      for (const Switch& sw : kSwitches)
        for (int np : {8, 12, 16}) {
          if ((s & (QUAD | SPLIT34)) && np != 16) continue;   // whole quads at 16-B aligned planes; a quad and a trio or four
          Case c;
          Facts& f = c.f;
          sw.set(c.w);
          c.sw = sw.name; c.mode = mode; c.shape = s;
          f.n_person = np; f.n_fam = nfam1 ? 1 : 5; f.chrom = chrom; f.numerics = numerics;
          f.max_nuc = (s & EMPTY) ? 0 : (s & TRIO) ? 3 : (s & NUC5) ? 5 : 4;
          f.denovo = denovo; f.quick_call = mode == 1 || mode == 2; f.vcf = vcf; f.use_plan1 = mode == 4;
          f.has_fp = s & HAS_FP; f.es_poly = s & ES_POLY; f.quad = s & QUAD; f.all_trio = s & TRIO; f.split34 = s & SPLIT34;
          c.unrelated = mode == 2;
          LanePlan& p = f.plan[mode == 4 ? 1 : 0];
          p.n_ext = (s & EXT) ? 3 : 0; p.units_empty = s & EMPTY; p.ep_dmax = (s & DMAX12) ? 12 : (s & ES_POLY) ? 8 : 0;
          // geometries: plan 0 forced by PM_BRENT_TS (every kForced) or by preference; the other plans by preference
          std::vector<std::pair<Geometry, bool>> geos;
          if (mode != 2 && mode != 4)
            for (const Geometry g : kForced) geos.push_back({g, true});
          const Geometry* order = (mode == 2 || mode == 4) ? kPeeled : preference(f, c.w);
          for (const Geometry* g = order; g->T; g++)
            if (reachable(order, g, mode != 2 && p.n_ext > 0)) geos.push_back({*g, false});
          for (const auto& [g, forced] : geos) {
            if (((s & QUAD) && g.T != 64) || ((s & SPLIT34) && (g.S != 16 || g.T > 128))) continue;
            if (mode == 2) { f.quick = g; f.plan[0] = {64, 8, p.n_ext, p.units_empty, p.ep_dmax}; }
            else { p.T = g.T; p.S = g.S; }
            for (int al : {16, 4, 1})
              for (int list = 0; list < 3; list++) {
                // lists: the unrelated plan runs 1 and 2; vcf_mode only 0; list 2 otherwise is --denovo's
                if (mode == 2 ? list == 0 : vcf ? list != 0 : (list == 2 && !denovo)) continue;
                c.align = al; c.list = list; c.forced = forced;
                visit(c, g);
              }
          }
        }
    }
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "cases")) {
    for_each_case(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), [](const Case& c, Geometry g) {
      printf("m%d s%03x %dx%d%s np%d al%d l%d %s -> %s\n", c.mode, c.shape, g.T, g.S, c.forced ? "!" : "", c.f.n_person, c.align, c.list, c.sw,
             select_text(c).c_str());
    });
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "summary")) {
    long cases = 0, bad = 0;
    std::vector<long> used(kTable.size(), 0);
    std::map<std::string, long> none;
    for (int num = 0; num < 3; num++)
      for (int dn = 0; dn < 2; dn++)
        for (int chrom = 0; chrom < 4; chrom++)
          for_each_case(num, dn, chrom, [&](const Case& c, Geometry) {
            const BrentKey k = brent_select(c.f, c.w, c.list, c.unrelated, c.align).key;
            const int i = table_index(k);
            cases++;
            if (i < 0) { none[key_text(k)]++; bad += !c.forced; }
            else used[i]++;
          });
    printf("cases %ld variants %zu\n", cases, kTable.size());
    for (const auto& [k, n] : none) printf("none %s (%ld cases)\n", k.c_str(), n);
    for (size_t i = 0; i < kTable.size(); i++)
      if (!used[i]) printf("unused %s\n", key_text(kTable[i]).c_str());
    if (bad) printf("FAIL: %ld cases with a default geometry have no kernel\n", bad);
    return bad ? 1 : 0;
  }
  if (argc == 7 && !strcmp(argv[1], "geometry")) {   // nuclear families: one unit each, so T x S slots hold T * S families
    Facts f;
    f.n_fam = atoi(argv[2]); f.n_person = atoi(argv[3]); f.max_nuc = atoi(argv[4]); f.denovo = atoi(argv[5]); f.numerics = atoi(argv[6]);
    const Geometry g = choose_geometry(f, EngineSwitches(), [&](int t, int s) { return f.n_fam <= t * s; });
    printf("%d %d\n", g.T, g.S);
    return 0;
  }
  fprintf(stderr, "usage: plan_check cases NUMERICS DENOVO CHROM | summary | geometry N_FAM N_PERSON MAX_NUC DENOVO NUMERICS\n");
  return 2;
}
