"""Every k_brent instantiation of polymutt_amd/csrc/brent_variants.h is launched on the GPU and compared with the CPU
oracle.  tests/test_cpu_brent_plan.py proves that every variant is selected by some case; this file proves that every
variant computes the right likelihoods.

A recipe is a workload (pedigree shape, family count, parameters, chromosome class), environment switches, a lane-plan
geometry forced with PM_BRENT_TS, and the variant the engine must launch for it.  The test asserts the plan (a forced
geometry that does not hold the pedigree is silently ignored), runs the sites, compares with parity.compare_results at
its usual tolerances and asserts pm_engine_brent_variants() == the recipe's variants.  test_every_variant_ran closes the
loop: the recipes' variants are exactly the parsed table, each named by one recipe.

Workloads vary the kernel, not the data: every site comes from the synthetic generator (shape "+dn": a planted de novo
child, so --denovo runs reach cfg-7 items); tests/test_gpu_hard_sites.py runs a subset of these recipes on the sites the
generator never makes (tests/hard_sites.py).  An oracle result depends on neither the geometry, the switches nor the
numerics and is computed once per (workload, --denovo, class).

Family counts (plan_units deals families to lanes family-major and round-robin, so slot row 1 fills once n_fam > T):
T - 8 families for S = 1 (phantom lanes in the last wave; two or more waves hold families when T > 64), T + 8 for
S > 1 (two slot rows hold families, the second mostly phantoms); + 1 for the `mixed` pedigrees that must not have
n_person % 4 == 0 (n_fam = 1 mod 8 gives n_person = 3 mod 4: no plane prefetch, no --denovo staging, no QUAD plan).
Quads give n_person % 16 == 0 (16-B prefetch pieces), the trio counts n_person % 16 == 8 (4-B pieces), 80 trios
n_person % 16 == 0 (--denovo staging).  Extended-family workloads hold 8 pedigrees (the serial oracle peels 10 states
under --denovo), so on one-wave plans their lanes' slot rows are empty; on the multi-wave plans the `quadext` shape
puts 1, 2 or 4 ext10 pedigrees next to T + 7 quads, whose units fill every wave."""
import collections
import os
import re
import shutil

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import ROOT
from oracle_binding import Oracle
from parity import compare_results

P, X, Y = pm.NUM_PRODUCT, pm.NUM_EXACT, pm.NUM_POLY
AUTO, CHRX, CHRY, CHRMT = pm.PM_CHR_AUTO, pm.PM_CHR_X, pm.PM_CHR_Y, pm.PM_CHR_MT
SITES_NUC, SITES_EXT = 64, 48
# Generator seeds, fixed per dataset.  A site gets cfgs 4-6 (item list 1 of a --denovo batch, n_cfg == 7) only when the
# first four leave var_post_prob < 0.99, about one site in a thousand of these pedigrees: the datasets that run under
# --denovo take the first seed whose sites hold one (searched once on the CPU oracle; workload() asserts it).
SEED = 13
SEEDS = {("ext10+dn", 8): 34, ("extmix+dn", 8): 34, ("mixed+dn", 57): 19, ("quad+dn", 72): 21, ("mixed+dn", 73): 34,
         ("trio+dn", 80): 4, ("mixed+dn", 137): 5, ("quadext+dn", 264): 2, ("mixed+dn", 265): 2, ("quadext+dn", 520): 7,
         ("mixed+dn", 521): 6, ("mixed+dn", 1017): 28, ("quadext+dn", 1032): 12, ("mixed+dn", 1033): 12}


def K(T, S, NUM, GEN=0, ES=0, DN=0, PF=0, EP=0, QD=0, NF=0, PD=8):
    """k_brent's template arguments in order, with the generator's defaults."""
    return (T, S, NUM, GEN, ES, DN, PF, EP, QD, NF, PD)


def parse_variants():
    """The PM_BRENT_X(part, T, S, NUM, GEN, ES, DN, PF, EP, QD, NF, PD) lines of brent_variants.h as 11-tuples."""
    word = {"PM_NUM_PRODUCT": P, "PM_NUM_EXACT": X, "PM_NUM_POLY": Y, "false": 0, "true": 1}
    text = open(os.path.join(ROOT, "polymutt_amd", "csrc", "brent_variants.h")).read()
    out = []
    for args in re.findall(r"^\s*PM_BRENT_X\(([^)]*)\)", text, re.M):
        a = [s.strip() for s in args.split(",")]
        assert len(a) == 12, args
        out.append(tuple(word[s] if s in word else int(s) for s in a[1:]))
    return out


Recipe = collections.namedtuple("Recipe", "name shape n_fam numerics denovo chrom env ts expect")


def _n(T, S, odd=False):
    return (T - 8 if S == 1 else T + 8) + (1 if odd else 0)


def _ext(T, S, shape64="ext10+dn"):
    """The extended-family workload of a geometry (module docstring)."""
    if T == 64:
        return shape64, 8
    return ("ext10+dn", 8) if (T, S) == (256, 1) else ("quadext+dn", T + 8)


ES_GEOS = [(64, 1), (64, 2), (64, 4), (64, 8), (256, 1), (256, 4), (512, 4), (1024, 4), (1024, 8)]
PLAIN_GEOS = [(64, 1), (64, 2), (64, 4), (64, 8), (64, 16), (128, 4), (128, 8), (128, 16), (256, 4), (512, 2), (512, 4),
              (1024, 1), (1024, 2), (1024, 4), (1024, 8)]
LEAN_DN_GEOS = [(64, 1), (64, 2), (64, 4), (64, 8), (64, 16), (128, 8), (512, 4), (1024, 4), (1024, 8)]
PF_GEOS = [(64, 1), (64, 2), (64, 4), (64, 8), (64, 16), (128, 16)]


def _recipes():
    R = []

    def add(name, shape, n_fam, numerics, denovo, chrom, env, ts, expect):
        R.append(Recipe(f"{ts[0]}x{ts[1]}-{name}", shape, n_fam, numerics, denovo, chrom, dict(env), ts, [expect]))

    # QUAD: every family a quad in person order, n_person % 16 == 0, POLY --denovo
    for S in (8, 16):
        add("quad", "quad+dn", 72, Y, 1, AUTO, {}, (64, S), K(64, S, Y, DN=1, QD=1))
    # lean --denovo that compiles only the LDS-staged hoisting: trios (no QUAD plan), n_person % 16 == 0
    add("lean-dn-pf", "trio+dn", 80, Y, 1, AUTO, {}, (64, 16), K(64, 16, Y, DN=1, PF=1))
    # lean --denovo without PF, direct loads (n_person % 4 == 3: no staging, no QUAD plan), 64 x 16 included
    for T, S in LEAN_DN_GEOS:
        add("lean-dn", "mixed+dn", _n(T, S, True), Y, 1, AUTO, {}, (T, S), K(T, S, Y, DN=1))
    # lean plain PF: any-size (quads, 16-B pieces), trio plans (4-B pieces), split trio / quad plans (4-B pieces)
    for T, S in PF_GEOS:
        add("pf", "quad+dn", _n(T, S), Y, 0, AUTO, {}, (T, S), K(T, S, Y, PF=1))
        add("pf-trio", "trio+dn", _n(T, S), Y, 0, AUTO, {}, (T, S), K(T, S, Y, PF=1, NF=3))
    for T in (64, 128):
        add("pf-split34", "mixed+dn", _n(T, 16), Y, 0, AUTO, {}, (T, 16), K(T, 16, Y, PF=1, NF=34))
    # extended families in polynomial form (POLY).  One-wave plans of pedigrees with extended families only take the
    # fused kernel (no k_brent) unless --denovo, PM_NO_FUSED or PM_NO_EP_ONLY; their 64 x {1, 2, 4} plans take NF = 1
    # unless PM_NO_EPO (ep_only stays a run-time mode of the NF = 0 kernel) or PM_NO_EP_ONLY (it does not)
    for T, S in ES_GEOS:
        for dn in (1, 0):
            shape, n = _ext(T, S)
            env = {}
            if T == 64 and S <= 4:
                env["PM_NO_EPO"] = "1"
            if T == 64 and not dn:
                env["PM_NO_FUSED"] = "1"
            add("ep" + "-dn" * dn, shape, n, Y, dn, AUTO, env, (T, S), K(T, S, P, 1, 1, dn, EP=1))
    for S in (1, 2, 4):
        for dn in (1, 0):
            add("ep-only" + "-dn" * dn, "ext10+dn", 8, Y, dn, AUTO, {} if dn else {"PM_NO_FUSED": "1"}, (64, S),
                K(64, S, P, 1, 1, dn, EP=1, NF=1))
    # ... with 5 or 6 founders per pedigree (extmix: roof2 and ext12 reach degree 12): PD = 12
    for S in (1, 2, 4, 8):
        for dn in (1, 0):
            env = {"PM_NO_EP_ONLY": "1"} if S <= 4 else {} if dn else {"PM_NO_FUSED": "1"}
            add("ep-hi" + "-dn" * dn, "extmix+dn", 8, Y, dn, AUTO, env, (64, S), K(64, S, P, 1, 1, dn, EP=1, PD=12))
    for S in (1, 2, 4):
        for dn in (1, 0):
            add("ep-only-hi" + "-dn" * dn, "extmix+dn", 8, Y, dn, AUTO, {} if dn else {"PM_NO_FUSED": "1"}, (64, S),
                K(64, S, P, 1, 1, dn, EP=1, NF=1, PD=12))
    # reference-order peels (PRODUCT and EXACT numerics)
    for T, S in ES_GEOS:
        shape, n = _ext(T, S)
        add("es-product", shape, n, P, 0, AUTO, {}, (T, S), K(T, S, P, 1, 1))
        add("es-exact", shape, n, X, 0, AUTO, {}, (T, S), K(T, S, X, 1, 1))
    # the 15 plain geometries: lean PRODUCT / EXACT / POLY without PF (n_person % 4 == 3) on the autosome, the generic
    # kernel on a chrX section (PRODUCT) and under the reference-order --denovo model (EXACT)
    for T, S in PLAIN_GEOS:
        n = _n(T, S, True)
        add("lean-product", "mixed+dn", n, P, 0, AUTO, {}, (T, S), K(T, S, P))
        add("lean-exact", "mixed+dn", n, X, 0, AUTO, {}, (T, S), K(T, S, X))
        add("lean-poly", "mixed+dn", n, Y, 0, AUTO, {}, (T, S), K(T, S, Y))
        add("generic-product-chrX", "mixed+dn", n, P, 0, CHRX, {}, (T, S), K(T, S, P, 1))
        add("generic-exact-dn", "mixed+dn", n, X, 1, AUTO, {}, (T, S), K(T, S, X, 1))
    return R


RECIPES = _recipes()


def _cross():
    """Run-time modes that share one instantiation, at two non-default multi-wave geometries: chrX, chrY, chrMT and
    --denovo with PRODUCT numerics on the generic kernel (nuclear pedigree) and on the reference-order ES kernel (quads
    with ext10 pedigrees among them; its key is the same with and without --denovo)."""
    R = []
    for T in (256, 1024):
        for tag, dn, chrom in (("chrX", 0, CHRX), ("chrY", 0, CHRY), ("chrMT", 0, CHRMT), ("dn", 1, AUTO)):
            R.append(Recipe(f"{T}x4-generic-{tag}", "mixed+dn", T + 9, P, dn, chrom, {}, (T, 4), [K(T, 4, P, 1)]))
            R.append(Recipe(f"{T}x4-es-{tag}", "quadext+dn", T + 8, P, dn, chrom, {}, (T, 4), [K(T, 4, P, 1, 1)]))
    return R


CROSS = _cross()

# geometries PM_BRENT_TS accepts but no kernel exists for (none_keys of tests/golden/brent_plan/selection_sha256.json):
# lean at 256 x 1, lean --denovo at 128 x 4, EP at 128 x 8
MISSING = [Recipe("256x1-lean-poly", "mixed+dn", 249, Y, 0, AUTO, {}, (256, 1), []),
           Recipe("128x4-lean-dn", "mixed+dn", 137, Y, 1, AUTO, {}, (128, 4), []),
           Recipe("128x8-ep", "ext10+dn", 8, Y, 0, AUTO, {}, (128, 8), [])]

_data, _oracle = {}, {}


def _params(r):
    return pm.Params.defaults(numerics=r.numerics, denovo=r.denovo, denovo_mut_rate=1e-5 if r.denovo else 1.5e-8)


def workload(r, tmp_root):
    """(pedigree, pl, dm, ref) of the recipe's dataset and the oracle's (results, calls) for its parameters, each computed
    once; the oracle's result is checked to exercise what the recipe is for."""
    dk = (r.shape, r.n_fam)
    if dk not in _data:
        d = os.path.join(str(tmp_root), f"{r.shape}_{r.n_fam}")
        nuclear = r.shape.split("+")[0] in ("quad", "trio", "mixed")
        pm.synth_write_dataset(d, r.shape, r.n_fam, SITES_NUC if nuclear else SITES_EXT, SEEDS.get(dk, SEED))
        ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
        cwd = os.getcwd()
        os.chdir(d)
        try:
            rd = pm.GlfReader(ped, "test.gif")
            (pos, ref, pl, dm), = [rd.read(1024) for _ in rd.sections()]
            rd.close()
        finally:
            os.chdir(cwd)
        shutil.rmtree(d)   # (one GLF file per person)
        for a in (ref, pl, dm):
            a.setflags(write=False)
        _data[dk] = (ped, pl, dm, ref)
    ped, pl, dm, ref = _data[dk]
    ok = dk + (r.denovo, r.chrom)
    if ok not in _oracle:
        ora = Oracle(ped.view, _params(r))
        ora.begin_section(r.chrom)
        o, oc = ora.run(pl, dm, ref)
        o.setflags(write=False)
        oc.setflags(write=False)
        assert (o["status"] == 0).sum() > 0 and (o["emit"] != 0).sum() > 0, ok
        if r.denovo:   # cfgs 4-6 too: all three item lists non-empty
            assert (o["n_cfg"][o["status"] == 0] == 7).any(), ok
        _oracle[ok] = (o, oc)
    return (ped, pl, dm, ref) + _oracle[ok]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("brent_variants")


def _run_recipe(r, tmp_root, monkeypatch):
    ped, pl, dm, ref, o, oc = workload(r, tmp_root)
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PM_BRENT_TS", "%d,%d" % r.ts)
    eng = pm.Engine(ped.view, _params(r), max_batch=len(ref))
    try:
        assert eng.plan() == r.ts   # (a geometry that does not hold the pedigree falls back to the preference order)
        assert eng.brent_variants() == []
        if r.chrom != AUTO:
            eng.begin_section(r.chrom)
        e, ec = eng.run(pl, dm, ref)
        st = compare_results(e, o, ec, oc, label=r.name + " ")
        assert st["called"] > 0 and st["emitted"] > 0
        assert sorted(eng.brent_variants()) == sorted(r.expect), r.name
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", RECIPES, ids=[r.name for r in RECIPES])
def test_variant_matches_oracle(built, tmp_root, monkeypatch, recipe):
    _run_recipe(recipe, tmp_root, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", CROSS, ids=[r.name for r in CROSS])
def test_runtime_modes_of_one_variant(built, tmp_root, monkeypatch, recipe):
    _run_recipe(recipe, tmp_root, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("recipe", MISSING, ids=[r.name for r in MISSING])
def test_geometry_without_kernel_is_an_error(built, tmp_root, monkeypatch, recipe):
    """A forced geometry the selection has no instantiation for: the run fails in the host-side lookup before any
    k_brent launch, the engine closes, and a fresh engine on its preferred plan matches the oracle."""
    r = recipe
    ped, pl, dm, ref, o, oc = workload(r, tmp_root)
    monkeypatch.setenv("PM_BRENT_TS", "%d,%d" % r.ts)
    eng = pm.Engine(ped.view, _params(r), max_batch=len(ref))
    try:
        assert eng.plan() == r.ts
        with pytest.raises(RuntimeError, match="no kernel variant for the lane plan"):
            eng.run(pl, dm, ref)
        assert eng.brent_variants() == []
    finally:
        eng.close()
    monkeypatch.delenv("PM_BRENT_TS")
    eng = pm.Engine(ped.view, _params(r), max_batch=len(ref))
    try:
        assert eng.plan() != r.ts
        e, ec = eng.run(pl, dm, ref)
        assert compare_results(e, o, ec, oc, label=r.name + " preferred plan ")["called"] > 0
    finally:
        eng.close()


def test_every_variant_ran():
    """The recipes of test_variant_matches_oracle name every instantiation of brent_variants.h exactly once and nothing
    else, so with that test's per-recipe equality every instantiation ran and matched the oracle; a variant added to
    tools/gen_brent_variants.py without a recipe fails here."""
    table = parse_variants()
    assert len(table) == len(set(table)) == 157
    named = [k for r in RECIPES for k in r.expect]
    dup = [k for k, c in collections.Counter(named).items() if c > 1]
    assert not dup, f"variants named by more than one recipe: {dup}"
    assert sorted(set(table) - set(named)) == [], "variants without a recipe"
    assert sorted(set(named) - set(table)) == [], "recipes that name no instantiation"
