"""The kernels on sites the synthetic generator never makes (tests/hard_sites.py): transversions and non-reference
allele pairs (maxidx 2-6, cfgs 4-6 on objectives that are not flat), ten dense PL bytes per person, records of
tests/golden/example, missing persons and families, extreme depths and mapping qualities, Mendelian errors with
saturated bytes, bad reference bases -- interleaved site by site, so called, filtered and bad-ref sites alternate inside
one k_prep block and the item lists are compacted around holes.

tests/test_gpu_brent_variants.py varies the kernel on generator data; this file takes one of its recipes per way the PL
bytes reach the arithmetic (the QUAD LDS ring, the 16-B / 4-B plane prefetch, the --denovo ten-plane staging, direct
loads, the generic kernel, the ES peels in polynomial and reference order, multi-wave plans), the JIT-fused kernel and
a --quick_call run, and runs each on hard_block() of the recipe's own pedigree against the CPU oracle, which
tests/test_cpu_oracle.py pins on the same builder's sites by the reference (the hard_* cases)."""
import numpy as np
import pytest

import hard_sites as hs
import polymutt_amd as pm
from oracle_binding import Oracle
from parity import compare_results
from test_gpu_brent_variants import AUTO, K, P, RECIPES, Y, Recipe, _params

SITES_NUC, SITES_EXT = 96, 48
SEED = 17
NAMES = ["64x16-quad", "64x8-quad", "64x16-lean-dn-pf", "64x16-lean-dn", "512x4-lean-dn", "64x16-pf", "128x16-pf",
         "64x16-pf-trio", "64x16-pf-split34", "64x1-lean-product", "64x16-lean-exact", "1024x4-lean-poly",
         "64x8-generic-product-chrX", "256x4-generic-exact-dn", "64x8-ep-dn", "64x8-ep", "64x2-ep-only", "64x8-ep-hi-dn",
         "64x8-es-product", "64x8-es-exact", "512x4-ep"]
_BY_NAME = {r.name: r for r in RECIPES}
# not in the variant table (ts None: the engine's own plan, asserted): extended pedigrees only, POLY, no --denovo, no
# switches -- the JIT-fused hoisting + Brent kernel, no k_brent launch; and --quick_call, whose pre-filter runs the
# generic PRODUCT kernel on the unrelated plan before the lean one on the family plan (plan_units keeps a family's
# <= 3-person founder chunks on one lane: a trio is one chunk, a quad two, and the quads among families 65-73 find no
# lane of 64 x 2 with two free slots, so that plan is 64 x 4)
EXTRA = [(Recipe("fused-ext10", "ext10+dn", 8, Y, 0, AUTO, {}, None, []), (64, 1), {}),
         (Recipe("quick-mixed73", "mixed+dn", 73, Y, 0, AUTO, {}, None, [K(64, 2, Y), K(64, 4, P, 1)]), (64, 2),
          {"quick_call": 1})]
RUNS = [(_BY_NAME[n], _BY_NAME[n].ts, {}) for n in NAMES] + EXTRA

_data, _oracle = {}, {}


def _block(r, tmp_root):
    dk = (r.shape, r.n_fam)
    if dk not in _data:
        nuclear = r.shape.split("+")[0] in ("quad", "trio", "mixed")
        ped = hs.load_pedigree(tmp_root, r.shape, r.n_fam)
        b = hs.hard_block(ped, SITES_NUC if nuclear else SITES_EXT, SEED, hs.ALL if nuclear else hs.EXTENDED_CLASSES)
        for a in b:
            a.setflags(write=False)
        _data[dk] = (ped,) + b
    return _data[dk]


def _par(r, extra):
    par = _params(r)
    for k, v in extra.items():
        setattr(par, k, v)
    return par


def _finite_where_called(o, oc, what):
    called = o["status"] == 0
    for k in range(7):
        assert np.isfinite(o["varllk"][called & (o["n_cfg"] > k), k]).all(), (what, k)
    em = o["emit"] != 0
    assert np.isfinite(o["af"][em]).all() and np.isfinite(o["denovo_lr"][em]).all() and np.isfinite(oc["dosage"]).all(), what


def workload(r, extra, tmp_root):
    """The recipe's pedigree, its hard block and the oracle's (results, calls, counters), each computed once."""
    ped, pl, dm, ref, cls = _block(r, tmp_root)
    ok = (r.shape, r.n_fam, r.denovo, r.chrom) + tuple(sorted(extra.items()))
    if ok not in _oracle:
        ora = Oracle(ped.view, _par(r, extra))
        ora.begin_section(r.chrom)
        o, oc = ora.run(pl, dm, ref)
        o.setflags(write=False)
        oc.setflags(write=False)
        _finite_where_called(o, oc, ok)   # (the `mendel` bytes saturate no likelihood of the oracle's)
        called = o["status"] == 0
        assert (o["status"][cls == "badref"] == 5).all() and called[cls != "badref"].sum() > 0
        if not extra and r.chrom == AUTO:   # what the classes are for (tests/test_cpu_hard_sites.py, at this size)
            assert set(o["maxidx"][called].tolist()) >= {0, 1, 2, 3, 4, 5, 6}, ok
            assert (o["n_cfg"][cls == "nonref"] == 7).all(), ok
        _oracle[ok] = (o, oc, ora.counters().as_array())
    return (ped, pl, dm, ref, cls) + _oracle[ok]


def _class_errors(e, o, cls):
    """Largest relative error of varllk[k < n_cfg] per class, over the sites the oracle called."""
    out = {}
    for c in dict.fromkeys(cls.tolist()):
        worst = 0.0
        for k in range(7):
            m = (cls == c) & (o["status"] == 0) & (o["n_cfg"] > k)
            if m.any():
                worst = max(worst, float((np.abs(e["varllk"][m, k] - o["varllk"][m, k]) / np.maximum(np.abs(o["varllk"][m, k]), 1e-300)).max()))
        out[c] = worst
    return out


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("hard_sites_gpu")


@pytest.mark.gpu
@pytest.mark.parametrize("recipe,plan,extra", RUNS, ids=[r[0].name for r in RUNS])
def test_hard_sites_match_oracle(built, tmp_root, monkeypatch, recipe, plan, extra):
    r = recipe
    ped, pl, dm, ref, cls, o, oc, ocnt = workload(r, extra, tmp_root)
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    if r.ts:
        monkeypatch.setenv("PM_BRENT_TS", "%d,%d" % r.ts)
    eng = pm.Engine(ped.view, _par(r, extra), max_batch=len(ref))
    try:
        assert eng.plan() == plan
        if r.chrom != AUTO:
            eng.begin_section(r.chrom)
        e, ec = eng.run(pl, dm, ref)
        for c, err in _class_errors(e, o, cls).items():
            print(f"hard {r.name} {c} max varllk rel err {err:.3g}")
        print(f"hard {r.name} variants {eng.brent_variants()}")
        st = compare_results(e, o, ec, oc, label=r.name + " ")
        assert st["called"] > 0 and st["emitted"] > 0
        assert (eng.counters().as_array() == ocnt).all(), (eng.counters().as_array(), ocnt)
        assert sorted(eng.brent_variants()) == sorted(r.expect), r.name
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["64x16-pf", "512x4-lean-dn"])
def test_filtered_sites_between_called_ones(built, tmp_root, monkeypatch, name):
    """hard_sites.filter_params: one site exactly on each filter's threshold, one just beyond it.  The engine's statuses
    are exactly the expected ones (k_prep's depth sum, samples-with-data share and average mapping quality), its filter
    counters the oracle's, and the called sites lying between filtered and bad-ref ones match the oracle."""
    r = _BY_NAME[name]
    ped, pl, dm, ref, cls = _block(r, tmp_root)
    par, want = hs.filter_params((pl, dm, ref, cls), numerics=r.numerics, denovo=r.denovo, denovo_mut_rate=_params(r).denovo_mut_rate)
    ora = Oracle(ped.view, par)
    o, oc = ora.run(pl, dm, ref)
    assert (o["status"] == want).all()
    _finite_where_called(o, oc, name)
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PM_BRENT_TS", "%d,%d" % r.ts)
    eng = pm.Engine(ped.view, par, max_batch=len(ref))
    try:
        assert eng.plan() == r.ts
        e, ec = eng.run(pl, dm, ref)
        assert (e["status"] == want).all(), np.nonzero(e["status"] != want)[0]
        st = compare_results(e, o, ec, oc, label=name + " filters ")
        assert st["called"] == (want == 0).sum() > 0 and st["emitted"] > 0
        c = eng.counters()
        assert [c.min_total_depth_filter, c.max_total_depth_filter, c.min_ps_filter, c.min_map_qual_filter] == \
            [int((want == k).sum()) for k in (1, 2, 3, 4)]
        assert (c.as_array() == ora.counters().as_array()).all()
        assert sorted(eng.brent_variants()) == sorted(r.expect)
    finally:
        eng.close()
