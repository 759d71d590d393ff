"""GPU tests of the joint call plane of the --in_vcf path (pm_engine_set_vcf_joint / pm_engine_vcf_joint, --vcf_joint).

* Optimality against the brute-force table of tests/vcf_joint_reference.py (the definition, without peeling or
  max-product; checked on the CPU by tests/test_cpu_vcf_joint.py) at the engine's own frequency, every row and family, on
  multi-family autosomal pedigrees: the table's J at the engine's assignment reaches the table's maximum to the project's
  relative likelihood tolerance, so a tie or near tie passes whichever way it fell; every trio of it is Mendelian-consistent.
* lp against log10(max / L) of the table; the same bytes within a family.
* Single-family prior mode, which the table does not restate: 10^lp is at most each member's posterior at its state.
* The plane is additive and deterministic: site results, genotype rows, the posterior plane, the phase plane and the de novo
  outputs are the same bytes with it on; the same plane run to run, across batch sizes and entry points; the schedule
  compiler does not change it; a stuck Brent keeps the returned rows; chrX / chrY / MT sections are (255, 0).
* A planted trio whose marginal calls no transmission allows gets the table's unique optimum.
* The CLI prints JG and JL and nothing else moves.

The tolerances are derived, not measured.  Optimality: 1e-9 relative, the project's likelihood tolerance (parity.py's
LK_RTOL is looser; 1e-9 is what the issue sets).  lp: one rounding of a double to float, 2^-24 relative, on top of the
project's DOSE_ATOL = 1e-9 for double-against-double arithmetic.  10^lp against a posterior that is a float itself, each
of them within 2^-25 of a value in [0, 1], and lp's own rounding moves 10^lp by less than another 2^-25: 3 x 2^-25.

Engine cases run 96 sites at max_batch = 64, so the second batch is partial; `extmix` has families of 11 and 12 members,
whose tables have up to 3^12 entries per site: it runs 16 sites at max_batch = 12.
"""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from parity import DOSE_ATOL
from test_brent_stuck import first_stuck, pick_itmax
from vcf_joint_reference import NONE, PLANTED_TRIO, PLANTED_TRIO_OWN_AF, JointFamilies, transmission, trio_block
import vcf_plane_common as common
from vcf_phase_reference import trio_pedigree

pytestmark = pytest.mark.gpu

OPT_RTOL = 1e-9
LP_RTOL = 2.0 ** -24
POST_ATOL = 3 * 2.0 ** -25 + DOSE_ATOL

# multi-family autosomal pedigrees, the smallest at which each kernel can still go wrong: two family sizes in one wave,
# more than 64 families (a lane takes a second family), the founder branch, peeled families alone (type 1 / 2 / 3 steps,
# marriage partials), one family of each of the five peel schedules; "nuclear": families of three and four children
# (k_vcf_joint_nuc's nuclear branch).  The synthetic shapes list the mother first in some families.
REF_CASES = [("mixed", 31), ("quad", 70), ("single", 12), ("ext10", 3), ("extmix", 5), ("nuclear", 0)]

def dataset(tmp_path_factory, shape, nfam):
    """(owner of the pedigree, its view, block, refalt, max_batch), generated once per case and left unchanged."""
    nsites, batch = (16, 12) if shape == "extmix" else (96, 64)
    return common.dataset(tmp_path_factory, "vj", shape, nfam, nsites) + (batch,)


def run_batches(eng, block, refalt, batch, entry="run", joint=True, post=False, phase=False):
    """Every batch through one entry point: (results, calls as (best, gq, label) int arrays, (g, lp) or None, posterior
    plane or None, phase plane or None)."""
    def fetch(c):
        a = b = None
        if joint:
            a, b = eng.vcf_joint()
            assert a.shape == b.shape == (len(c), eng.n_person) and a.dtype == np.uint8 and b.dtype == np.float32
        return a, b, eng.vcf_posteriors() if post else None, eng.vcf_phase() if phase else None
    res, calls, got = common.run_batches(eng, block, refalt, batch, entry, fetch)
    g, lp, po, ph = ([x[i] for x in got] for i in range(4))
    return (res, calls, (np.concatenate(g), np.concatenate(lp)) if joint else None,
            np.concatenate(po) if post else None, np.concatenate(ph) if phase else None)


def plane_bytes(j):
    return j[0].tobytes() + j[1].tobytes()


def check_plane(g, lp, fams, label):
    """What holds for every autosomal plane: states 0..2 or NONE, finite lp <= 0 (to its rounding), NONE and lp = 0
    together and for whole families, lp the same bytes within a family."""
    assert np.isin(g, (0, 1, 2, NONE)).all(), label
    assert np.isfinite(lp).all() and (lp <= 2.0 ** -23).all(), label
    assert (lp[g == NONE] == 0).all(), label
    for F in fams.fams:
        sl = slice(F["p0"], F["p0"] + F["m"])
        none = g[:, sl] == NONE
        assert (none.all(axis=1) | ~none.any(axis=1)).all(), label
        assert (lp[:, sl].view(np.uint32) == lp[:, sl.start:sl.start + 1].view(np.uint32)).all(), label


@pytest.mark.parametrize("numerics", [pm.NUM_POLY, pm.NUM_EXACT])
@pytest.mark.parametrize("shape,nfam", REF_CASES)
def test_joint_calls_are_optimal(built, tmp_path_factory, shape, nfam, numerics):
    ped, view, block, refalt, batch = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1, numerics=numerics), max_batch=batch)
    eng.set_vcf_joint(True)
    res, calls, (g, lp), _, _ = run_batches(eng, block, refalt, batch)
    eng.close()
    assert (res["call_row"] >= 0).all() and len(g) == len(refalt)   # every site of these blocks is written
    fams = JointFamilies(view)
    label = f"{shape} {nfam} numerics {numerics}"
    check_plane(g, lp, fams, label)
    sol = fams.solve(block, refalt, res["af"], g)
    consistent = fams.mendel_consistent(g)
    worst_opt = worst_lp = 0.0
    ties = 0
    for k, (F, r) in enumerate(zip(fams.fams, sol)):
        has = r["max"] > 0
        none = g[:, F["p0"]] == NONE
        assert (none == ~(has & (r["L"] > 0))).all(), (label, k)
        J = r["J_at"][has]
        # optimality: the table's J at the engine's assignment against the table's maximum -- every row, ties included
        short = 1 - J / r["max"][has]
        worst_opt = max(worst_opt, short.max(initial=0.0))
        assert (J >= r["max"][has] * (1 - OPT_RTOL)).all(), (label, k, short.max())
        assert (J > 0).all() and consistent[has, k].all(), (label, k)   # J > 0: every trio of it has T > 0
        ties += int((r["n_best"][has] > 1).sum())
        ref_lp = np.log10(r["max"][has] / r["L"][has])
        d = np.abs(lp[has, F["p0"]].astype(np.float64) - ref_lp)
        bound = LP_RTOL * np.abs(ref_lp) + DOSE_ATOL
        worst_lp = max(worst_lp, (d / bound).max(initial=0.0))
        assert (d <= bound).all(), (label, k, d.max(), np.argwhere(d > bound)[:5])
    print(f"{label}: largest 1 - J(engine) / max J = {worst_opt:.3g} (bound {OPT_RTOL:.3g}); largest |lp - reference| / "
          f"bound = {worst_lp:.3g}; {ties} rows x families with a tied maximum")
    assert (g != NONE).any()


@pytest.mark.parametrize("shape,nfam", [("quad", 1), ("ext10", 1)])
def test_single_family_prior_mode(built, tmp_path_factory, shape, nfam):
    """The lone quad (the fixed single-trio prior in the closed form) and the lone ext10 family (peeled), pinned through the
    oracle-pinned posterior plane: a joint assignment's posterior cannot exceed any member's marginal at its state."""
    ped, view, block, refalt, batch = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
    eng.set_vcf_joint(True)
    eng.set_vcf_posteriors(True)
    res, calls, (g, lp), post, _ = run_batches(eng, block, refalt, batch, post=True)
    eng.close()
    fams = JointFamilies(view)
    check_plane(g, lp, fams, f"{shape} {nfam}")
    has = g[:, 0] != NONE
    assert has.any()
    assert fams.mendel_consistent(g)[has].all()
    p_at = np.take_along_axis(post.astype(np.float64)[has], g[has].astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    over = 10.0 ** lp[has].astype(np.float64) - p_at
    print(f"{shape} {nfam}: largest 10^lp - posterior at g = {over.max():.3g} (bound {POST_ATOL:.3g}); {has.sum()} rows")
    assert (over <= POST_ATOL).all(), (over.max(), np.argwhere(over > POST_ATOL)[:5])


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("single", 12), ("extmix", 5), ("nuclear", 0)])   # lean, generic, peeled
def test_determinism_and_feature_off_identity(built, tmp_path_factory, shape, nfam):
    ped, view, block, refalt, batch = dataset(tmp_path_factory, shape, nfam)
    par = pm.Params.defaults(vcf_mode=1)
    plain = pm.Engine(view, par, max_batch=batch)   # never has the feature on (the posterior and phase planes it has)
    eng = pm.Engine(view, par, max_batch=batch)
    for e in (plain, eng):
        e.set_vcf_posteriors(True)
        e.set_vcf_phase(True)
    eng.set_vcf_joint(True)
    planes = []
    for entry in ("run", "run_vcf", "submit"):
        r0, c0, _, q0, h0 = run_batches(plain, block, refalt, batch, entry, joint=False, post=True, phase=True)
        r1, c1, j1, q1, h1 = run_batches(eng, block, refalt, batch, entry, post=True, phase=True)
        assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes(), entry
        assert q0.tobytes() == q1.tobytes() and h0.tobytes() == h1.tobytes(), entry
        planes.append(plane_bytes(j1))
    assert planes[0] == planes[1] == planes[2]
    assert plane_bytes(run_batches(eng, block, refalt, batch)[2]) == planes[0]   # run to run
    other = pm.Engine(view, par, max_batch=batch - 5)   # another batch size, an engine of its own
    other.set_vcf_joint(True)
    assert plane_bytes(run_batches(other, block, refalt, batch - 5)[2]) == planes[0]
    other.close()
    eng.set_vcf_joint(False)   # off again: the same bytes still, and no plane
    r0, c0, _, q0, h0 = run_batches(plain, block, refalt, batch, "run", joint=False, post=True, phase=True)
    r1, c1, _, q1, h1 = run_batches(eng, block, refalt, batch, "run", joint=False, post=True, phase=True)
    assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes() and q0.tobytes() == q1.tobytes() and h0.tobytes() == h1.tobytes()
    with pytest.raises(RuntimeError, match="feature is off"):
        eng.vcf_joint()
    eng.set_vcf_joint(True)   # on again: no batch has filled the new plane
    a, b = eng.vcf_joint()
    assert a.shape == b.shape == (0, eng.n_person)
    plain.close()
    eng.close()


@pytest.mark.parametrize("chrom", [pm.PM_CHR_X, pm.PM_CHR_Y, pm.PM_CHR_MT])
@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("ext10", 3)])
def test_no_joint_calls_off_the_autosomes(built, tmp_path_factory, shape, nfam, chrom):
    """A chrX / chrY / MT section's plane is (255, 0) everywhere -- also right after an autosomal batch filled it -- and the
    next autosomal section's is what it was."""
    ped, view, block, refalt, batch = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
    eng.set_vcf_joint(True)
    auto = run_batches(eng, block, refalt, batch)[2]
    assert (auto[0] != NONE).any()
    eng.begin_section(chrom)
    res, calls, (g, lp), _, _ = run_batches(eng, block, refalt, batch)
    assert len(g) == (res["call_row"] >= 0).sum() > 0 and (g == NONE).all() and (lp.view(np.uint32) == 0).all()
    eng.begin_section(pm.PM_CHR_AUTO)
    again = run_batches(eng, block, refalt, batch)[2]
    eng.close()
    assert plane_bytes(again) == plane_bytes(auto)


def test_setter_errors_and_denovo_outputs(built, tmp_path_factory):
    ped, view, block, refalt, batch = dataset(tmp_path_factory, "mixed", 31)
    glf = pm.Engine(view, pm.Params.defaults(), max_batch=batch)
    with pytest.raises(RuntimeError, match="vcf_mode"):
        glf.set_vcf_joint(True)
    glf.close()
    outs = []
    zeros = np.zeros(block.shape[:2], np.uint32)
    for with_joint in (False, True):
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_denovo(True)
        eng.set_vcf_denovo_detail(2, 2)
        if with_joint:
            eng.set_vcf_joint(True)
            eng.submit(block[:batch], zeros[:batch], refalt[:batch])
            lib = pm.load_library()
            assert lib.pm_engine_set_vcf_joint(eng.h, 0) == -1 and b"not been collected" in lib.pm_last_error()
            n = C.c_int32(0)
            assert lib.pm_engine_vcf_joint(eng.h, C.byref(n), None) == -1 and b"not been collected" in lib.pm_last_error()
            eng.collect()
        got = []
        for s in range(0, len(refalt), batch):
            sl = slice(s, s + batch)
            r, c = eng.run(block[sl], zeros[sl], refalt[sl])
            top_f, sum_f, _ = eng.vcf_denovo_families()
            top_c, _ = eng.vcf_denovo_carriers()
            got.append(b"".join(a.tobytes() for a in (r, c, eng.vcf_denovo_rows(), top_f, sum_f, top_c)))
            if with_joint:
                assert len(eng.vcf_joint()[0]) == len(c)
        if with_joint:   # neither feature switches the other off
            eng.set_vcf_denovo(False)
            eng.run(block[:batch], zeros[:batch], refalt[:batch])
            assert len(eng.vcf_joint()[0]) == batch
            eng.set_vcf_phase(True)
            eng.set_vcf_phase(False)
            eng.run(block[:batch], zeros[:batch], refalt[:batch])
            assert len(eng.vcf_joint()[0]) == batch
        outs.append(got)
        eng.close()
    assert outs[0] == outs[1]
    assert any((np.frombuffer(g, np.uint8) != 0).any() for g in outs[0])


def test_schedule_compiler_on_and_off(built, tmp_path_factory, monkeypatch):
    ped, view, block, refalt, batch = dataset(tmp_path_factory, "ext10", 3)
    planes = []
    for no_jit in (False, True):
        if no_jit:
            monkeypatch.setenv("PM_NO_JIT", "1")
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_joint(True)
        planes.append(run_batches(eng, block, refalt, batch)[2])
        eng.close()
    assert plane_bytes(planes[0]) == plane_bytes(planes[1]) and (planes[0][0] != NONE).any()


@pytest.mark.parametrize("shape,nfam", [("ext10", 3), ("extmix", 5)])
def test_peel_workspace_in_lds_and_in_hbm(built, tmp_path_factory, monkeypatch, shape, nfam):
    """k_vcf_joint_es<true> and k_vcf_joint_es<false> (PM_ES_POST_HBM: the pass's own workspace buffer, which an engine
    allocates only then) write the same plane."""
    ped, view, block, refalt, batch = dataset(tmp_path_factory, shape, nfam)
    planes = []
    for hbm in (False, True):
        if hbm:
            monkeypatch.setenv("PM_ES_POST_HBM", "1")   # (read when the engine is created)
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_joint(True)
        planes.append(run_batches(eng, block, refalt, batch)[2])
        eng.set_vcf_joint(False)
        eng.set_vcf_joint(True)   # freed and allocated again
        planes.append(run_batches(eng, block, refalt, batch)[2])
        eng.close()
    assert len({plane_bytes(p) for p in planes}) == 1 and (planes[0][0] != NONE).any()


def test_stuck_site_keeps_the_returned_rows(built, tmp_path_factory, monkeypatch):
    ped, view, block, refalt, batch = dataset(tmp_path_factory, "mixed", 31)
    par = pm.Params.defaults(vcf_mode=1)
    eng = pm.Engine(view, par, max_batch=batch)
    eng.set_vcf_joint(True)
    res, calls, (g, lp), _, _ = run_batches(eng, block, refalt, batch)
    eng.close()
    k, s = pick_itmax(res)
    assert first_stuck(res, k) == s
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))   # (read when the engine is created)
    eng = pm.Engine(view, par, max_batch=batch)
    eng.set_vcf_joint(True)
    zeros = np.zeros(block.shape[:2], np.uint32)
    b0 = s // batch * batch
    for t in range(0, b0, batch):   # the batches before the stuck site's run as usual
        eng.run(block[t:t + batch], zeros[t:t + batch], refalt[t:t + batch])
        assert plane_bytes(eng.vcf_joint()) == plane_bytes((g[t:t + batch], lp[t:t + batch]))
    with pytest.raises(pm.engine.BrentStuck) as ei:
        eng.run(block[b0:b0 + batch], zeros[b0:b0 + batch], refalt[b0:b0 + batch])
    assert ei.value.site == s - b0
    got = eng.vcf_joint()
    assert len(got[0]) == len(ei.value.calls) == s - b0   # the rows the batch returned: those before the stuck site
    assert plane_bytes(got) == plane_bytes((g[b0:s], lp[b0:s]))
    eng.close()


def _planted(trio):
    ped = trio_pedigree(8)
    block, refalt = trio_block(*trio, 8, 4)
    eng = pm.Engine(ped, pm.Params.defaults(vcf_mode=1), max_batch=4)
    eng.set_vcf_joint(True)
    res, calls = eng.run(block, np.zeros(block.shape[:2], np.uint32), refalt)
    g, lp = eng.vcf_joint()
    eng.close()
    assert (res["call_row"] >= 0).all() and len(g) == 4
    fams = JointFamilies(ped)
    return fams, fams.solve(block, refalt, res["af"], g), res, calls, g, lp


def test_planted_trio_gets_the_joint_optimum(built):
    """PLANTED_TRIO_OWN_AF in every family of an 8-trio pedigree.  At the engine's own af the table confirms the premise
    (marginal argmaxes with T = 0, a unique maximum with a runner-up of at most 0.8 of it), the genotype rows' marginal
    calls are those inconsistent ones, and g is the table's argmax exactly."""
    fams, sol, res, calls, g, lp = _planted(PLANTED_TRIO_OWN_AF)
    T = transmission()
    print(f"engine af {res['af'][0]:.6f}")
    for F, r in zip(fams.fams, sol):
        sl = slice(F["p0"], F["p0"] + 3)
        marginal = r["marg"].argmax(axis=2)
        assert (T[marginal[:, 0], marginal[:, 1], marginal[:, 2]] == 0).all(), marginal
        assert (r["n_best"] == 1).all() and (r["second"] <= 0.8 * r["max"]).all()
        best = calls["best"][:, sl].astype(np.int64)
        assert (calls["gq"][:, sl] > 0).all() and (best == marginal).all(), best   # what GT prints
        assert (T[best[:, 0], best[:, 1], best[:, 2]] == 0).all()
        assert (g[:, sl] == r["argmax"]).all(), (g[:, sl], r["argmax"])
        assert (r["J_at"] == r["max"]).all()
    assert fams.mendel_consistent(g).all()


def test_planted_trio_of_the_first_example(built):
    """PLANTED_TRIO the same way.  With it in every family the engine's own af is 0.54, not the 0.95 at which its marginal
    calls are inconsistent: there they are the consistent (1/1, 0/0, 0/1), so that premise is not asserted here (it is,
    at 0.95, in tests/test_cpu_vcf_joint.py).  The optimum is unique, and g is the table's argmax exactly."""
    fams, sol, res, calls, g, lp = _planted(PLANTED_TRIO)
    print(f"engine af {res['af'][0]:.6f}")
    for F, r in zip(fams.fams, sol):
        assert (r["n_best"] == 1).all() and (r["second"] <= 0.8 * r["max"]).all()
        assert (g[:, F["p0"]:F["p0"] + 3] == r["argmax"]).all()
    assert fams.mendel_consistent(g).all()


# ---------------------------------------------------------------------------------------------------------------- CLI

JG_HEADER = ('##FORMAT=<ID=JG,Number=1,Type=String,Description="Genotype in the Family\'s Most Probable Joint Configuration">')
JL_HEADER = '##FORMAT=<ID=JL,Number=1,Type=Float,Description="Log10 Posterior Probability of That Configuration">'
SRC, _cli, _same = common.SRC, common.cli, common.same


def _strip(lines):
    """The output without the JG and JL header lines and sub-fields."""
    return common.strip_fields(lines, ("JG", "JL"), lambda fmt, k: fmt[k + 2] in ("PL", "GL") and k == len(fmt) - 3)


def _example_plane():
    """The example's records through the Python engine: {(chrom, pos): (g, lp) per VCF sample column} for the records the
    --in_vcf path computes (one-base REF and ALT, some sample with data), PL bytes placed as the host driver places them."""
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    person = {pid: p for p, pid in enumerate(ped.pids())}   # (later families win, as in the driver)
    base = {"A": 1, "C": 2, "G": 3, "T": 4}
    from vcf_posterior_reference import three
    keys, rows, refalt, cols = [], [], [], None
    for l in gzip.open(SRC, "rt"):
        if l.startswith("##"):
            continue
        c = l.rstrip("\n").split("\t")
        if l.startswith("#"):
            cols = [person[s] for s in c[9:]]
            continue
        if c[3] not in base or c[4] not in base:
            continue
        k = c[8].split(":").index("PL")
        pls = [[int(x) for x in v.split(":")[k].split(",")] for v in c[9:]]
        if not any(any(t) for t in pls):
            continue
        ra = base[c[3]] | base[c[4]] << 4
        row = np.zeros((ped.n_person, 10), np.uint8)
        for p, t in zip(cols, pls):
            row[p, three(ra)] = np.minimum(t, 255)
        keys.append((c[0], c[1]))
        rows.append(row)
        refalt.append(ra)
    block, refalt = np.stack(rows), np.array(refalt, np.uint8)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=len(refalt))
    eng.set_vcf_joint(True)
    res, calls = eng.run_vcf(block, refalt)
    g, lp = eng.vcf_joint()
    eng.close()
    assert (res["call_row"] >= 0).all()
    return {key: (g[i][cols], lp[i][cols]) for i, key in enumerate(keys)}, ped, cols


def test_cli_prints_jg_and_jl(built, tmp_path):
    plain = _cli(tmp_path, "plain.vcf", [])
    exp = gzip.open(os.path.join(EXAMPLE, "testvcf.out.vcf.body.gz"), "rt").read().splitlines()
    assert [l for l in plain if not l.startswith("##")] == exp   # without the flag: the committed output of before
    got = _cli(tmp_path, "joint.vcf", ["--vcf_joint"])
    hdr = [l for l in got if l.startswith("##FORMAT")]
    k = next(i for i, l in enumerate(hdr) if l.startswith("##FORMAT=<ID=DP,"))
    assert hdr[k + 1] == JG_HEADER and hdr[k + 2] == JL_HEADER and hdr[k + 3].startswith("##FORMAT=<ID=PL,")
    assert all(l.split("\t")[8] in ("GT:GQ:DP:JG:JL:PL", "GT:GQ:DP:JG:JL:GL") for l in got if not l.startswith("#"))
    assert _same(_strip(got), plain)
    # the text against the plane of the same records through the Python engine
    plane, ped, cols = _example_plane()
    fam_of = np.searchsorted(ped.fam_start(), np.array(cols), side="right")
    names = {0: "0/0", 1: "0/1", 2: "1/1"}
    compared = differ = 0
    for l in got:
        if l.startswith("#"):
            continue
        c = l.split("\t")
        key = (c[0], c[1])
        if key not in plane:
            continue
        g, lp = plane[key]
        jl = {}
        for i, v in enumerate(c[9:]):
            f = v.split(":")
            want = (names[int(g[i])], "%.2f" % float(lp[i])) if g[i] != NONE else (".", ".")
            assert (f[3], f[4]) == want, (key, i, v, want)
            jl.setdefault(fam_of[i], set()).add(f[4])
            compared += 1
            differ += f[0] not in ("./.", f[3])
        assert all(len(s) == 1 for s in jl.values()), (key, jl)   # one JL per family
    assert compared > 1000 and differ > 0, (compared, differ)   # (somewhere JG differs from the marginal GT)
    assert _same(_cli(tmp_path, "b7.vcf", ["--vcf_joint", "--batch", "7"]), got)
    assert _same(_cli(tmp_path, "e3.vcf", ["--vcf_joint", "--engines", "3", "--batch", "1000"]), got)


def test_cli_combines_with_posteriors_phase_and_denovo(built, tmp_path):
    other = ["--vcf_posteriors", "--vcf_phase", "--vcf_denovo", "--vcf_denovo_families", "2", "--vcf_denovo_carriers", "2"]
    a, b = _cli(tmp_path, "other.vcf", other), _cli(tmp_path, "other_joint.vcf", other + ["--vcf_joint"])
    hdr = [l for l in b if l.startswith("##FORMAT")]
    k = next(i for i, l in enumerate(hdr) if l.startswith("##FORMAT=<ID=PQ,"))
    assert hdr[k + 1] == JG_HEADER and hdr[k + 2] == JL_HEADER and hdr[k + 3].startswith("##FORMAT=<ID=PL,")
    assert all(l.split("\t")[8] in ("GT:GQ:DP:DS:GP:PQ:JG:JL:PL", "GT:GQ:DP:DS:GP:PQ:JG:JL:GL") for l in b if not l.startswith("#"))
    info = lambda ls: [l.split("\t")[7] for l in ls if not l.startswith("#")]
    assert info(a) == info(b) and any("DQ=" in x for x in info(a))
    assert _same(_strip(b), a)
    # with --vcf_posteriors alone the two header lines follow GP's
    c = _cli(tmp_path, "post_joint.vcf", ["--vcf_posteriors", "--vcf_joint"])
    hdr = [l for l in c if l.startswith("##FORMAT")]
    k = next(i for i, l in enumerate(hdr) if l.startswith("##FORMAT=<ID=GP,"))
    assert hdr[k + 1] == JG_HEADER and hdr[k + 2] == JL_HEADER and hdr[k + 3].startswith("##FORMAT=<ID=PL,")
    # the joint call agrees with the printed posteriors: 10^JL is at most GP at JG, to the print rounding of both
    checked = 0
    for l in b:
        if l.startswith("#"):
            continue
        for v in l.split("\t")[9:]:
            f = v.split(":")
            if f[6] == "." or f[4] == ".":
                continue
            gp = [float(x) for x in f[4].split(",")]
            assert 10.0 ** (float(f[7]) - 0.005) <= gp[("0/0", "0/1", "1/1").index(f[6])] + 0.0005 + POST_ATOL, v
            checked += 1
    assert checked > 1000


def test_cli_records_without_data_and_shards(built, tmp_path):
    """Records without data print the previous computed record's JG and JL, like its GT and GQ -- also when that record was
    computed by the shard before (the carried state travels in the shards' exchange): two shards on the one GPU write the
    one-process output, and a blanked record's sample fields are those of the record before it."""
    from test_cpu_host import run_sharded, vcf_body
    from vcf_edits import write_nodata_vcf
    src = str(tmp_path / "in.vcf")
    blanked = sorted(write_nodata_vcf(src, worlds=(2,)))
    args = ["-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--vcf_joint"]
    one = str(tmp_path / "one.vcf")
    r1 = subprocess.run([pm.BIN_PATH] + args + ["--out_vcf", one], cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    recs = {tuple(l.split("\t")[:2]): l.split("\t") for l in vcf_body(one)[1:]}   # (chromosome, position) -> record
    inp = [tuple(l.split("\t")[:2]) for l in open(src).read().splitlines() if not l.startswith("#")]
    fields = lambda c: [":".join(v.split(":")[:2] + v.split(":")[3:5]) for v in c[9:]]   # GT, GQ, JG, JL
    carried = carried_joint = 0
    for i in blanked:   # (records the path does not write, multi-allelic ones, are in neither)
        if i > 0 and inp[i] in recs and inp[i - 1] in recs:
            assert fields(recs[inp[i]]) == fields(recs[inp[i - 1]]), inp[i]
            carried += 1
            carried_joint += any(v.split(":")[2] != "." for v in fields(recs[inp[i]]))
    assert carried > 0 and carried_joint > 0
    sh = str(tmp_path / "sharded.vcf")
    r2 = run_sharded(EXAMPLE, args + ["--out_vcf", sh], 2)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert vcf_body(sh) == vcf_body(one)
    assert not [f for f in os.listdir(str(tmp_path)) if ".part" in f]
