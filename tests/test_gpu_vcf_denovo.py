"""De novo calling from VCF input (pm_engine_set_vcf_denovo, --vcf_denovo): the three-genotype mutation model against the
unchanged CPU oracle.

A vcf_mode block carries data in the three genotypes of (ref, alt) only.  The oracle's 10-state de novo objective
(pmo_poly_loglik(..., denovo = 1)) on a block whose seven other genotype columns are 255 (likelihood 10^-25.5) is the
three-state model to ~1e-13 relative in log10 likelihood, so it pins N = varllk[2] and DQ = denovo_lr at the usual
LLK_RTOL.  A pedigree of one nuclear family is peeled by the vcf_mode engine: the oracle then gets a copy of the pedigree
with fam_kind = PM_FAM_EXTENDED (its peeling steps kept), so it peels with Hardy-Weinberg priors too.
"""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
import oracle_binding
from conftest import EXAMPLE
from fixtures import read_dataset
from oracle_binding import Oracle
from parity import FLAT_RTOL, FREQ_ATOL, LLK_RTOL
from polymutt_amd.engine import PedigreeStruct, SITE_DTYPE
from test_gpu_vcf import _vcf_block

pytestmark = pytest.mark.gpu

PM_FAM_EXTENDED = 2
MASKED = ("denovo_lr",)          # plus slot 2 of varllk / varfreq / evals
PARENT_PL, CHILD_PL = (0, 150, 255), (120, 0, 150)

CASES = [("trio", 3), ("quad", 70), ("mixed", 31), ("single", 12), ("ext10", 3), ("roof", 3), ("roof2", 2), ("extmix", 5),
         ("quad", 1), ("ext10", 1)]
NUMERICS_CASES = [CASES[0], CASES[2], CASES[4]]


def _gi(b1, b2):
    b1, b2 = min(b1, b2), max(b1, b2)
    return (b1 - 1) * (10 - b1) // 2 + (b2 - b1)


def _three(refalt):
    a1, a2 = int(refalt) & 15, int(refalt) >> 4
    return a1, a2, [_gi(a1, a1), _gi(a1, a2), _gi(a2, a2)]


def _arrays(ped):
    v = ped.view
    fs = np.ctypeslib.as_array(v.fam_start, shape=(v.n_fam + 1,)).copy()
    fo = np.ctypeslib.as_array(v.is_founder, shape=(v.n_person,)).copy()
    return fs, fo


def make_block(ped, pl, refalt, fill=255):
    """The VCF-like block: per person the three (ref, alt) PLs with their minimum subtracted, a de novo event planted on
    every 8th site in the first family with a non-founder (the planted child rotates over its non-founders), the seven
    other columns `fill`.  Returns (block, planted site indices)."""
    fs, fo = _arrays(ped)
    n, npers = pl.shape[0], pl.shape[1]
    fam = next((f for f in range(len(fs) - 1) if not fo[fs[f]:fs[f + 1]].all()), None)
    kids = [] if fam is None else [p for p in range(fs[fam], fs[fam + 1]) if not fo[p]]
    block = np.full((n, npers, 10), fill, np.uint8)
    planted = []
    for i in range(n):
        _, _, g = _three(refalt[i])
        tri = pl[i][:, g].astype(np.int32)
        tri -= tri.min(axis=1, keepdims=True)
        if kids and i % 8 == 0:
            tri[fs[fam]:fs[fam + 1]] = PARENT_PL
            tri[kids[(i // 8) % len(kids)]] = CHILD_PL
            planted.append(i)
        block[i][:, g] = tri.astype(np.uint8)
    return block, planted


def oracle_view(ped):
    """The pedigree the oracle gets: for exactly one nuclear family a copy with fam_kind = EXTENDED (see the module text)."""
    v = ped.view
    if not (v.n_fam == 1 and v.fam_kind[0] == 0):
        return v, None
    v2 = PedigreeStruct()
    C.memmove(C.byref(v2), C.byref(v), C.sizeof(v))
    kinds = (C.c_int32 * 1)(PM_FAM_EXTENDED)
    v2.fam_kind = C.cast(kinds, C.POINTER(C.c_int32))
    return v2, kinds


def oracle_values(ped, par, block, refalt):
    """Per site (N, maximiser, evaluations, D, maximiser, evaluations) from pmo_poly_loglik with denovo = 1 and 0."""
    view, keep = oracle_view(ped)
    ora = Oracle(view, par)
    L = oracle_binding.lib()
    out = np.zeros((len(refalt), 6))
    for i in range(len(refalt)):
        a1, a2, _ = _three(refalt[i])
        site = np.ascontiguousarray(block[i])
        for k, dn in ((0, 1), (3, 0)):
            mn, ev = C.c_double(0), C.c_int32(0)
            out[i, k] = L.pmo_poly_loglik(ora.h, site.ctypes.data, a1, a2, dn, C.byref(mn), C.byref(ev))
            out[i, k + 1], out[i, k + 2] = mn.value, ev.value
    del ora, keep
    return out


_DATA = {}


def dataset(tmp_path_factory, shape, nfam, nsites=96):
    """(ped, block, refalt, planted, oracle values), generated and evaluated by the oracle once per case."""
    key = (shape, nfam, nsites)
    if key not in _DATA:
        d = str(tmp_path_factory.mktemp(f"vdn_{shape}_{nfam}"))
        pm.synth_write_dataset(d, shape, nfam, nsites, 53)
        ped, secs, _ = read_dataset(d)
        (label, pos, ref, pl, dm), = secs
        refalt = _vcf_block(pl, ref, 5)
        block, planted = make_block(ped, pl.reshape(len(ref), ped.n_person, 10), refalt)
        par = pm.Params.defaults(vcf_mode=1)
        ov = oracle_values(ped, par, block, refalt)
        ov.setflags(write=False)
        block.setflags(write=False)
        _DATA[key] = (ped, block, refalt, planted, ov)
    return _DATA[key]


def run_batches(eng, block, refalt, batch=64):
    res, calls = [], []
    zeros = np.zeros(block.shape[:2], np.uint32)
    for s in range(0, len(refalt), batch):
        r, c = eng.run(block[s:s + batch], zeros[s:s + batch], refalt[s:s + batch])
        res.append(r)
        calls.append(c)
    return np.concatenate(res), np.concatenate(calls)


def check_against_oracle(res, ov, planted, has_kid, founders_only, label):
    assert len(res) == len(ov)
    called = res["status"] == 0
    assert called.all(), f"{label}: every site of these blocks is called; none may drop out of the comparison"
    Ne, No, Do = res["varllk"][:, 2], ov[:, 0], ov[:, 3]
    DQe, DQo = res["denovo_lr"], ov[:, 0] - ov[:, 3]
    errN, errQ = np.abs(Ne - No), np.abs(DQe - DQo)
    print(f"{label}: max |N_e - N_o| / |N_o| = {(errN / np.abs(No)).max():.3g}, max |DQ_e - DQ_o| = {errQ.max():.3g}, "
          f"max planted oracle DQ = {DQo[planted].max() if len(planted) else float('nan'):.3f}")
    bad = np.nonzero(errN > LLK_RTOL * np.abs(No))[0]
    assert not len(bad), (label, "N", int(bad[0]), Ne[bad[0]], No[bad[0]])
    bad = np.nonzero(errQ > LLK_RTOL * (np.abs(No) + np.abs(Do)))[0]
    assert not len(bad), (label, "DQ", int(bad[0]), DQe[bad[0]], DQo[bad[0]])
    flat = errN / np.maximum(np.abs(No), 1e-300) <= FLAT_RTOL   # parity.py's rule for a flat objective
    div = np.abs(res["varfreq"][:, 2] - ov[:, 1]) > FREQ_ATOL
    assert not (div & ~flat).any(), (label, "varfreq[2]", int(np.nonzero(div & ~flat)[0][0]))
    assert (res["evals"][:, 2] > 0).all(), label
    if founders_only:   # no transmission, no mutation term
        assert (np.abs(DQe) <= LLK_RTOL * 2 * np.abs(Do)).all(), label
    if has_kid:
        assert len(planted) and DQo[planted].max() > 3, (label, DQo[planted])
        assert DQe[planted].max() > 3, label


@pytest.mark.parametrize("shape,nfam", CASES)
def test_vcf_denovo_matches_oracle(built, tmp_path_factory, shape, nfam):
    """N and DQ of every site against the oracle; the figures are printed before the assertions."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=64)
    eng.set_vcf_denovo(True)
    res, _ = run_batches(eng, block, refalt)
    eng.close()
    check_against_oracle(res, ov, planted, shape != "single", shape == "single", f"{shape}/{nfam}")


@pytest.mark.parametrize("numerics", [pm.NUM_POLY, pm.NUM_EXACT])
@pytest.mark.parametrize("shape,nfam", NUMERICS_CASES)
def test_vcf_denovo_numerics(built, tmp_path_factory, shape, nfam, numerics):
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1, numerics=numerics), max_batch=64)
    eng.set_vcf_denovo(True)
    res, _ = run_batches(eng, block, refalt)
    eng.close()
    check_against_oracle(res, ov, planted, True, False, f"{shape}/{nfam}/num{numerics}")


def test_vcf_denovo_config5_lean_plan(built, tmp_path_factory):
    """Config 5's geometry: 2000 mixed trio / quad families, 128 sites in two batches."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "mixed", 2000, 128)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=64)
    eng.set_vcf_denovo(True)
    res, _ = run_batches(eng, block, refalt)
    eng.close()
    check_against_oracle(res, ov, planted, True, False, "mixed/2000")


def _masked(res):
    r = res.copy()
    r["denovo_lr"] = 0
    for f in ("varllk", "varfreq", "evals"):
        r[f][:, 2] = 0
    return r.tobytes()


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("extmix", 5)])
def test_vcf_denovo_side_effects(built, tmp_path_factory, shape, nfam):
    """On: only the four result fields change.  Off: the bytes of an engine that never heard of the feature."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    par = pm.Params.defaults(vcf_mode=1)
    fresh = pm.Engine(ped.view, par, max_batch=64)
    r0, c0 = run_batches(fresh, block, refalt)
    fresh.close()
    eng = pm.Engine(ped.view, par, max_batch=64)
    r_off, c_off = run_batches(eng, block, refalt)
    assert r_off.tobytes() == r0.tobytes() and c_off.tobytes() == c0.tobytes()
    eng.set_vcf_denovo(True)
    r_on, c_on = run_batches(eng, block, refalt)
    assert r_on.tobytes() != r0.tobytes()
    assert _masked(r_on) == _masked(r0) and c_on.tobytes() == c0.tobytes()
    eng.set_vcf_denovo(False)
    r_back, c_back = run_batches(eng, block, refalt)
    assert r_back.tobytes() == r0.tobytes() and c_back.tobytes() == c0.tobytes()
    eng.close()


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("roof", 3)])
def test_vcf_denovo_reads_three_planes_only(built, tmp_path_factory, shape, nfam):
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    noisy = np.random.default_rng(11).integers(0, 256, block.shape, dtype=np.uint8)
    for i in range(len(refalt)):   # the same three planes
        _, _, g = _three(refalt[i])
        noisy[i][:, g] = block[i][:, g]
    assert (noisy != block).any()
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=64)
    eng.set_vcf_denovo(True)
    ra, ca = run_batches(eng, block, refalt)
    rb, cb = run_batches(eng, noisy, refalt)
    eng.close()
    assert ra.tobytes() == rb.tobytes() and ca.tobytes() == cb.tobytes()


def test_vcf_denovo_entry_points_agree(built, tmp_path_factory):
    """run, run_vcf, submit / collect and run_device + sync give the same result bytes."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "mixed", 31)
    n, npers = 64, ped.n_person
    pl, ra = np.ascontiguousarray(block[:n]), np.ascontiguousarray(refalt[:n])
    zeros = np.zeros((n, npers), np.uint32)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=n)
    eng.set_vcf_denovo(True)
    r_run, _ = eng.run(pl, zeros, ra)
    assert (r_run["evals"][:, 2] > 0).all() and (r_run["varllk"][:, 2] != 0).all()
    r_vcf, _ = eng.run_vcf(pl, ra)
    eng.submit(pl, zeros, ra)
    r_sc, _ = eng.collect()
    d_src, d_pl = eng.alloc(n * npers * 10), eng.alloc(n * npers * 10)
    d_ref, d_res = eng.alloc(n), eng.alloc(n * SITE_DTYPE.itemsize)
    eng.to_device(d_src, pl, n * npers * 10)
    eng.to_device(d_ref, ra, n)
    eng.to_planar(n, d_src, d_pl)
    eng.run_device(n, d_pl, None, d_ref, d_res, None)
    eng.sync()
    r_dev = np.zeros(n, dtype=SITE_DTYPE)
    eng.to_host(r_dev, d_res, n * SITE_DTYPE.itemsize)
    for p in (d_src, d_pl, d_ref, d_res):
        eng.free(p)
    eng.close()
    assert r_vcf.tobytes() == r_run.tobytes()
    assert r_sc.tobytes() == r_run.tobytes()
    assert r_dev.tobytes() == r_run.tobytes()


def test_vcf_denovo_skips_non_autosomal_sections(built, tmp_path_factory):
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "mixed", 31)
    par = pm.Params.defaults(vcf_mode=1)
    off = pm.Engine(ped.view, par, max_batch=64)
    off.begin_section(pm.PM_CHR_X)
    r0, c0 = run_batches(off, block, refalt)
    off.close()
    eng = pm.Engine(ped.view, par, max_batch=64)
    eng.set_vcf_denovo(True)
    eng.begin_section(pm.PM_CHR_X)
    r1, c1 = run_batches(eng, block, refalt)
    assert r1.tobytes() == r0.tobytes() and c1.tobytes() == c0.tobytes()
    eng.begin_section(pm.PM_CHR_AUTO)   # and on again on the next autosome
    r2, _ = run_batches(eng, block, refalt)
    assert (r2["evals"][:, 2] > 0).all()
    eng.close()


def test_vcf_denovo_stuck_site(built, tmp_path_factory, monkeypatch):
    """PM_TEST_ITMAX (tests/test_brent_stuck.py): PM_EBRENT and pm_engine_stuck_site = the first site at which the
    oracle's standard or de novo Brent needs ITMAX loop evaluations (evals - 3, from its normal run)."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "quad", 70)
    loops = np.stack([ov[:, 2], ov[:, 5]], axis=1).astype(int) - 3   # de novo, standard
    best = None
    for k in sorted(set(int(x) for x in loops.ravel() if x > 0)):
        idx = np.nonzero((loops >= k).any(axis=1))[0]
        # an ITMAX at which the de novo Brent is the one that stops first, nearest the middle of the first batch
        if len(idx) and 0 < idx[0] < 64 and loops[idx[0], 0] >= k > loops[idx[0], 1]:
            if best is None or abs(idx[0] - 32) < abs(best[1] - 32):
                best = (k, int(idx[0]))
    if best is None:   # (no site where only the de novo Brent stops: take any)
        for k in sorted(set(int(x) for x in loops.ravel() if x > 0)):
            idx = np.nonzero((loops >= k).any(axis=1))[0]
            if len(idx) and 0 < idx[0] < 64:
                best = (k, int(idx[0]))
    assert best is not None
    k, s = best
    par = pm.Params.defaults(vcf_mode=1)
    eng = pm.Engine(ped.view, par, max_batch=64)
    eng.set_vcf_denovo(True)
    zeros = np.zeros((64, ped.n_person), np.uint32)
    res, calls = eng.run(block[:64], zeros, refalt[:64])
    assert eng.stuck_site() == -1
    eng.close()
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))
    eng = pm.Engine(ped.view, par, max_batch=64)
    eng.set_vcf_denovo(True)
    with pytest.raises(pm.engine.BrentStuck) as ei:
        eng.run(block[:64], zeros, refalt[:64])
    e = ei.value
    assert e.site == s == eng.stuck_site(), (e.site, s, k)
    for f in ("status", "emit", "maxidx", "n_cfg", "call_row", "evals", "varllk", "denovo_lr"):
        assert (e.results[f][:s] == res[f][:s]).all(), f
    nrows = int((res["call_row"][:s] >= 0).sum())
    assert len(e.calls) == nrows and (e.calls == calls[:nrows]).all()
    eng.close()


def test_vcf_denovo_api_errors(built, tmp_path_factory):
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "trio", 3)
    lib = pm.load_library()
    glf = pm.Engine(ped.view, pm.Params.defaults(denovo=1), max_batch=8)
    assert lib.pm_engine_set_vcf_denovo(glf.h, 1) == -1   # PM_EINVAL
    assert b"vcf_mode" in lib.pm_last_error()
    glf.close()
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=8)
    zeros = np.zeros((8, ped.n_person), np.uint32)
    eng.submit(block[:8], zeros, refalt[:8])
    assert lib.pm_engine_set_vcf_denovo(eng.h, 1) == -1
    assert b"not been collected" in lib.pm_last_error()
    r_off, _ = eng.collect()
    assert (r_off["evals"][:, 2] == 0).all()
    # the per-family and per-person features keep refusing vcf_mode engines
    assert lib.pm_engine_set_denovo_families(eng.h, 1, 0) == -1
    assert lib.pm_engine_set_denovo_carriers(eng.h, 1, 0) == -1
    eng.set_vcf_denovo(True)
    r_on, _ = eng.run(block[:8], zeros, refalt[:8])
    assert (r_on["evals"][:, 2] > 0).all()
    eng.close()


# ------------------------------------------------------------------------------------------------
# CLI: --vcf_denovo on the example input

PLANT_RECORD, PLANT_FAMILY = 100, ("5", "6", "7", "8")   # fam2 of example/test.ped: parents 5, 6, children 7, 8


def _write_planted_vcf(path):
    """tests/vcf_edits.py's edited input (indels, dropped records) with the planted pattern in fam2 at one SNV record."""
    from vcf_edits import EDITS, write_edited_vcf
    assert PLANT_RECORD not in EDITS
    write_edited_vcf(path)
    lines = open(path).read().splitlines()
    head = next(l for l in lines if l.startswith("#CHROM")).split("\t")
    k = -1
    for j, l in enumerate(lines):
        if l.startswith("#"):
            continue
        k += 1
        if k != PLANT_RECORD:
            continue
        c = l.split("\t")
        assert len(c[3]) == 1 and len(c[4]) == 1 and c[8].split(":")[-1] == "PL"
        for col in range(9, len(c)):
            if head[col] in PLANT_FAMILY:
                f = c[col].split(":")
                f[-1] = ",".join(str(x) for x in (CHILD_PL if head[col] == "7" else PARENT_PL))
                c[col] = ":".join(f)
        lines[j] = "\t".join(c)
        planted = c
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return head, planted


def _run_cli(src, out, *extra):
    r = subprocess.run([pm.BIN_PATH, "-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--out_vcf", out] + list(extra),
                       cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return open(out).read().splitlines()


def test_cli_vcf_denovo(built, tmp_path):
    import re
    src = str(tmp_path / "in.vcf")
    head, planted = _write_planted_vcf(src)
    plain = _run_cli(src, str(tmp_path / "plain.vcf"))
    also_denovo = _run_cli(src, str(tmp_path / "dn.vcf"), "--denovo")   # --denovo alone stays the silent no-op
    tagged = _run_cli(src, str(tmp_path / "tagged.vcf"), "--vcf_denovo")
    strip_cmd = [l for l in plain if not l.startswith("##Polymutt=")]
    assert [l for l in also_denovo if not l.startswith("##Polymutt=")] == strip_cmd
    dq_head = [l for l in tagged if l.startswith("##INFO=<ID=DQ,")]
    assert len(dq_head) == 1
    stripped = [re.sub(r";DQ=[-0-9.einf]+", "", l) for l in tagged if not l.startswith("##INFO=<ID=DQ,")]
    assert [l for l in stripped if not l.startswith("##Polymutt=")] == strip_cmd
    recs = [l.split("\t") for l in tagged if not l.startswith("#")]
    with_dq = [c for c in recs if ";DQ=" in c[7]]
    assert with_dq
    for c in with_dq:
        assert len(c[3]) == 1 and len(c[4]) == 1, "no indel record carries the tag"
        assert re.search(r";DP=\d+;DQ=-?\d+\.\d{3}$", c[7]), c[7]
    # the planted record against the oracle's value for its PLs
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    person = {pid: i for i, pid in enumerate(ped.pids())}
    a1, a2 = "ACGT".index(planted[3]) + 1, "ACGT".index(planted[4]) + 1
    g = [_gi(a1, a1), _gi(a1, a2), _gi(a2, a2)]
    block = np.full((1, ped.n_person, 10), 255, np.uint8)
    for col in range(9, len(planted)):
        pls = [min(255, int(x)) for x in planted[col].split(":")[-1].split(",")]
        block[0, person[head[col]], g] = pls
    ov = oracle_values(ped, pm.Params.defaults(vcf_mode=1), block, np.array([a1 | (a2 << 4)], np.uint8))
    dq = ov[0, 0] - ov[0, 3]
    assert dq > 3, dq
    got = [c for c in recs if c[1] == planted[1] and c[0] == planted[0]]
    assert len(got) == 1
    assert got[0][7].endswith(";DQ=%.3f" % dq), (got[0][7], dq)
