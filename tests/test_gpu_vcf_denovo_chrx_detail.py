"""GPU tests of the families and children behind each DQ of a chrX section (pm_engine_set_vcf_denovo_chrx_detail, the
k_vdn_who_x kernels, and the CLI's --vcf_denovo_chrX_detail).

A row is a called site of a PM_CHR_X section whose DQ is at or above denovo_min_llr (1e-300 here).  Per row and family,
D_f = log10 L_f^dn(varfreq[2]) - log10 L_f^std(varfreq[1]); per row and non-founder c,
pp_c = Sum_{a in {0,2}, b} J_c(a, b, NonMendX(a, b, sex_c)) / L_f^dn, in the sex-aware three-state model.  The judge is
tests/chrx_detail_reference.py (joint-state einsum contractions, no peeling), which
tests/test_cpu_vcf_denovo_chrx_detail.py pins against the CPU oracle first.

Cases: the shapes of tests/test_gpu_vcf_denovo_chrx.py with its sex-aware plants, 96 sites in 64-site batches (the second
batch is partial), and 16-site cases on each side of the 128-term boundary between k_vdn_who_x<64> and <256>, with and
without a child.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import polymutt_amd as pm
from chrx_detail_reference import SiteDetail, chrx_tables
from chrx_reference import Pedigree as RefPedigree, three
from conftest import EXAMPLE
from parity import LLK_RTOL
from test_gpu_denovo_carriers import expected_top as expected_carriers, non_founders
from test_gpu_denovo_families import expected_top as expected_families
from test_gpu_vcf_denovo import _arrays, run_batches
from test_gpu_vcf_denovo_chrx import (FAM1, MALE, PLANT_DAUGHTER, PLANT_SON, _one_family_block, _run_cli, _write_planted_vcf,
                                      dataset, mutation_matrices, x_engine)
from test_gpu_vcf_denovo_detail import TAGS, _read, _strip, _tops, detail_batches, expected_rows

pytestmark = pytest.mark.gpu

CASES = [("trio", 3, 96), ("quad", 5, 96), ("mixed", 31, 96), ("ext10", 1, 96), ("roof", 3, 96), ("extmix", 5, 96),
         ("roof2", 1, 96), ("trio", 129, 16),   # the eight of the reference's own check (test_cpu_vcf_denovo_chrx_detail.py)
         ("trio", 128, 16), ("single", 12, 96), ("single", 129, 16)]
MIN_LLR = 1e-300

_runs, _ctx = {}, {}


def detail_engine(ped, fam_k=8, car_k=8, want_all=True, switch=True, **kw):
    eng = x_engine(ped, denovo_min_llr=kw.pop("denovo_min_llr", MIN_LLR), **kw)
    if fam_k or car_k:
        eng.set_vcf_denovo_detail(fam_k, car_k, want_all)
    if switch:
        eng.set_vcf_denovo_chrx_detail(True)
    return eng


def shared_run(tmp_path_factory, shape, nfam, nsites):
    """One engine pass per case (fam_k = car_k = 8, the full matrices), shared by the tests that read it."""
    key = (shape, nfam, nsites)
    if key not in _runs:
        ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
        eng = detail_engine(ped)
        _runs[key] = detail_batches(eng, block, refalt)
        eng.close()
    return _runs[key]


def context(ped):
    """(reference pedigree, M, A4) per pedigree."""
    if id(ped) not in _ctx:
        M, A4 = mutation_matrices(ped, pm.Params.defaults(vcf_mode=1))
        _ctx[id(ped)] = (RefPedigree(ped.view), M, A4)
    return _ctx[id(ped)]


def site_detail(ped, block, refalt, i):
    rp, M, A4 = context(ped)
    return SiteDetail(rp, block[i], refalt[i], chrx_tables(M, A4, refalt[i]))


def plant_kids(ped):
    fs, fo = _arrays(ped)
    fam = next((f for f in range(len(fs) - 1) if not fo[fs[f]:fs[f + 1]].all()), None)
    return fam, ([] if fam is None else [p for p in range(fs[fam], fs[fam + 1]) if not fo[p]])


@pytest.mark.parametrize("shape,nfam,nsites", CASES)
def test_rows(built, tmp_path_factory, shape, nfam, nsites):
    """1. the rows are {status == 0, evals[2] > 0, denovo_lr >= threshold} of the engine's own results, per batch; the
    readers' lengths and shapes agree; a case with a child has rows, some of them with reference DQ > 3."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    dqr = rv[:, 0] - rv[:, 2]
    total = strong = 0
    for s, res, calls, rows, fam, car in shared_run(tmp_path_factory, shape, nfam, nsites):
        assert rows.dtype == np.int32 and rows.tolist() == expected_rows(res).tolist(), (shape, nfam, s)
        assert len(fam[0]) == len(fam[1]) == len(fam[2]) == len(car[0]) == len(car[1]) == len(rows)
        assert fam[0].shape[1:] == (8,) and fam[2].shape[1:] == (ped.n_fam,) and car[1].shape[1:] == (ped.n_person,)
        total += len(rows)
        strong += int((dqr[s + rows] > 3).sum())
    print(f"{shape}/{nfam}: {total} rows, {strong} with reference DQ > 3")
    if shape == "single":
        # no transmission, no mutation term: the engine's own denovo_lr is rounding noise of either sign, and at 1e-300 a
        # positive one is a row (tests/test_gpu_vcf_denovo_detail.py::test_rows); at the default threshold there is none
        assert (dqr <= LLK_RTOL * 2 * np.abs(rv[:, 2])).all()
        for s, res, calls, rows, fam, car in shared_run(tmp_path_factory, shape, nfam, nsites):
            r = res[rows]
            assert (np.abs(r["denovo_lr"]) <= LLK_RTOL * 2 * np.abs(r["varllk"][:, 1])).all()
            assert (car[0]["person"] == -1).all() and (car[1]["pp"] == 0).all()
        eng = detail_engine(ped, denovo_min_llr=pm.Params.defaults(vcf_mode=1).denovo_min_llr)
        for s, res, calls, rows, fam, car in detail_batches(eng, block, refalt):
            assert len(rows) == 0 and len(fam[0]) == len(fam[1]) == len(fam[2]) == len(car[0]) == len(car[1]) == 0
            assert (res["evals"][:, 2] > 0).all()
        eng.close()
    elif nsites == 16:
        assert total >= 2 and strong >= 1, (shape, nfam, total, strong)
    else:
        assert total >= 8 and strong >= 4, (shape, nfam, total, strong)


@pytest.mark.parametrize("shape,nfam,nsites", CASES)
def test_family_terms_match_reference(built, tmp_path_factory, shape, nfam, nsites):
    """2. all[row][f] against the reference at the engine's varfreq[2] / varfreq[1], within
    LLK_RTOL (|l_dn| + |l_std|) + 1e-10; sum against denovo_lr and all.sum(1) within LLK_RTOL (|varllk[2]| + |varllk[1]|);
    top = the stable descending ranking of all, byte for byte."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    worst = worst_sum = 0.0
    for s, res, calls, rows, (top, tot, full), car in shared_run(tmp_path_factory, shape, nfam, nsites):
        r = res[rows]
        bound = LLK_RTOL * (np.abs(r["varllk"][:, 2]) + np.abs(r["varllk"][:, 1]))
        if len(rows):
            worst_sum = max(worst_sum, float((np.abs(tot - r["denovo_lr"]) / bound).max()))
        assert (np.abs(tot - r["denovo_lr"]) <= bound).all(), (shape, nfam, s)
        assert (np.abs(tot - full.sum(axis=1)) <= bound).all(), (shape, nfam, s)
        fam, lr = expected_families(full, 8)
        assert np.array_equal(top["fam"], fam), (shape, nfam, s)
        assert top["lr"].tobytes() == lr.tobytes() and not top["pad"].any()
        for k, i in enumerate(rows):
            exp, mag = site_detail(ped, block, refalt, s + i).family_terms(float(res["varfreq"][i, 2]), float(res["varfreq"][i, 1]))
            err, bnd = np.abs(full[k] - exp), LLK_RTOL * mag + 1e-10
            worst = max(worst, float((err / bnd).max()))
            assert (err <= bnd).all(), (shape, nfam, s + i, int(np.argmax(err / bnd)), float(err.max()))
    print(f"{shape}/{nfam}: worst family error / bound = {worst:.3g}, worst sum error / bound = {worst_sum:.3g}")


def check_child(sd, f, c_local, male, x, entry):
    """One child's entry against the reference; returns error / bound."""
    ref = sd.child(f, c_local, x)
    g = sd.g
    bound = np.log(10) * LLK_RTOL * ref["mag"] * ref["pp"] + 1e-12
    err = abs(float(entry["pp"]) - ref["pp"])
    assert err <= bound, (f, c_local, float(entry["pp"]), ref["pp"], bound)
    assert 0.0 <= entry["pp"] <= 1.0
    ev = (int(entry["fa_g"]), int(entry["mo_g"]), int(entry["kid_g"]))
    L = ref["L"]
    jmax = max(ref["terms"].values()) / L if ref["terms"] else 0.0
    if ev == (-1, -1, -1):
        assert jmax <= bound, (f, c_local, ev, jmax)
    else:
        assert ev[0] in (g[0], g[2]), (f, c_local, ev)   # a father is hemizygous
        assert ev[1] in g and ev[2] in g, (f, c_local, ev)
        if male:
            assert ev[2] in (g[0], g[2]), (f, c_local, ev)   # and so is a son
        a, b, st = g.index(ev[0]), g.index(ev[1]), g.index(ev[2])
        assert st in sd.t.nonmend(a, b, male), (f, c_local, ev)
        assert ref["terms"][(a, b)] / L >= jmax - bound, (f, c_local, ev, ref["terms"], L)
        K = ref["K"]
        singles = {t: float(K[a, b, t]) / L for t in sd.t.nonmend(a, b, male)}
        assert singles[st] >= max(singles.values()) - bound, (f, c_local, ev, singles)
    return err / bound


@pytest.mark.parametrize("shape,nfam,nsites", CASES)
def test_carriers_match_reference(built, tmp_path_factory, shape, nfam, nsites):
    """3. every non-founder of every row: pp within ln(10) LLK_RTOL (|log10 L_f| + max |log10 J|) pp + 1e-12 and in [0, 1];
    the event valid for the sexes and maximal within the bound; founders blank; top = the stable ranking of all; on
    planted rows with reference DQ > 3 the planted child is top[row][0] with pp > 0.99; roof2's plain-T children have
    pp == 0."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    rp, M, A4 = context(ped)
    kids = non_founders(ped.view)
    founder = np.ones(ped.n_person, bool)
    founder[kids] = False
    fam0, pk = plant_kids(ped)
    where = {}   # person -> (family, local index, male, mutates)
    for f, (p0, n, founders, fk) in enumerate(rp.fams):
        for i, fa, mo, male, mutates in fk:
            where[p0 + i] = (f, i, male, mutates)
    assert sorted(where) == kids.tolist()
    dqr = rv[:, 0] - rv[:, 2]
    worst, n_checked, n_planted, n_plain = 0.0, 0, 0, 0
    for s, res, calls, rows, fam, (top, full) in shared_run(tmp_path_factory, shape, nfam, nsites):
        if len(kids):
            assert top.tobytes() == expected_carriers(full, kids, 8).tobytes(), (shape, nfam, s)
        else:
            assert (top["person"] == -1).all() and (top["pp"] == 0).all()
        for k, i in enumerate(rows):
            ent = full[k]
            assert (ent["person"] == np.arange(ped.n_person)).all() and not ent["pad"].any()
            f_ = ent[founder]
            assert (f_["fa_g"] == -1).all() and (f_["mo_g"] == -1).all() and (f_["kid_g"] == -1).all() and (f_["pp"] == 0.0).all()
            assert ((ent["pp"] >= 0) & (ent["pp"] <= 1)).all()
            sd = site_detail(ped, block, refalt, s + i)
            x = float(res["varfreq"][i, 2])
            for c in kids:
                f, cl, male, mutates = where[int(c)]
                worst = max(worst, check_child(sd, f, cl, male, x, ent[c]))
                n_checked += 1
                if not mutates:   # reached only through a type-3 step with a marriage partial: plain T there
                    assert ent[c]["pp"] == 0.0 and int(ent[c]["kid_g"]) == -1, (shape, nfam, s + i, int(c), ent[c])
                    n_plain += 1
            if (s + i) in planted and dqr[s + i] > 3:
                child = pk[((s + i) // 8) % len(pk)]
                assert where[child][3], (shape, nfam, s + i, child)   # (a plain-T child cannot give DQ > 3)
                assert top[k, 0]["person"] == child and top[k, 0]["pp"] > 0.99, (shape, nfam, s + i, top[k, 0], child)
                n_planted += 1
    print(f"{shape}/{nfam}: worst carrier error / bound = {worst:.3g} over {n_checked} children, {n_planted} planted rows, "
          f"{n_plain} plain-T entries")
    if shape != "single":
        assert n_planted >= (1 if nsites == 16 else 4), (shape, nfam, n_planted)
    if shape == "roof2":
        assert n_plain > 0


def test_sex_awareness(built, tmp_path_factory):
    """4. a hemizygous-reference son of an alternate-allele father is Mendelian on X: no row at the default threshold, and
    at 1e-300 his pp stays below the reference's value plus the bound; a daughter of the same parents with the same data
    is top[0]."""
    refalts = np.array([1 | (3 << 4), 1 | (2 << 4)], np.uint8)
    ped = dataset(tmp_path_factory, "trio", 3, 96)[0]
    rp, M, A4 = context(ped)
    sex = np.ctypeslib.as_array(ped.view.sex, shape=(ped.n_person,))
    fs, _ = _arrays(ped)
    assert sex[fs[0] + 2] == MALE
    block = _one_family_block(ped, 0, 2, refalts)
    eng = detail_engine(ped, denovo_min_llr=pm.Params.defaults(vcf_mode=1).denovo_min_llr)
    (s, res, calls, rows, fam, car), = detail_batches(eng, block, refalts)
    eng.close()
    assert len(rows) == 0 and (res["evals"][:, 2] > 0).all()
    eng = detail_engine(ped)
    (s, res, calls, rows, fam, (top, full)), = detail_batches(eng, block, refalts)
    eng.close()
    for k, i in enumerate(rows):
        sd = site_detail(ped, block, refalts, i)
        ref = sd.child(0, 2, float(res["varfreq"][i, 2]))
        bound = np.log(10) * LLK_RTOL * ref["mag"] * ref["pp"] + 1e-12
        print(f"son on chrX, site {i}: engine pp {full[k][fs[0] + 2]['pp']:.3g}, reference {ref['pp']:.3g}")
        assert ref["pp"] < 0.01 and full[k][fs[0] + 2]["pp"] <= ref["pp"] + bound
    ped = dataset(tmp_path_factory, "mixed", 31, 96)[0]
    sex = np.ctypeslib.as_array(ped.view.sex, shape=(ped.n_person,))
    fs, _ = _arrays(ped)
    assert fs[2] - fs[1] == 4 and sex[fs[1] + 3] != MALE
    block = _one_family_block(ped, 1, 3, refalts)
    eng = detail_engine(ped, denovo_min_llr=pm.Params.defaults(vcf_mode=1).denovo_min_llr)
    (s, res, calls, rows, fam, (top, full)), = detail_batches(eng, block, refalts)
    eng.close()
    assert rows.tolist() == [0, 1]
    for k in range(2):
        g = three(refalts[k])[2]
        print(f"daughter on chrX, site {k}: top {top[k, 0]}")
        assert top[k, 0]["person"] == fs[1] + 3 and top[k, 0]["pp"] > 0.99
        assert (int(top[k, 0]["fa_g"]), int(top[k, 0]["mo_g"]), int(top[k, 0]["kid_g"])) == (g[2], g[0], g[0])
        assert fam[0][k, 0]["fam"] == 1


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("extmix", 5)])
def test_additivity(built, tmp_path_factory, shape, nfam):
    """5. switch on: the results and genotype rows of chrX batches are those of set_vcf_denovo_chrx alone; an autosomal
    section of the same engine gives the bytes of an engine without the switch; switch off, or any of the three other
    setters called again: 0 rows on X; chrY / MT: 0 rows."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, 96)
    plain = x_engine(ped, denovo_min_llr=MIN_LLR)
    r0, c0 = run_batches(plain, block, refalt)
    plain.close()
    base = detail_engine(ped, switch=False)
    x_off = detail_batches(base, block, refalt)
    base.begin_section(pm.PM_CHR_AUTO)
    a_off = detail_batches(base, block, refalt)
    base.close()
    assert all(len(b[3]) == 0 for b in x_off)
    eng = detail_engine(ped)
    x_on = detail_batches(eng, block, refalt)
    assert np.concatenate([b[1] for b in x_on]).tobytes() == r0.tobytes()
    assert np.concatenate([b[2] for b in x_on]).tobytes() == c0.tobytes()
    assert sum(len(b[3]) for b in x_on) >= 8
    assert _tops(x_on) == _tops(shared_run(tmp_path_factory, shape, nfam, 96))
    eng.begin_section(pm.PM_CHR_AUTO)
    a_on = detail_batches(eng, block, refalt)
    assert sum(len(b[3]) for b in a_on) >= 8
    for x, y in zip(a_off, a_on):
        assert x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes() and x[3].tobytes() == y[3].tobytes()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x[4] + x[5], y[4] + y[5]))
    for chrom in (pm.PM_CHR_Y, pm.PM_CHR_MT):
        eng.begin_section(chrom)
        assert all(len(b[3]) == 0 for b in detail_batches(eng, block, refalt))
    eng.begin_section(pm.PM_CHR_X)
    assert _tops(detail_batches(eng, block, refalt)) == _tops(x_on)
    eng.set_vcf_denovo_chrx_detail(False)
    off = detail_batches(eng, block, refalt)
    assert all(len(b[3]) == 0 for b in off)
    assert np.concatenate([b[1] for b in off]).tobytes() == r0.tobytes()
    for again in ("detail", "chrx", "vcf_denovo"):
        eng.set_vcf_denovo_chrx_detail(True)
        assert len(detail_batches(eng, block[:64], refalt[:64])[0][3]) > 0
        if again == "detail":
            eng.set_vcf_denovo_detail(8, 8, True)
        elif again == "chrx":
            eng.set_vcf_denovo_chrx(True)
        else:
            eng.set_vcf_denovo(True)
            eng.set_vcf_denovo_chrx(True)
            eng.set_vcf_denovo_detail(8, 8, True)
        got = detail_batches(eng, block[:64], refalt[:64])[0]
        assert len(got[3]) == 0 and (got[1]["evals"][:, 2] > 0).all(), again
    eng.close()


@pytest.mark.parametrize("shape,nfam,nsites", [("mixed", 31, 96), ("roof", 3, 96), ("trio", 129, 16)])
def test_top_only(built, tmp_path_factory, shape, nfam, nsites):
    """6. want_all = False and k < 8 (the per-block line buffers): top equals the matching columns of the full run."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    eng = detail_engine(ped, 2, 3, False)
    got = detail_batches(eng, block, refalt, 2, 3)
    eng.close()
    for x, y in zip(got, shared_run(tmp_path_factory, shape, nfam, nsites)):
        assert x[3].tobytes() == y[3].tobytes()
        assert x[4][2] is None and x[5][1] is None
        assert x[4][0].tobytes() == np.ascontiguousarray(y[4][0][:, :2]).tobytes() and x[4][1].tobytes() == y[4][1].tobytes()
        assert x[5][0].tobytes() == np.ascontiguousarray(y[5][0][:, :3]).tobytes()


@pytest.mark.parametrize("shape,nfam,nsites", [("extmix", 5, 96), ("trio", 129, 16)])
def test_determinism(built, tmp_path_factory, shape, nfam, nsites):
    """7. two runs of one case give identical bytes in every output."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    eng = detail_engine(ped)
    again = detail_batches(eng, block, refalt)
    eng.close()
    for x, y in zip(again, shared_run(tmp_path_factory, shape, nfam, nsites)):
        assert x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes() and x[3].tobytes() == y[3].tobytes()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x[4] + x[5], y[4] + y[5]))


def test_setter_errors(built, tmp_path_factory):
    """8. PM_EINVAL with its message for each precondition; afterwards the engine still runs."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "trio", 3, 96)
    lib = pm.load_library()
    err = lambda: lib.pm_last_error()
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(None, 1) == -1 and b"invalid arguments" in err()
    glf = pm.Engine(ped.view, pm.Params.defaults(denovo=1), max_batch=8)
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(glf.h, 1) == -1 and b"without vcf_mode" in err()
    glf.close()
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1, denovo_min_llr=MIN_LLR), max_batch=8)
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(eng.h, 1) == -1 and b"vcf_denovo_chrx is off" in err()
    eng.set_vcf_denovo(True)
    eng.set_vcf_denovo_detail(2, 2)
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(eng.h, 1) == -1 and b"vcf_denovo_chrx is off" in err()
    eng.set_vcf_denovo_detail(0, 0)
    eng.set_vcf_denovo_chrx(True)
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(eng.h, 1) == -1 and b"vcf_denovo_detail is off" in err()
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(eng.h, 0) == -1   # (the preconditions hold for off as well)
    eng.set_vcf_denovo_detail(2, 2)
    eng.begin_section(pm.PM_CHR_X)
    zeros = np.zeros((8, ped.n_person), np.uint32)
    eng.submit(block[:8], zeros, refalt[:8])
    assert lib.pm_engine_set_vcf_denovo_chrx_detail(eng.h, 1) == -1 and b"not been collected" in err()
    eng.collect()
    assert len(eng.vcf_denovo_rows()) == 0
    eng.set_vcf_denovo_chrx_detail(True)
    res, _ = eng.run(block[:8], zeros, refalt[:8])
    rows, fam, car = _read(eng, 2, 2)
    assert rows.tolist() == expected_rows(res).tolist() and len(rows) >= 1 and fam[0].shape == (len(rows), 2)
    eng.set_vcf_denovo_chrx_detail(False)
    eng.run(block[:8], zeros, refalt[:8])
    assert len(eng.vcf_denovo_rows()) == 0
    eng.close()


def test_cli_chrx_detail(built, tmp_path):
    """9. --vcf_denovo_chrX_detail on the planted chrX VCF of tests/test_gpu_vcf_denovo_chrx.py."""
    src = str(tmp_path / "in.vcf")
    head, planted = _write_planted_vcf(src)
    label = planted[PLANT_DAUGHTER][0]
    base = ["--vcf_denovo", "--vcf_denovo_chrX", "--vcf_denovo_families", "2", "--vcf_denovo_carriers", "2"]
    body = lambda lines: [l for l in lines if not l.startswith("##Polymutt=")]
    before = _run_cli(src, str(tmp_path / "before.vcf"), "--chrX", label, *base)
    assert not any(";DNF" in l or ";DNC" in l for l in before if not l.startswith("#"))
    after = _run_cli(src, str(tmp_path / "after.vcf"), "--chrX", label, *base, "--vcf_denovo_chrX_detail")
    assert [l for l in after if l.startswith("#") and not l.startswith("##Polymutt=")] == \
        [l for l in before if l.startswith("#") and not l.startswith("##Polymutt=")]
    recs = [l.split("\t") for l in after if not l.startswith("#")]
    strip_tags = lambda c: "\t".join(c[:7] + [";".join(kv for kv in c[7].split(";") if kv.split("=")[0] not in TAGS)] + c[8:])
    assert [strip_tags(c) for c in recs] == [l for l in before if not l.startswith("#")]   # without the tags: the same bytes
    n_dq = 0
    for c in recs:
        keys = [kv.split("=")[0] for kv in c[7].split(";")]
        if "DQ" in keys:
            n_dq += 1
            assert keys[keys.index("DQ"):] == ["DQ"] + TAGS, c[7]
            assert len(c[3]) == 1 and len(c[4]) == 1, "no indel record carries the tags"
        else:
            assert not set(keys) & set(TAGS), c[7]
    assert n_dq >= 2
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    pids, fs = ped.pids(), ped.fam_start()
    fam1 = next(f for f in range(ped.n_fam) if FAM1[2] in pids[fs[f]:fs[f + 1]])
    famid = ped.lib.pmh_pedigree_famid(ped.h, fam1).decode()
    for k, kid in ((PLANT_DAUGHTER, "3"), (PLANT_SON, "4")):
        rec = planted[k]
        got = [c for c in recs if c[0] == rec[0] and c[1] == rec[1]]
        assert len(got) == 1
        kv = dict(x.split("=", 1) for x in got[0][7].split(";"))
        print(f"record {k}: DQ={kv['DQ']} DNF={kv['DNF']} DNFLR={kv['DNFLR']} DNC={kv['DNC']} DNCP={kv['DNCP']} DNCE={kv['DNCE']}")
        assert kv["DNF"].split(",")[0] == famid and float(kv["DNFLR"].split(",")[0]) > 3, kv
        assert all(re.fullmatch(r"-?\d+\.\d{3}", v) for v in kv["DNFLR"].split(",")), kv["DNFLR"]
        assert kv["DNC"].split(",")[0] == kid and float(kv["DNCP"].split(",")[0]) > 0.99, kv
        r, a = rec[3], rec[4]
        het = "".join(sorted(r + a))
        want = f"{r}x{r}{r}>{het}" if kid == "3" else f"{r}x{r}{r}>{a}"   # a male's genotype is his single allele
        assert kv["DNCE"].split(",")[0] == want, (kv["DNCE"], want)
    # autosomal records (no --chrX match: every record is autosomal) are unchanged by the flag
    auto0 = _run_cli(src, str(tmp_path / "auto0.vcf"), *base)
    auto1 = _run_cli(src, str(tmp_path / "auto1.vcf"), *base, "--vcf_denovo_chrX_detail")
    assert body(auto1) == body(auto0) and any(";DNC=" in l for l in auto0)
