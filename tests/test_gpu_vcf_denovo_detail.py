"""GPU tests of the families and children behind each DQ of --vcf_denovo (pm_engine_set_vcf_denovo_detail and its readers,
the k_vdn_rows and k_vdn_who kernels, and the CLI's --vcf_denovo_families / --vcf_denovo_carriers tags).

A row is a called site whose DQ is at or above denovo_min_llr (1e-300 here: every site with positive de novo evidence).
Per row and family, D_f = log10 L_f^dn(varfreq[2]) - log10 L_f^std(varfreq[1]); per row and non-founder c,
pp_c = Sum_{a,b} J_c(a, b, NonMend3(a, b)) / L_f^dn in the three states of the record's (ref, alt).  The oracle side of every
check runs on the CPU with the vcf_mode oracle on the 255-filled blocks of tests/test_gpu_vcf_denovo.py: a family's term is
the oracle's objective differenced with that family's rows set to 0, a clamp is the person's disallowed bytes among the
three planes set to 255 (tests/test_cpu_vcf_denovo_detail.py pins the identities both rest on).

Cases: the ten of tests/test_gpu_vcf_denovo.py (96 sites in 64-site batches: the second batch is partial), 130 quads (the
256-thread kernel, families across its waves) and 300 mixed families (more terms than threads).  Oracle values on the CPU
gave 10 to 14 rows per case with a child and 10 to 12 planted sites with DQ > 3; the all-founder case has none.
"""
import ctypes as C
import re

import numpy as np
import pytest

import polymutt_amd as pm
from oracle_binding import Oracle
from parity import LLK_RTOL
from polymutt_amd.engine import FAM_LR_DTYPE, PERSON_DN_DTYPE, SITE_DTYPE
from test_gpu_denovo_carriers import MaskedOracle, expected_top as expected_carriers, non_founders, ped_arrays
from test_gpu_denovo_families import expected_top as expected_families
from test_gpu_vcf_denovo import (CASES as BASE_CASES, _arrays, _run_cli, _three, _write_planted_vcf, dataset, oracle_view)

pytestmark = pytest.mark.gpu

CASES = BASE_CASES + [("quad", 130), ("mixed", 300)]
BATCH = 64
MIN_LLR = 1e-300
GENO = ["AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT"]
MEND3 = {(0, 0): {0}, (0, 1): {0, 1}, (0, 2): {1}, (1, 0): {0, 1}, (1, 1): {0, 1, 2}, (1, 2): {1, 2}, (2, 0): {1},
         (2, 1): {1, 2}, (2, 2): {2}}   # the states a child can take from parents in states (a, b)

_runs = {}


def _par():
    return pm.Params.defaults(vcf_mode=1, denovo_min_llr=MIN_LLR)


def _engine(ped, fam_k=8, car_k=8, want_all=True, batch=BATCH):
    eng = pm.Engine(ped.view, _par(), max_batch=batch)
    eng.set_vcf_denovo(True)
    if fam_k or car_k:
        eng.set_vcf_denovo_detail(fam_k, car_k, want_all)
    return eng


def _read(eng, fam_k, car_k):
    rows = eng.vcf_denovo_rows()
    fam = eng.vcf_denovo_families() if fam_k else None
    car = eng.vcf_denovo_carriers() if car_k else None
    return rows, fam, car


def detail_batches(eng, block, refalt, fam_k=8, car_k=8, batch=BATCH):
    """The dataset through the engine in batches: per batch (first site, results, calls, rows, (top, sum, all), (top, all))."""
    out = []
    zeros = np.zeros(block.shape[:2], np.uint32)
    for s in range(0, len(refalt), batch):
        res, calls = eng.run(block[s:s + batch], zeros[s:s + batch], refalt[s:s + batch])
        out.append((s, res, calls) + _read(eng, fam_k, car_k))
    return out


def shared_run(tmp_path_factory, shape, nfam):
    """One engine pass per case (fam_k = car_k = 8, the full matrices), shared by the tests that read it."""
    key = (shape, nfam)
    if key not in _runs:
        ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
        eng = _engine(ped)
        _runs[key] = detail_batches(eng, block, refalt)
        eng.close()
    return _runs[key]


def expected_rows(res):
    return np.nonzero((res["status"] == 0) & (res["evals"][:, 2] > 0) & (res["denovo_lr"] >= MIN_LLR))[0]


@pytest.mark.parametrize("shape,nfam", CASES)
def test_rows(built, tmp_path_factory, shape, nfam):
    """1. the row list is {i : status == 0 and denovo_lr >= threshold} of the engine's own results, in order, per batch; the
    readers' lengths equal it; every case with a child has at least 8 rows, 4 of them with oracle DQ > 3."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    dqo = ov[:, 0] - ov[:, 3]
    total = strong = 0
    for s, res, calls, rows, fam, car in shared_run(tmp_path_factory, shape, nfam):
        assert rows.dtype == np.int32 and rows.tolist() == expected_rows(res).tolist(), (shape, nfam, s)
        assert len(fam[0]) == len(fam[1]) == len(fam[2]) == len(car[0]) == len(car[1]) == len(rows)
        assert fam[0].shape[1:] == (8,) and fam[2].shape[1:] == (ped.n_fam,) and car[1].shape[1:] == (ped.n_person,)
        total += len(rows)
        strong += int((dqo[s + rows] > 3).sum())
    print(f"{shape}/{nfam}: {total} rows, {strong} with oracle DQ > 3")
    if shape == "single":
        # No transmission, no mutation term: the oracle's DQ is <= 0 everywhere.  The engine's N and D come from two Brent
        # runs of the same function (the standard item's and the de novo item's), so its own denovo_lr is rounding noise of
        # either sign, and at 1e-300 a positive one is a row by the rule above (measured: 2 of 96 sites, DQ ~1e-15).  Such
        # rows carry nothing; the batch without any row is taken at the default threshold, where no site of this case can
        # be one.
        assert (dqo <= 0).all()
        noise = 0.0
        for s, res, calls, rows, fam, car in shared_run(tmp_path_factory, shape, nfam):
            r = res[rows]
            noise = max([noise] + np.abs(r["denovo_lr"]).tolist())
            assert (np.abs(r["denovo_lr"]) <= LLK_RTOL * 2 * np.abs(r["varllk"][:, 1])).all()
            assert (car[0]["person"] == -1).all() and (car[1]["pp"] == 0).all()
        print(f"{shape}/{nfam}: largest |DQ| of a row = {noise:.3g}")
        eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)   # denovo_min_llr = 0.01
        eng.set_vcf_denovo(True)
        eng.set_vcf_denovo_detail(8, 8, True)
        for s, res, calls, rows, fam, car in detail_batches(eng, block, refalt):
            assert len(rows) == 0 and len(fam[0]) == len(fam[1]) == len(fam[2]) == len(car[0]) == len(car[1]) == 0
            assert (res["evals"][:, 2] > 0).all()
        eng.close()
    else:
        assert total >= 8 and strong >= 4, (shape, nfam, total, strong)


def oracle_family_terms(ora, fs, site, a1, a2, x_dn, x_std):
    """(D_f, |l_f^dn| + |l_f^std|) per family: the oracle's objective differenced with family f's rows set to 0."""
    full_dn, full_std = ora.objective(site, a1, a2, x_dn, 1), ora.objective(site, a1, a2, x_std, 0)
    nf = len(fs) - 1
    D, mag = np.zeros(nf), np.zeros(nf)
    for f in range(nf):
        cut = site.copy()
        cut[fs[f]:fs[f + 1]] = 0
        l_dn = ora.objective(cut, a1, a2, x_dn, 1) - full_dn
        l_std = ora.objective(cut, a1, a2, x_std, 0) - full_std
        D[f], mag[f] = l_dn - l_std, abs(l_dn) + abs(l_std)
    return D, mag


@pytest.mark.parametrize("shape,nfam", CASES)
def test_family_terms_match_oracle(built, tmp_path_factory, shape, nfam):
    """2. all[row][f] against the oracle at the engine's varfreq[2] (de novo) and varfreq[1] (standard), within
    LLK_RTOL (|l_dn| + |l_std|) + 1e-10; sum against denovo_lr and all.sum(1) within LLK_RTOL (|varllk[2]| + |varllk[1]|);
    top = the stable descending argsort."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    view, keep = oracle_view(ped)
    ora = Oracle(view, pm.Params.defaults(vcf_mode=1))
    fs, _ = _arrays(ped)
    worst = worst_sum = 0.0
    for s, res, calls, rows, (top, tot, full), car in shared_run(tmp_path_factory, shape, nfam):
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
            a1, a2, _ = _three(refalt[s + i])
            exp, mag = oracle_family_terms(ora, fs, np.ascontiguousarray(block[s + i]), a1, a2,
                                           float(res["varfreq"][i, 2]), float(res["varfreq"][i, 1]))
            err, bnd = np.abs(full[k] - exp), LLK_RTOL * mag + 1e-10
            worst = max(worst, float((err / bnd).max()))
            assert (err <= bnd).all(), (shape, nfam, s + i, int(np.argmax(err / bnd)), float(err.max()))
    print(f"{shape}/{nfam}: worst family error / bound = {worst:.3g}, worst sum error / bound = {worst_sum:.3g}")
    del ora, keep


def check_child(M, g, c, fa, mo, entry):
    """One child's entry against the masked oracle in the three states g; returns error / bound."""
    J = {}
    for (a, b), mend in MEND3.items():
        non = [s for s in range(3) if s not in mend]
        J[(a, b)] = M.ratio({fa: [g[a]], mo: [g[b]], c: [g[s] for s in non]}) if non else 0.0
    pp = sum(J.values())
    bound = np.log(10) * LLK_RTOL * (abs(M.full) + M.mag) * pp + 1e-12
    err = abs(float(entry["pp"]) - pp)
    assert err <= bound, (c, float(entry["pp"]), pp, bound)
    assert 0.0 <= entry["pp"] <= 1.0
    ev = (int(entry["fa_g"]), int(entry["mo_g"]), int(entry["kid_g"]))
    jmax = max(J.values())
    if ev == (-1, -1, -1):
        assert jmax <= bound, (c, ev, jmax)
    else:
        assert ev[0] in g and ev[1] in g and ev[2] in g, (c, ev)
        a, b, s = g.index(ev[0]), g.index(ev[1]), g.index(ev[2])
        assert s not in MEND3[(a, b)], (c, ev)
        assert J[(a, b)] >= jmax - bound, (c, ev, J[(a, b)], jmax)
        Js = {t: M.ratio({fa: [g[a]], mo: [g[b]], c: [g[t]]}) for t in range(3) if t not in MEND3[(a, b)]}
        assert Js[s] >= max(Js.values()) - bound, (c, ev, Js)
    return err / bound


@pytest.mark.parametrize("shape,nfam", CASES)
def test_carriers_match_oracle(built, tmp_path_factory, shape, nfam):
    """3. all[row][c] and the event against the masked oracle, bound ln(10) LLK_RTOL (|full| + max |masked|) pp + 1e-12, on up
    to 6 rows per case, planted and unplanted (with more than 40 non-founders: the engine's top-8 plus every 7th child);
    founders blank, 0 <= pp <= 1 and top = the stable ranking of all on every row; on planted rows with oracle DQ > 3 the
    planted child is top[row][0] with pp > 0.99."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    view, keep = oracle_view(ped)
    ora = Oracle(view, pm.Params.defaults(vcf_mode=1))
    _, _, fa, mo = ped_arrays(ped.view)
    kids = non_founders(ped.view)
    founder = np.ones(ped.n_person, bool)
    founder[kids] = False
    fs, fo = _arrays(ped)
    fam0 = next((f for f in range(len(fs) - 1) if not fo[fs[f]:fs[f + 1]].all()), None)
    plant_kids = [] if fam0 is None else [p for p in range(fs[fam0], fs[fam0 + 1]) if not fo[p]]
    dqo = ov[:, 0] - ov[:, 3]
    worst, picked, n_planted_checked = 0.0, {True: 0, False: 0}, 0
    for s, res, calls, rows, fam, (top, full) in shared_run(tmp_path_factory, shape, nfam):
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
            a1, a2, g = _three(refalt[s + i])
            is_planted = (s + i) in planted
            if is_planted and dqo[s + i] > 3:
                child = plant_kids[((s + i) // 8) % len(plant_kids)]
                assert top[k, 0]["person"] == child and top[k, 0]["pp"] > 0.99, (shape, nfam, s + i, top[k, 0], child)
                assert (int(top[k, 0]["fa_g"]), int(top[k, 0]["mo_g"]), int(top[k, 0]["kid_g"])) == (g[0], g[0], g[1])
                n_planted_checked += 1
            if picked[is_planted] >= 3:
                continue
            picked[is_planted] += 1
            M = MaskedOracle(ora, np.ascontiguousarray(block[s + i]), a1, a2, float(res["varfreq"][i, 2]))
            todo = kids
            if len(kids) > 40:
                todo = sorted(set(int(p) for p in top[k]["person"] if p >= 0) | set(int(p) for p in kids[::7]))
            for c in todo:
                worst = max(worst, check_child(M, g, int(c), int(fa[c]), int(mo[c]), ent[c]))
    print(f"{shape}/{nfam}: worst carrier error / bound = {worst:.3g} over {picked[True]} planted and {picked[False]} other rows")
    if shape != "single":
        assert picked[True] >= 1 and n_planted_checked >= 4, (picked, n_planted_checked)
    del ora, keep


def _tops(batches):
    return [(rows.tobytes(), fam[0].tobytes(), fam[1].tobytes(), car[0].tobytes()) for _, _, _, rows, fam, car in batches]


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("extmix", 5)])
def test_side_effects(built, tmp_path_factory, shape, nfam):
    """4. detail on: the results and the genotype rows are those of set_vcf_denovo(True) alone; off again: a fresh
    engine's; want_all = False gives the same top."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    fresh = _engine(ped, 0, 0)
    b0 = detail_batches(fresh, block, refalt, 0, 0)
    fresh.close()
    eng = _engine(ped, 0, 0)
    eng.set_vcf_denovo_detail(8, 8, True)
    b_on = detail_batches(eng, block, refalt)
    eng.set_vcf_denovo_detail(8, 8, False)
    b_top = detail_batches(eng, block, refalt)
    eng.set_vcf_denovo_detail(0, 0)
    b_off = detail_batches(eng, block, refalt, 0, 0)
    eng.close()
    for x, y, z, w in zip(b0, b_on, b_top, b_off):
        for other in (y, z, w):
            assert other[1].tobytes() == x[1].tobytes() and other[2].tobytes() == x[2].tobytes()
        assert len(w[3]) == 0 and len(y[3]) == len(expected_rows(x[1]))
        assert z[4][2] is None and z[5][1] is None
    assert [t[:2] + t[3:] for t in _tops(b_top)] == [t[:2] + t[3:] for t in _tops(b_on)]
    assert _tops(b_on) == _tops(shared_run(tmp_path_factory, shape, nfam))   # (and a second engine gives the same bytes)


def test_entry_points_agree(built, tmp_path_factory):
    """5. run, run_vcf, submit / collect and run_device + sync give identical row lists and top bytes, twice over."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "mixed", 31)
    n, npers = 64, ped.n_person
    pl, ra = np.ascontiguousarray(block[:n]), np.ascontiguousarray(refalt[:n])
    zeros = np.zeros((n, npers), np.uint32)
    eng = _engine(ped, 4, 4, False, batch=n)
    got = []
    for rep in range(2):
        eng.run(pl, zeros, ra)
        got.append(_read(eng, 4, 4))
        eng.run_vcf(pl, ra)
        got.append(_read(eng, 4, 4))
        eng.submit(pl, zeros, ra)
        eng.collect()
        got.append(_read(eng, 4, 4))
        d_src, d_pl = eng.alloc(n * npers * 10), eng.alloc(n * npers * 10)
        d_ref, d_res = eng.alloc(n), eng.alloc(n * SITE_DTYPE.itemsize)
        eng.to_device(d_src, pl, n * npers * 10)
        eng.to_device(d_ref, ra, n)
        eng.to_planar(n, d_src, d_pl)
        eng.run_device(n, d_pl, None, d_ref, d_res, None)
        eng.sync()
        got.append(_read(eng, 4, 4))
        for p in (d_src, d_pl, d_ref, d_res):
            eng.free(p)
    eng.close()
    rows0, fam0, car0 = got[0]
    assert len(rows0) >= 4
    for rows, fam, car in got[1:]:
        assert rows.tobytes() == rows0.tobytes()
        assert fam[0].tobytes() == fam0[0].tobytes() and fam[1].tobytes() == fam0[1].tobytes() and fam[2] is None
        assert car[0].tobytes() == car0[0].tobytes() and car[1] is None


def test_non_autosomal_sections_have_no_rows(built, tmp_path_factory):
    """5. a chrX section gives n_rows == 0 (and the readers succeed); rows come back on the next autosome."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "mixed", 31)
    eng = _engine(ped)
    first = detail_batches(eng, block, refalt)
    eng.begin_section(pm.PM_CHR_X)
    for s, res, calls, rows, fam, car in detail_batches(eng, block, refalt):
        assert len(rows) == 0 and len(fam[0]) == len(fam[1]) == len(fam[2]) == len(car[0]) == len(car[1]) == 0
        assert (res["evals"][:, 2] == 0).all()
    eng.begin_section(pm.PM_CHR_AUTO)
    assert _tops(detail_batches(eng, block, refalt)) == _tops(first)
    eng.close()


def test_stuck_site_keeps_the_rows_before_it(built, tmp_path_factory, monkeypatch):
    """5. under PM_TEST_ITMAX (chosen as tests/test_gpu_vcf_denovo.py::test_vcf_denovo_stuck_site does) the rows before the
    stuck site equal the normal run's."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "quad", 70)
    loops = np.stack([ov[:, 2], ov[:, 5]], axis=1).astype(int) - 3   # de novo, standard
    best = None
    for k in sorted(set(int(x) for x in loops.ravel() if x > 0)):
        idx = np.nonzero((loops >= k).any(axis=1))[0]
        if len(idx) and 0 < idx[0] < 64 and loops[idx[0], 0] >= k > loops[idx[0], 1]:
            if best is None or abs(idx[0] - 32) < abs(best[1] - 32):
                best = (k, int(idx[0]))
    if best is None:
        for k in sorted(set(int(x) for x in loops.ravel() if x > 0)):
            idx = np.nonzero((loops >= k).any(axis=1))[0]
            if len(idx) and 0 < idx[0] < 64:
                best = (k, int(idx[0]))
    assert best is not None
    k, s = best
    zeros = np.zeros((64, ped.n_person), np.uint32)
    eng = _engine(ped)
    eng.run(block[:64], zeros, refalt[:64])
    rows0, fam0, car0 = _read(eng, 8, 8)
    eng.close()
    keep = int((rows0 < s).sum())
    assert 0 < keep, (rows0, s)
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))
    eng = _engine(ped)
    with pytest.raises(pm.engine.BrentStuck) as ei:
        eng.run(block[:64], zeros, refalt[:64])
    assert ei.value.site == s == eng.stuck_site(), (ei.value.site, s, k)
    rows, fam, car = _read(eng, 8, 8)
    eng.close()
    assert rows.tolist() == rows0[:keep].tolist()
    for a, b in zip(fam + car, fam0 + car0):
        assert a.tobytes() == b[:keep].tobytes()


def test_api_errors(built, tmp_path_factory):
    """6. every PM_EINVAL with its message; afterwards the engine still runs; the GLF-path setters still refuse."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, "trio", 3)
    lib = pm.load_library()
    err = lambda: lib.pm_last_error()
    glf = pm.Engine(ped.view, pm.Params.defaults(denovo=1), max_batch=8)
    assert lib.pm_engine_set_vcf_denovo_detail(glf.h, 1, 1, 0) == -1 and b"vcf_mode" in err()
    glf.close()
    eng = pm.Engine(ped.view, _par(), max_batch=8)
    zeros = np.zeros((8, ped.n_person), np.uint32)
    assert lib.pm_engine_set_vcf_denovo_detail(eng.h, 1, 1, 0) == -1 and b"vcf_denovo" in err()
    n = C.c_int32(7)
    assert lib.pm_engine_vcf_denovo_rows(eng.h, C.byref(n), None) == 0 and n.value == 0   # off: no rows
    eng.set_vcf_denovo(True)
    for fk, ck in ((-1, 1), (9, 1), (1, -1), (1, 9)):
        assert lib.pm_engine_set_vcf_denovo_detail(eng.h, fk, ck, 0) == -1 and b"1..8" in err(), (fk, ck)
    eng.submit(block[:8], zeros, refalt[:8])
    assert lib.pm_engine_set_vcf_denovo_detail(eng.h, 1, 1, 0) == -1 and b"not been collected" in err()
    eng.collect()
    # a want_all matrix above 1 GiB: max_batch x n_person x 16 bytes
    big = pm.Engine(ped.view, _par(), max_batch=(1 << 30) // (16 * ped.n_person) + 1)
    big.set_vcf_denovo(True)
    assert lib.pm_engine_set_vcf_denovo_detail(big.h, 0, 1, 1) == -1 and b"1 GiB" in err()
    assert lib.pm_engine_set_vcf_denovo_detail(big.h, 1, 1, 0) == 0
    big.close()
    # a reader for a half that is off, and the full matrix without want_all
    top_f, top_c = np.zeros((8, 2), FAM_LR_DTYPE), np.zeros((8, 2), PERSON_DN_DTYPE)
    full_f, full_c = np.zeros((8, ped.n_fam)), np.zeros((8, ped.n_person), PERSON_DN_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    eng.set_vcf_denovo_detail(2, 0)
    assert lib.pm_engine_vcf_denovo_carriers(eng.h, ptr(top_c), None) == -1 and b"off" in err()
    assert lib.pm_engine_vcf_denovo_families(eng.h, ptr(top_f), None, ptr(full_f)) == -1 and b"want_all" in err()
    eng.set_vcf_denovo_detail(0, 2)
    assert lib.pm_engine_vcf_denovo_families(eng.h, ptr(top_f), None, None) == -1 and b"off" in err()
    assert lib.pm_engine_vcf_denovo_carriers(eng.h, ptr(top_c), ptr(full_c)) == -1 and b"want_all" in err()
    # pm_engine_set_vcf_denovo(eng, 0) also switches the detail off
    eng.set_vcf_denovo_detail(2, 2)
    eng.set_vcf_denovo(False)
    assert lib.pm_engine_vcf_denovo_families(eng.h, ptr(top_f), None, None) == -1 and b"off" in err()
    assert lib.pm_engine_set_vcf_denovo_detail(eng.h, 2, 2, 0) == -1 and b"vcf_denovo" in err()
    # the per-family and per-person features of the GLF path keep refusing vcf_mode engines
    assert lib.pm_engine_set_denovo_families(eng.h, 1, 0) == -1
    assert lib.pm_engine_set_denovo_carriers(eng.h, 1, 0) == -1
    # and the engine still runs
    eng.set_vcf_denovo(True)
    eng.set_vcf_denovo_detail(2, 2)
    res, _ = eng.run(block[:8], zeros, refalt[:8])
    rows, fam, car = _read(eng, 2, 2)
    assert rows.tolist() == expected_rows(res).tolist() and len(rows) >= 1 and fam[0].shape == (len(rows), 2)
    eng.close()


# ------------------------------------------------------------------------------------------------
# CLI: --vcf_denovo_families / --vcf_denovo_carriers on the example input with a planted event

TAGS = ["DNF", "DNFLR", "DNC", "DNCP", "DNCE"]


def _strip(lines, tags=TAGS):
    out = []
    for l in lines:
        if l.startswith("##Polymutt=") or any(l.startswith(f"##INFO=<ID={t},") for t in tags):
            continue
        if not l.startswith("#"):
            c = l.split("\t")
            c[7] = ";".join(kv for kv in c[7].split(";") if kv.split("=")[0] not in tags)
            l = "\t".join(c)
        out.append(l)
    return out


def test_cli_tags(built, tmp_path):
    import os
    from conftest import EXAMPLE
    src = str(tmp_path / "in.vcf")
    head, planted = _write_planted_vcf(src)
    tagged = _run_cli(src, str(tmp_path / "dn.vcf"), "--vcf_denovo")
    both = _run_cli(src, str(tmp_path / "both.vcf"), "--vcf_denovo", "--vcf_denovo_families", "2", "--vcf_denovo_carriers", "2")
    assert _strip(both) == [l for l in tagged if not l.startswith("##Polymutt=")]
    info = [l[len("##INFO=<ID="):].split(",")[0] for l in both if l.startswith("##INFO=<ID=")]
    assert info[info.index("DQ"):info.index("DQ") + 6] == ["DQ"] + TAGS
    recs = [l.split("\t") for l in both if not l.startswith("#")]
    n_dq = 0
    for c in recs:
        keys = [kv.split("=")[0] for kv in c[7].split(";")]
        if "DQ" in keys:
            n_dq += 1
            assert keys[keys.index("DQ"):] == ["DQ"] + TAGS, c[7]
            assert len(c[3]) == 1 and len(c[4]) == 1
        else:
            assert not set(keys) & set(TAGS), c[7]
    assert n_dq >= 1
    # the planted record: fam2 (parents 5, 6, children 7, 8), child 7 het, everyone else of the family hom-ref
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    pids = ped.pids()
    fs = ped.fam_start()
    fam_of_7 = next(f for f in range(ped.n_fam) if "7" in pids[fs[f]:fs[f + 1]])
    famid = ped.lib.pmh_pedigree_famid(ped.h, fam_of_7).decode()
    got = [c for c in recs if c[0] == planted[0] and c[1] == planted[1]]
    assert len(got) == 1
    kv = dict(x.split("=", 1) for x in got[0][7].split(";"))
    assert kv["DNF"].split(",")[0] == famid, (kv["DNF"], famid)
    assert len(kv["DNF"].split(",")) == 2 and len(kv["DNFLR"].split(",")) == 2
    assert all(re.fullmatch(r"-?\d+\.\d{3}", v) for v in kv["DNFLR"].split(",")), kv["DNFLR"]
    assert float(kv["DNFLR"].split(",")[0]) > 3
    assert kv["DNC"].split(",")[0] == "7" and float(kv["DNCP"].split(",")[0]) > 0.99, kv
    r, a = planted[3], planted[4]
    het = "".join(sorted(r + a))   # two-letter genotypes from the GLF index: alleles in A, C, G, T order
    assert kv["DNCE"].split(",")[0] == f"{r}{r}x{r}{r}>{het}", kv["DNCE"]
    # one flag alone prints only its own tags
    fam_only = _run_cli(src, str(tmp_path / "f.vcf"), "--vcf_denovo", "--vcf_denovo_families", "2")
    car_only = _run_cli(src, str(tmp_path / "c.vcf"), "--vcf_denovo", "--vcf_denovo_carriers", "2")
    assert _strip(fam_only, TAGS[:2]) == _strip(both) and not any(f";{t}=" in l for l in fam_only for t in TAGS[2:])
    assert _strip(car_only, TAGS[2:]) == _strip(both) and not any(f";{t}=" in l for l in car_only for t in TAGS[:2])
    assert [l for l in _strip(both, TAGS[2:]) if ";DNF=" in l] == [l for l in _strip(fam_only, []) if ";DNF=" in l]
    assert [l for l in _strip(both, TAGS[:2]) if ";DNC=" in l] == [l for l in _strip(car_only, []) if ";DNC=" in l]
