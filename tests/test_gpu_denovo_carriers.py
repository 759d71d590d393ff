"""GPU tests of the per-person de novo posteriors (pm_engine_set_denovo_carriers / pm_engine_denovo_carriers, the
k_person_dn kernel, and the CLI's --denovo_carriers tags).

For a written record and a non-founder c with father fa and mother mo, pp_c = Sum_{a,b} J_c(a, b, NonMend(a, b)) / L_f
in the de novo model at the record's alleles and frequency, J_c(a, b, S) being the family likelihood restricted to
G_fa = a, G_mo = b, G_c in S.  The oracle side of every check runs on the CPU: clamping a person to a genotype set is
setting the person's other PL bytes to 255, and the unchanged oracle's objective (minus the sum of the families' log10
likelihoods) differenced with and without the clamps is log10 (J / L_f).

Datasets: the shapes, seeds and flags of tests/test_gpu_denovo_families.py (all_sites = 1, denovo_min_llr = 1e-300,
64-site batches).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE, ROOT
from fixtures import LLK_RTOL
from oracle_binding import Oracle
from test_gpu_denovo_families import BATCH, CASES, _phred, check_rows, dataset

pytestmark = pytest.mark.gpu

DT = pm.engine.PERSON_DN_DTYPE
GENO = ["AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT"]
ALLELES = [(1, 1), (1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (2, 4), (3, 3), (3, 4), (4, 4)]   # GLF order
GI = {al: g for g, al in enumerate(ALLELES)}

_runs = {}


def gi(x, y):
    return GI[(min(x, y), max(x, y))]


def non_mendelian(a, b):
    """The genotypes that cannot take one allele from a and one from b (autosomal rule)."""
    mend = {gi(x, y) for x in ALLELES[a] for y in ALLELES[b]}
    return [g for g in range(10) if g not in mend]


def ped_arrays(view):
    """(fam_start, fam_kind, father, mother) of a PedigreeStruct; father / mother are person indices or -1."""
    fs = np.ctypeslib.as_array(view.fam_start, shape=(view.n_fam + 1,)).copy()
    kind = np.ctypeslib.as_array(view.fam_kind, shape=(view.n_fam,)).copy()
    fa = np.ctypeslib.as_array(view.father, shape=(view.n_person,)).copy()
    mo = np.ctypeslib.as_array(view.mother, shape=(view.n_person,)).copy()
    return fs, kind, fa, mo


def non_founders(view):
    fs, kind, fa, mo = ped_arrays(view)
    out = []
    for f in range(view.n_fam):
        if kind[f] == pm.FAM_FOUNDERS:
            continue
        out += [p for p in range(fs[f], fs[f + 1]) if fa[p] >= 0 and mo[p] >= 0]
    return np.array(out, dtype=np.int64)


def engine_batches(D, car_k, want_all=True, how="run", batch=BATCH, pl=None, fam_k=0):
    """The dataset through an engine in batches: per batch (first site, results, calls, top, all, families)."""
    pl = D["pl"] if pl is None else pl
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=batch)
    eng.begin_section(D["chrom"])
    if fam_k:
        eng.set_denovo_families(fam_k, True)
    if car_k:
        eng.set_denovo_carriers(car_k, want_all)
    out = []
    for s in range(0, len(D["ref"]), batch):
        sl = slice(s, s + batch)
        if how == "run":
            res, calls = eng.run(pl[sl], D["dm"][sl], D["ref"][sl])
        else:
            eng.submit(pl[sl], D["dm"][sl], D["ref"][sl])
            res, calls = eng.collect()
        top, full = eng.denovo_carriers() if car_k else (None, None)
        fam = eng.denovo_families() if fam_k else None
        if car_k:
            assert len(top) == len(calls) == int((res["call_row"] >= 0).sum())
        out.append((s, res, calls, top, full, fam))
    eng.close()
    return out


def shared_run(name, tmp_path_factory):
    """One engine pass per case (top_k = 8, the full matrix), shared by the tests that read it."""
    if name not in _runs:
        _runs[name] = engine_batches(dataset(name, tmp_path_factory), 8)
    return _runs[name]


def site_model(ref, r):
    """(a1, a2, x): the alleles and frequency of the de novo numerator of a written record."""
    if r["maxidx"] == 0:
        return int(ref), (3 if ref == 4 else int(ref) + 1), 1.0
    return int(r["allele1"]), int(r["allele2"]), float(r["varfreq"][r["maxidx"]])


class MaskedOracle:
    """J / L_f of one site by PL masking: ratio({person: genotypes allowed})."""

    def __init__(self, ora, pl_site, a1, a2, x):
        self.ora, self.pl, self.m = ora, pl_site, (a1, a2, x)
        self.full = ora.objective(pl_site, a1, a2, x, 1)
        self.mag = 0.0   # max |objective| of the masked calls

    def ratio(self, clamps):
        cut = self.pl.copy()
        for p, allowed in clamps.items():
            keep = np.zeros(10, bool)
            keep[list(allowed)] = True
            cut[p, ~keep] = 255
        v = self.ora.objective(cut, *self.m, 1)
        if not np.isfinite(v):
            return 0.0
        self.mag = max(self.mag, abs(v))
        return 10.0 ** (self.full - v)


def parent_genotypes(is_founder_parent, a1, a2):
    return sorted({gi(a1, a1), gi(a1, a2), gi(a2, a2)}) if is_founder_parent else list(range(10))


def check_child(M, c, fa, mo, fa_founder, mo_founder, entry, closure=False):
    """One child's entry against the masked oracle; returns error / bound."""
    a1, a2, _ = M.m
    pairs = [(a, b) for a in parent_genotypes(fa_founder, a1, a2) for b in parent_genotypes(mo_founder, a1, a2)]
    J = {ab: M.ratio({fa: [ab[0]], mo: [ab[1]], c: non_mendelian(*ab)}) for ab in pairs}
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
        assert (ev[0], ev[1]) in J and ev[2] in non_mendelian(ev[0], ev[1]), (c, ev)
        assert J[(ev[0], ev[1])] >= jmax - bound, (c, ev, J[(ev[0], ev[1])], jmax)
        Jg = {g: M.ratio({fa: [ev[0]], mo: [ev[1]], c: [g]}) for g in non_mendelian(ev[0], ev[1])}
        assert Jg[ev[2]] >= max(Jg.values()) - bound, (c, ev, Jg)
    if closure:   # the masking reference itself: the joint over (a, b, g) sums to the family likelihood
        tot = sum(M.ratio({fa: [a], mo: [b], c: [g]}) for a, b in pairs for g in range(10))
        assert abs(tot - 1.0) <= 1e-12, (c, tot)
    return err / bound


@pytest.mark.parametrize("name", list(CASES))
def test_posteriors_match_oracle(built, tmp_path_factory, name):
    """1. all[row][c].pp and the event against the masked oracle.  Bound: ln(10) LLK_RTOL (|obj_full| + max |obj_masked|)
    pp + 1e-12 (LLK_RTOL on the two log-likelihoods differenced; the floor covers the 10^-25.5 leak of a masked byte).
    At least 4 rows per case, monomorphic and polymorphic ones; with more than 40 non-founders, per row the engine's
    top-8 persons plus every 7th non-founder."""
    D = dataset(name, tmp_path_factory)
    batches = shared_run(name, tmp_path_factory)
    check_rows(batches)
    view = D["ped"].view
    fs, kind, fa, mo = ped_arrays(view)
    kids = non_founders(view)
    founder = np.ones(view.n_person, bool)
    founder[kids] = False
    ora = Oracle(view, D["par"])
    ora.begin_section(D["chrom"])
    picked = []   # up to 3 monomorphic and 3 polymorphic rows
    for s, res, calls, top, full, _ in batches:
        for i in np.nonzero(res["call_row"] >= 0)[0]:
            mono = res["maxidx"][i] == 0
            if sum(1 for *_, m in picked if m == mono) < 3:
                picked.append((s, i, res, top, full, mono))
    assert len(picked) >= 4 and {m for *_, m in picked} == {True, False}
    worst, closed = 0.0, False
    for s, i, res, top, full, mono in picked:
        row = res["call_row"][i]
        ent = full[row]
        assert (ent["person"] == np.arange(view.n_person)).all() and not ent["pad"].any()
        fo = ent[founder]
        assert (fo["fa_g"] == -1).all() and (fo["mo_g"] == -1).all() and (fo["kid_g"] == -1).all() and (fo["pp"] == 0.0).all()
        assert ((ent["pp"] >= 0) & (ent["pp"] <= 1)).all()
        M = MaskedOracle(ora, D["pl"][s + i], *site_model(int(D["ref"][s + i]), res[i]))
        todo = kids
        if len(kids) > 40:
            todo = sorted(set(int(p) for p in top[row]["person"] if p >= 0) | set(int(p) for p in kids[::7]))
        for c in todo:
            worst = max(worst, check_child(M, c, fa[c], mo[c], founder[fa[c]], founder[mo[c]], ent[c], closure=not closed))
            closed = True
    print(f"{name}: worst error / bound = {worst:.3g} over {len(picked)} rows")


def expected_top(ent, kids, k):
    """The stable descending argsort of the non-founders' pp (ties by lower person index), padded."""
    out = np.zeros((len(ent), k), dtype=DT)
    out["person"] = -1
    out["fa_g"] = out["mo_g"] = out["kid_g"] = -1
    for r in range(len(ent)):
        order = kids[np.argsort(-ent[r]["pp"][kids], kind="stable")][:k]
        out[r, :len(order)] = ent[r][order]
    return out


@pytest.mark.parametrize("name", ["quad1", "trio3", "mixed31", "quad70", "quad130", "extmix10"])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_ranking(built, tmp_path_factory, name, k):
    """2. top = the stable descending argsort of the engine's own full matrix, bytewise, padding included."""
    D = dataset(name, tmp_path_factory)
    kids = non_founders(D["ped"].view)
    nrows = 0
    for s, res, calls, top, full, _ in engine_batches(D, k):
        assert top.tobytes() == expected_top(full, kids, k).tobytes(), (name, s)
        nrows += len(full)
    assert nrows >= 8
    if name in ("quad1", "trio3"):
        assert len(kids) < 8


def test_ranking_ties(built, tmp_path_factory):
    """2. kids of families without data (all PL 0) have bit-equal posteriors: ties rank by person index."""
    D = dataset("quad70", tmp_path_factory)
    fs = D["ped"].fam_start()
    kids = non_founders(D["ped"].view)
    pl = D["pl"].copy()
    for f in range(70):
        if f % 9:   # data only in families 0, 9, ..., 63
            pl[:, fs[f]:fs[f + 1]] = 0
    tied = rows = 0
    for s, res, calls, top, full, _ in engine_batches(D, 8, pl=pl):
        assert top.tobytes() == expected_top(full, kids, 8).tobytes(), s
        rows += len(full)
        tied += int((top["pp"][:, 1:] == top["pp"][:, :-1]).any(axis=1).sum())
    assert rows >= 1 and tied >= 1, (rows, tied)


def test_planted_carrier_ranks_first(built):
    """3. twelve quads; a het kid of hom-ref parents planted on a monomorphic site (person 14) and on a site where the
    alternative allele also segregates in other families (person 30): top[0] names the kid and the event AA x AA > AG."""
    import bench
    ped = bench.quad_pedigree(pm, 12, 2)
    npers = ped.n_person
    assert npers == 48
    sites = np.zeros((2, npers, 10), np.uint8)
    sites[:, :] = _phred("RR")
    sites[0, 3 * 4 + 2] = _phred("RA")
    for f in (1, 4, 9):
        sites[1, f * 4] = _phred("RA")
        sites[1, f * 4 + 3] = _phred("RA")
    sites[1, 7 * 4 + 2] = _phred("RA")
    dm = np.full((2, npers), 20 | (60 << 24), np.uint32)
    ref = np.array([1, 1], np.uint8)
    par = pm.Params.defaults(denovo=1, denovo_mut_rate=1.5e-7, all_sites=1, denovo_min_llr=1e-300)
    eng = pm.Engine(ped, par, max_batch=2)
    eng.set_denovo_carriers(4, True)
    res, calls = eng.run(sites, dm, ref)
    top, full = eng.denovo_carriers()
    eng.close()
    assert len(calls) == 2 and res["maxidx"][0] == 0 and res["maxidx"][1] >= 1, res[["maxidx", "emit", "denovo_lr"]]
    print("planted pp:", top["pp"][:, 0], "others max:", [float(np.delete(full[r]["pp"], p).max()) for r, p in ((0, 14), (1, 30))])
    for r, p in ((0, 14), (1, 30)):
        t = top[r, 0]
        assert t["person"] == p and (t["fa_g"], t["mo_g"], t["kid_g"]) == (0, 0, 2), t
        assert t["pp"] > 0.5
        assert np.delete(full[r]["pp"], p).max() < 1e-9


def test_paths_agree_bit_for_bit(built, tmp_path_factory):
    """4. run, submit / collect and run_device + sync give identical bits, and so do two runs."""
    for name in ("quad130", "ext10x3"):
        D = dataset(name, tmp_path_factory)
        a = shared_run(name, tmp_path_factory)
        b = engine_batches(D, 8, how="run")
        c = engine_batches(D, 8, how="submit")
        for x, y, z in zip(a, b, c):
            for j in (3, 4):
                assert x[j].tobytes() == y[j].tobytes() == z[j].tobytes(), (name, x[0], j)
        ped, n = D["ped"], BATCH
        npers = ped.n_person
        eng = pm.Engine(ped.view, D["par"], max_batch=n)
        eng.begin_section(D["chrom"])
        eng.set_denovo_carriers(8, True)
        d_pl, d_dm, d_ref = eng.alloc(n * npers * 10), eng.alloc(n * npers * 4), eng.alloc(n)
        eng.to_device(d_pl, pm.planar(D["pl"][:n]), n * npers * 10)
        eng.to_device(d_dm, D["dm"][:n], n * npers * 4)
        eng.to_device(d_ref, D["ref"][:n], n)
        eng.run_device(n, d_pl, d_dm, d_ref, None, None)
        eng.sync()
        top, full = eng.denovo_carriers()
        for p in (d_pl, d_dm, d_ref):
            eng.free(p)
        eng.close()
        assert len(top) == len(a[0][3]) > 0
        assert top.tobytes() == a[0][3].tobytes() and full.tobytes() == a[0][4].tobytes()


@pytest.mark.parametrize("name", ["quad130", "extmix10"])
def test_no_side_effects(built, tmp_path_factory, name):
    """5. results and genotype rows are byte-identical with the feature off, on, and on together with the family
    feature; the family outputs are byte-identical with and without carriers; the lean form (no full matrix) agrees."""
    D = dataset(name, tmp_path_factory)
    on = shared_run(name, tmp_path_factory)
    off = engine_batches(D, 0)
    both = engine_batches(D, 8, fam_k=8)
    fam_only = engine_batches(D, 0, fam_k=8)
    lean = engine_batches(D, 2, want_all=False)
    for x, y, z, w, v in zip(on, off, both, fam_only, lean):
        assert x[1].tobytes() == y[1].tobytes() == z[1].tobytes() == v[1].tobytes()
        assert x[2].tobytes() == y[2].tobytes() == z[2].tobytes() == v[2].tobytes()
        assert x[3].tobytes() == z[3].tobytes() and x[4].tobytes() == z[4].tobytes()
        for j in range(3):
            assert z[5][j].tobytes() == w[5][j].tobytes()
        assert v[4] is None and v[3].tobytes() == np.ascontiguousarray(x[3][:, :2]).tobytes()


def test_rows_before_a_stuck_site(built, tmp_path_factory, monkeypatch):
    """6. after PM_EBRENT (ITMAX lowered with PM_TEST_ITMAX) the rows before the stuck site equal the undisturbed run's."""
    from test_brent_stuck import first_stuck
    D = dataset("quad70", tmp_path_factory)
    full = shared_run("quad70", tmp_path_factory)
    s, res, calls, top, allm, _ = max(full, key=lambda b: len(b[3]))
    ev = res["evals"]
    loop = np.where(ev >= 3, ev - 3, -1).max(axis=1)
    before = lambda k: int((res["call_row"][:first_stuck(res, k)] >= 0).sum())
    k = max(sorted(set(int(x) for x in loop if x > 0)), key=before)   # the ITMAX that leaves the most rows complete
    assert before(k) >= 1
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=BATCH)
    eng.begin_section(D["chrom"])
    eng.set_denovo_carriers(8, True)
    with pytest.raises(pm.engine.BrentStuck) as e:
        eng.run(D["pl"][s:s + BATCH], D["dm"][s:s + BATCH], D["ref"][s:s + BATCH])
    top2, all2 = eng.denovo_carriers()
    eng.close()
    n = int((res["call_row"][:e.value.site] >= 0).sum())
    assert 1 <= n == len(e.value.calls) == len(top2) < len(top)
    assert top2.tobytes() == top[:n].tobytes() and all2.tobytes() == allm[:n].tobytes()


def test_api_argument_errors(built, tmp_path_factory):
    """7. the PM_EINVAL cases."""
    D = dataset("trio3", tmp_path_factory)
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=BATCH)
    for k in (-1, 9):
        with pytest.raises(RuntimeError, match="top_k"):
            eng.set_denovo_carriers(k)
    with pytest.raises(RuntimeError, match="off"):
        eng.denovo_carriers()
    eng.set_denovo_carriers(2)   # without want_all: the full matrix is refused by the library
    top = np.zeros((BATCH, 2), DT)
    full = np.zeros((BATCH, eng.n_person), DT)
    rc = eng.lib.pm_engine_denovo_carriers(eng.h, top.ctypes.data, full.ctypes.data)
    assert rc == -1 and b"want_all" in eng.lib.pm_last_error()
    sl = slice(0, BATCH)
    eng.submit(D["pl"][sl], D["dm"][sl], D["ref"][sl])
    with pytest.raises(RuntimeError, match="not been collected"):
        eng.set_denovo_carriers(3)
    eng.collect()
    n = pm.engine.i32(0)
    eng.set_denovo_carriers(0)
    assert eng.lib.pm_engine_denovo_rows(eng.h, n) == 0 and n.value == 0
    eng.close()
    for kw, msg in ((dict(denovo=0), "denovo"), (dict(vcf_mode=1), "vcf_mode")):
        eng = pm.Engine(D["ped"].view, pm.Params.defaults(**kw), max_batch=BATCH)
        with pytest.raises(RuntimeError, match=msg):
            eng.set_denovo_carriers(2)
        eng.close()
    big = pm.Engine(D["ped"].view, D["par"], max_batch=1 << 26)   # 2^26 x 9 persons x 16 B > 1 GiB
    with pytest.raises(RuntimeError, match="1 GiB"):
        big.set_denovo_carriers(2, True)
    big.close()


def test_rows_are_reported_with_either_feature(built, tmp_path_factory):
    """pm_engine_denovo_rows reports the row count with carriers alone on."""
    D = dataset("trio3", tmp_path_factory)
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=len(D["ref"]))
    eng.begin_section(D["chrom"])
    eng.set_denovo_carriers(1)
    res, calls = eng.run(D["pl"], D["dm"], D["ref"])
    n = pm.engine.i32(0)
    assert eng.lib.pm_engine_denovo_rows(eng.h, n) == 0 and n.value == len(calls) > 0
    eng.close()


TAGS = re.compile(r";DNC=([^;\t]+);DNCP=([^;\t]+);DNCE=([^;\t]+)")
FAM_TAGS = re.compile(r";DNF=([^;\t]+);DNFLR=([^;\t]+)")
CLI_ARGS = ["-p", "test.ped", "-d", "test.dat", "-g", "test.gif", "--denovo", "--rate_denovo", "1.5e-07",
            "--denovo_carriers", "2"]


def _check_cli_output(text, families=False):
    lines = text.splitlines()
    head = [l for l in lines if l.startswith("##INFO=<ID=DN")]
    want = (["##INFO=<ID=DNF", "##INFO=<ID=DNFLR"] if families else []) + ["##INFO=<ID=DNC", "##INFO=<ID=DNCP", "##INFO=<ID=DNCE"]
    assert [h.split(",")[0] for h in head] == want
    dq = [i for i, l in enumerate(lines) if l.startswith("##INFO=<ID=DQ")][0]
    assert lines[dq + 1: dq + 1 + len(want)] == head
    body = [l for l in lines if not l.startswith("##")]
    golden = [l for l in open(os.path.join(EXAMPLE, "test.denovo.out.vcf")).read().splitlines() if not l.startswith("##")]
    assert [FAM_TAGS.sub("", TAGS.sub("", l)) for l in body] == golden
    recs = [l for l in body if not l.startswith("#")]
    assert recs
    if families:   # DNC comes after DNFLR
        assert all(re.search(r";DNFLR=[^;\t]+(;DNC=|\t)", l) for l in recs)
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    cwd = os.getcwd()
    os.chdir(EXAMPLE)
    try:
        rd = pm.GlfReader(ped, "test.gif")
        secs = [rd.read(maxpos + 16) for label, maxpos in rd.sections()]
        (pos, ref, pl, dm), = secs
    finally:
        os.chdir(cwd)
    pid = ped.pids()
    eng = pm.Engine(ped.view, pm.Params.defaults(denovo=1, denovo_mut_rate=1.5e-07), max_batch=len(ref))
    eng.set_denovo_carriers(2)
    res, calls = eng.run(pl, dm, ref)
    top, _ = eng.denovo_carriers()
    eng.close()
    by_pos = {int(pos[i]): top[res["call_row"][i]] for i in np.nonzero(res["call_row"] >= 0)[0]}
    assert len(by_pos) == len(recs)
    tagged = 0
    for l in recs:
        m = TAGS.search(l)
        t = by_pos[int(l.split("\t")[1])]
        t = t[t["person"] >= 0]
        if len(t) == 0:
            assert m is None
            continue
        tagged += 1
        assert m.group(1).split(",") == [pid[p] for p in t["person"]], l[:200]
        assert m.group(2).split(",") == ["%.4g" % v for v in t["pp"]], l[:200]
        assert m.group(3).split(",") == ["%sx%s>%s" % (GENO[e["fa_g"]], GENO[e["mo_g"]], GENO[e["kid_g"]]) for e in t], l[:200]
    assert tagged >= 1


def test_cli_tags(built, tmp_path):
    """8. --denovo_carriers 2 on the example: the golden records plus the tags, which name the engine's persons."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + CLI_ARGS + ["--out_vcf", str(out)], cwd=EXAMPLE, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _check_cli_output(out.read_text())


def test_cli_tags_after_the_family_tags(built, tmp_path):
    """8. with --denovo_families too, the header lines and the tags follow DNFLR's."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + CLI_ARGS + ["--denovo_families", "2", "--out_vcf", str(out)], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _check_cli_output(out.read_text(), families=True)


@pytest.mark.parametrize("protocol", ["direct", "shard"])
def test_cli_tags_through_launcher(built, tmp_path, protocol):
    """8. the same through polymutt_amd.launch at world size 1 (the flag travels in argv): the one-process path, and
    the shard protocol over one rank."""
    from test_cpu_host import _free_port
    out = tmp_path / "out.vcf"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "polymutt_amd.launch"]
    if protocol == "shard":
        env["PM_COLLECTIVE"] = "gloo"
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "1", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), "-m", "polymutt_amd.launch"]
    r = subprocess.run(cmd + CLI_ARGS + ["--out_vcf", str(out)], cwd=EXAMPLE, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _check_cli_output(out.read_text())
