"""GPU tests of the per-family de novo evidence (pm_engine_set_denovo_families / pm_engine_denovo_families, the
k_fam_dnlr kernel, and the CLI's --denovo_families tags).

A de novo record's DQ (pm_site_result.denovo_lr) is a sum over families of D_f = log10 L_f under the mutation model
minus log10 L_f under the plain one (the plain PL sum on monomorphic rows).  The oracle side of every check runs on
the CPU: the unchanged oracle's objective (minus the sum of the families' log10 likelihoods) is differenced with one
family's PL rows set to 0, which removes exactly that family's term.

Datasets: the synthetic "+dn" shapes of tests/golden/synth/cases.json with each case's flags plus all_sites = 1 and
denovo_min_llr = 1e-300, so that every site with positive de novo evidence is a written row.  Sizes cross the kernel's
edges: 1 family (the lone-nuclear prior), 3, 31 mixed trios / quads / founders, 70 (two waves of families, not a
multiple of 64) and 130 quads (three waves), peeled families; 64-site batches, so several batches run and some have
no row at all.  Seeds and site counts were chosen with Oracle.run so that every case has at least 8 rows, monomorphic
and polymorphic ones.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE, ROOT
from fixtures import LLK_RTOL, params_and_chrom, read_dataset
from oracle_binding import Oracle

pytestmark = pytest.mark.gpu

BATCH = 64
DN6 = ["--denovo", "--rate_denovo", "1e-6"]
DN5 = ["--denovo", "--rate_denovo", "1e-5"]
# name: (shape, families, sites, seed, flags of the shape's case in cases.json [+ the chromosome class])
CASES = {
    "quad1": ("quad+dn", 1, 400, 18, DN6),
    "trio3": ("trio+dn", 3, 400, 2, DN5),
    "mixed31": ("mixed+dn", 31, 300, 3, DN5),
    "quad70": ("quad+dn", 70, 300, 3, DN6),
    "quad130": ("quad+dn", 130, 300, 3, DN6),
    "ext10x3": ("ext10+dn", 3, 300, 3, DN6),
    "extmix10": ("extmix+dn", 10, 300, 3, DN6),
    "mixed31_chrX": ("mixed+dn", 31, 300, 1, DN5 + ["--chrX", "1"]),
}

_data, _runs = {}, {}


def dataset(name, tmp_path_factory):
    if name not in _data:
        shape, nfam, sites, seed, flags = CASES[name]
        d = str(tmp_path_factory.mktemp(name))
        pm.synth_write_dataset(d, shape, nfam, sites, seed)
        ped, secs, _ = read_dataset(d)
        (label, pos, ref, pl, dm), = secs
        par, chrom = params_and_chrom(flags, all_sites=1, denovo_min_llr=1e-300)
        _data[name] = dict(ped=ped, ref=ref, pl=pl, dm=dm, par=par, chrom=chrom)
    return _data[name]


def engine_batches(D, top_k, want_all=True, how="run", batch=BATCH, pl=None):
    """The dataset through an engine in batches: per batch (first site, results, calls, top, sum, all)."""
    pl = D["pl"] if pl is None else pl
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=batch)
    eng.begin_section(D["chrom"])
    if top_k:
        eng.set_denovo_families(top_k, want_all)
    out = []
    for s in range(0, len(D["ref"]), batch):
        sl = slice(s, s + batch)
        if how == "run":
            res, calls = eng.run(pl[sl], D["dm"][sl], D["ref"][sl])
        else:
            eng.submit(pl[sl], D["dm"][sl], D["ref"][sl])
            res, calls = eng.collect()
        fam = eng.denovo_families() if top_k else (None, None, None)
        if top_k:
            assert len(fam[0]) == len(fam[1]) == len(calls) == int((res["call_row"] >= 0).sum())
        out.append((s, res, calls) + tuple(fam))
    eng.close()
    return out


def shared_run(name, tmp_path_factory):
    """One engine pass per case (top_k = 8, the full matrix), shared by the tests that read it."""
    if name not in _runs:
        _runs[name] = engine_batches(dataset(name, tmp_path_factory), 8)
    return _runs[name]


def check_rows(batches):
    rows = np.concatenate([r[r["call_row"] >= 0] for _, r, *_ in batches])
    assert len(rows) >= 8 and (rows["maxidx"] == 0).any() and (rows["maxidx"] >= 1).any(), \
        (len(rows), int((rows["maxidx"] == 0).sum()))
    return rows


def assert_blank_identity(ora, n_person):
    """The differencing rests on this: a family whose PL rows are all 0 contributes log10(1) = 0."""
    blank = np.zeros((n_person, 10), np.uint8)
    for dn in (0, 1):
        for x in (0.3, 0.9999) + ((1.0,) if dn else ()):
            v = ora.objective(blank, 1, 3, x, dn)
            assert abs(v) <= 1e-12, (dn, x, v)


def oracle_family_terms(ora, fam_start, pl_site, ref, r, n_fam):
    """(D_f, |llk_f^dn| + |llk_f^std|) per family from the oracle's objective at the engine's reported minimisers."""
    mono = r["maxidx"] == 0
    if mono:
        a1, a2, x_dn, x_std = int(ref), (3 if ref == 4 else int(ref) + 1), 1.0, None
    else:
        a1, a2, x_dn = int(r["allele1"]), int(r["allele2"]), float(r["varfreq"][r["maxidx"]])
        x_std = float(r["af"]) if n_fam > 1 else 0.5   # (a lone nuclear family's prior does not depend on it)
    href = (ref - 1) * (10 - ref) // 2   # glfHandler genotype index of (ref, ref)
    full_dn = ora.objective(pl_site, a1, a2, x_dn, 1)
    full_std = None if mono else ora.objective(pl_site, a1, a2, x_std, 0)
    D, mag = np.zeros(n_fam), np.zeros(n_fam)
    for f in range(n_fam):
        cut = pl_site.copy()
        cut[fam_start[f]:fam_start[f + 1]] = 0
        l_dn = -(full_dn - ora.objective(cut, a1, a2, x_dn, 1))
        if mono:
            l_std = float(np.sum(-pl_site[fam_start[f]:fam_start[f + 1], href].astype(np.float64) / 10))
        else:
            l_std = -(full_std - ora.objective(cut, a1, a2, x_std, 0))
        D[f], mag[f] = l_dn - l_std, abs(l_dn) + abs(l_std)
    return D, mag


@pytest.mark.parametrize("name", list(CASES))
def test_family_terms_match_oracle(built, tmp_path_factory, name):
    """1. every family of every row against the oracle, to LLK_RTOL of the two family log-likelihoods differenced."""
    D = dataset(name, tmp_path_factory)
    batches = shared_run(name, tmp_path_factory)
    check_rows(batches)
    ped = D["ped"]
    ora = Oracle(ped.view, D["par"])
    ora.begin_section(D["chrom"])
    assert_blank_identity(ora, ped.n_person)
    fs = ped.fam_start()
    worst = 0.0
    for s, res, calls, top, tot, full in batches:
        for i in np.nonzero(res["call_row"] >= 0)[0]:
            row = res["call_row"][i]
            exp, mag = oracle_family_terms(ora, fs, D["pl"][s + i], int(D["ref"][s + i]), res[i], ped.n_fam)
            err = np.abs(full[row] - exp)
            bound = LLK_RTOL * mag + 1e-10
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (name, s + i, int(np.argmax(err / bound)), float(err.max()))
    print(f"{name}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("name", list(CASES))
def test_sum_is_the_record_dq(built, tmp_path_factory, name):
    """2. sum = Sum_f D_f = the record's denovo_lr (itself pinned to the reference dumps elsewhere)."""
    batches = shared_run(name, tmp_path_factory)
    zero_row_batches = 0
    for s, res, calls, top, tot, full in batches:
        em = res[res["call_row"] >= 0]
        zero_row_batches += len(em) == 0
        assert (em["call_row"] == np.arange(len(em))).all()
        bound = LLK_RTOL * (np.abs(em["varllk"][np.arange(len(em)), em["maxidx"]]) + np.abs(em["denovo_lr"]))
        assert (np.abs(tot - em["denovo_lr"]) <= bound).all(), (name, s)
        assert (np.abs(tot - full.sum(axis=1)) <= bound).all(), (name, s)
        if full.shape[1] == 1:
            assert (np.abs(full[:, 0] - em["denovo_lr"]) <= bound).all(), (name, s)
    if name in ("quad1", "trio3"):   # (chosen so: batches without any row run the kernel's empty case)
        assert zero_row_batches >= 1


def expected_top(full, k):
    order = np.argsort(-full, axis=1, kind="stable")[:, :k]   # descending, ties by lower family index
    fam = np.full((len(full), k), -1, np.int32)
    lr = np.zeros((len(full), k))
    n = order.shape[1]
    fam[:, :n] = order
    lr[:, :n] = np.take_along_axis(full, order, axis=1)
    return fam, lr


@pytest.mark.parametrize("name", ["quad1", "trio3", "mixed31", "quad70", "quad130", "extmix10"])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_ranking(built, tmp_path_factory, name, k):
    """3. top = the stable descending argsort of the full matrix; entries past n_fam are {-1, 0}."""
    D = dataset(name, tmp_path_factory)
    nrows = 0
    for s, res, calls, top, tot, full in engine_batches(D, k):
        fam, lr = expected_top(full, k)
        assert np.array_equal(top["fam"], fam), (name, s)
        assert top["lr"].tobytes() == lr.tobytes() and not top["pad"].any()
        nrows += len(full)
    assert nrows >= 8


def test_ranking_ties(built, tmp_path_factory):
    """3. families without data (all PL 0) have bit-equal terms: the ranking breaks the ties by family index."""
    D = dataset("quad70", tmp_path_factory)
    fs = D["ped"].fam_start()
    pl = D["pl"].copy()
    for f in range(70):
        if f % 9:   # data only in families 0, 9, ..., 63
            pl[:, fs[f]:fs[f + 1]] = 0
    tied = rows = 0
    for s, res, calls, top, tot, full in engine_batches(D, 8, pl=pl):
        fam, lr = expected_top(full, 8)
        assert np.array_equal(top["fam"], fam) and top["lr"].tobytes() == lr.tobytes(), s
        rows += len(full)
        tied += int((lr[:, 1:] == lr[:, :-1]).any(axis=1).sum())
    assert rows >= 1 and tied >= 1, (rows, tied)


def _phred(geno, ref=1, alt=3):
    """A person's 10 PL bytes for a confident call of 'RR', 'RA' or 'AA' (ref A, alt G: genotype indices 0, 2, 7)."""
    gi = lambda a, b: (a - 1) * (10 - a) // 2 + (b - a)
    rr, ra, aa = gi(ref, ref), gi(min(ref, alt), max(ref, alt)), gi(alt, alt)
    pl = np.full(10, 255, np.uint8)   # genotypes one allele away from a homozygous call get 60, the rest 255
    if geno == "RR":
        pl[rr], pl[ra], pl[aa] = 0, 60, 255
        pl[[1, 3]] = 60   # A/C, A/T
    elif geno == "RA":
        pl[rr], pl[ra], pl[aa] = 90, 0, 90
    else:
        pl[rr], pl[ra], pl[aa] = 255, 60, 0
        pl[[5, 8]] = 60   # C/G, G/T
    return pl


def test_planted_carrier_ranks_first(built):
    """4. twelve quads (father, mother, two kids); a het kid of hom-ref parents is planted in one family: on a
    monomorphic site (family 3) and on a site where the alternative allele also segregates in other families
    (family 7).  The planted family is top[0] in both."""
    import bench
    ped = bench.quad_pedigree(pm, 12, 2)
    npers = ped.n_person
    assert npers == 48
    sites = np.zeros((2, npers, 10), np.uint8)
    sites[:, :] = _phred("RR")
    sites[0, 3 * 4 + 2] = _phred("RA")             # family 3, first kid
    for f in (1, 4, 9):                            # inherited hets: the father and one kid
        sites[1, f * 4] = _phred("RA")
        sites[1, f * 4 + 3] = _phred("RA")
    sites[1, 7 * 4 + 2] = _phred("RA")             # family 7, first kid, parents hom-ref
    dm = np.full((2, npers), 20 | (60 << 24), np.uint32)
    ref = np.array([1, 1], np.uint8)
    par = pm.Params.defaults(denovo=1, denovo_mut_rate=1.5e-7, all_sites=1, denovo_min_llr=1e-300)
    eng = pm.Engine(ped, par, max_batch=2)
    eng.set_denovo_families(4, True)
    res, calls = eng.run(sites, dm, ref)
    top, tot, full = eng.denovo_families()
    eng.close()
    assert len(calls) == 2 and res["maxidx"][0] == 0 and res["maxidx"][1] >= 1, res[["maxidx", "emit", "denovo_lr"]]
    assert top["fam"][0, 0] == 3 and top["fam"][1, 0] == 7, top
    assert top["lr"][0, 0] > 1.0 and top["lr"][1, 0] > 5 * np.abs(np.delete(full[1], 7)).max()
    assert np.abs(np.delete(full[0], 3)).max() < 1e-3   # no evidence anywhere else on the monomorphic site


def test_paths_agree_bit_for_bit(built, tmp_path_factory):
    """5. run, submit / collect and run_device + sync give identical bits, and so do two runs."""
    D = dataset("quad130", tmp_path_factory)
    a = shared_run("quad130", tmp_path_factory)
    b = engine_batches(D, 8, how="run")
    c = engine_batches(D, 8, how="submit")
    for x, y, z in zip(a, b, c):
        for j in (3, 4, 5):
            assert x[j].tobytes() == y[j].tobytes() == z[j].tobytes(), (x[0], j)
    # device-resident: the first batch's sites in the planar layout
    ped, n = D["ped"], BATCH
    npers = ped.n_person
    eng = pm.Engine(ped.view, D["par"], max_batch=n)
    eng.begin_section(D["chrom"])
    eng.set_denovo_families(8, True)
    d_pl, d_dm, d_ref = eng.alloc(n * npers * 10), eng.alloc(n * npers * 4), eng.alloc(n)
    eng.to_device(d_pl, pm.planar(D["pl"][:n]), n * npers * 10)
    eng.to_device(d_dm, D["dm"][:n], n * npers * 4)
    eng.to_device(d_ref, D["ref"][:n], n)
    eng.run_device(n, d_pl, d_dm, d_ref, None, None)
    eng.sync()
    top, tot, full = eng.denovo_families()
    for p in (d_pl, d_dm, d_ref):
        eng.free(p)
    eng.close()
    assert len(top) == len(a[0][3]) > 0
    assert top.tobytes() == a[0][3].tobytes() and tot.tobytes() == a[0][4].tobytes() and full.tobytes() == a[0][5].tobytes()


@pytest.mark.parametrize("name", ["quad130", "extmix10"])
def test_results_do_not_depend_on_the_feature(built, tmp_path_factory, name):
    """6. results and genotype rows are byte-identical with the feature off, on, and on without the full matrix."""
    D = dataset(name, tmp_path_factory)
    on = shared_run(name, tmp_path_factory)
    off = engine_batches(D, 0)
    lean = engine_batches(D, 2, want_all=False)
    for x, y, z in zip(on, off, lean):
        assert x[1].tobytes() == y[1].tobytes() == z[1].tobytes() and x[2].tobytes() == y[2].tobytes() == z[2].tobytes()
        assert z[5] is None and z[3].tobytes() == np.ascontiguousarray(x[3][:, :2]).tobytes() and z[4].tobytes() == x[4].tobytes()


def test_rows_before_a_stuck_site(built, tmp_path_factory, monkeypatch):
    """After PM_EBRENT (ITMAX lowered with PM_TEST_ITMAX) the rows of the sites before the stuck one are handed out,
    as the genotype rows are, with the values of the undisturbed run."""
    from test_brent_stuck import first_stuck
    D = dataset("quad70", tmp_path_factory)
    full = shared_run("quad70", tmp_path_factory)
    s, res, calls, top, tot, allm = max(full, key=lambda b: len(b[3]))
    ev = res["evals"]
    loop = np.where(ev >= 3, ev - 3, -1).max(axis=1)
    before = lambda k: int((res["call_row"][:first_stuck(res, k)] >= 0).sum())
    k = max(sorted(set(int(x) for x in loop if x > 0)), key=before)   # the ITMAX that leaves the most rows complete
    assert before(k) >= 1
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=BATCH)
    eng.begin_section(D["chrom"])
    eng.set_denovo_families(8, True)
    with pytest.raises(pm.engine.BrentStuck) as e:
        eng.run(D["pl"][s:s + BATCH], D["dm"][s:s + BATCH], D["ref"][s:s + BATCH])
    top2, tot2, all2 = eng.denovo_families()
    eng.close()
    n = int((res["call_row"][:e.value.site] >= 0).sum())
    assert 1 <= n == len(e.value.calls) == len(top2) < len(top)
    assert top2.tobytes() == top[:n].tobytes() and tot2.tobytes() == tot[:n].tobytes() and all2.tobytes() == allm[:n].tobytes()


def test_api_argument_errors(built, tmp_path_factory):
    D = dataset("trio3", tmp_path_factory)
    eng = pm.Engine(D["ped"].view, D["par"], max_batch=BATCH)
    for k in (-1, 9):
        with pytest.raises(RuntimeError, match="top_k"):
            eng.set_denovo_families(k)
    with pytest.raises(RuntimeError, match="off"):
        eng.denovo_families()
    eng.close()
    for kw, msg in ((dict(denovo=0), "denovo"), (dict(vcf_mode=1), "vcf_mode")):
        eng = pm.Engine(D["ped"].view, pm.Params.defaults(**kw), max_batch=BATCH)
        with pytest.raises(RuntimeError, match=msg):
            eng.set_denovo_families(2)
        eng.close()
    big = pm.Engine(D["ped"].view, D["par"], max_batch=1 << 26)   # 2^26 x 3 families x 8 B > 1 GiB
    with pytest.raises(RuntimeError, match="1 GiB"):
        big.set_denovo_families(2, True)
    big.close()


TAGS = re.compile(r";DNF=([^;\t]+);DNFLR=([^;\t]+)")
CLI_ARGS = ["-p", "test.ped", "-d", "test.dat", "-g", "test.gif", "--denovo", "--rate_denovo", "1.5e-07",
            "--denovo_families", "2"]


def _check_cli_output(text):
    lines = text.splitlines()
    head = [l for l in lines if l.startswith("##INFO=<ID=DN")]
    assert [h.split(",")[0] for h in head] == ["##INFO=<ID=DNF", "##INFO=<ID=DNFLR"]
    dq = [i for i, l in enumerate(lines) if l.startswith("##INFO=<ID=DQ")][0]
    assert lines[dq + 1: dq + 3] == head
    body = [l for l in lines if not l.startswith("##")]
    golden = [l for l in open(os.path.join(EXAMPLE, "test.denovo.out.vcf")).read().splitlines() if not l.startswith("##")]
    assert [TAGS.sub("", l) for l in body] == golden
    recs = [l for l in body if not l.startswith("#")]
    assert recs and all(TAGS.search(l) for l in recs)
    # the same sites through the engine
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    cwd = os.getcwd()
    os.chdir(EXAMPLE)
    try:
        rd = pm.GlfReader(ped, "test.gif")
        secs = [rd.read(maxpos + 16) for label, maxpos in rd.sections()]   # (read inside the section loop)
        (pos, ref, pl, dm), = secs
    finally:
        os.chdir(cwd)
    famid = [ped.lib.pmh_pedigree_famid(ped.h, f).decode() for f in range(ped.n_fam)]
    eng = pm.Engine(ped.view, pm.Params.defaults(denovo=1, denovo_mut_rate=1.5e-07), max_batch=len(ref))
    eng.set_denovo_families(2)
    res, calls = eng.run(pl, dm, ref)
    top, tot, _ = eng.denovo_families()
    eng.close()
    by_pos = {int(pos[i]): top[res["call_row"][i]] for i in np.nonzero(res["call_row"] >= 0)[0]}
    assert len(by_pos) == len(recs)
    for l in recs:
        m = TAGS.search(l)
        t = by_pos[int(l.split("\t")[1])]
        assert m.group(1).split(",") == [famid[f] for f in t["fam"]], l[:200]
        assert m.group(2).split(",") == ["%.3f" % v for v in t["lr"]], l[:200]


def test_cli_tags(built, tmp_path):
    """7. --denovo_families 2 on the example: the golden records plus the tags, which name the engine's families."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + CLI_ARGS + ["--out_vcf", str(out)], cwd=EXAMPLE, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _check_cli_output(out.read_text())


@pytest.mark.parametrize("protocol", ["direct", "shard"])
def test_cli_tags_through_launcher(built, tmp_path, protocol):
    """7. the same through polymutt_amd.launch at world size 1 (the flag travels in argv): the one-process path, and
    the shard protocol over one rank (the records go through a part file and the merge)."""
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
