"""GPU tests of the genotype posterior plane of the --in_vcf path (pm_engine_set_vcf_posteriors / pm_engine_vcf_posteriors,
--vcf_posteriors).

* GP against the numpy reference of tests/vcf_posterior_reference.py (the definition, without peeling; validated against
  the CPU oracle by tests/test_cpu_vcf_posteriors.py) at the engine's own frequency, on multi-family autosomal pedigrees.
* DS = p[1] + 2 p[2] against the unchanged CPU oracle's dosage on every chromosome class, single families included: this
  pins the single-family prior mode and the chrX / chrY rules.
* The plane is additive: site results, genotype rows and the de novo outputs are the same bytes with it on, through every
  entry point; the schedule compiler does not change it; a stuck Brent keeps the rows the batch returned.
* The CLI prints DS and GP and nothing else moves.

The float tolerance is derived, not measured: one rounding of a value in [0, 1] to float moves it by at most 2^-25 (half
an ulp of the largest binade), on top of the project's DOSE_ATOL = 1e-9 for double-against-double arithmetic.  DS adds one
value and twice another: 3 x 2^-25.

Every engine case runs 96 sites at max_batch = 64, so the second batch is partial.
"""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from oracle_binding import Oracle
from parity import DOSE_ATOL, _nonfinite_problem
from test_brent_stuck import first_stuck, pick_itmax
import vcf_plane_common as common
from vcf_posterior_reference import Families, three

pytestmark = pytest.mark.gpu

GP_ATOL = 2.0 ** -25 + DOSE_ATOL
DS_ATOL = 3 * 2.0 ** -25 + DOSE_ATOL
BATCH, NSITES = 64, 96
MALE, FEMALE = 1, 2
LBL_DOT = 4   # pm_label_kind PM_LBL_DOT

# multi-family autosomal pedigrees, the smallest at which each kernel can still go wrong: two family sizes in one wave,
# more than 64 families (a lane takes a second family), the founder branch, peeled families alone, one family of each of
# the five peel schedules
GP_CASES = [("mixed", 31), ("quad", 70), ("single", 12), ("ext10", 3), ("extmix", 5)]
# test_engine_vcf_mode_matches_oracle's shapes plus a lone peeled family
DS_CASES = [("quad", 40), ("mixed", 31), ("single", 12), ("ext10", 8), ("roof", 8), ("quad", 1), ("ext10", 1)]

PEEL_CASES = [("ext10", 3, 96, 64), ("extmix", 5, 16, 12)]   # (shape, families, sites, max_batch)


def dataset(tmp_path_factory, shape, nfam, nsites=NSITES):
    """(ped, block, refalt), generated once per case and left unchanged."""
    ped, _, block, refalt = common.dataset(tmp_path_factory, "vp", shape, nfam, nsites)
    return ped, block, refalt


def run_batches(eng, block, refalt, entry="run", posteriors=True, batch=BATCH):
    """Every batch through one entry point: (results, calls as (best, gq, label) int arrays, plane or None)."""
    def fetch(c):
        p = eng.vcf_posteriors()
        assert p.shape == (len(c), eng.n_person, 3) and p.dtype == np.float32
        return p
    res, calls, post = common.run_batches(eng, block, refalt, batch, entry, fetch if posteriors else lambda c: None)
    return res, calls, (np.concatenate(post) if posteriors else None)


def check_plane(post, calls, label):
    """What holds for every plane: finite values in [0, 1], rows summing to 1 (or all zero), argmax = the row's best."""
    assert np.isfinite(post).all(), label
    assert (post >= 0).all() and (post <= 1).all(), label
    s = post.astype(np.float64).sum(axis=-1)
    zero = (post == 0).all(axis=-1)
    assert (np.abs(s - 1)[~zero] <= 3 * 2.0 ** -25).all(), (label, np.abs(s - 1)[~zero].max())
    top = np.sort(post.astype(np.float64), axis=-1)
    clear = (top[..., 2] - top[..., 1] > 1e-6) & ~zero
    assert clear.any(), label
    assert np.array_equal(post.argmax(axis=-1)[clear], calls[..., 0][clear].astype(np.int64)), label


def compare_gp(post, ref, label):
    problems = []
    _nonfinite_problem(label + " GP", post.astype(np.float64), ref, problems)
    assert not problems, problems
    d = np.abs(post.astype(np.float64) - ref)
    print(f"{label}: max |GP - reference| = {d.max():.3g} (bound {GP_ATOL:.3g})")
    assert (d <= GP_ATOL).all(), (label, d.max(), np.argwhere(d > GP_ATOL)[:5])


@pytest.mark.parametrize("numerics", [pm.NUM_POLY, pm.NUM_EXACT])
@pytest.mark.parametrize("shape,nfam", GP_CASES)
def test_gp_matches_reference(built, tmp_path_factory, shape, nfam, numerics):
    ped, block, refalt = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1, numerics=numerics), max_batch=BATCH)
    eng.set_vcf_posteriors(True)
    res, calls, post = run_batches(eng, block, refalt)
    eng.close()
    assert (res["call_row"] >= 0).all() and len(post) == len(refalt)   # every site of these blocks is written
    ref = Families(ped.view).posteriors(block, refalt, res["af"])
    compare_gp(post, ref, f"{shape} {nfam} numerics {numerics}")   # every row, every person
    check_plane(post, calls, f"{shape} {nfam}")


def test_gp_large_nuclear_families(built):
    """Nuclear families of three and four children next to a trio and a quad: the closed form over any number of
    children (k_vcf_post_nuc's nuclear branch, which no synthetic shape reaches) against the numpy reference."""
    sizes = [5, 3, 6, 4, 5]
    sex, founder, father, mother = [], [], [], []
    p0 = 0
    for m in sizes:
        for j in range(m):
            sex.append(MALE if j == 0 else FEMALE if j == 1 else 1 + (j % 2))
            founder.append(1 if j < 2 else 0)
            father.append(-1 if j < 2 else p0)
            mother.append(-1 if j < 2 else p0 + 1)
        p0 += m
    ped = pm.pedigree_from_arrays(sizes, [2] * len(sizes), [pm.FAM_NUCLEAR] * len(sizes), sex, founder, father, mother)
    rng = np.random.default_rng(11)
    n, npers = NSITES, sum(sizes)
    ref_base = rng.integers(1, 5, n).astype(np.uint8)
    refalt = (ref_base | (np.array([{1: 3, 2: 4, 3: 1, 4: 2}[int(r)] for r in ref_base], np.uint8) << 4)).astype(np.uint8)
    block = np.full((n, npers, 10), 255, np.uint8)
    fams = Families(ped)
    for i in range(n):
        # genotypes drawn down the pedigree at a site frequency, PLs that favour them by a random margin
        f = rng.choice([0.95, 0.7, 0.5])
        gt = np.zeros(npers, np.int64)
        q0 = 0
        for m in sizes:
            gt[q0:q0 + 2] = rng.binomial(2, 1 - f, 2)
            for j in range(2, m):
                gt[q0 + j] = rng.binomial(1, gt[q0] / 2) + rng.binomial(1, gt[q0 + 1] / 2)
            q0 += m
        tri = rng.integers(5, 80, (npers, 3))
        tri[np.arange(npers), gt] = 0
        block[i][:, three(refalt[i])] = tri.astype(np.uint8)
    for numerics in (pm.NUM_POLY, pm.NUM_EXACT):
        eng = pm.Engine(ped, pm.Params.defaults(vcf_mode=1, numerics=numerics), max_batch=BATCH)
        eng.set_vcf_posteriors(True)
        res, calls, post = run_batches(eng, block, refalt)
        eng.close()
        assert (res["call_row"] >= 0).all()
        compare_gp(post, fams.posteriors(block, refalt, res["af"]), f"nuclear 5/3/6/4/5 numerics {numerics}")
        check_plane(post, calls, "nuclear 5/3/6/4/5")


@pytest.mark.parametrize("chrom", [pm.PM_CHR_AUTO, pm.PM_CHR_X, pm.PM_CHR_Y, pm.PM_CHR_MT])
@pytest.mark.parametrize("shape,nfam", DS_CASES)
def test_ds_matches_oracle(built, tmp_path_factory, shape, nfam, chrom):
    """DS against the unchanged oracle under NUM_EXACT (the engine and the oracle take the same evaluation path there), on
    the rows whose af agrees with the oracle's to 1e-12 -- a condition, not a measurement: at most 5% of a case's rows may
    fall outside it."""
    ped, block, refalt = dataset(tmp_path_factory, shape, nfam)
    par = pm.Params.defaults(vcf_mode=1, numerics=pm.NUM_EXACT)
    eng = pm.Engine(ped.view, par, max_batch=BATCH)
    eng.set_vcf_posteriors(True)
    eng.begin_section(chrom)
    res, calls, post = run_batches(eng, block, refalt)
    eng.close()
    ora = Oracle(ped.view, par)
    ora.begin_section(chrom)
    ores, ocalls = ora.run(block, np.zeros(block.shape[:2], np.uint32), refalt)
    rows = res["call_row"] >= 0   # (the engine numbers a batch's rows, the oracle the run's: the same sites, in order)
    assert np.array_equal(rows, ores["call_row"] >= 0) and len(post) == len(ocalls) == rows.sum()
    gate = np.abs(res["af"][rows] - ores["af"][rows]) <= 1e-12
    share = 1 - gate.mean()
    print(f"{shape} {nfam} chrom {chrom}: {share:.2%} of the rows outside the af gate")
    assert share <= 0.05, share
    p = post.astype(np.float64)
    ds = p[..., 1] + 2 * p[..., 2]
    problems = []
    _nonfinite_problem("DS", ds, ocalls["dosage"], problems)
    assert not problems, problems
    d = np.abs(ds - ocalls["dosage"])[gate]
    print(f"{shape} {nfam} chrom {chrom}: max |DS - oracle| = {d.max():.3g} (bound {DS_ATOL:.3g})")
    assert (d <= DS_ATOL).all(), (d.max(), np.argwhere(d > DS_ATOL)[:5])
    check_plane(post, calls, f"{shape} {nfam} chrom {chrom}")
    sex = np.ctypeslib.as_array(ped.view.sex, shape=(ped.n_person,))
    if chrom == pm.PM_CHR_X:
        assert (post[:, sex == MALE, 1] == 0).all()
    if chrom == pm.PM_CHR_MT:
        assert (post[..., 1] == 0).all()
    if chrom == pm.PM_CHR_Y:
        assert (post[:, sex == FEMALE] == 0).all() and (post[:, sex == MALE, 1] == 0).all()
        assert (calls[:, sex == FEMALE, 2] == LBL_DOT).all()


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("single", 12), ("extmix", 5)])   # lean, generic, peeled
def test_feature_off_identity_and_entry_points(built, tmp_path_factory, shape, nfam):
    ped, block, refalt = dataset(tmp_path_factory, shape, nfam)
    par = pm.Params.defaults(vcf_mode=1)
    plain = pm.Engine(ped.view, par, max_batch=BATCH)   # never has the feature on
    eng = pm.Engine(ped.view, par, max_batch=BATCH)
    eng.set_vcf_posteriors(True)
    planes = []
    for entry in ("run", "run_vcf", "submit"):
        r0, c0, _ = run_batches(plain, block, refalt, entry, posteriors=False)
        r1, c1, p1 = run_batches(eng, block, refalt, entry)
        assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes(), entry
        planes.append(p1)
    assert planes[0].tobytes() == planes[1].tobytes() == planes[2].tobytes()
    eng.set_vcf_posteriors(False)   # off again: the same bytes still, and no plane
    r0, c0, _ = run_batches(plain, block, refalt, "run", posteriors=False)
    r1, c1, _ = run_batches(eng, block, refalt, "run", posteriors=False)
    assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes()
    with pytest.raises(RuntimeError, match="feature is off"):
        eng.vcf_posteriors()
    eng.set_vcf_posteriors(True)   # on again: no batch has filled the new plane
    assert eng.vcf_posteriors().shape == (0, ped.n_person, 3)
    plain.close()
    eng.close()


def test_setter_errors_and_denovo_outputs(built, tmp_path_factory):
    ped, block, refalt = dataset(tmp_path_factory, "mixed", 31)
    glf = pm.Engine(ped.view, pm.Params.defaults(), max_batch=BATCH)
    with pytest.raises(RuntimeError, match="vcf_mode"):
        glf.set_vcf_posteriors(True)
    glf.close()
    outs = []
    zeros = np.zeros(block.shape[:2], np.uint32)
    for with_post in (False, True):
        eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)
        eng.set_vcf_denovo(True)
        eng.set_vcf_denovo_detail(2, 2)
        if with_post:
            eng.set_vcf_posteriors(True)
            eng.submit(block[:BATCH], zeros[:BATCH], refalt[:BATCH])
            lib = pm.load_library()
            assert lib.pm_engine_set_vcf_posteriors(eng.h, 0) == -1 and b"not been collected" in lib.pm_last_error()
            n = C.c_int32(0)
            assert lib.pm_engine_vcf_posteriors(eng.h, C.byref(n), None) == -1 and b"not been collected" in lib.pm_last_error()
            eng.collect()
        got = []
        for s in range(0, len(refalt), BATCH):
            sl = slice(s, s + BATCH)
            r, c = eng.run(block[sl], zeros[sl], refalt[sl])
            top_f, sum_f, _ = eng.vcf_denovo_families()
            top_c, _ = eng.vcf_denovo_carriers()
            got.append(b"".join(a.tobytes() for a in (r, c, eng.vcf_denovo_rows(), top_f, sum_f, top_c)))
            if with_post:
                assert len(eng.vcf_posteriors()) == len(c)
        if with_post:   # neither feature switches the other off
            eng.set_vcf_denovo(False)
            eng.run(block[:BATCH], zeros[:BATCH], refalt[:BATCH])
            assert len(eng.vcf_posteriors()) == BATCH
        outs.append(got)
        eng.close()
    assert outs[0] == outs[1]
    assert any((np.frombuffer(g, np.uint8) != 0).any() for g in outs[0])


def test_schedule_compiler_on_and_off(built, tmp_path_factory, monkeypatch):
    ped, block, refalt = dataset(tmp_path_factory, "ext10", 3)
    planes = []
    for no_jit in (False, True):
        if no_jit:
            monkeypatch.setenv("PM_NO_JIT", "1")
        eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)
        eng.set_vcf_posteriors(True)
        planes.append(run_batches(eng, block, refalt)[2])
        eng.close()
    assert planes[0].tobytes() == planes[1].tobytes() and (planes[0] != 0).any()


@pytest.mark.parametrize("shape,nfam,nsites,batch", PEEL_CASES)
def test_peel_workspace_in_lds_and_in_hbm(built, tmp_path_factory, monkeypatch, shape, nfam, nsites, batch):
    """k_vcf_post_es<true> and k_vcf_post_es<false> (PM_ES_POST_HBM) write the same plane: the two workspaces hold the same
    doubles in the same order.  Site results and genotype rows are the same bytes too."""
    ped, block, refalt = dataset(tmp_path_factory, shape, nfam, nsites)
    outs = []
    for hbm in (False, True):
        if hbm:
            monkeypatch.setenv("PM_ES_POST_HBM", "1")   # (read when the engine is created)
        eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_posteriors(True)
        outs.append(run_batches(eng, block, refalt, batch=batch))
        eng.close()
    (r0, c0, p0), (r1, c1, p1) = outs
    assert p0.tobytes() == p1.tobytes() and (p0 != 0).any()
    assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes()


def test_stuck_site_keeps_the_returned_rows(built, tmp_path_factory, monkeypatch):
    ped, block, refalt = dataset(tmp_path_factory, "mixed", 31)
    par = pm.Params.defaults(vcf_mode=1)
    eng = pm.Engine(ped.view, par, max_batch=BATCH)
    eng.set_vcf_posteriors(True)
    res, calls, post = run_batches(eng, block, refalt)
    eng.close()
    k, s = pick_itmax(res)
    assert first_stuck(res, k) == s
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))   # (read when the engine is created)
    eng = pm.Engine(ped.view, par, max_batch=BATCH)
    eng.set_vcf_posteriors(True)
    zeros = np.zeros(block.shape[:2], np.uint32)
    b0 = s // BATCH * BATCH
    for t in range(0, b0, BATCH):   # the batches before the stuck site's run as usual
        eng.run(block[t:t + BATCH], zeros[t:t + BATCH], refalt[t:t + BATCH])
        assert eng.vcf_posteriors().tobytes() == post[t:t + BATCH].tobytes()
    with pytest.raises(pm.engine.BrentStuck) as ei:
        eng.run(block[b0:b0 + BATCH], zeros[b0:b0 + BATCH], refalt[b0:b0 + BATCH])
    assert ei.value.site == s - b0
    got = eng.vcf_posteriors()
    assert len(got) == len(ei.value.calls) == s - b0   # the rows the batch returned: those before the stuck site
    assert got.tobytes() == post[b0:s].tobytes()
    eng.close()


_cli = common.cli


def _strip(lines):
    """The output without the two header lines and without the DS and GP sub-fields."""
    return common.strip_fields(lines, ("DS", "GP"), lambda fmt, k: k == 3)


def test_cli_prints_ds_and_gp(built, tmp_path):
    plain = _cli(tmp_path, "plain.vcf", [])
    exp = gzip.open(os.path.join(EXAMPLE, "testvcf.out.vcf.body.gz"), "rt").read().splitlines()
    assert [l for l in plain if not l.startswith("##")] == exp
    got = _cli(tmp_path, "post.vcf", ["--vcf_posteriors"])
    hdr = [l for l in got if l.startswith("##FORMAT")]
    k = next(i for i, l in enumerate(hdr) if l.startswith("##FORMAT=<ID=DP,"))
    assert hdr[k + 1] == '##FORMAT=<ID=DS,Number=1,Type=Float,Description="Dosage: Defined As the Expected Alternative Allele Count">'
    assert hdr[k + 2] == '##FORMAT=<ID=GP,Number=G,Type=Float,Description="Genotype Posterior Probabilities Given the Pedigree">'

    def same(a, b):   # (the ##Polymutt= line records the command line)
        drop = lambda ls: [l for l in ls if not l.startswith("##Polymutt=")]
        return drop(a) == drop(b)
    assert same(_strip(got), plain)
    samples = called = 0
    for l in got:
        if l.startswith("#"):
            continue
        for v in l.split("\t")[9:]:
            gt, _, _, ds, gp = v.split(":")[:5]
            if gp == ".":
                assert ds == "."
                continue
            g = [float(x) for x in gp.split(",")]
            assert len(g) == 3   # (the example's records are autosomal: diploid)
            # the print rounding of three %.3f values and one two-decimal value
            assert abs(float(ds) - (g[1] + 2 * g[2])) <= 0.0005 * 3 + 0.005 + 1e-12, v
            samples += 1
            top = sorted(g)
            if gt != "./." and top[2] != top[1]:
                assert gt == ["0/0", "0/1", "1/1"][int(np.argmax(g))], v
                called += 1
    assert samples > 1000 and called > 1000
    assert same(_cli(tmp_path, "b7.vcf", ["--vcf_posteriors", "--batch", "7"]), got)
    assert same(_cli(tmp_path, "e3.vcf", ["--vcf_posteriors", "--engines", "3", "--batch", "1000"]), got)
    dn = ["--vcf_denovo", "--vcf_denovo_families", "2", "--vcf_denovo_carriers", "2"]
    a, b = _cli(tmp_path, "dn.vcf", dn), _cli(tmp_path, "dnp.vcf", dn + ["--vcf_posteriors"])
    info = lambda ls: [l.split("\t")[7] for l in ls if not l.startswith("#")]
    assert info(a) == info(b) and any("DQ=" in x for x in info(a))
    assert same(_strip(b), a)


def test_cli_records_without_data_and_shards(built, tmp_path):
    """Records without data print the previous computed record's DS and GP, like its GT and GQ -- also when that record
    was computed by the shard before (the carried state travels in the shards' exchange): two shards on the one GPU
    write the one-process output, and a blanked record's sample fields are those of the record before it."""
    from test_cpu_host import run_sharded, vcf_body
    from vcf_edits import write_nodata_vcf
    src = str(tmp_path / "in.vcf")
    blanked = sorted(write_nodata_vcf(src, worlds=(2,)))
    args = ["-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--vcf_posteriors"]
    one = str(tmp_path / "one.vcf")
    r1 = subprocess.run([pm.BIN_PATH] + args + ["--out_vcf", one], cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    recs = {tuple(l.split("\t")[:2]): l.split("\t") for l in vcf_body(one)[1:]}   # (chromosome, position) -> record
    inp = [tuple(l.split("\t")[:2]) for l in open(src).read().splitlines() if not l.startswith("#")]
    fields = lambda c: [":".join(v.split(":")[:2] + v.split(":")[3:5]) for v in c[9:]]   # GT, GQ, DS, GP
    carried = 0
    for i in blanked:   # (records the path does not write, multi-allelic ones, are in neither)
        if i > 0 and inp[i] in recs and inp[i - 1] in recs:
            assert fields(recs[inp[i]]) == fields(recs[inp[i - 1]]), inp[i]
            carried += 1
    assert carried > 0
    sh = str(tmp_path / "sharded.vcf")
    r2 = run_sharded(EXAMPLE, args + ["--out_vcf", sh], 2)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert vcf_body(sh) == vcf_body(one)
    assert not [f for f in os.listdir(str(tmp_path)) if ".part" in f]
