"""De novo calling on chrX VCF records (pm_engine_set_vcf_denovo_chrx, --vcf_denovo_chrX): the sex-aware three-state model
against an independent numpy reference.

The CPU oracle cannot pin N here: its de novo model uses the autosomal transmission on every chromosome.  The reference
(tests/chrx_reference.py) forms each family's likelihood from the model's definition by an einsum contraction over every
member's three states -- no peeling -- takes the mutation matrix M from the oracle (pmo_geno_mut_matrix) and A4 from its
formula, reads the children that do not mutate from the pedigree's peel steps, and maximises with a restatement of
brent_core.h's state machine.  tests/test_cpu_vcf_denovo_chrx.py pins that reference against the oracle's standard chrX
objective before it judges the engine here.  D, the value subtracted in DQ = N - D, is by the specification the standard
chrX objective at the engine's varfreq[1]; the reference evaluates it there.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
import oracle_binding
from chrx_reference import Pedigree as RefPedigree, SiteModel, allele_mut_matrix, brent_max, gi, reference_values, three
from conftest import EXAMPLE
from fixtures import read_dataset
from oracle_binding import Oracle
from parity import FLAT_RTOL, FREQ_ATOL, LLK_RTOL
from polymutt_amd.engine import SITE_DTYPE
from test_gpu_vcf import _vcf_block
from test_gpu_vcf_denovo import _arrays, _masked, run_batches

pytestmark = pytest.mark.gpu

MALE = 1
PARENT_PL, DAUGHTER_PL, SON_PL = (0, 150, 255), (120, 0, 150), (150, 255, 0)
CASES = [("trio", 3, 32), ("quad", 5, 32), ("mixed", 31, 32), ("single", 12, 32), ("ext10", 1, 32), ("roof", 3, 32),
         ("extmix", 5, 32), ("roof2", 1, 8)]   # roof2: its type-3 step with a marriage partial is the :1391 quirk
# the kernel choice: up to 128 terms (peeled families + founder persons) one wave, k_vdn_brent_x<64>; above, <256>
CASES += [("trio", 128, 8), ("trio", 129, 8), ("single", 129, 8)]


def mutation_matrices(ped, par):
    """(M, A4): the 10 x 10 genotype mutation matrix from the oracle, the allele one from its formula."""
    L = oracle_binding.lib()
    L.pmo_geno_mut_matrix.restype = C.POINTER(C.c_double)
    L.pmo_geno_mut_matrix.argtypes = [C.c_void_p]
    ora = Oracle(ped.view, par)
    M = np.array([L.pmo_geno_mut_matrix(ora.h)[k] for k in range(100)])
    del ora
    return M, allele_mut_matrix(par.denovo_mut_rate, par.denovo_tstv)


def make_block_x(ped, pl, refalt, fill=255):
    """make_block of tests/test_gpu_vcf_denovo.py with sex-aware plants: on every 8th site the first family with a
    non-founder is set to PARENT_PL and one of its non-founders (rotating) to DAUGHTER_PL (heterozygous under reference
    parents) or SON_PL (hemizygous alternate under a reference mother)."""
    fs, fo = _arrays(ped)
    sex = np.ctypeslib.as_array(ped.view.sex, shape=(ped.n_person,))
    n, npers = pl.shape[0], pl.shape[1]
    fam = next((f for f in range(len(fs) - 1) if not fo[fs[f]:fs[f + 1]].all()), None)
    kids = [] if fam is None else [p for p in range(fs[fam], fs[fam + 1]) if not fo[p]]
    block = np.full((n, npers, 10), fill, np.uint8)
    planted = []
    for i in range(n):
        _, _, g = three(refalt[i])
        tri = pl[i][:, g].astype(np.int32)
        tri -= tri.min(axis=1, keepdims=True)
        if kids and i % 8 == 0:
            kid = kids[(i // 8) % len(kids)]
            tri[fs[fam]:fs[fam + 1]] = PARENT_PL
            tri[kid] = SON_PL if sex[kid] == MALE else DAUGHTER_PL
            planted.append(i)
        block[i][:, g] = tri.astype(np.uint8)
    return block, planted


_DATA = {}


def dataset(tmp_path_factory, shape, nfam, nsites=32):
    """(ped, block, refalt, planted, reference values, reference site models), built once per case.  Before any engine
    runs, the reference alone must see the plants: the largest planted DQ exceeds 3."""
    key = (shape, nfam, nsites)
    if key not in _DATA:
        d = str(tmp_path_factory.mktemp(f"vdnx_{shape}_{nfam}"))
        pm.synth_write_dataset(d, shape, nfam, nsites, 53)
        ped, secs, _ = read_dataset(d)
        (label, pos, ref, pl, dm), = secs
        refalt = _vcf_block(pl, ref, 5)
        block, planted = make_block_x(ped, pl.reshape(len(ref), ped.n_person, 10), refalt)
        par = pm.Params.defaults(vcf_mode=1)
        M, A4 = mutation_matrices(ped, par)
        rv, models = reference_values(RefPedigree(ped.view), M, A4, block, refalt, par.precision)
        if planted:
            dq = rv[planted, 0] - rv[planted, 2]
            assert dq.max() > 3, (shape, nfam, dq)
        rv.setflags(write=False)
        block.setflags(write=False)
        _DATA[key] = (ped, block, refalt, planted, rv, models)
    return _DATA[key]


def x_engine(ped, max_batch=64, **kw):
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1, **kw), max_batch=max_batch)
    eng.set_vcf_denovo(True)
    eng.set_vcf_denovo_chrx(True)
    eng.begin_section(pm.PM_CHR_X)
    return eng


def check_against_reference(res, rv, models, planted, has_kid, founders_only, label):
    """check_against_oracle's shape: N and DQ at every site, the maximiser where the objective is not flat, and the
    reference's value at the engine's own maximiser."""
    assert len(res) == len(rv)
    assert (res["status"] == 0).all(), f"{label}: every site of these blocks is called; none may drop out of the comparison"
    Ne, Nr = res["varllk"][:, 2], rv[:, 0]
    Dr = np.array([m.loglik(float(x), False) for m, x in zip(models, res["varfreq"][:, 1])])   # D at the engine's varfreq[1]
    DQe, DQr = res["denovo_lr"], Nr - Dr
    own = np.array([m.loglik(float(x), True) for m, x in zip(models, res["varfreq"][:, 2])])
    errN, errQ, errO, errD = np.abs(Ne - Nr), np.abs(DQe - DQr), np.abs(Ne - own), np.abs(res["varllk"][:, 1] - Dr)
    print(f"{label}: max |N_e - N_r| / |N_r| = {(errN / np.abs(Nr)).max():.3g}, max |DQ_e - DQ_r| = {errQ.max():.3g}, "
          f"max |N_e - ref(varfreq[2])| / |N_e| = {(errO / np.abs(Ne)).max():.3g}, "
          f"max |varllk[1] - ref_std(varfreq[1])| / |.| = {(errD / np.abs(Dr)).max():.3g}, "
          f"max planted reference DQ = {DQr[planted].max() if len(planted) else float('nan'):.3f}")
    bad = np.nonzero(errN > LLK_RTOL * np.abs(Nr))[0]
    assert not len(bad), (label, "N", int(bad[0]), Ne[bad[0]], Nr[bad[0]])
    bad = np.nonzero(errQ > LLK_RTOL * (np.abs(Nr) + np.abs(Dr)))[0]
    assert not len(bad), (label, "DQ", int(bad[0]), DQe[bad[0]], DQr[bad[0]])
    bad = np.nonzero(errO > LLK_RTOL * np.abs(own))[0]
    assert not len(bad), (label, "N at the engine's own maximiser", int(bad[0]), Ne[bad[0]], own[bad[0]])
    bad = np.nonzero(errD > LLK_RTOL * np.abs(Dr))[0]   # (the reference's standard objective is the engine's)
    assert not len(bad), (label, "varllk[1]", int(bad[0]), res["varllk"][bad[0], 1], Dr[bad[0]])
    flat = errN / np.maximum(np.abs(Nr), 1e-300) <= FLAT_RTOL   # parity.py's rule for a flat objective
    div = np.abs(res["varfreq"][:, 2] - rv[:, 1]) > FREQ_ATOL
    assert not (div & ~flat).any(), (label, "varfreq[2]", int(np.nonzero(div & ~flat)[0][0]))
    assert (res["evals"][:, 2] > 0).all(), label
    if founders_only:   # no transmission, no mutation term
        assert (np.abs(DQe) <= LLK_RTOL * 2 * np.abs(Dr)).all(), label
    if has_kid:
        assert len(planted) and DQr[planted].max() > 3, (label, DQr[planted])
        assert DQe[planted].max() > 3, label


@pytest.mark.parametrize("shape,nfam,nsites", CASES)
def test_chrx_matches_reference(built, tmp_path_factory, shape, nfam, nsites):
    """N and DQ of every site against the reference; the figures are printed before the assertions."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam, nsites)
    eng = x_engine(ped)
    res, _ = run_batches(eng, block, refalt)
    eng.close()
    check_against_reference(res, rv, models, planted, shape != "single", shape == "single", f"{shape}/{nfam}")


def test_chrx_matches_reference_exact_numerics(built, tmp_path_factory):
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "mixed", 31)
    eng = x_engine(ped, numerics=pm.NUM_EXACT)
    res, _ = run_batches(eng, block, refalt)
    eng.close()
    check_against_reference(res, rv, models, planted, True, False, "mixed/31/exact")


# ------------------------------------------------------------------------------------------------
# sex-awareness: a hemizygous-reference son of an alternate-allele father is Mendelian on X, impossible on an autosome

def _one_family_block(ped, fam, kid_local, refalts):
    """Father (255, 255, 0), mother (0, 150, 255), the chosen child (0, 255, 150), every other person without data."""
    fs, _ = _arrays(ped)
    block = np.full((len(refalts), ped.n_person, 10), 255, np.uint8)
    for i, ra in enumerate(refalts):
        _, _, g = three(ra)
        tri = np.zeros((ped.n_person, 3), np.uint8)
        tri[fs[fam]], tri[fs[fam] + 1], tri[fs[fam] + kid_local] = (255, 255, 0), (0, 150, 255), (0, 255, 150)
        block[i][:, g] = tri
    return block


def _reference_dq(ped, block, refalts, x_std):
    par = pm.Params.defaults(vcf_mode=1)
    M, A4 = mutation_matrices(ped, par)
    rp = RefPedigree(ped.view)
    out = []
    for i, ra in enumerate(refalts):
        m = SiteModel(rp, M, A4, block[i], ra)
        N, xN, _, ok = brent_max(lambda f: m.loglik(f, True), par.precision)
        D, xD, _, ok0 = brent_max(lambda f: m.loglik(f, False), par.precision)
        assert ok and ok0
        out.append((N, N - D, N - (m.loglik(float(x_std[i]), False) if x_std is not None else D)))
    return np.array(out)


def test_chrx_is_sex_aware(built, tmp_path_factory):
    refalts = np.array([1 | (3 << 4), 1 | (2 << 4)], np.uint8)   # A>G (a transition), A>C (a transversion)
    # a son: trio families (father, mother, son)
    ped = dataset(tmp_path_factory, "trio", 3)[0]
    sex = np.ctypeslib.as_array(ped.view.sex, shape=(ped.n_person,))
    fs, _ = _arrays(ped)
    assert sex[fs[0] + 2] == MALE
    block = _one_family_block(ped, 0, 2, refalts)
    alone = _reference_dq(ped, block, refalts, None)
    assert (alone[:, 1] < 0.5).all(), alone   # the reference alone: Mendelian on X
    eng = x_engine(ped)
    res, _ = run_batches(eng, block, refalts)
    ref = _reference_dq(ped, block, refalts, res["varfreq"][:, 1])
    print("son on chrX: engine DQ", res["denovo_lr"], "reference", ref[:, 2])
    assert (np.abs(res["varllk"][:, 2] - ref[:, 0]) <= LLK_RTOL * np.abs(ref[:, 0])).all(), (res["varllk"][:, 2], ref[:, 0])
    assert (np.abs(res["denovo_lr"] - ref[:, 2]) <= LLK_RTOL * 2 * np.abs(ref[:, 0])).all(), (res["denovo_lr"], ref[:, 2])
    assert (res["denovo_lr"] < 0.5).all()
    eng.begin_section(pm.PM_CHR_AUTO)   # the same engine, the same block, an autosome: an impossible genotype
    auto, _ = run_batches(eng, block, refalts)
    eng.close()
    print("son on an autosome: engine DQ", auto["denovo_lr"])
    assert (auto["denovo_lr"] > 3).all(), auto["denovo_lr"]
    # a daughter: the second child of mixed's family 1
    ped = dataset(tmp_path_factory, "mixed", 31)[0]
    sex = np.ctypeslib.as_array(ped.view.sex, shape=(ped.n_person,))
    fs, _ = _arrays(ped)
    assert fs[2] - fs[1] == 4 and sex[fs[1] + 3] != MALE
    block = _one_family_block(ped, 1, 3, refalts)
    eng = x_engine(ped)
    res, _ = run_batches(eng, block, refalts)
    eng.close()
    ref = _reference_dq(ped, block, refalts, res["varfreq"][:, 1])
    print("daughter on chrX: engine DQ", res["denovo_lr"], "reference", ref[:, 2])
    assert (np.abs(res["varllk"][:, 2] - ref[:, 0]) <= LLK_RTOL * np.abs(ref[:, 0])).all(), (res["varllk"][:, 2], ref[:, 0])
    assert (np.abs(res["denovo_lr"] - ref[:, 2]) <= LLK_RTOL * 2 * np.abs(ref[:, 0])).all(), (res["denovo_lr"], ref[:, 2])


# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("extmix", 5)])
def test_chrx_side_effects(built, tmp_path_factory, shape, nfam):
    """On chrX -- off: the bytes of an engine that never heard of the feature; on: only the four result fields change.  On
    an autosome the X switch changes nothing."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam)
    par = pm.Params.defaults(vcf_mode=1)
    fresh = pm.Engine(ped.view, par, max_batch=64)
    fresh.begin_section(pm.PM_CHR_X)
    r0, c0 = run_batches(fresh, block, refalt)
    fresh.close()
    eng = pm.Engine(ped.view, par, max_batch=64)
    eng.set_vcf_denovo(True)
    a_off, ca_off = run_batches(eng, block, refalt)   # an autosomal section, --vcf_denovo alone
    eng.begin_section(pm.PM_CHR_X)
    r_off, c_off = run_batches(eng, block, refalt)
    assert r_off.tobytes() == r0.tobytes() and c_off.tobytes() == c0.tobytes()
    eng.set_vcf_denovo_chrx(True)
    r_on, c_on = run_batches(eng, block, refalt)
    assert r_on.tobytes() != r0.tobytes()
    assert (r_on["evals"][:, 2] > 0).all()
    assert _masked(r_on) == _masked(r0) and c_on.tobytes() == c0.tobytes()
    eng.begin_section(pm.PM_CHR_AUTO)
    a_on, ca_on = run_batches(eng, block, refalt)
    assert a_on.tobytes() == a_off.tobytes() and ca_on.tobytes() == ca_off.tobytes()
    eng.begin_section(pm.PM_CHR_X)
    eng.set_vcf_denovo_chrx(False)
    r_back, c_back = run_batches(eng, block, refalt)
    assert r_back.tobytes() == r0.tobytes() and c_back.tobytes() == c0.tobytes()
    eng.close()


def test_chrx_entry_points_agree(built, tmp_path_factory):
    """run, run_vcf, submit / collect and run_device + sync give the same result bytes on a chrX section."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "mixed", 31)
    n, npers = 32, ped.n_person
    pl, ra = np.ascontiguousarray(block[:n]), np.ascontiguousarray(refalt[:n])
    zeros = np.zeros((n, npers), np.uint32)
    eng = x_engine(ped, max_batch=n)
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


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("roof", 3)])
def test_chrx_reads_three_planes_only(built, tmp_path_factory, shape, nfam):
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, shape, nfam)
    noisy = np.random.default_rng(11).integers(0, 256, block.shape, dtype=np.uint8)
    for i in range(len(refalt)):   # the same three planes
        _, _, g = three(refalt[i])
        noisy[i][:, g] = block[i][:, g]
    assert (noisy != block).any()
    eng = x_engine(ped)
    ra, ca = run_batches(eng, block, refalt)
    rb, cb = run_batches(eng, noisy, refalt)
    eng.close()
    assert (ra["evals"][:, 2] > 0).all()
    assert ra.tobytes() == rb.tobytes() and ca.tobytes() == cb.tobytes()


def test_chrx_sections_and_detail(built, tmp_path_factory):
    """chrY and MT sections stay untouched with everything on; on chrX the detail has no rows while DQ is filled."""
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "mixed", 31)
    par = pm.Params.defaults(vcf_mode=1)
    eng = x_engine(ped)
    eng.set_vcf_denovo_detail(2, 2)
    for chrom in (pm.PM_CHR_Y, pm.PM_CHR_MT):
        off = pm.Engine(ped.view, par, max_batch=64)
        off.begin_section(chrom)
        r0, c0 = run_batches(off, block, refalt)
        off.close()
        eng.begin_section(chrom)
        r1, c1 = run_batches(eng, block, refalt)
        assert r1.tobytes() == r0.tobytes() and c1.tobytes() == c0.tobytes(), chrom
        assert len(eng.vcf_denovo_rows()) == 0
    eng.begin_section(pm.PM_CHR_X)
    rx, _ = run_batches(eng, block, refalt)
    assert (rx["evals"][:, 2] > 0).all() and (rx["denovo_lr"][planted] >= par.denovo_min_llr).any()
    assert len(eng.vcf_denovo_rows()) == 0
    eng.begin_section(pm.PM_CHR_AUTO)   # and the rows are back on the next autosome
    run_batches(eng, block, refalt)
    assert len(eng.vcf_denovo_rows()) > 0
    eng.close()


def test_chrx_api_errors(built, tmp_path_factory):
    ped, block, refalt, planted, rv, models = dataset(tmp_path_factory, "trio", 3)
    lib = pm.load_library()
    glf = pm.Engine(ped.view, pm.Params.defaults(denovo=1), max_batch=8)
    assert lib.pm_engine_set_vcf_denovo_chrx(glf.h, 1) == -1   # PM_EINVAL
    assert b"without vcf_mode" in lib.pm_last_error()
    glf.close()
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=8)
    assert lib.pm_engine_set_vcf_denovo_chrx(eng.h, 1) == -1
    assert b"vcf_denovo is off" in lib.pm_last_error()
    eng.set_vcf_denovo(True)
    eng.begin_section(pm.PM_CHR_X)
    zeros = np.zeros((8, ped.n_person), np.uint32)
    eng.submit(block[:8], zeros, refalt[:8])
    assert lib.pm_engine_set_vcf_denovo_chrx(eng.h, 1) == -1
    assert b"not been collected" in lib.pm_last_error()
    r_off, _ = eng.collect()
    assert (r_off["evals"][:, 2] == 0).all()
    eng.set_vcf_denovo_chrx(True)
    r_on, _ = eng.run(block[:8], zeros, refalt[:8])
    assert (r_on["evals"][:, 2] > 0).all()
    eng.set_vcf_denovo(False)   # clears the X switch too
    eng.set_vcf_denovo(True)
    r_clear, _ = eng.run(block[:8], zeros, refalt[:8])
    assert r_clear.tobytes() == r_off.tobytes()
    eng.close()


# ------------------------------------------------------------------------------------------------
# CLI: --vcf_denovo_chrX on the example input, its chromosome declared X

PLANT_DAUGHTER, PLANT_SON = 100, 200   # record indices; fam1 of example/test.ped: parents 1, 2, daughter 3, son 4
FAM1 = ("1", "2", "3", "4")


def _write_planted_vcf(path):
    from vcf_edits import EDITS, write_edited_vcf
    assert PLANT_DAUGHTER not in EDITS and PLANT_SON not in EDITS
    write_edited_vcf(path)
    lines = open(path).read().splitlines()
    head = next(l for l in lines if l.startswith("#CHROM")).split("\t")
    planted, k = {}, -1
    for j, l in enumerate(lines):
        if l.startswith("#"):
            continue
        k += 1
        if k not in (PLANT_DAUGHTER, PLANT_SON):
            continue
        kid, kid_pl = ("3", DAUGHTER_PL) if k == PLANT_DAUGHTER else ("4", SON_PL)
        c = l.split("\t")
        assert len(c[3]) == 1 and len(c[4]) == 1 and c[8].split(":")[-1] == "PL"
        for col in range(9, len(c)):
            if head[col] in FAM1:
                f = c[col].split(":")
                f[-1] = ",".join(str(x) for x in (kid_pl if head[col] == kid else PARENT_PL))
                c[col] = ":".join(f)
        lines[j] = "\t".join(c)
        planted[k] = c
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return head, planted


def _run_cli(src, out, *extra):
    r = subprocess.run([pm.BIN_PATH, "-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--out_vcf", out] + list(extra),
                       cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return open(out).read().splitlines()


def test_cli_vcf_denovo_chrx(built, tmp_path):
    src = str(tmp_path / "in.vcf")
    head, planted = _write_planted_vcf(src)
    label = planted[PLANT_DAUGHTER][0]
    assert all(l.split("\t")[0] == label for l in open(src) if not l.startswith("#"))
    alone = _run_cli(src, str(tmp_path / "alone.vcf"), "--vcf_denovo", "--chrX", label)
    assert not any(";DQ=" in l for l in alone if not l.startswith("#")), "without the flag chrX records carry no tag"
    tagged = _run_cli(src, str(tmp_path / "tagged.vcf"), "--vcf_denovo", "--chrX", label, "--vcf_denovo_chrX")
    stripped = [re.sub(r";DQ=[-0-9.einf]+", "", l) for l in tagged]
    assert [l for l in stripped if not l.startswith("##Polymutt=")] == [l for l in alone if not l.startswith("##Polymutt=")]
    recs = [l.split("\t") for l in tagged if not l.startswith("#")]
    with_dq = [c for c in recs if ";DQ=" in c[7]]
    assert with_dq
    for c in with_dq:
        assert len(c[3]) == 1 and len(c[4]) == 1, "no indel record carries the tag"
        assert re.search(r";DP=\d+;DQ=-?\d+\.\d{3}$", c[7]), c[7]
    # the planted records against the reference's value for their PLs
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    person = {pid: i for i, pid in enumerate(ped.pids())}
    par = pm.Params.defaults(vcf_mode=1)
    M, A4 = mutation_matrices(ped, par)
    rp = RefPedigree(ped.view)
    for k, rec in planted.items():
        a1, a2 = "ACGT".index(rec[3]) + 1, "ACGT".index(rec[4]) + 1
        g = [gi(a1, a1), gi(a1, a2), gi(a2, a2)]
        site = np.full((ped.n_person, 10), 255, np.uint8)
        for col in range(9, len(rec)):
            site[person[head[col]], g] = [min(255, int(x)) for x in rec[col].split(":")[-1].split(",")]
        m = SiteModel(rp, M, A4, site, a1 | (a2 << 4))
        N, _, _, ok1 = brent_max(lambda f: m.loglik(f, True), par.precision)
        D, _, _, ok0 = brent_max(lambda f: m.loglik(f, False), par.precision)
        assert ok1 and ok0 and N - D > 3, (k, N - D)
        got = [c for c in recs if c[1] == rec[1] and c[0] == rec[0]]
        assert len(got) == 1
        mt = re.search(r";DQ=(-?\d+\.\d{3})$", got[0][7])
        assert mt, (k, got[0][7])
        print(f"record {k}: printed DQ {mt.group(1)}, reference {N - D:.6f}")
        assert abs(float(mt.group(1)) - (N - D)) <= 0.0005 + 1e-6, (k, mt.group(1), N - D)
    # the detail stays autosomal only: DQ alone on chrX records
    detail = _run_cli(src, str(tmp_path / "detail.vcf"), "--vcf_denovo", "--chrX", label, "--vcf_denovo_chrX",
                      "--vcf_denovo_families", "2")
    body = [l for l in detail if not l.startswith("#")]
    assert any(";DQ=" in l for l in body)
    assert not any(";DNF" in l or ";DNC" in l for l in body)
