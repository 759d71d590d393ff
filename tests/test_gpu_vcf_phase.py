"""GPU tests of the transmission phase plane of the --in_vcf path (pm_engine_set_vcf_phase / pm_engine_vcf_phase,
--vcf_phase).

* (p12, p21) against the numpy reference of tests/vcf_phase_reference.py (the definition, without peeling; checked on the
  CPU by tests/test_cpu_vcf_phase.py) at the engine's own frequency, every row and person, on multi-family autosomal
  pedigrees: one case per kernel and per way it can go wrong.
* Plane invariants: finite values in [0, 1], founders exactly (0, 0), p12 + p21 = the posterior plane's p[1] (which the
  oracle pins, single families included: this pins the single-family prior mode), all zero on chrX / chrY / MT.
* The plane is additive: site results, genotype rows, the posterior plane and the de novo outputs are the same bytes with
  it on, through every entry point; the schedule compiler does not change it; a stuck Brent keeps the returned rows.
* The CLI prints PQ and phased GTs and nothing else moves.

The float tolerance is derived, not measured: one rounding of a value in [0, 1] to float moves it by at most 2^-25 (half
an ulp of the largest binade), on top of the project's DOSE_ATOL = 1e-9 for double-against-double arithmetic.  p12 + p21
against p[1] compares three rounded values: 3 x 2^-25.

Every engine case runs 96 sites at max_batch = 64, so the second batch is partial.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from parity import DOSE_ATOL, _nonfinite_problem
from test_brent_stuck import first_stuck, pick_itmax
import vcf_plane_common as common
from vcf_phase_reference import PhaseFamilies

pytestmark = pytest.mark.gpu

PH_ATOL = 2.0 ** -25 + DOSE_ATOL
SUM_ATOL = 3 * 2.0 ** -25 + DOSE_ATOL
BATCH, NSITES = 64, 96

# multi-family autosomal pedigrees, the smallest at which each kernel can still go wrong: two family sizes in one wave,
# more than 64 families (a lane takes a second family), the founder branch, peeled families alone, one family of each of
# the five peel schedules; "nuclear": families of three and four children (k_vcf_phase_nuc's nuclear branch)
REF_CASES = [("mixed", 31), ("quad", 70), ("single", 12), ("ext10", 3), ("extmix", 5), ("nuclear", 0)]

PEEL_CASES = [("ext10", 3, 96, 64), ("extmix", 5, 16, 12)]   # (shape, families, sites, max_batch)


def dataset(tmp_path_factory, shape, nfam, nsites=NSITES):
    """(owner of the pedigree, its view, block, refalt), generated once per case and left unchanged."""
    return common.dataset(tmp_path_factory, "vph", shape, nfam, nsites)


def run_batches(eng, block, refalt, entry="run", phase=True, post=False, batch=BATCH):
    """Every batch through one entry point: (results, calls as (best, gq, label) int arrays, phase plane or None,
    posterior plane or None)."""
    def fetch(c):
        p = None
        if phase:
            p = eng.vcf_phase()
            assert p.shape == (len(c), eng.n_person, 2) and p.dtype == np.float32
        return p, eng.vcf_posteriors() if post else None
    res, calls, got = common.run_batches(eng, block, refalt, batch, entry, fetch)
    return (res, calls, np.concatenate([g[0] for g in got]) if phase else None,
            np.concatenate([g[1] for g in got]) if post else None)


def check_plane(ph, founders, label):
    """What holds for every plane: finite values in [0, 1], p12 + p21 <= 1 to the rounding, founders exactly (0, 0)."""
    assert np.isfinite(ph).all(), label
    assert (ph >= 0).all() and (ph <= 1).all(), label
    assert (ph.astype(np.float64).sum(axis=-1) <= 1 + 2.0 ** -24).all(), label
    assert (ph[:, founders] == 0).all(), label


@pytest.mark.parametrize("numerics", [pm.NUM_POLY, pm.NUM_EXACT])
@pytest.mark.parametrize("shape,nfam", REF_CASES)
def test_phase_matches_reference(built, tmp_path_factory, shape, nfam, numerics):
    ped, view, block, refalt = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1, numerics=numerics), max_batch=BATCH)
    eng.set_vcf_phase(True)
    res, calls, ph, _ = run_batches(eng, block, refalt)
    eng.close()
    assert (res["call_row"] >= 0).all() and len(ph) == len(refalt)   # every site of these blocks is written
    fams = PhaseFamilies(view)
    ref = fams.phase(block, refalt, res["af"])
    label = f"{shape} {nfam} numerics {numerics}"
    problems = []
    _nonfinite_problem(label + " phase", ph.astype(np.float64), ref, problems)
    assert not problems, problems
    d = np.abs(ph.astype(np.float64) - ref)   # every row, every person
    print(f"{label}: max |phase - reference| = {d.max():.3g} (bound {PH_ATOL:.3g})")
    assert (d <= PH_ATOL).all(), (label, d.max(), np.argwhere(d > PH_ATOL)[:5])
    check_plane(ph, fams.is_founder, label)
    if not fams.is_founder.all():
        assert (ph[:, ~fams.is_founder] != 0).any(), label


@pytest.mark.parametrize("shape,nfam", REF_CASES + [("quad", 1), ("ext10", 1)])
def test_phase_sums_to_the_het_posterior(built, tmp_path_factory, shape, nfam):
    """With the posterior plane also on: |p12 + p21 - p[1]| <= 3 x 2^-25 + DOSE_ATOL for every non-founder.  The lone
    quad and the lone ext10 family pin the single-family prior mode through the oracle-pinned posterior plane."""
    ped, view, block, refalt = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)
    eng.set_vcf_phase(True)
    eng.set_vcf_posteriors(True)
    res, calls, ph, post = run_batches(eng, block, refalt, post=True)
    eng.close()
    founders = PhaseFamilies(view).is_founder
    check_plane(ph, founders, f"{shape} {nfam}")
    kids = ~founders
    if not kids.any():
        return
    s = ph.astype(np.float64)[:, kids].sum(axis=-1)
    p1 = post.astype(np.float64)[:, kids, 1]
    problems = []
    _nonfinite_problem(f"{shape} {nfam} p12 + p21", s, p1, problems)
    assert not problems, problems
    d = np.abs(s - p1)
    print(f"{shape} {nfam}: max |p12 + p21 - p[1]| = {d.max():.3g} (bound {SUM_ATOL:.3g})")
    assert (d <= SUM_ATOL).all(), (d.max(), np.argwhere(d > SUM_ATOL)[:5])
    assert (p1 > 0.5).any()


@pytest.mark.parametrize("chrom", [pm.PM_CHR_X, pm.PM_CHR_Y, pm.PM_CHR_MT])
@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("ext10", 3)])
def test_no_phase_off_the_autosomes(built, tmp_path_factory, shape, nfam, chrom):
    """A chrX / chrY / MT section's plane is all zero -- also right after an autosomal batch filled it -- and the next
    autosomal section's is what it was."""
    ped, view, block, refalt = dataset(tmp_path_factory, shape, nfam)
    eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)
    eng.set_vcf_phase(True)
    _, _, auto, _ = run_batches(eng, block, refalt)
    assert (auto != 0).any()
    eng.begin_section(chrom)
    res, calls, ph, _ = run_batches(eng, block, refalt)
    assert len(ph) == (res["call_row"] >= 0).sum() > 0 and (ph == 0).all()
    eng.begin_section(pm.PM_CHR_AUTO)
    _, _, again, _ = run_batches(eng, block, refalt)
    eng.close()
    assert again.tobytes() == auto.tobytes()


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("single", 12), ("extmix", 5)])   # lean, generic, peeled
def test_feature_off_identity_and_entry_points(built, tmp_path_factory, shape, nfam):
    ped, view, block, refalt = dataset(tmp_path_factory, shape, nfam)
    par = pm.Params.defaults(vcf_mode=1)
    plain = pm.Engine(view, par, max_batch=BATCH)   # never has the feature on (the posterior plane it has)
    plain.set_vcf_posteriors(True)
    eng = pm.Engine(view, par, max_batch=BATCH)
    eng.set_vcf_posteriors(True)
    eng.set_vcf_phase(True)
    planes = []
    for entry in ("run", "run_vcf", "submit"):
        r0, c0, _, q0 = run_batches(plain, block, refalt, entry, phase=False, post=True)
        r1, c1, p1, q1 = run_batches(eng, block, refalt, entry, post=True)
        assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes() and q0.tobytes() == q1.tobytes(), entry
        planes.append(p1)
    assert planes[0].tobytes() == planes[1].tobytes() == planes[2].tobytes()
    eng.set_vcf_phase(False)   # off again: the same bytes still, and no plane
    r0, c0, _, q0 = run_batches(plain, block, refalt, "run", phase=False, post=True)
    r1, c1, _, q1 = run_batches(eng, block, refalt, "run", phase=False, post=True)
    assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes() and q0.tobytes() == q1.tobytes()
    with pytest.raises(RuntimeError, match="feature is off"):
        eng.vcf_phase()
    eng.set_vcf_phase(True)   # on again: no batch has filled the new plane
    assert eng.vcf_phase().shape == (0, eng.n_person, 2)
    plain.close()
    eng.close()


def test_setter_errors_and_denovo_outputs(built, tmp_path_factory):
    ped, view, block, refalt = dataset(tmp_path_factory, "mixed", 31)
    glf = pm.Engine(view, pm.Params.defaults(), max_batch=BATCH)
    with pytest.raises(RuntimeError, match="vcf_mode"):
        glf.set_vcf_phase(True)
    glf.close()
    outs = []
    zeros = np.zeros(block.shape[:2], np.uint32)
    for with_phase in (False, True):
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)
        eng.set_vcf_denovo(True)
        eng.set_vcf_denovo_detail(2, 2)
        if with_phase:
            eng.set_vcf_phase(True)
            eng.submit(block[:BATCH], zeros[:BATCH], refalt[:BATCH])
            lib = pm.load_library()
            assert lib.pm_engine_set_vcf_phase(eng.h, 0) == -1 and b"not been collected" in lib.pm_last_error()
            n = C.c_int32(0)
            assert lib.pm_engine_vcf_phase(eng.h, C.byref(n), None) == -1 and b"not been collected" in lib.pm_last_error()
            eng.collect()
        got = []
        for s in range(0, len(refalt), BATCH):
            sl = slice(s, s + BATCH)
            r, c = eng.run(block[sl], zeros[sl], refalt[sl])
            top_f, sum_f, _ = eng.vcf_denovo_families()
            top_c, _ = eng.vcf_denovo_carriers()
            got.append(b"".join(a.tobytes() for a in (r, c, eng.vcf_denovo_rows(), top_f, sum_f, top_c)))
            if with_phase:
                assert len(eng.vcf_phase()) == len(c)
        if with_phase:   # neither feature switches the other off
            eng.set_vcf_denovo(False)
            eng.run(block[:BATCH], zeros[:BATCH], refalt[:BATCH])
            assert len(eng.vcf_phase()) == BATCH
        outs.append(got)
        eng.close()
    assert outs[0] == outs[1]
    assert any((np.frombuffer(g, np.uint8) != 0).any() for g in outs[0])


def test_schedule_compiler_on_and_off(built, tmp_path_factory, monkeypatch):
    ped, view, block, refalt = dataset(tmp_path_factory, "ext10", 3)
    planes = []
    for no_jit in (False, True):
        if no_jit:
            monkeypatch.setenv("PM_NO_JIT", "1")
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=BATCH)
        eng.set_vcf_phase(True)
        planes.append(run_batches(eng, block, refalt)[2])
        eng.close()
    assert planes[0].tobytes() == planes[1].tobytes() and (planes[0] != 0).any()


@pytest.mark.parametrize("shape,nfam,nsites,batch", PEEL_CASES)
def test_peel_workspace_in_lds_and_in_hbm(built, tmp_path_factory, monkeypatch, shape, nfam, nsites, batch):
    """k_vcf_phase_es<true> and k_vcf_phase_es<false> (PM_ES_POST_HBM) write the same plane: the two workspaces hold the
    same doubles in the same order.  Site results and genotype rows are the same bytes too."""
    ped, view, block, refalt = dataset(tmp_path_factory, shape, nfam, nsites)
    outs = []
    for hbm in (False, True):
        if hbm:
            monkeypatch.setenv("PM_ES_POST_HBM", "1")   # (read when the engine is created)
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_phase(True)
        outs.append(run_batches(eng, block, refalt, batch=batch))
        eng.close()
    (r0, c0, p0, _), (r1, c1, p1, _) = outs
    assert p0.tobytes() == p1.tobytes() and (p0 != 0).any()
    assert r0.tobytes() == r1.tobytes() and c0.tobytes() == c1.tobytes()


def test_stuck_site_keeps_the_returned_rows(built, tmp_path_factory, monkeypatch):
    ped, view, block, refalt = dataset(tmp_path_factory, "mixed", 31)
    par = pm.Params.defaults(vcf_mode=1)
    eng = pm.Engine(view, par, max_batch=BATCH)
    eng.set_vcf_phase(True)
    res, calls, ph, _ = run_batches(eng, block, refalt)
    eng.close()
    k, s = pick_itmax(res)
    assert first_stuck(res, k) == s
    monkeypatch.setenv("PM_TEST_ITMAX", str(k))   # (read when the engine is created)
    eng = pm.Engine(view, par, max_batch=BATCH)
    eng.set_vcf_phase(True)
    zeros = np.zeros(block.shape[:2], np.uint32)
    b0 = s // BATCH * BATCH
    for t in range(0, b0, BATCH):   # the batches before the stuck site's run as usual
        eng.run(block[t:t + BATCH], zeros[t:t + BATCH], refalt[t:t + BATCH])
        assert eng.vcf_phase().tobytes() == ph[t:t + BATCH].tobytes()
    with pytest.raises(pm.engine.BrentStuck) as ei:
        eng.run(block[b0:b0 + BATCH], zeros[b0:b0 + BATCH], refalt[b0:b0 + BATCH])
    assert ei.value.site == s - b0
    got = eng.vcf_phase()
    assert len(got) == len(ei.value.calls) == s - b0   # the rows the batch returned: those before the stuck site
    assert got.tobytes() == ph[b0:s].tobytes()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- CLI

PQ_HEADER = ('##FORMAT=<ID=PQ,Number=1,Type=Integer,Description="Phred-scaled quality of the transmission phase of GT '
             '(paternal|maternal)">')


_cli, _same = common.cli, common.same


def _strip(lines):
    """The output without the PQ header line and sub-field and with every phased GT unphased again."""
    return common.strip_fields(lines, ("PQ",), lambda fmt, k: fmt[k + 1] in ("PL", "GL") and k == len(fmt) - 2, unphase=True)


def _founder_columns(lines):
    """Per sample column of the output: is the sample a founder (both parents 0 in the example's pedigree file)."""
    founder = {}
    for l in open(os.path.join(EXAMPLE, "test.ped")):
        t = l.split()
        if len(t) >= 4:
            founder[t[1]] = t[2] == "0" and t[3] == "0"
    head = next(l for l in lines if l.startswith("#CHROM")).split("\t")[9:]
    return [founder[s] for s in head]


def _samples(lines):
    """(GT, PQ text, is founder) of every sample of every record."""
    fo = _founder_columns(lines)
    for l in lines:
        if l.startswith("#"):
            continue
        c = l.split("\t")
        k = c[8].split(":").index("PQ")
        for i, v in enumerate(c[9:]):
            f = v.split(":")
            yield f[0], f[k], fo[i]


def test_cli_prints_pq_and_phased_gt(built, tmp_path):
    plain = _cli(tmp_path, "plain.vcf", [])
    got = _cli(tmp_path, "phase.vcf", ["--vcf_phase"])
    hdr = [l for l in got if l.startswith("##FORMAT")]
    k = next(i for i, l in enumerate(hdr) if l.startswith("##FORMAT=<ID=DP,"))
    assert hdr[k + 1] == PQ_HEADER and hdr[k + 2].startswith("##FORMAT=<ID=PL,")
    assert all(l.split("\t")[8] in ("GT:GQ:DP:PQ:PL", "GT:GQ:DP:PQ:GL") for l in got if not l.startswith("#"))
    assert _same(_strip(got), plain)
    # every | sits on a non-founder het with PQ >= 10; every unphased sample with a PQ is a het non-founder below it
    phased = below = 0
    for gt, pq, founder in _samples(got):
        if "|" in gt:
            assert gt in ("0|1", "1|0") and not founder and pq != "." and 10 <= int(pq) <= 99, (gt, pq, founder)
            phased += 1
        elif pq != ".":
            assert gt == "0/1" and not founder and 0 <= int(pq) < 10, (gt, pq, founder)
            below += 1
        if founder or gt not in ("0/1", "0|1", "1|0"):
            assert pq == ".", (gt, pq, founder)
    assert phased > 0 and below > 0, (phased, below)
    # --vcf_phase_minPQ 0 phases every considered sample, 99 only those with PQ 99
    all_ph = _cli(tmp_path, "pq0.vcf", ["--vcf_phase", "--vcf_phase_minPQ", "0"])
    assert _same(_strip(all_ph), plain)
    n0 = 0
    for (gt, pq, founder), (gt_d, pq_d, _) in zip(_samples(all_ph), _samples(got)):
        assert pq == pq_d and (pq == ".") == ("|" not in gt), (gt, pq)
        if "|" in gt_d:
            assert gt == gt_d
        n0 += "|" in gt
    assert n0 == phased + below
    top = _cli(tmp_path, "pq99.vcf", ["--vcf_phase", "--vcf_phase_minPQ", "99"])
    assert _same(_strip(top), plain)
    n99 = 0
    for gt, pq, founder in _samples(top):
        assert ("|" in gt) == (pq == "99"), (gt, pq)
        n99 += "|" in gt
    assert 0 < n99 <= phased
    assert _same(_cli(tmp_path, "b7.vcf", ["--vcf_phase", "--batch", "7"]), got)
    assert _same(_cli(tmp_path, "e3.vcf", ["--vcf_phase", "--engines", "3", "--batch", "1000"]), got)


def test_cli_combines_with_posteriors_and_denovo(built, tmp_path):
    both = ["--vcf_posteriors", "--vcf_denovo", "--vcf_denovo_families", "2", "--vcf_denovo_carriers", "2"]
    a, b = _cli(tmp_path, "other.vcf", both), _cli(tmp_path, "other_phase.vcf", both + ["--vcf_phase"])
    hdr = [l for l in b if l.startswith("##FORMAT")]
    k = next(i for i, l in enumerate(hdr) if l.startswith("##FORMAT=<ID=GP,"))
    assert hdr[k + 1] == PQ_HEADER and hdr[k + 2].startswith("##FORMAT=<ID=PL,")
    assert all(l.split("\t")[8] in ("GT:GQ:DP:DS:GP:PQ:PL", "GT:GQ:DP:DS:GP:PQ:GL") for l in b if not l.startswith("#"))
    info = lambda ls: [l.split("\t")[7] for l in ls if not l.startswith("#")]
    assert info(a) == info(b) and any("DQ=" in x for x in info(a))
    assert _same(_strip(b), a)
    assert any("|" in gt for gt, _, _ in _samples(b))
    # the phase agrees with the printed posteriors: a phased sample's GP[1] is the largest
    for l in b:
        if l.startswith("#"):
            continue
        for v in l.split("\t")[9:]:
            f = v.split(":")
            if "|" in f[0]:
                g = [float(x) for x in f[4].split(",")]
                assert g[1] == max(g), v


def test_cli_records_without_data_and_shards(built, tmp_path):
    """Records without data print the previous computed record's phase, like its GT and GQ -- also when that record was
    computed by the shard before (the carried state travels in the shards' exchange): two shards on the one GPU write the
    one-process output, and a blanked record's sample fields are those of the record before it."""
    from test_cpu_host import run_sharded, vcf_body
    from vcf_edits import write_nodata_vcf
    src = str(tmp_path / "in.vcf")
    blanked = sorted(write_nodata_vcf(src, worlds=(2,)))
    args = ["-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--vcf_phase"]
    one = str(tmp_path / "one.vcf")
    r1 = subprocess.run([pm.BIN_PATH] + args + ["--out_vcf", one], cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    recs = {tuple(l.split("\t")[:2]): l.split("\t") for l in vcf_body(one)[1:]}   # (chromosome, position) -> record
    inp = [tuple(l.split("\t")[:2]) for l in open(src).read().splitlines() if not l.startswith("#")]
    fields = lambda c: [":".join(v.split(":")[:2] + v.split(":")[3:4]) for v in c[9:]]   # GT, GQ, PQ
    carried = carried_phase = 0
    for i in blanked:   # (records the path does not write, multi-allelic ones, are in neither)
        if i > 0 and inp[i] in recs and inp[i - 1] in recs:
            assert fields(recs[inp[i]]) == fields(recs[inp[i - 1]]), inp[i]
            carried += 1
            carried_phase += any("|" in v for v in fields(recs[inp[i]]))
    assert carried > 0 and carried_phase > 0
    sh = str(tmp_path / "sharded.vcf")
    r2 = run_sharded(EXAMPLE, args + ["--out_vcf", sh], 2)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert vcf_body(sh) == vcf_body(one)
    assert not [f for f in os.listdir(str(tmp_path)) if ".part" in f]
