"""GPU tests of the pedigree check of the --in_vcf path (pm_engine_set_vcf_pedcheck / pm_engine_reset_vcf_pedcheck /
pm_engine_vcf_pedcheck, --vcf_pedcheck).

* The sums against the brute-force table of tests/vcf_pedcheck_reference.py (the definition, without peeling; checked on the
  CPU by tests/test_cpu_vcf_pedcheck.py) at the engine's own row frequencies, on the smallest shapes that reach each kernel:
  person and n exactly, |q 2^-28 - S| <= n (2^-29 + 1e-9) -- the derived quantisation bound and the project's bound for one
  double evaluation against another, per counted row.
* Integer sums: the same rows in one batch, in three, through submit / collect and run to run are the same int64 values;
  reset and off / on start from zero; a chrX section adds nothing.
* Additive: site results, genotype rows, the three planes and the de novo outputs are the same bytes with the feature on.
* Discrimination: a child whose data are an unrelated founder's, and a trio whose father's are.
* The CLI report against the engine, with and without the flag, records without data, a chrX record, two shards.

Largest deviation measured on the MI355X, as a share of the bound: lean 0.026, striding 0.020, single 0.019, nuc 0.061, es
0.071 (LDS and HBM workspace: the same sums), the discrimination runs 0.035 / 0.074 / 0.038.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
import vcf_pedcheck_reference as R
import vcf_plane_common as common

pytestmark = pytest.mark.gpu

THETA = pm.Params.defaults().theta

SHAPES = R.SHAPES
_CASES = {}


def case(tmp_path_factory, name):
    """(ped, block, refalt, max_batch), generated once and left unchanged."""
    if name not in _CASES:
        fams, rows, batch = SHAPES[name]
        ped = R.write_pedigree(str(tmp_path_factory.mktemp("pc_" + name)), fams)
        block, refalt, _ = R.simulate(ped.view, rows, 17)
        block.setflags(write=False)
        _CASES[name] = (ped, block, refalt, batch)
    return _CASES[name]


def row_freq(res):
    """The written rows' sites and the frequency the passes behind the posterior stage take for them (lean_row)."""
    rows = np.flatnonzero(res["call_row"] >= 0)
    return rows, np.where(res["maxidx"][rows] == 0, 1 - THETA, res["af"][rows])


def engine_sums(view, block, refalt, batch, entry="run", eng=None):
    own = eng is None
    if own:
        eng = pm.Engine(view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_pedcheck(True)
    res, _, _ = common.run_batches(eng, block, refalt, batch, entry, lambda c: None)
    pc = eng.vcf_pedcheck()
    if own:
        eng.close()
    return res, pc


def check_against_reference(view, block, refalt, res, pc, label):
    rows, f = row_freq(res)
    ref = R.PedcheckFamilies(view).solve(block[rows], refalt[rows], f)
    assert pc.person.dtype == np.int32 and pc.n.dtype == np.int64 and pc.q.dtype == np.int64 and pc.llr.dtype == np.float64
    assert (pc.person == ref["person"]).all(), label
    assert (ref["n"] == len(rows)).all(), label   # (the reference counts every row: the engine cannot hide a skipped one)
    assert (pc.n == ref["n"]).all(), (label, pc.n, ref["n"])
    assert (pc.llr == pc.q * 2.0 ** -28).all()
    dev = np.abs(pc.llr - ref["S"])
    bnd = R.bound(ref["n"])[:, None]
    print(f"{label}: {len(rows)} rows, largest |q 2^-28 - S| = {dev.max():.3g} = {(dev / bnd).max():.3g} of the bound {bnd.min():.3g}")
    assert (dev <= bnd).all(), (label, dev, bnd)
    return ref


@pytest.mark.parametrize("name", ["lean", "striding", "single", "nuc"])
def test_sums_match_the_table(built, tmp_path_factory, name):
    ped, block, refalt, batch = case(tmp_path_factory, name)
    res, pc = engine_sums(ped.view, block, refalt, batch)
    ref = check_against_reference(ped.view, block, refalt, res, pc, name)
    assert len(pc.person) > 0 and (ref["n"] > 0).all()


def test_sums_match_the_table_peeled_lds_and_hbm(built, tmp_path_factory, monkeypatch):
    """k_vcf_pedcheck_es<true> and <false> (PM_ES_POST_HBM, read when the engine is created): d has children of its own."""
    ped, block, refalt, batch = case(tmp_path_factory, "es")
    got = []
    for hbm in (False, True):
        if hbm:
            monkeypatch.setenv("PM_ES_POST_HBM", "1")
        res, pc = engine_sums(ped.view, block, refalt, batch)
        check_against_reference(ped.view, block, refalt, res, pc, "es hbm" if hbm else "es lds")
        got.append(pc)
    assert (got[0].q == got[1].q).all() and (got[0].n == got[1].n).all()


@pytest.mark.parametrize("name", ["lean", "nuc", "es"])
def test_integer_sums_do_not_depend_on_the_split(built, tmp_path_factory, name):
    ped, block, refalt, batch = case(tmp_path_factory, name)
    n = len(refalt)
    res, one = engine_sums(ped.view, block, refalt, n)
    assert (one.n > 0).all()
    same = lambda a, b: (a.person == b.person).all() and (a.n == b.n).all() and (a.q == b.q).all()
    assert same(one, engine_sums(ped.view, block, refalt, n)[1])                      # run to run
    assert same(one, engine_sums(ped.view, block, refalt, (n + 2) // 3)[1])            # three batches
    assert same(one, engine_sums(ped.view, block, refalt, (n + 2) // 3, "submit")[1])  # submit / collect
    assert same(one, engine_sums(ped.view, block, refalt, (n + 2) // 3, "run_vcf")[1])
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=n)
    with pytest.raises(RuntimeError, match="feature is off"):
        eng.vcf_pedcheck()
    with pytest.raises(RuntimeError, match="feature is off"):
        eng.reset_vcf_pedcheck()
    eng.set_vcf_pedcheck(True)
    zero = eng.vcf_pedcheck()
    assert (zero.person == one.person).all() and not zero.n.any() and not zero.q.any()
    assert same(one, engine_sums(ped.view, block, refalt, n, eng=eng)[1])
    eng.set_vcf_pedcheck(True)   # on while on: the sums stay
    assert same(one, eng.vcf_pedcheck())
    twice = engine_sums(ped.view, block, refalt, n, eng=eng)[1]   # the sums live across batches
    assert (twice.n == 2 * one.n).all() and (twice.q == 2 * one.q).all()
    eng.reset_vcf_pedcheck()
    zero = eng.vcf_pedcheck()
    assert not zero.n.any() and not zero.q.any()
    assert same(one, engine_sums(ped.view, block, refalt, n, eng=eng)[1])
    eng.set_vcf_pedcheck(False)
    eng.set_vcf_pedcheck(True)   # off then on starts from zero
    zero = eng.vcf_pedcheck()
    assert not zero.n.any() and not zero.q.any()
    eng.begin_section(pm.PM_CHR_X)   # a chrX section adds nothing
    engine_sums(ped.view, block, refalt, n, eng=eng)
    zero = eng.vcf_pedcheck()
    assert not zero.n.any() and not zero.q.any()
    eng.begin_section(pm.PM_CHR_AUTO)
    assert same(one, engine_sums(ped.view, block, refalt, n, eng=eng)[1])
    eng.close()


@pytest.mark.parametrize("name", ["lean", "nuc", "es"])
def test_every_other_output_is_the_same_bytes(built, tmp_path_factory, name):
    ped, block, refalt, batch = case(tmp_path_factory, name)
    zeros = np.zeros(block.shape[:2], np.uint32)
    outs = []
    for on in (False, True):
        eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
        eng.set_vcf_posteriors(True)
        eng.set_vcf_phase(True)
        eng.set_vcf_joint(True)
        eng.set_vcf_denovo(True)
        eng.set_vcf_denovo_detail(2, 2)
        if on:
            eng.set_vcf_pedcheck(True)
        got = []
        for s in range(0, len(refalt), batch):
            sl = slice(s, s + batch)
            r, c = eng.run(block[sl], zeros[sl], refalt[sl])
            top_f, sum_f, _ = eng.vcf_denovo_families()
            top_c, _ = eng.vcf_denovo_carriers()
            parts = (r, c, eng.vcf_posteriors(), eng.vcf_phase(), *eng.vcf_joint(), eng.vcf_denovo_rows(), top_f, sum_f, top_c)
            got.append(b"".join(np.ascontiguousarray(a).tobytes() for a in parts))
        if on:
            assert eng.vcf_pedcheck().n.any()
            eng.set_vcf_phase(False)   # the phase plane's lists are its own: the check keeps running without them
            eng.reset_vcf_pedcheck()
            eng.run(block[:batch], zeros[:batch], refalt[:batch])
            assert eng.vcf_pedcheck().n.any()
        outs.append(got)
        eng.close()
    assert outs[0] == outs[1]


def test_setter_errors(built, tmp_path_factory):
    ped, block, refalt, batch = case(tmp_path_factory, "lean")
    glf = pm.Engine(ped.view, pm.Params.defaults(), max_batch=batch)
    with pytest.raises(RuntimeError, match="vcf_mode"):
        glf.set_vcf_pedcheck(True)
    glf.close()
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=batch)
    eng.set_vcf_pedcheck(True)
    zeros = np.zeros(block.shape[:2], np.uint32)
    eng.submit(block[:batch], zeros[:batch], refalt[:batch])
    lib = pm.load_library()
    k = C.c_int32(0)
    for rc in (lib.pm_engine_set_vcf_pedcheck(eng.h, 0), lib.pm_engine_reset_vcf_pedcheck(eng.h),
               lib.pm_engine_vcf_pedcheck(eng.h, C.byref(k), None)):
        assert rc == -1 and b"not been collected" in lib.pm_last_error()
    eng.collect()
    assert lib.pm_engine_vcf_pedcheck(eng.h, C.byref(k), None) == 0 and k.value == 3   # out == NULL: the count alone
    assert eng.vcf_pedcheck().n.all()
    eng.close()


# ------------------------------------------------------------------------------------------------------ discrimination

def test_swapped_child_and_swapped_father_are_found(built, tmp_path_factory):
    """tests/test_cpu_vcf_pedcheck.py shows the margins in the reference at the generating frequencies; here the engine runs
    at its own, the reference follows it, the margins still hold there, and the engine agrees in sign and within the bound."""
    ped, block, refalt, _ = R.discrimination_case(str(tmp_path_factory.mktemp("pc_disc")))
    view = ped.view
    n = len(refalt)
    res, pc = engine_sums(view, block, refalt, n)
    ref = check_against_reference(view, block, refalt, res, pc, "stated pedigree")
    assert (ref["S"] >= 5).all() and (pc.llr >= 5).all(), ref["S"]
    kids = list(ref["person"])
    # the first trio's child takes an unrelated founder's data
    c, u = R.DISC_CHILD, R.DISC_FOUNDER
    sw = R.swap_columns(block, c, u)
    res, pc = engine_sums(view, sw, refalt, n)
    ref = check_against_reference(view, sw, refalt, res, pc, "child swapped")
    k = kids.index(c)
    assert ref["S"][k, 2] <= -5 and pc.llr[k, 2] <= -5, (ref["S"][k], pc.llr[k])
    others = [i for i in range(len(kids)) if i != k]
    assert (ref["S"][others] >= 5).all() and (pc.llr[others] >= 5).all()
    assert (np.sign(pc.llr) == np.sign(ref["S"])).all()
    # the second trio's father takes the founder's
    fa, c2 = R.DISC_FATHER, R.DISC_FATHER_CHILD
    sw = R.swap_columns(block, fa, u)
    res, pc = engine_sums(view, sw, refalt, n)
    ref = check_against_reference(view, sw, refalt, res, pc, "father swapped")
    k = kids.index(c2)
    assert ref["S"][k, 0] <= -5 and ref["S"][k, 1] >= 5, ref["S"][k]
    assert pc.llr[k, 0] <= -5 and pc.llr[k, 1] >= 5, pc.llr[k]
    assert (np.sign(pc.llr) == np.sign(ref["S"])).all()


# ---------------------------------------------------------------------------------------------------------------- CLI

HEADER = ["#polymutt pedcheck v1: log10 LR of each stated parent link against an unrelated one, summed over N_SITES autosomal records",
          "FAMILY\tPERSON\tFATHER\tMOTHER\tN_SITES\tLLR_FATHER\tLLR_MOTHER\tLLR_BOTH\tSUSPECT"]


_records = R.example_records


def _expected_report(src):
    """The report's text from Engine.vcf_pedcheck() on the same records."""
    ped, block, refalt = _records(src)
    eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=len(refalt))
    eng.set_vcf_pedcheck(True)
    eng.run_vcf(block, refalt)
    pc = eng.vcf_pedcheck()
    eng.close()
    pids, start = ped.pids(), ped.fam_start()
    as_arr = np.ctypeslib.as_array
    father, mother = as_arr(ped.view.father, shape=(ped.n_person,)), as_arr(ped.view.mother, shape=(ped.n_person,))
    lib = pm.load_library()
    lines = list(HEADER)
    for p, n, q in zip(pc.person, pc.n, pc.q):
        llr = [float(np.ldexp(float(x), -28)) if n else 0.0 for x in q]
        sus = ",".join(name for name, v in zip(("father", "mother", "both"), llr) if v < 0) or "."
        fam = lib.pmh_pedigree_famid(ped.h, int(np.searchsorted(start, p, side="right") - 1)).decode()
        lines.append("\t".join([fam, pids[p], pids[father[p]], pids[mother[p]], str(int(n))] + ["%.2f" % v for v in llr] + [sus]))
    return lines, pc


def _run(tmp_path, name, extra, src=common.SRC):
    out = tmp_path / (name + ".vcf")
    r = subprocess.run([pm.BIN_PATH, "-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--out_vcf", str(out)] + extra,
                       cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out.read_text().splitlines(), r.stdout


def _stdout(text):   # (the lines that record the command line or the clock)
    return [l for l in text.splitlines() if "vcf_pedcheck" not in l and "out_vcf" not in l and not l.startswith(("Analysis", "Running time"))]


def test_cli_report_matches_the_engine(built, tmp_path):
    rep = tmp_path / "pedcheck.txt"
    plain, so0 = _run(tmp_path, "plain", [])
    got, so1 = _run(tmp_path, "pc", ["--vcf_pedcheck", str(rep)])
    assert common.same(got, plain) and _stdout(so0) == _stdout(so1)   # the VCF and stdout do not move
    exp, pc = _expected_report(common.SRC)
    text = rep.read_text()
    assert text.endswith("\n") and text.splitlines() == exp
    # fam1 and fam2 are as stated.  fam3's GLF_Index column is a permutation (9 -> 4, 10 -> 1, 11 -> 2, 12 -> 3) that the
    # --in_vcf path, which maps samples by id, does not apply: the VCF's column 9 holds the mother's data, 10 and 11 the two
    # children's and 12 the father's.  So 11's stated father is a true parent of it and its stated mother a sibling, and
    # 12's stated father is its spouse and its stated mother its child: the check finds exactly that.
    assert len(pc.person) == 6 and (pc.n > 8000).all() and (pc.llr[:4] > 5).all()
    assert pc.llr[4, 0] > 5 and pc.llr[4, 1] < -5 and pc.llr[5, 0] < -5 and pc.llr[5, 1] > 5, pc.llr[4:]
    assert [l.split("\t")[8] for l in exp[2:]] == [".", ".", ".", ".", "mother,both", "father,both"]
    # any batch size, any number of pipelined engines, every other --vcf_ flag: the same report
    for k, extra in enumerate((["--batch", "7"], ["--engines", "3", "--batch", "1000"],
                               ["--vcf_posteriors", "--vcf_phase", "--vcf_joint", "--vcf_denovo", "--vcf_denovo_families", "2"])):
        other = tmp_path / f"pedcheck{k}.txt"
        _run(tmp_path, f"pc{k}", extra + ["--vcf_pedcheck", str(other)])
        assert other.read_text() == text, extra


def test_cli_records_without_data_chrx_and_shards(built, tmp_path):
    """A record blanked to no data and a record moved to chrX change no count but their own; two shards on the one GPU write
    the one-process report and VCF."""
    from test_cpu_host import run_sharded, vcf_body
    from vcf_edits import write_nodata_vcf
    src = str(tmp_path / "in.vcf")
    blanked = sorted(write_nodata_vcf(src, worlds=(2,)))
    lines = open(src).read().splitlines()
    body = [i for i, l in enumerate(lines) if not l.startswith("#")]
    moved = body[len(body) // 3]
    assert len(body) // 3 not in blanked
    lines[moved] = "X" + lines[moved][lines[moved].index("\t"):]
    with open(src, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    whole, _ = _expected_report(common.SRC)
    exp, pc = _expected_report(src)
    n_whole = int(whole[2].split("\t")[4])
    assert (pc.n == n_whole - len(blanked) - 1).all(), (pc.n, n_whole, len(blanked))
    one_rep, sh_rep = tmp_path / "one.txt", tmp_path / "sharded.txt"
    one, _ = _run(tmp_path, "one", ["--vcf_pedcheck", str(one_rep)], src)
    assert one_rep.read_text().splitlines() == exp
    sh = str(tmp_path / "sharded.vcf")
    r = run_sharded(EXAMPLE, ["-p", "test.ped", "-d", "test.dat", "--in_vcf", src, "--vcf_pedcheck", str(sh_rep), "--out_vcf", sh], 2)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sh_rep.read_text() == one_rep.read_text()
    assert vcf_body(sh) == vcf_body(str(tmp_path / "one.vcf"))
    assert not [f for f in os.listdir(str(tmp_path)) if ".part" in f]


def test_cli_needs_in_vcf(built, tmp_path):
    rep = tmp_path / "pedcheck.txt"
    r = subprocess.run([pm.BIN_PATH, "-p", "test.ped", "-d", "test.dat", "-g", "test.gif", "--out_vcf", str(tmp_path / "o.vcf"),
                        "--vcf_pedcheck", str(rep)], cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "FATAL ERROR" in r.stdout and "--vcf_pedcheck needs --in_vcf" in r.stdout, r.stdout[-1000:]
    assert not rep.exists()
