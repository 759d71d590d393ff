"""Device-free checks of the joint call plane of the --in_vcf path (pm_engine_set_vcf_joint, --vcf_joint): the brute-force
table of tests/vcf_joint_reference.py itself (before it judges the engine in tests/test_gpu_vcf_joint.py), the premise of
the feature on a hand-built trio (marginal calls that no transmission allows, a unique joint optimum), the two new
symbols under an unchanged ABI version, the register-resident kernels read from the built gfx950 code object, and the
CLI's flag errors on the CPU driver."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from oracle_binding import Oracle
from test_cpu_kernel_resources import _resources
from vcf_joint_reference import PLANTED_TRIO, PLANTED_TRIO_07, PLANTED_TRIO_OWN_AF, JointFamilies, make_case, transmission, trio_block
from vcf_phase_reference import large_nuclear_case, trio_pedigree
from vcf_posterior_reference import Families

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]
SYMBOLS = ["pm_engine_set_vcf_joint", "pm_engine_vcf_joint"]
VJ_KERNELS = [
    "k_vcf_joint_lean(DevArgs, VjArgs)",
    "k_vcf_joint_nuc(DevArgs, VjArgs)",
    "void k_vcf_joint_es<true>(DevArgs, VjArgs)",     # peel workspace in LDS
    "void k_vcf_joint_es<false>(DevArgs, VjArgs)",    # ... in HBM
]


def _case(tmp_path, shape, nfam):
    """(owner, view, block, refalt): the view's arrays live as long as the owner does."""
    if shape == "nuclear":
        ped, block, refalt = large_nuclear_case()
        return ped, ped, block, refalt
    ped, block, refalt = make_case(str(tmp_path), shape, nfam)
    return ped, ped.view, block, refalt


def test_symbols_and_methods(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbols
    raw = C.CDLL(pm.LIB_PATH)
    for s in SYMBOLS:
        assert s in pm.engine.EXPORTS and hasattr(raw, s), s
    assert callable(getattr(pm.Engine, "set_vcf_joint")) and callable(getattr(pm.Engine, "vcf_joint"))

    class Row(C.Structure):   # pm_vcf_joint
        _fields_ = [("lp", C.c_float), ("g", C.c_uint8), ("pad", C.c_uint8 * 3)]
    assert C.sizeof(Row) == 8 == pm.VCF_JOINT_DTYPE.itemsize and C.alignment(Row) == 4
    assert pm.VCF_JOINT_DTYPE.fields["lp"][1] == Row.lp.offset == 0 and pm.VCF_JOINT_DTYPE.fields["g"][1] == Row.g.offset == 4


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("ext10", 3), ("nuclear", 0)])
def test_table_marginals_are_the_posterior_reference(built, tmp_path, shape, nfam):
    """The table is the distribution behind the posterior plane: its marginals equal tests/vcf_posterior_reference.py's
    posteriors (itself held to the oracle by tests/test_cpu_vcf_posteriors.py) to 1e-12, at the oracle's af; its maximum is
    attained, never above L, and evaluate() at the argmax returns it."""
    ped, view, block, refalt = _case(tmp_path, shape, nfam)
    ora = Oracle(view, pm.Params.defaults(vcf_mode=1))
    ores, ocalls = ora.run(block, np.zeros(block.shape[:2], np.uint32), refalt)
    assert (ores["emit"] == 1).all() and len(ocalls) == len(refalt)   # every site of these blocks is written
    fams = JointFamilies(view)
    sol = fams.solve(block, refalt, ores["af"])
    post = Families(view).posteriors(block, refalt, ores["af"])
    g = np.zeros((len(refalt), fams.n_person), np.int64)
    worst = 0.0
    for F, r in zip(fams.fams, sol):
        sl = slice(F["p0"], F["p0"] + F["m"])
        worst = max(worst, np.abs(r["marg"] - post[:, sl]).max())
        assert (r["max"] > 0).all() and (r["max"] <= r["L"]).all() and (r["n_best"] >= 1).all()
        assert (r["second"] < r["max"]).all()
        g[:, sl] = r["argmax"]
    print(f"{shape} {nfam}: max |table marginal - posterior reference| = {worst:.3g}")
    assert worst <= 1e-12
    J = fams.evaluate(block, refalt, ores["af"], g)
    assert (J == np.stack([r["max"] for r in sol], axis=1)).all()
    assert fams.mendel_consistent(g).all()


@pytest.mark.parametrize("freq,trio,marginal_calls,joint_calls", [
    (0.95, PLANTED_TRIO, (0, 0, 1), (0, 1, 1)),
    (0.7, PLANTED_TRIO_07, (0, 0, 1), (2, 0, 1)),       # (PLANTED_TRIO fails the premise at 0.7: see below)
    (0.8, PLANTED_TRIO_OWN_AF, (0, 0, 1), (0, 1, 1)),   # tests/test_gpu_vcf_joint.py plants it at the engine's own af
])
def test_planted_trio_has_inconsistent_marginal_calls_and_a_unique_joint_optimum(freq, trio, marginal_calls, joint_calls):
    """The premise of the feature, asserted: at this frequency the trio's marginal argmaxes form a trio with T = 0, while
    the table's argmax is unique, Mendelian-consistent, and its runner-up has at most 0.8 of its mass.  The first trio
    holds it at 0.95 and not at 0.7, where its marginal calls are (1/1, 0/0, 0/1): the trio for 0.7 comes from a search."""
    ped = trio_pedigree(2)
    fams = JointFamilies(ped)
    block, refalt = trio_block(*trio, 2)
    sol = fams.solve(block, refalt, np.array([freq]))
    T = transmission()
    for r in sol:
        marginal = r["marg"][0].argmax(axis=1)
        assert tuple(marginal) == marginal_calls and T[marginal[0], marginal[1], marginal[2]] == 0, marginal
        best = r["argmax"][0]
        assert r["n_best"][0] == 1 and tuple(best) == joint_calls and T[best[0], best[1], best[2]] > 0, best
        ratio = r["second"][0] / r["max"][0]
        print(f"freq {freq}: joint optimum {r['max'][0] / r['L'][0]:.3f} of the mass, runner-up / best = {ratio:.3f}")
        assert ratio <= 0.8, ratio
    g = np.array([marginal_calls * 2])
    assert not fams.mendel_consistent(g).any() and (fams.evaluate(block, refalt, np.array([freq]), g) == 0).all()


def test_the_first_planted_trio_is_consistent_at_0_7():
    fams = JointFamilies(trio_pedigree(2))
    block, refalt = trio_block(*PLANTED_TRIO, 2)
    r = fams.solve(block, refalt, np.array([0.7]))[0]
    assert tuple(r["marg"][0].argmax(axis=1)) == (2, 0, 1) == tuple(r["argmax"][0])


def test_vcf_joint_kernels_do_not_spill():
    res = _resources()
    for k in VJ_KERNELS:
        assert k in res, [n for n in res if "vcf_joint" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])


def test_cli_argument_errors(cpu_driver, tmp_path):
    """Raised while the command line is parsed: before the pedigree is read or an evaluator made."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out), "-g", "test.gif", "--vcf_joint"], cwd=EXAMPLE, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and "--vcf_joint needs --in_vcf" in r.stdout, r.stdout[-1000:]
    assert not out.exists()


def test_cpu_evaluator_refuses_the_flag(cpu_driver, tmp_path):
    """The host driver on another evaluator (the CPU oracle's) ends with the SiteEvaluator default's message."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out), "--in_vcf", "testvcf.in.vcf.gz", "--vcf_joint"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--vcf_joint is not supported by this evaluator" in r.stdout, r.stdout[-1000:]
