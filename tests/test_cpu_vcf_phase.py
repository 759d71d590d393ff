"""Device-free checks of the transmission phase plane of the --in_vcf path (pm_engine_set_vcf_phase, --vcf_phase): the
numpy reference of tests/vcf_phase_reference.py itself (before it judges the engine in tests/test_gpu_vcf_phase.py), that
the GPU cases hold both clearly phased and unphased children, the two new symbols under an unchanged ABI version, the
three register-resident kernels read from the built gfx950 code object, and the CLI's flag errors on the CPU driver."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from oracle_binding import Oracle
from test_cpu_kernel_resources import _resources
from vcf_phase_reference import PhaseFamilies, large_nuclear_case, make_case, phase_confidence, three, trio_pedigree
from vcf_posterior_reference import Families

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]
SYMBOLS = ["pm_engine_set_vcf_phase", "pm_engine_vcf_phase"]
VPH_KERNELS = [
    "k_vcf_phase_lean(DevArgs, VphArgs)",
    "k_vcf_phase_nuc(DevArgs, VphArgs)",
    "void k_vcf_phase_es<true>(DevArgs, VphArgs)",     # peel workspace in LDS
    "void k_vcf_phase_es<false>(DevArgs, VphArgs)",    # ... in HBM
]
# tests/test_gpu_vcf_phase.py's engine cases (96 sites each); "nuclear" is the 5/3/6/4/5 pedigree
GPU_CASES = [("mixed", 31), ("quad", 70), ("single", 12), ("ext10", 3), ("extmix", 5), ("nuclear", 0)]


def _case(tmp_path, shape, nfam):
    """(owner, view, block, refalt): the view's arrays live as long as the owner does."""
    if shape == "nuclear":
        ped, block, refalt = large_nuclear_case()
        return ped, ped, block, refalt
    ped, block, refalt = make_case(str(tmp_path), shape, nfam)
    return ped, ped.view, block, refalt


def _oracle(view, block, refalt):
    ora = Oracle(view, pm.Params.defaults(vcf_mode=1))
    ores, ocalls = ora.run(block, np.zeros(block.shape[:2], np.uint32), refalt)
    assert (ores["emit"] == 1).all() and len(ocalls) == len(refalt)   # every site of these blocks is written
    return ores, ocalls


def test_symbols_and_methods(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbols
    raw = C.CDLL(pm.LIB_PATH)
    for s in SYMBOLS:
        assert s in pm.engine.EXPORTS and hasattr(raw, s), s
    assert callable(getattr(pm.Engine, "set_vcf_phase")) and callable(getattr(pm.Engine, "vcf_phase"))

    class Row(C.Structure):   # pm_vcf_phase
        _fields_ = [("p12", C.c_float), ("p21", C.c_float)]
    assert C.sizeof(Row) == 8 == pm.VCF_PHASE_DTYPE.itemsize and C.alignment(Row) == 4


@pytest.mark.parametrize("shape,nfam", [("mixed", 31), ("ext10", 3), ("extmix", 5)])
def test_reference_sums_to_the_het_posterior(built, tmp_path, shape, nfam):
    """The two ordered het states are the unordered one split: p12 + p21 = p[1] of the posterior reference (itself held
    to the oracle by tests/test_cpu_vcf_posteriors.py) to 1e-12 for every non-founder, at the oracle's af; founders (0, 0)."""
    ped, view, block, refalt = _case(tmp_path, shape, nfam)
    ores, _ = _oracle(view, block, refalt)
    fams = PhaseFamilies(view)
    ph = fams.phase(block, refalt, ores["af"])
    post = Families(view).posteriors(block, refalt, ores["af"])
    assert np.isfinite(ph).all() and (ph >= 0).all() and (ph <= 1).all()
    assert (ph[:, fams.is_founder] == 0).all()
    kids = ~fams.is_founder
    assert kids.any()
    d = np.abs(ph[:, kids].sum(axis=-1) - post[:, kids, 1])
    print(f"{shape} {nfam}: max |p12 + p21 - p[1]| = {d.max():.3g}")
    assert (d <= 1e-12).all(), d.max()


def _trio_block(fa, mo, kid):
    """One site (A ref, G alt) of two identical trios with the given (PL11, PL12, PL22) triples."""
    refalt = np.array([1 | 3 << 4], np.uint8)
    block = np.full((1, 6, 10), 255, np.uint8)
    for t in range(2):
        for j, tri in enumerate((fa, mo, kid)):
            block[0, 3 * t + j, three(refalt[0])] = tri
    return block, refalt


def test_reference_on_hand_built_trios():
    ped = trio_pedigree(2)
    fams = PhaseFamilies(ped)
    hom1, het, hom2, flat = (0, 255, 255), (255, 0, 255), (255, 255, 0), (0, 0, 0)
    af = np.array([0.5])
    ph = fams.phase(*_trio_block(hom1, hom2, flat), af)    # father certain 0/0, mother certain 1/1: a1 from the father
    assert (ph[0, [2, 5], 0] >= 0.999).all() and (ph[0, [2, 5], 1] <= 0.001).all(), ph
    ph = fams.phase(*_trio_block(hom2, hom1, flat), af)    # the mirror case
    assert (ph[0, [2, 5], 1] >= 0.999).all() and (ph[0, [2, 5], 0] <= 0.001).all(), ph
    ph = fams.phase(*_trio_block(het, het, het), af)       # both parents certain het: nothing tells the two orders apart
    assert (ph[0, [2, 5], 0] == ph[0, [2, 5], 1]).all() and (ph[0, [2, 5], 0] > 0.49).all(), ph
    assert (ph[0, [0, 1, 3, 4]] == 0).all()


@pytest.mark.parametrize("shape,nfam", GPU_CASES)
def test_gpu_cases_hold_phased_and_unphased_children(built, tmp_path, shape, nfam):
    """A condition on the data, so that the GPU comparison is not vacuous: at the oracle's af, among the non-founders
    the oracle calls het, at least one has hi / (lo + hi) >= 0.9 and at least one <= 0.6.  (A case that fails gets another
    seed here, not another bound.)  `single` is the founder branch: it has no non-founder, and that is what is checked."""
    ped, view, block, refalt = _case(tmp_path, shape, nfam)
    ores, ocalls = _oracle(view, block, refalt)
    fams = PhaseFamilies(view)
    if shape == "single":
        assert fams.is_founder.all()
        return
    ph = fams.phase(block, refalt, ores["af"])
    het = (ocalls["best"] == 1) & ~fams.is_founder[None, :]
    assert het.any()
    conf = phase_confidence(ph)[het]
    conf = conf[np.isfinite(conf)]
    print(f"{shape} {nfam}: {len(conf)} het non-founders, {(conf >= 0.9).sum()} with hi/(lo+hi) >= 0.9, {(conf <= 0.6).sum()} <= 0.6")
    assert (conf >= 0.9).any() and (conf <= 0.6).any()


def test_vcf_phase_kernels_do_not_spill():
    res = _resources()
    for k in VPH_KERNELS:
        assert k in res, [n for n in res if "vcf_phase" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])


@pytest.mark.parametrize("extra,message", [
    (["-g", "test.gif", "--vcf_phase"], "--vcf_phase needs --in_vcf"),
    (["--in_vcf", "testvcf.in.vcf.gz", "--vcf_phase_minPQ", "20"], "--vcf_phase_minPQ needs --vcf_phase"),
    (["--in_vcf", "testvcf.in.vcf.gz", "--vcf_phase", "--vcf_phase_minPQ", "100"], "--vcf_phase_minPQ takes a quality from 0 to 99"),
    (["--in_vcf", "testvcf.in.vcf.gz", "--vcf_phase", "--vcf_phase_minPQ", "-1"], "--vcf_phase_minPQ takes a quality from 0 to 99"),
])
def test_cli_argument_errors(cpu_driver, tmp_path, extra, message):
    """Raised while the command line is parsed: before the pedigree is read or an evaluator made."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out)] + extra, cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and message in r.stdout, r.stdout[-1000:]
    assert not out.exists()


def test_cpu_evaluator_refuses_the_flag(cpu_driver, tmp_path):
    """The host driver on another evaluator (the CPU oracle's) ends with the SiteEvaluator default's message."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out), "--in_vcf", "testvcf.in.vcf.gz", "--vcf_phase"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--vcf_phase is not supported by this evaluator" in r.stdout, r.stdout[-1000:]
