"""Device-free checks of the genotype posterior plane of the --in_vcf path (pm_engine_set_vcf_posteriors,
--vcf_posteriors): the two new symbols under an unchanged ABI version, the Python methods, the CLI's argument error
(raised while the command line is parsed), the CPU driver's refusal of the flag, the three register-resident kernels read
from the built gfx950 code object, and the numpy reference of tests/vcf_posterior_reference.py against the unchanged CPU
oracle -- which validates the reference before it judges the engine (tests/test_gpu_vcf_posteriors.py)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from oracle_binding import Oracle
from parity import DOSE_ATOL, _nonfinite_problem
from test_cpu_kernel_resources import _resources

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]
SYMBOLS = ["pm_engine_set_vcf_posteriors", "pm_engine_vcf_posteriors"]
VP_KERNELS = [
    "k_vcf_post_lean(DevArgs, VpArgs)",
    "k_vcf_post_nuc(DevArgs, VpArgs)",
    "void k_vcf_post_es<true>(DevArgs, VpArgs)",     # peel workspace in LDS
    "void k_vcf_post_es<false>(DevArgs, VpArgs)",    # ... in HBM
]
# multi-family pedigrees on an autosome (the reference's domain): two family sizes in one wave, more than 64 families,
# founders only, peeled families alone, one family of each of the five peel schedules
CASES = [("mixed", 31), ("quad", 70), ("single", 12), ("ext10", 3), ("extmix", 5)]


def test_symbols_and_methods(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbols
    raw = C.CDLL(pm.LIB_PATH)
    for s in SYMBOLS:
        assert s in pm.engine.EXPORTS and hasattr(raw, s), s
    assert callable(getattr(pm.Engine, "set_vcf_posteriors")) and callable(getattr(pm.Engine, "vcf_posteriors"))

    class Row(C.Structure):   # pm_vcf_post
        _fields_ = [("p", C.c_float * 3)]
    assert C.sizeof(Row) == 12 == pm.VCF_POST_DTYPE.itemsize and C.alignment(Row) == 4


def test_cli_argument_error(built, tmp_path):
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + BASE + [str(out), "-g", "test.gif", "--vcf_posteriors"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and "--vcf_posteriors needs --in_vcf" in r.stdout, r.stdout[-1000:]
    assert not out.exists()


def test_cpu_evaluator_refuses_the_flag(cpu_driver, tmp_path):
    """The host driver on another evaluator (the CPU oracle's) ends with the SiteEvaluator default's message."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out), "--in_vcf", "testvcf.in.vcf.gz", "--vcf_posteriors"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not supported by this evaluator" in r.stdout, r.stdout[-1000:]


def test_vcf_posterior_kernels_do_not_spill():
    res = _resources()
    for k in VP_KERNELS:
        assert k in res, [n for n in res if "vcf_post" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])


@pytest.mark.parametrize("shape,nfam", CASES)
def test_reference_matches_oracle(built, tmp_path, shape, nfam):
    """The numpy reference at the oracle's own af: its dosage p[1] + 2 p[2] is the oracle's to DOSE_ATOL on every person
    of every site, and its argmax the oracle's best wherever the two largest values differ by more than 1e-9."""
    from vcf_posterior_reference import Families, make_case
    ped, block, refalt = make_case(str(tmp_path), shape, nfam)
    par = pm.Params.defaults(vcf_mode=1)
    ora = Oracle(ped.view, par)
    ores, ocalls = ora.run(block, np.zeros(block.shape[:2], np.uint32), refalt)
    assert (ores["emit"] == 1).all() and len(ocalls) == len(refalt)   # every site of these blocks is written
    fams = Families(ped.view)
    post = fams.posteriors(block, refalt, ores["af"])
    ds = post[..., 1] + 2 * post[..., 2]
    problems = []
    _nonfinite_problem("dosage", ds, ocalls["dosage"], problems)
    assert not problems, problems
    d = np.abs(ds - ocalls["dosage"])
    print(f"{shape} {nfam}: max |DS - oracle| = {d.max():.3g}")
    assert (d <= DOSE_ATOL).all(), (d.max(), np.argwhere(d > DOSE_ATOL)[:5])
    top = np.sort(post, axis=-1)
    clear = top[..., 2] - top[..., 1] > 1e-9
    assert clear.any()
    assert np.array_equal(post.argmax(axis=-1)[clear], ocalls["best"][clear].astype(np.int64))
