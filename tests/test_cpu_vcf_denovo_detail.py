"""Device-free checks of the families and children behind each DQ of --vcf_denovo (pm_engine_set_vcf_denovo_detail): the
new symbols under an unchanged ABI version, the Python methods, the CLI's argument errors (raised while the command line
is parsed), the CPU driver's refusal of the flags, the new kernels read from the built gfx950 code object, and the
oracle-only identities the GPU checks of tests/test_gpu_vcf_denovo_detail.py rest on."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
from oracle_binding import Oracle
from parity import LLK_RTOL
from test_cpu_kernel_resources import _resources
from test_gpu_vcf_denovo import CASES, _arrays, _three, dataset, oracle_view

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]
IN_VCF = ["--in_vcf", "testvcf.in.vcf.gz"]
SYMBOLS = ["pm_engine_set_vcf_denovo_detail", "pm_engine_vcf_denovo_rows", "pm_engine_vcf_denovo_families",
           "pm_engine_vcf_denovo_carriers"]
METHODS = ["set_vcf_denovo_detail", "vcf_denovo_rows", "vcf_denovo_families", "vcf_denovo_carriers"]
WHO_KERNELS = [
    "k_vdn_rows(DevArgs, int*)",
    "void k_vdn_who<64>(DevArgs, VdnArgs, VdnWhoArgs)",
    "void k_vdn_who<256>(DevArgs, VdnArgs, VdnWhoArgs)",
]


def test_symbols_and_methods(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbols
    raw = C.CDLL(pm.LIB_PATH)
    for s in SYMBOLS:
        assert s in pm.engine.EXPORTS and hasattr(raw, s), s
    for m in METHODS:
        assert callable(getattr(pm.Engine, m)), m


@pytest.mark.parametrize("extra,message", [
    (IN_VCF + ["--vcf_denovo_families", "2"], "--vcf_denovo_families needs --vcf_denovo"),
    (IN_VCF + ["--vcf_denovo_carriers", "2"], "--vcf_denovo_carriers needs --vcf_denovo"),
    (IN_VCF + ["--vcf_denovo", "--vcf_denovo_families", "0"], "--vcf_denovo_families takes a family count from 1 to 8"),
    (IN_VCF + ["--vcf_denovo", "--vcf_denovo_families", "9"], "--vcf_denovo_families takes a family count from 1 to 8"),
    (IN_VCF + ["--vcf_denovo", "--vcf_denovo_carriers", "0"], "--vcf_denovo_carriers takes a person count from 1 to 8"),
    (IN_VCF + ["--vcf_denovo", "--vcf_denovo_carriers", "9"], "--vcf_denovo_carriers takes a person count from 1 to 8"),
])
def test_cli_argument_errors(built, tmp_path, extra, message):
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + BASE + [str(out)] + extra, cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and message in r.stdout, r.stdout[-1000:]
    assert not out.exists()


@pytest.mark.parametrize("flag", ["--vcf_denovo_families", "--vcf_denovo_carriers"])
def test_cpu_evaluator_refuses_the_flags(cpu_driver, tmp_path, flag):
    """The host driver on another evaluator (the CPU oracle's) ends with a SiteEvaluator default's message."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out)] + IN_VCF + ["--vcf_denovo", flag, "2"], cwd=EXAMPLE,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not supported by this evaluator" in r.stdout, r.stdout[-1000:]


def test_who_kernels_do_not_spill():
    res = _resources()
    for k in WHO_KERNELS:
        assert k in res, [n for n in res if "vdn" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])


# ------------------------------------------------------------------------------------------------
# the oracle-only identities (vcf_mode oracle, 255-filled blocks, oracle_view)

def _oracle(ped):
    view, keep = oracle_view(ped)
    return Oracle(view, pm.Params.defaults(vcf_mode=1)), keep


@pytest.mark.parametrize("shape,nfam", CASES)
def test_blank_block_contributes_nothing(built, tmp_path_factory, shape, nfam):
    """An all-zero block gives |objective| <= 1e-12 under both models: a blanked family drops out of a difference."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    ora, keep = _oracle(ped)
    blank = np.zeros((ped.n_person, 10), np.uint8)
    for dn in (0, 1):
        for x in (0.3, 0.9999):
            v = ora.objective(blank, 1, 3, x, dn)
            assert abs(v) <= 1e-12, (shape, nfam, dn, x, v)


@pytest.mark.parametrize("shape,nfam", [c for c in CASES if c[0] != "single"])
def test_three_state_joint_closes(built, tmp_path_factory, shape, nfam):
    """For a child, the joint over (father a, mother b, child s) in the three states of (ref, alt) sums to 1 within 1e-12:
    the masked oracle (a clamp sets the person's disallowed bytes among the three planes to 255) is a probability."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    ora, keep = _oracle(ped)
    v = ped.view
    fa = np.ctypeslib.as_array(v.father, shape=(v.n_person,))
    mo = np.ctypeslib.as_array(v.mother, shape=(v.n_person,))
    kids = [p for p in range(v.n_person) if fa[p] >= 0 and mo[p] >= 0]
    assert kids
    worst = 0.0
    for i in (planted[0], planted[0] + 1):
        a1, a2, g = _three(refalt[i])
        site = np.ascontiguousarray(block[i])
        full = ora.objective(site, a1, a2, float(ov[i, 1]), 1)
        for c in (kids[0], kids[-1]):
            tot = 0.0
            for a in range(3):
                for b in range(3):
                    for s in range(3):
                        cut = site.copy()
                        for p, st in ((fa[c], a), (mo[c], b), (c, s)):
                            for t in range(3):
                                if t != st:
                                    cut[p, g[t]] = 255
                        tot += 10.0 ** (full - ora.objective(cut, a1, a2, float(ov[i, 1]), 1))
            worst = max(worst, abs(tot - 1.0))
            assert abs(tot - 1.0) <= 1e-12, (shape, nfam, i, c, tot)
    print(f"{shape}/{nfam}: max |joint - 1| = {worst:.3g}")


@pytest.mark.parametrize("shape,nfam", CASES)
def test_family_differences_sum_to_dq(built, tmp_path_factory, shape, nfam):
    """Sum_f of the blank-family differences equals N_o - D_o within LLK_RTOL (|N_o| + |D_o|)."""
    ped, block, refalt, planted, ov = dataset(tmp_path_factory, shape, nfam)
    ora, keep = _oracle(ped)
    fs, _ = _arrays(ped)
    sites = (planted[:1] if len(planted) else []) + [1, 95]
    worst = 0.0
    for i in sites:
        a1, a2, _ = _three(refalt[i])
        site = np.ascontiguousarray(block[i])
        No, xN, Do, xD = ov[i, 0], float(ov[i, 1]), ov[i, 3], float(ov[i, 4])
        full_dn, full_std = ora.objective(site, a1, a2, xN, 1), ora.objective(site, a1, a2, xD, 0)
        tot = 0.0
        for f in range(len(fs) - 1):
            cut = site.copy()
            cut[fs[f]:fs[f + 1]] = 0
            tot += (ora.objective(cut, a1, a2, xN, 1) - full_dn) - (ora.objective(cut, a1, a2, xD, 0) - full_std)
        bound = LLK_RTOL * (abs(No) + abs(Do))
        worst = max(worst, abs(tot - (No - Do)) / bound)
        assert abs(tot - (No - Do)) <= bound, (shape, nfam, i, tot, No - Do, bound)
    print(f"{shape}/{nfam}: worst |sum - DQ| / bound = {worst:.3g}")
