"""Device-free checks of the families and children behind each DQ on chrX (pm_engine_set_vcf_denovo_chrx_detail,
--vcf_denovo_chrX_detail): the new symbol under an unchanged ABI version, the Python method, the CLI's argument errors
(raised while the command line is parsed), the CPU driver's refusal of the flag, the k_vdn_who_x kernels read from the
built gfx950 code object -- and the numpy reference tests/test_gpu_vcf_denovo_chrx_detail.py judges the engine with
(tests/chrx_detail_reference.py), pinned here before it judges anything: with the autosomal tables substituted it
reproduces the CPU oracle's family terms and child posteriors; with identity mutation matrices it has no mutation term;
its family terms sum to the chrX reference's DQ; and it sees its own planted events.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import polymutt_amd as pm
from chrx_detail_reference import SiteDetail, autosomal_tables, chrx_tables
from chrx_reference import Pedigree as RefPedigree, allele_mut_matrix, three
from conftest import EXAMPLE
from oracle_binding import Oracle
from parity import LLK_RTOL
from test_cpu_kernel_resources import _resources
from test_gpu_denovo_carriers import MaskedOracle
from test_gpu_vcf_denovo import _arrays, dataset as auto_dataset, oracle_view
from test_gpu_vcf_denovo_chrx import dataset as x_dataset, mutation_matrices
from test_gpu_vcf_denovo_detail import check_child as check_child_oracle, oracle_family_terms

BASE = ["-p", "test.ped", "-d", "test.dat", "--out_vcf"]
IN_VCF = ["--in_vcf", "testvcf.in.vcf.gz", "--chrX", "1"]
WHO_X_KERNELS = ["void k_vdn_who_x<64>(DevArgs, VdnXArgs, VdnWhoArgs)", "void k_vdn_who_x<256>(DevArgs, VdnXArgs, VdnWhoArgs)"]
X_CASES = [("trio", 3, 96), ("quad", 5, 96), ("mixed", 31, 96), ("ext10", 1, 96), ("roof", 3, 96), ("extmix", 5, 96),
           ("roof2", 1, 96), ("trio", 129, 16)]


def test_symbol_and_method(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbol
    assert "pm_engine_set_vcf_denovo_chrx_detail" in pm.engine.EXPORTS
    assert hasattr(C.CDLL(pm.LIB_PATH), "pm_engine_set_vcf_denovo_chrx_detail")
    assert callable(getattr(pm.Engine, "set_vcf_denovo_chrx_detail"))


@pytest.mark.parametrize("extra,message", [
    (["--vcf_denovo", "--vcf_denovo_families", "2", "--vcf_denovo_chrX_detail"], "--vcf_denovo_chrX_detail needs --vcf_denovo_chrX"),
    (["--vcf_denovo", "--vcf_denovo_carriers", "2", "--vcf_denovo_chrX_detail"], "--vcf_denovo_chrX_detail needs --vcf_denovo_chrX"),
    (["--vcf_denovo", "--vcf_denovo_chrX", "--vcf_denovo_chrX_detail"],
     "--vcf_denovo_chrX_detail needs --vcf_denovo_families and / or --vcf_denovo_carriers"),
    (["--vcf_denovo_chrX_detail"], "--vcf_denovo_chrX_detail needs --vcf_denovo_chrX"),
])
def test_cli_argument_errors(built, tmp_path, extra, message):
    """Raised while the command line is parsed: before the pedigree is read or an engine created (no GPU here)."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([pm.BIN_PATH] + BASE + [str(out)] + IN_VCF + extra, cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout[-1000:] + r.stderr[-1000:]
    assert "FATAL ERROR" in r.stdout and message in r.stdout, r.stdout[-1000:]
    assert not out.exists()


def test_cpu_evaluator_refuses_the_flag(cpu_driver, tmp_path):
    """The host driver on another evaluator (the CPU oracle's) ends with a SiteEvaluator default's message."""
    out = tmp_path / "out.vcf"
    r = subprocess.run([cpu_driver] + BASE + [str(out)] + IN_VCF + ["--vcf_denovo", "--vcf_denovo_chrX", "--vcf_denovo_families", "2",
                                                                    "--vcf_denovo_chrX_detail"],
                       cwd=EXAMPLE, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not supported by this evaluator" in r.stdout, r.stdout[-1000:]


def test_who_x_kernels_do_not_spill():
    res = _resources()
    for k in WHO_X_KERNELS:
        assert k in res, [n for n in res if "vdn" in n]
        assert int(res[k]["private_segment_fixed_size"]) == 0, (k, res[k])


# ------------------------------------------------------------------------------------------------
# the reference, pinned

@pytest.mark.parametrize("shape,nfam", [("ext10", 1), ("roof2", 1)])
def test_reference_with_autosomal_tables_matches_oracle(built, tmp_path_factory, shape, nfam):
    """One T, M3, Hardy-Weinberg for every founder and the autosomal Mendelian masks substituted: the reference's family
    terms and child posteriors are the CPU oracle's, within the bounds of tests/test_gpu_vcf_denovo_detail.py (the
    blank-family differences of oracle_family_terms, the masked oracle of its check_child)."""
    ped, block, refalt, planted, ov = auto_dataset(tmp_path_factory, shape, nfam)
    view, keep = oracle_view(ped)
    par = pm.Params.defaults(vcf_mode=1)
    ora = Oracle(view, par)
    M, _ = mutation_matrices(ped, par)
    rp = RefPedigree(ped.view)
    fs, _ = _arrays(ped)
    worst_f = worst_c = 0.0
    n_pos = 0
    for i in planted[:6] + [1, 95]:
        a1, a2, g = three(refalt[i])
        site = np.ascontiguousarray(block[i])
        xN, xD = float(ov[i, 1]), float(ov[i, 4])
        sd = SiteDetail(rp, site, refalt[i], autosomal_tables(M, refalt[i]))
        D, mag = sd.family_terms(xN, xD)
        exp, omag = oracle_family_terms(ora, fs, site, a1, a2, xN, xD)
        err, bnd = np.abs(D - exp), LLK_RTOL * omag + 1e-10
        worst_f = max(worst_f, float((err / bnd).max()))
        assert (err <= bnd).all(), (shape, i, D, exp)
        Mo = MaskedOracle(ora, site, a1, a2, xN)
        for f, (p0, n, founders, kids) in enumerate(rp.fams):
            for c, fa, mo, male, mutates in kids:
                ref = sd.child(f, c, xN)
                ev = sd.event_glf(ref["event"])
                entry = {"pp": ref["pp"], "fa_g": ev[0], "mo_g": ev[1], "kid_g": ev[2]}
                worst_c = max(worst_c, check_child_oracle(Mo, g, p0 + c, p0 + fa, p0 + mo, entry))
                n_pos += ref["pp"] > 0.5
                if not mutates:
                    assert ref["pp"] == 0.0 and ref["event"] == (-1, -1, -1)
    print(f"{shape}/{nfam}: worst family error / bound = {worst_f:.3g}, worst child error / bound = {worst_c:.3g}, "
          f"{n_pos} children with pp > 0.5")
    assert n_pos >= 2
    del ora, keep


@pytest.mark.parametrize("shape,nfam,nsites", [("mixed", 31, 96), ("roof2", 1, 96)])
def test_identity_mutation_gives_no_mutation_term(built, tmp_path_factory, shape, nfam, nsites):
    """With identity mutation matrices every pp is exactly 0 and every D_f is the difference of the standard factor at
    the two frequencies."""
    ped, block, refalt, planted, rv, models = x_dataset(tmp_path_factory, shape, nfam, nsites)
    rp = RefPedigree(ped.view)
    M, A4 = np.eye(10).ravel(), np.eye(4)
    for i in (planted[0], 1):
        sd = SiteDetail(rp, block[i], refalt[i], chrx_tables(M, A4, refalt[i]))
        D, _ = sd.family_terms(0.3, 0.6)
        for f, (p0, n, founders, kids) in enumerate(rp.fams):
            assert D[f] == sd.family_log10(f, 0.3, False) - sd.family_log10(f, 0.6, False), (shape, i, f)
            for c, fa, mo, male, mutates in kids:
                ref = sd.child(f, c, 0.3)
                assert ref["pp"] == 0.0 and ref["event"] == (-1, -1, -1), (shape, i, f, c, ref)


@pytest.mark.parametrize("shape,nfam,nsites", X_CASES)
def test_reference_sees_its_plants(built, tmp_path_factory, shape, nfam, nsites):
    """Sum_f D_f = N(x_N) - D(x_D) of the chrX reference within LLK_RTOL (|N| + |D|); the case has sites with DQ > 0 and
    planted sites with DQ > 3, on which the planted child is first with pp > 0.99; roof2's plain-T plants have pp = 0."""
    ped, block, refalt, planted, rv, models = x_dataset(tmp_path_factory, shape, nfam, nsites)
    par = pm.Params.defaults(vcf_mode=1)
    M, A4 = mutation_matrices(ped, par)
    assert np.array_equal(A4, allele_mut_matrix(par.denovo_mut_rate, par.denovo_tstv))
    rp = RefPedigree(ped.view)
    fs, fo = _arrays(ped)
    fam0 = next(f for f in range(len(fs) - 1) if not fo[fs[f]:fs[f + 1]].all())
    pk = [p for p in range(fs[fam0], fs[fam0 + 1]) if not fo[p]]
    mutates = {rp.fams[fam0][0] + k[0]: k[4] for k in rp.fams[fam0][3]}
    dq = rv[:, 0] - rv[:, 2]
    few = nsites == 16
    assert int((dq > 0).sum()) >= (2 if few else 8), (shape, nfam, dq)
    strong = [i for i in planted if dq[i] > 3]
    assert len(strong) >= (2 if few else 4), (shape, nfam, dq[planted])
    worst, smallest, n_plain = 0.0, 1.0, 0
    for i in planted:
        sd = SiteDetail(rp, block[i], refalt[i], chrx_tables(M, A4, refalt[i]))
        xN, xD = float(rv[i, 1]), float(rv[i, 3])
        D, _ = sd.family_terms(xN, xD)
        N, Dstd = models[i].loglik(xN, True), models[i].loglik(xD, False)
        bound = LLK_RTOL * (abs(N) + abs(Dstd))
        worst = max(worst, abs(D.sum() - (N - Dstd)) / bound)
        assert abs(D.sum() - (N - Dstd)) <= bound, (shape, nfam, i, D.sum(), N - Dstd)
        child = pk[(i // 8) % len(pk)]
        if not mutates[child]:
            assert sd.child(fam0, child - fs[fam0], xN)["pp"] == 0.0, (shape, nfam, i, child)
            n_plain += 1
        if i not in strong:
            continue
        assert mutates[child]
        pps = {p: sd.child(fam0, p - fs[fam0], xN)["pp"] for p in pk}
        assert max(pps, key=lambda p: (pps[p], -p)) == child and pps[child] > 0.99, (shape, nfam, i, child, pps)
        assert int(np.argmax(D)) == fam0
        smallest = min(smallest, pps[child])
    print(f"{shape}/{nfam}: {int((dq > 0).sum())} sites with DQ > 0, {len(strong)} planted with DQ > 3 of {len(planted)}, smallest planted "
          f"pp = {smallest:.4f}, {n_plain} plain-T plants with pp = 0, worst |sum - DQ| / bound = {worst:.3g}")
    if shape == "roof2":
        assert n_plain == 2
