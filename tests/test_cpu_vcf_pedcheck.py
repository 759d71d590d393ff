"""CPU tests of the pedigree check of the --in_vcf path: the brute-force reference (tests/vcf_pedcheck_reference.py) against
itself, the conditions the GPU tests rest on, and the public surface (no GPU needed).

* T_fa, T_mo and T_un are distributions over the child's state.
* For a child without descendants L_both = L(the family without it) x lkSinglePerson(it).
* Exchanging the father's and the mother's data exchanges LLR_FATHER and LLR_MOTHER.
* The single-family prior table is what d_parent_prior's default branch holds, and off it is Hardy-Weinberg.
* On every input the GPU tests run the reference counts every row: a GPU test that asserts n cannot hide a skipped row.
* The discrimination data set has its margins in the reference alone.
"""
import ctypes as C
import os

import numpy as np
import pytest

import polymutt_amd as pm
from conftest import EXAMPLE
import vcf_pedcheck_reference as R

TOL = 1e-12   # two orders of the same double sums


def test_symbols_and_bindings(built):
    lib = pm.load_library()
    assert lib.pm_abi_version() == 8   # additive: callers detect the feature by the symbols
    for name in ("pm_engine_set_vcf_pedcheck", "pm_engine_reset_vcf_pedcheck", "pm_engine_vcf_pedcheck"):
        assert name in pm.engine.EXPORTS and hasattr(C.CDLL(pm.LIB_PATH), name)
    for name in ("set_vcf_pedcheck", "reset_vcf_pedcheck", "vcf_pedcheck"):
        assert callable(getattr(pm.Engine, name))
    assert pm.VCF_PEDCHECK_DTYPE.itemsize == 40


def test_alternative_tables_are_distributions():
    f = np.array([0.02, 0.3, 0.5, 0.77, 0.999])
    T = R.transmission()
    for t in R.alt_tables(f):
        assert t.shape == (5, 3, 3, 3) and np.abs(t.sum(axis=3) - 1).max() <= 1e-15
    t_fa, t_mo, t_un = R.alt_tables(f)
    assert (t_fa == t_fa[:, :1]).all() and (t_mo == t_mo[:, :, :1]).all()       # the unrelated parent's state does not matter
    assert np.abs(t_fa - np.swapaxes(t_mo, 1, 2)).max() <= 1e-16                # mirrors of each other
    # a homozygous a1 mother and a population father: the child is a1a1 with probability f, else heterozygous
    assert np.abs(t_fa[:, 0, 0, :] - np.stack([f, 1 - f, 0 * f], axis=1)).max() <= 1e-15
    assert (T.sum(axis=2) == 1).all()


@pytest.fixture(scope="module")
def mixed(built, tmp_path_factory):
    ped = R.write_pedigree(str(tmp_path_factory.mktemp("pc_cpu")), [R.TRIO, R.QUAD_MOTHER_FIRST, R.PAIR, R.GEN3, R.NUC6])
    block, refalt, f = R.simulate(ped.view, 60, 3)
    return ped, block, refalt, f, R.PedcheckFamilies(ped.view).solve(block, refalt, f)


def test_loader_lists_the_quad_mother_first(mixed):
    ped = mixed[0]
    father = np.ctypeslib.as_array(ped.view.father, shape=(ped.n_person,))
    p0 = int(ped.fam_start()[1])
    assert ped.pids()[p0].endswith("a_mo") and father[p0 + 2] == p0 + 1 and father[p0 + 3] == p0 + 1


def test_both_unrelated_factorises(built, mixed, tmp_path_factory):
    """c without descendants: L_both = L(family without c) x Sum_g pi(g) l_c(g), for a trio's child, a quad's, one of four
    and a grandchild."""
    ped, block, refalt, f, ref = mixed
    pids = ped.pids()
    lk = R.likelihoods(block, refalt)
    prior = R.pi_of(f)
    for fam_k, fam, child in ((0, R.TRIO, "c"), (1, R.QUAD_MOTHER_FIRST, "c2"), (4, R.NUC6, "c1"), (3, R.GEN3, "k2")):
        less = [m for m in fam if m[0] != child]
        sub = R.write_pedigree(str(tmp_path_factory.mktemp("pc_less")), [less])
        cols = [pids.index(f"F{fam_k}_{pid.split('_', 1)[1]}") for pid in sub.pids()]
        F = R.PedcheckFamilies(sub.view).fams[0]
        without = R.PedcheckFamilies(sub.view).family_sums(F, lk[:, cols], prior, [R.transmission()] * len(F["kids"]))
        c = pids.index(f"F{fam_k}_{child}")
        single = (prior * lk[:, c]).sum(axis=1)
        k = list(ref["person"]).index(c)
        assert np.abs(ref["L"][k, :, 3] / (without * single) - 1).max() <= TOL, (fam_k, child)


def test_exchanging_the_parents_exchanges_the_two_sums(mixed):
    ped, block, refalt, f, ref = mixed
    fams = R.PedcheckFamilies(ped.view)
    for fam_k in (0, 1, 4):   # the nuclear families: both parents are founders
        p0 = int(ped.fam_start()[fam_k])
        sw = fams.solve(R.swap_columns(block, p0, p0 + 1), refalt, f)
        for k, p in enumerate(ref["person"]):
            inside = p0 <= p < ped.fam_start()[fam_k + 1]
            want = ref["S"][k][[1, 0, 2]] if inside else ref["S"][k]
            assert np.abs(sw["S"][k] - want).max() <= 1e-9, (fam_k, p)
            assert not inside or abs(ref["S"][k, 0] - ref["S"][k, 1]) > 1e-3   # (the exchange is visible)


def test_single_family_prior_mode(built, tmp_path_factory):
    ped = R.write_pedigree(str(tmp_path_factory.mktemp("pc_one")), [R.TRIO])
    block, refalt, f = R.simulate(ped.view, 40, 5)
    fams = R.PedcheckFamilies(ped.view)
    hw = fams.solve(block, refalt, f)
    off = fams.solve(block, refalt, f, trio_prior=np.zeros(40, bool))
    assert np.abs(off["L"] / hw["L"] - 1).max() <= TOL
    on = fams.solve(block, refalt, f, trio_prior=np.ones(40, bool))
    lk = R.likelihoods(block, refalt)
    L0 = np.einsum("za,zb,ab,abk,zk->z", lk[:, 0], lk[:, 1], R.TRIO_PRIOR, R.transmission(), lk[:, 2])
    assert np.abs(on["L"][0, :, 0] / L0 - 1).max() <= TOL
    assert abs(R.TRIO_PRIOR.sum() - 1) <= 1e-15 and (R.TRIO_PRIOR == R.TRIO_PRIOR.T).all()
    assert (on["n"] == 40).all() and np.abs(on["S"] - hw["S"]).max() > 1e-3


def test_quantised_sums_stay_within_the_bound(mixed):
    ref = mixed[4]
    assert (np.abs(ref["q"] * 2.0 ** -28 - ref["S"]) <= ref["n"][:, None] * R.Q_BOUND + 1e-12).all()
    assert R.bound(1) == 2.0 ** -29 + 1e-9


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_reference_counts_every_row_of_the_gpu_inputs(built, tmp_path_factory, name):
    fams, rows, _ = R.SHAPES[name]
    ped = R.write_pedigree(str(tmp_path_factory.mktemp("pc_" + name)), fams)
    block, refalt, f = R.simulate(ped.view, rows, 17)   # (the GPU tests' data; there the frequency is the engine's own)
    for freq in (f, np.full(rows, 0.999), np.full(rows, 0.5)):   # generating, monomorphic rows' 1 - theta, mid
        ref = R.PedcheckFamilies(ped.view).solve(block, refalt, freq)
        assert len(ref["person"]) > 0 and (ref["n"] == rows).all(), name


def test_reference_counts_every_row_of_the_example(built):
    ped, block, refalt = R.example_records(os.path.join(EXAMPLE, "testvcf.in.vcf.gz"))
    n = len(refalt)
    assert n > 8000
    for freq in (0.999, 0.8, 0.3):
        ref = R.PedcheckFamilies(ped.view).solve(block, refalt, np.full(n, freq))
        assert len(ref["person"]) == 6 and (ref["n"] == n).all(), freq


def test_discrimination_margins_in_the_reference(built, tmp_path_factory):
    ped, block, refalt, f = R.discrimination_case(str(tmp_path_factory.mktemp("pc_disc")))
    assert block.shape == (R.DISC_ROWS, 12, 10)
    fams = R.PedcheckFamilies(ped.view)
    kids = list(fams.persons)
    assert kids == [2, 5, 8, 9]
    stated = fams.solve(block, refalt, f)
    assert (stated["n"] == R.DISC_ROWS).all() and (stated["S"] >= 5).all(), stated["S"]
    child = fams.solve(R.swap_columns(block, R.DISC_CHILD, R.DISC_FOUNDER), refalt, f)
    k = kids.index(R.DISC_CHILD)
    assert child["S"][k, 2] <= -5, child["S"][k]
    others = [i for i in range(len(kids)) if i != k]
    assert (child["S"][others] == stated["S"][others]).all()   # every untouched family's values are unchanged
    father = fams.solve(R.swap_columns(block, R.DISC_FATHER, R.DISC_FOUNDER), refalt, f)
    k = kids.index(R.DISC_FATHER_CHILD)
    assert father["S"][k, 0] <= -5 and father["S"][k, 1] >= 5, father["S"][k]
    others = [i for i in range(len(kids)) if i != k]
    assert (father["S"][others] == stated["S"][others]).all()
    assert (father["n"] == R.DISC_ROWS).all() and (child["n"] == R.DISC_ROWS).all()
