"""An independent numpy reference for the transmission phase plane of the --in_vcf path (pm_engine_set_vcf_phase,
include/polymutt_engine.h) -- TEST INFRASTRUCTURE ONLY.

tests/vcf_posterior_reference.py's joint sum, with one change: for the child c whose phase is asked, the state axis of
its three unordered genotypes is replaced by the four ordered ones (paternal allele | maternal allele)
    a1|a1, a1|a2, a2|a1, a2|a2
with the likelihoods (l11, l12, l12, l22), the transmission into c
    tau_a(paternal allele) x tau_b(maternal allele),   tau_0 = (1, 0), tau_1 = (1/2, 1/2), tau_2 = (0, 1)
from a father in state a and a mother in state b, and, for every child of c, the usual transmission read through c's
unordered genotype.  p12 and p21 are the two middle marginals over the total.  No peeling and no weight shortcut: the
sum is an einsum contraction over every member's state index.

Like the posterior reference it covers autosomal sections of pedigrees with more than one family (Hardy-Weinberg priors
everywhere); the single-family prior mode is pinned through the posterior plane (p12 + p21 = p[1]).
"""
import numpy as np

import polymutt_amd as pm
from vcf_posterior_reference import make_case, three, transmission  # noqa: F401  (make_case: re-exported for the tests)

MALE, FEMALE = 1, 2
UNORDERED = [0, 1, 1, 2]   # ordered state -> unordered genotype


def ordered_transmission():
    """T4[father][mother][ordered child]: the father's allele times the mother's."""
    tau = {0: (1.0, 0.0), 1: (0.5, 0.5), 2: (0.0, 1.0)}   # state -> P(passes a1), P(passes a2)
    T4 = np.zeros((3, 3, 4))
    for a in range(3):
        for b in range(3):
            for p in range(2):
                for m in range(2):
                    T4[a, b, 2 * p + m] = tau[a][p] * tau[b][m]
    return T4


class PhaseFamilies:
    """Per family of a pm_pedigree view: its persons, founders and each non-founder's parents (family-local)."""

    def __init__(self, view):
        nf, n = view.n_fam, view.n_person
        as_arr = np.ctypeslib.as_array
        self.n_person = n
        fam_start = as_arr(view.fam_start, shape=(nf + 1,)).copy()
        self.is_founder = as_arr(view.is_founder, shape=(n,)).copy().astype(bool)
        father = as_arr(view.father, shape=(n,)).copy()
        mother = as_arr(view.mother, shape=(n,)).copy()
        self.fams = []
        self._paths = {}
        for f in range(nf):
            p0, p1 = int(fam_start[f]), int(fam_start[f + 1])
            m = p1 - p0
            assert m <= 26, "one einsum letter per member"
            founders = [i for i in range(m) if self.is_founder[p0 + i]]
            kids = [(i, int(father[p0 + i]) - p0, int(mother[p0 + i]) - p0) for i in range(m) if not self.is_founder[p0 + i]]
            for i, fa, mo in kids:
                assert 0 <= fa < m and 0 <= mo < m and fa != mo, "a non-founder has both parents in its family"
            letters = [chr(ord("a") + i) for i in range(m)]
            subs = ",".join(["Z" + c for c in letters] + [letters[fa] + letters[mo] + letters[i] for i, fa, mo in kids])
            self.fams.append({"p0": p0, "m": m, "founders": founders, "kids": kids, "subs": subs, "letters": letters})

    def _path(self, F, c, ops):
        key = (F["subs"], c)
        if key not in self._paths:
            dummy = [np.ones((2,) + o.shape[1:]) for o in ops[:F["m"]]] + list(ops[F["m"]:])
            self._paths[key] = np.einsum_path(F["subs"] + "->Z" + F["letters"][c], *dummy, optimize="greedy")[0]
        return self._paths[key]

    def phase(self, block, refalt, af):
        """[n, n_person, 2] = (p12, p21): block [n, n_person, 10] phred bytes, refalt [n], af [n] the frequency of the
        reference allele at each site.  Founders are (0, 0), and so is a person whose total is zero."""
        n = len(refalt)
        g = np.array([three(r) for r in refalt])
        lk = 10.0 ** (-np.take_along_axis(np.asarray(block), g[:, None, :], axis=2).astype(np.float64) / 10.0)   # [n, np, 3]
        f = np.asarray(af, dtype=np.float64)
        prior = np.stack([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)], axis=1)                                     # [n, 3]
        T, T4 = transmission(), ordered_transmission()
        out = np.zeros((n, self.n_person, 2))
        for F in self.fams:
            vec = [lk[:, F["p0"] + i] * (prior if i in F["founders"] else 1.0) for i in range(F["m"])]
            for c, _, _ in F["kids"]:
                ops = list(vec)
                ops[c] = vec[c][:, UNORDERED]   # (l11, l12, l12, l22): c is no founder, so no prior rides along
                for i, fa, mo in F["kids"]:
                    if i == c:
                        ops.append(T4)
                    elif fa == c:
                        ops.append(T[UNORDERED, :, :])
                    elif mo == c:
                        ops.append(T[:, UNORDERED, :])
                    else:
                        ops.append(T)
                marg = np.einsum(F["subs"] + "->Z" + F["letters"][c], *ops, optimize=self._path(F, c, ops))   # [n, 4]
                s = marg.sum(axis=1, keepdims=True)
                q = np.divide(marg, s, out=np.zeros_like(marg), where=s != 0)
                out[:, F["p0"] + c, 0] = q[:, 1]
                out[:, F["p0"] + c, 1] = q[:, 2]
        return out


def large_nuclear_case(nsites=96):
    """(ped, block, refalt): the nuclear 5/3/6/4/5 pedigree and sites of
    tests/test_gpu_vcf_posteriors.py::test_gp_large_nuclear_families, built the same way from the same seed -- families of
    three and four children, which the closed form over any number of children takes and no synthetic shape reaches."""
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
    n, npers = nsites, sum(sizes)
    ref_base = rng.integers(1, 5, n).astype(np.uint8)
    refalt = (ref_base | (np.array([{1: 3, 2: 4, 3: 1, 4: 2}[int(r)] for r in ref_base], np.uint8) << 4)).astype(np.uint8)
    block = np.full((n, npers, 10), 255, np.uint8)
    for i in range(n):
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
    block.setflags(write=False)
    return ped, block, refalt


def trio_pedigree(n_trios=2):
    """n_trios father / mother / child families (more than one: Hardy-Weinberg priors, the reference's domain)."""
    sizes = [3] * n_trios
    sex, founder, father, mother = [], [], [], []
    for t in range(n_trios):
        sex += [MALE, FEMALE, MALE]
        founder += [1, 1, 0]
        father += [-1, -1, 3 * t]
        mother += [-1, -1, 3 * t + 1]
    return pm.pedigree_from_arrays(sizes, [2] * n_trios, [pm.FAM_NUCLEAR] * n_trios, sex, founder, father, mother)


def phase_confidence(ph):
    """hi / (lo + hi) of a (p12, p21) array; nan where both are zero."""
    lo, hi = ph.min(axis=-1), ph.max(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(lo + hi > 0, hi / (lo + hi), np.nan)
