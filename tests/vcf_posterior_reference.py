"""An independent numpy reference for the genotype posteriors of the --in_vcf path (pm_engine_set_vcf_posteriors,
include/polymutt_engine.h) -- TEST INFRASTRUCTURE ONLY.

The definition, without peeling and without the engine's code: for one family, one site and a frequency f of the
reference allele, the joint sum over every member's three (ref, alt) genotypes of
    Hardy-Weinberg founder priors (f^2, 2 f (1 - f), (1 - f)^2)
  x every member's likelihood 10^(-PL / 10) of that genotype
  x one autosomal Mendelian transmission per non-founder,
marginalised to each member and normalised.  The sum is an einsum contraction over the members' state indices.

It covers autosomal sections of pedigrees with more than one family (Hardy-Weinberg priors everywhere).  Single-family
pedigrees (the fixed single-trio prior) and chrX / chrY / MT sections are pinned by the CPU oracle instead.
"""
import numpy as np

import polymutt_amd as pm
from fixtures import read_dataset
from test_gpu_vcf import _vcf_block
from test_gpu_vcf_denovo import make_block


def gi(b1, b2):
    b1, b2 = min(b1, b2), max(b1, b2)
    return (b1 - 1) * (10 - b1) // 2 + (b2 - b1)


def three(refalt):
    a1, a2 = int(refalt) & 15, int(refalt) >> 4
    return [gi(a1, a1), gi(a1, a2), gi(a2, a2)]


def transmission():
    """T[father][mother][child]: each parent passes one of its two alleles with probability 1/2."""
    passes = {0: (1.0, 0.0), 1: (0.5, 0.5), 2: (0.0, 1.0)}   # state -> P(passes ref), P(passes alt)
    T = np.zeros((3, 3, 3))
    for i in range(3):
        for j in range(3):
            (fr, fa), (mr, ma) = passes[i], passes[j]
            T[i, j, 0] = fr * mr
            T[i, j, 1] = fr * ma + fa * mr
            T[i, j, 2] = fa * ma
    return T


class Families:
    """Per family of a pm_pedigree view: its persons, which are founders, and each non-founder's parents (family-local)."""

    def __init__(self, view):
        nf, n = view.n_fam, view.n_person
        as_arr = np.ctypeslib.as_array
        self.n_person = n
        fam_start = as_arr(view.fam_start, shape=(nf + 1,)).copy()
        is_founder = as_arr(view.is_founder, shape=(n,)).copy()
        father = as_arr(view.father, shape=(n,)).copy()
        mother = as_arr(view.mother, shape=(n,)).copy()
        self.fams = []
        T = transmission()
        for f in range(nf):
            p0, p1 = int(fam_start[f]), int(fam_start[f + 1])
            m = p1 - p0
            assert m <= 26, "one einsum letter per member"
            founders = [i for i in range(m) if is_founder[p0 + i]]
            kids = [(i, int(father[p0 + i]) - p0, int(mother[p0 + i]) - p0) for i in range(m) if not is_founder[p0 + i]]
            for i, fa, mo in kids:
                assert 0 <= fa < m and 0 <= mo < m, "a non-founder has both parents in its family"
            letters = [chr(ord("a") + i) for i in range(m)]
            # operands: one vector per member (prior x likelihood, or the likelihood alone), one T per non-founder
            subs = ["Z" + c for c in letters] + [letters[fa] + letters[mo] + letters[i] for i, fa, mo in kids]
            subs = ",".join(subs)
            dummy = [np.ones((2, 3))] * m + [T] * len(kids)   # (the contraction order per member, found once)
            paths = [np.einsum_path(subs + "->Z" + c, *dummy, optimize="greedy")[0] for c in letters]
            self.fams.append({"p0": p0, "m": m, "founders": founders, "subs": subs, "letters": letters,
                              "trans": [T] * len(kids), "paths": paths})

    def posteriors(self, block, refalt, af):
        """[n, n_person, 3]: block [n, n_person, 10] phred bytes, refalt [n], af [n] the frequency of the reference allele
        at each site.  The sites ride along as a batch index of the contraction (Z); every site is summed on its own."""
        n = len(refalt)
        g = np.array([three(r) for r in refalt])
        lk = 10.0 ** (-np.take_along_axis(np.asarray(block), g[:, None, :], axis=2).astype(np.float64) / 10.0)   # [n, np, 3]
        f = np.asarray(af, dtype=np.float64)
        prior = np.stack([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)], axis=1)                                     # [n, 3]
        out = np.zeros((n, self.n_person, 3))
        for F in self.fams:
            vec = [lk[:, F["p0"] + i] * (prior if i in F["founders"] else 1.0) for i in range(F["m"])]
            ops = vec + F["trans"]
            for i in range(F["m"]):
                marg = np.einsum(F["subs"] + "->Z" + F["letters"][i], *ops, optimize=F["paths"][i])
                s = marg.sum(axis=1, keepdims=True)
                out[:, F["p0"] + i] = np.divide(marg, s, out=np.zeros_like(marg), where=s != 0)
        return out


def make_case(directory, shape, nfam, nsites=96, seed=53):
    """(ped, block [n, n_person, 10], refalt [n]) built as tests/test_gpu_vcf.py and tests/test_gpu_vcf_denovo.py build
    their vcf_mode blocks: a synthetic dataset, a biallelic (ref, alt) per site, the three PLs of that pair with their
    minimum subtracted and a de novo event planted on every 8th site."""
    pm.synth_write_dataset(directory, shape, nfam, nsites, seed)
    ped, secs, _ = read_dataset(directory)
    (label, pos, ref, pl, dm), = secs
    refalt = _vcf_block(pl, ref, 5)
    block, _ = make_block(ped, pl.reshape(len(ref), ped.n_person, 10), refalt)
    block.setflags(write=False)
    return ped, block, refalt
