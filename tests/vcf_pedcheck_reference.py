"""A brute-force numpy reference for the pedigree check of the --in_vcf path (pm_engine_set_vcf_pedcheck,
include/polymutt_engine.h) -- TEST INFRASTRUCTURE ONLY.

For one family of m members, one site and a frequency f of the reference allele, the full table over {0, 1, 2}^m of
    J(g) = founder priors x every member's likelihood 10^(-PL / 10) of its state
         x one transmission table per non-founder,
as tests/vcf_joint_reference.py builds it, summed over all 3^m assignments: no peeling.  For a non-founder c the sum is
taken four times: L0 with the Mendelian T for everybody, and L_fa, L_mo, L_both with c's table alone replaced by
    T_fa[a][b][k] = Sum_a' pi(a') T[a'][b][k],  T_mo[a][b][k] = Sum_b' pi(b') T[a][b'][k],  T_un[a][b][k] = pi(k),
pi = (f^2, 2 f (1 - f), (1 - f)^2).  A row's values are x_h = log10(L0 / L_h); the row counts when all four sums are finite
and positive; the quantised sums are Sum rint(x_h 2^28) as int64 (rint rounds to even, as llrint does).

Founder priors: Hardy-Weinberg pi at every founder, or -- `trio_prior`, the single-family prior mode of the nuclear closed
form -- the fixed table of SetParentPriorSingleTrio over the two parents of a nuclear family on rows that are not
monomorphic.  A vcf_mode engine peels a lone family (lane plan 1) under Hardy-Weinberg priors, as its planes do, so the
GPU tests of a single family compare with trio_prior off; the mode is kept here and checked on the CPU.
"""
import gzip
import os

import numpy as np

import polymutt_amd as pm
from conftest import EXAMPLE
from vcf_posterior_reference import three, transmission

SCALE = 2.0 ** 28
Q_BOUND = 2.0 ** -29      # a row's quantisation error
ROW_ATOL = 1e-9           # the project's bound for one double evaluation against another (parity.DOSE_ATOL)
CHUNK_ENTRIES = 1 << 22
TRIO_PRIOR = np.array([[0.0, 0.24, 0.04], [0.24, 0.16, 0.08], [0.04, 0.08, 0.12]])   # d_parent_prior's default branch


def pi_of(f):
    f = np.asarray(f, dtype=np.float64)
    return np.stack([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)], axis=-1)


def likelihoods(block, refalt):
    """[n, n_person, 3]: 10^(-PL / 10) of the three genotypes of each site's (ref, alt)."""
    g = np.array([three(r) for r in refalt])
    return 10.0 ** (-np.take_along_axis(np.asarray(block), g[:, None, :], axis=2).astype(np.float64) / 10.0)


def alt_tables(f):
    """(T_fa, T_mo, T_un), each [n, 3, 3, 3] indexed [site][father][mother][child], at the frequencies f [n]."""
    T, pi = transmission(), pi_of(f)
    t_fa = np.einsum("zx,xbk->zbk", pi, T)[:, None, :, :] * np.ones((1, 3, 1, 1))
    t_mo = np.einsum("zx,axk->zak", pi, T)[:, :, None, :] * np.ones((1, 1, 3, 1))
    t_un = pi[:, None, None, :] * np.ones((1, 3, 3, 1))
    return t_fa, t_mo, t_un


class PedcheckFamilies:
    """Per family of a pm_pedigree view: its persons, founders and each non-founder's (member, father, mother)."""

    def __init__(self, view):
        nf, n = view.n_fam, view.n_person
        as_arr = np.ctypeslib.as_array
        self.n_person = n
        fam_start = as_arr(view.fam_start, shape=(nf + 1,)).copy()
        is_founder = as_arr(view.is_founder, shape=(n,)).copy().astype(bool)
        father = as_arr(view.father, shape=(n,)).copy()
        mother = as_arr(view.mother, shape=(n,)).copy()
        self.fams = []
        for f in range(nf):
            p0, p1 = int(fam_start[f]), int(fam_start[f + 1])
            m = p1 - p0
            assert m <= 12, "3^m entries per site"
            founders = [i for i in range(m) if is_founder[p0 + i]]
            kids = [(i, int(father[p0 + i]) - p0, int(mother[p0 + i]) - p0) for i in range(m) if not is_founder[p0 + i]]
            for i, fa, mo in kids:
                assert 0 <= fa < m and 0 <= mo < m and fa != mo, "a non-founder has both parents in its family"
            letters = [chr(ord("a") + i) for i in range(m)]
            self.fams.append({"p0": p0, "m": m, "founders": founders, "kids": kids, "letters": letters})
        self.persons = np.array([F["p0"] + i for F in self.fams for i, _, _ in F["kids"]], np.int32)   # ascending

    def family_sums(self, F, lk, prior, tables, trio_prior=None):
        """[n]: Sum over all 3^m assignments of family F; tables: one [3, 3, 3] or [n, 3, 3, 3] operand per kid of F["kids"];
        trio_prior [n] bool: rows whose two first members (the parents of a nuclear family) take TRIO_PRIOR jointly."""
        n, m, L = len(prior), F["m"], F["letters"]
        out = np.zeros(n)
        step = max(1, CHUNK_ENTRIES // 3 ** m)
        for s in range(0, n, step):
            sl = slice(s, min(n, s + step))
            ops, subs = [], []
            for i in range(m):
                ops.append(lk[sl, F["p0"] + i] * (prior[sl] if i in F["founders"] else 1.0))
                subs.append("Z" + L[i])
            if trio_prior is not None:
                assert F["founders"] == [0, 1] and all({fa, mo} == {0, 1} for _, fa, mo in F["kids"]), "a nuclear family"
                ops[0], ops[1] = lk[sl, F["p0"]], lk[sl, F["p0"] + 1]
                hw = prior[sl][:, :, None] * prior[sl][:, None, :]
                ops.append(np.where(trio_prior[sl][:, None, None], TRIO_PRIOR[None], hw))
                subs.append("Z" + L[0] + L[1])
            for (i, fa, mo), t in zip(F["kids"], tables):
                ops.append(t[sl] if t.ndim == 4 else t)
                subs.append(("Z" if t.ndim == 4 else "") + L[fa] + L[mo] + L[i])
            J = np.einsum(",".join(subs) + "->Z" + "".join(L), *ops)   # the whole table, one axis per member
            out[sl] = J.reshape(J.shape[0], -1).sum(axis=1)
        return out

    def solve(self, block, refalt, f, trio_prior=None, only=None):
        """block [n, n_person, 10] phred bytes, refalt [n], f [n] the row's frequency of the reference allele.  Returns a dict
        of arrays over the k non-founders by ascending person index: "person" [k], "x" [k, n, 3] (father, mother, both;
        nan where the row does not count), "counted" [k, n], "n" [k] int64, "S" [k, 3] = Sum x, "q" [k, 3] int64, and
        "L" [k, n, 4] the four sums.  only: the persons to compute (the others' rows stay uncounted)."""
        lk = likelihoods(block, refalt)
        f = np.asarray(f, dtype=np.float64)
        prior, T, alts = pi_of(f), transmission(), alt_tables(f)
        n, k = len(refalt), len(self.persons)
        L = np.full((k, n, 4), np.nan)
        at = 0
        for F in self.fams:
            plain = [T] * len(F["kids"])
            L0 = None
            for ci, (c, _, _) in enumerate(F["kids"]):
                if only is None or F["p0"] + c in only:
                    if L0 is None:
                        L0 = self.family_sums(F, lk, prior, plain, trio_prior)
                    L[at, :, 0] = L0
                    for h in range(3):
                        tabs = list(plain)
                        tabs[ci] = alts[h]
                        L[at, :, 1 + h] = self.family_sums(F, lk, prior, tabs, trio_prior)
                at += 1
        counted = (np.isfinite(L) & (L > 0)).all(axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.log10(L[:, :, :1] / L[:, :, 1:])
        x = np.where(counted[:, :, None], x, np.nan)
        xs = np.where(counted[:, :, None], x, 0.0)
        return {"person": self.persons.copy(), "x": x, "counted": counted, "n": counted.sum(axis=1).astype(np.int64),
                "S": xs.sum(axis=1), "q": np.rint(xs * SCALE).astype(np.int64).sum(axis=1), "L": L}


def bound(n):
    """|q 2^-28 - S| for n counted rows: the quantisation and one double evaluation per row."""
    return np.asarray(n, dtype=np.float64) * (Q_BOUND + ROW_ATOL)


# ------------------------------------------------------------------------------------------------ pedigrees and data

MALE, FEMALE = 1, 2
TRIO = [("f", None, None, MALE), ("m", None, None, FEMALE), ("c", "f", "m", MALE)]
# (the loader orders a family's founders by id: the mother's sorts first here, so the children's father is person p0 + 1)
QUAD_MOTHER_FIRST = [("a_mo", None, None, FEMALE), ("b_fa", None, None, MALE), ("c1", "b_fa", "a_mo", FEMALE), ("c2", "b_fa", "a_mo", MALE)]
PAIR = [("u1", None, None, MALE), ("u2", None, None, FEMALE)]
NUC6 = TRIO[:2] + [("c%d" % i, "f", "m", 1 + i % 2) for i in range(4)]   # a nuclear family with 4 children
# three generations, 7 persons: the grandparents' daughter d has three children with the founder s
GEN3 = [("gf", None, None, MALE), ("gm", None, None, FEMALE), ("s", None, None, MALE), ("d", "gf", "gm", FEMALE),
        ("k1", "s", "d", MALE), ("k2", "s", "d", FEMALE), ("k3", "s", "d", MALE)]


# The GPU tests' shapes, the smallest that reach each kernel (tests/test_gpu_vcf_pedcheck.py; the CPU tests show that the
# reference counts every row of them).
# name -> (families, rows, max_batch): the second batch is partial; "striding" is one batch whose grid gives every thread of
# k_vcf_pedcheck_lean more than one row and every accumulator more than one block
SHAPES = {
    "lean": ([TRIO, QUAD_MOTHER_FIRST, PAIR], 200, 128),
    "striding": ([TRIO, QUAD_MOTHER_FIRST, PAIR], 3000, 3000),
    "single": ([TRIO], 150, 96),
    "nuc": ([NUC6, TRIO], 120, 96),
    "es": ([GEN3, TRIO], 120, 96),
}


def write_pedigree(directory, families):
    """A Merlin .dat / .ped pair for `families` (lists of (id, father, mother, sex)) through the native loader, which also
    builds the peeling schedules: the loaded pm.Pedigree."""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "test.dat"), "w") as fh:
        fh.write("T\tGLF_Index\n")
    idx = 0
    with open(os.path.join(directory, "test.ped"), "w") as fh:
        for k, fam in enumerate(families):
            for pid, fa, mo, sex in fam:
                idx += 1
                name = lambda x: "0" if x is None else f"F{k}_{x}"
                fh.write(f"F{k}\t{name(pid)}\t{name(fa)}\t{name(mo)}\t{sex}\t{idx}\n")
    return pm.Pedigree(os.path.join(directory, "test.dat"), os.path.join(directory, "test.ped"))


def simulate(view, nsites, seed, freqs=(0.95, 0.8, 0.6, 0.4)):
    """(block [n, n_person, 10], refalt [n], f [n]): per site a frequency f of the reference allele, founders' states from
    Hardy-Weinberg, everybody else's by Mendelian transmission, and per person three PLs with 0 at the true state and
    5..79 elsewhere."""
    as_arr = np.ctypeslib.as_array
    npers = view.n_person
    founder = as_arr(view.is_founder, shape=(npers,)).astype(bool)
    father, mother = as_arr(view.father, shape=(npers,)), as_arr(view.mother, shape=(npers,))
    rng = np.random.default_rng(seed)
    ref_base = rng.integers(1, 5, nsites).astype(np.uint8)
    refalt = (ref_base | (np.array([{1: 3, 2: 4, 3: 1, 4: 2}[int(r)] for r in ref_base], np.uint8) << 4)).astype(np.uint8)
    f = rng.choice(freqs, nsites)
    block = np.full((nsites, npers, 10), 255, np.uint8)
    for i in range(nsites):
        gt = np.full(npers, -1, np.int64)
        gt[founder] = rng.binomial(2, 1 - f[i], founder.sum())
        while (gt < 0).any():
            for p in np.flatnonzero(gt < 0):
                if gt[father[p]] >= 0 and gt[mother[p]] >= 0:
                    gt[p] = rng.binomial(1, gt[father[p]] / 2) + rng.binomial(1, gt[mother[p]] / 2)
        tri = rng.integers(5, 80, (npers, 3))
        tri[np.arange(npers), gt] = 0
        block[i][:, three(refalt[i])] = tri.astype(np.uint8)
    return block, refalt, f


def swap_columns(block, p, q):
    """The block with the PL columns of persons p and q exchanged."""
    out = np.array(block)
    out[:, [p, q]] = out[:, [q, p]]
    return out


# The discrimination data set: two trios, the quad and two unrelated founders; persons in the loader's order: trio 0 = 0, 1,
# 2; trio 1 = 3, 4, 5; quad = 6..9; founders = 10, 11.  A wrong father makes rows at which unlinking either parent repairs
# the Mendelian error, and in a trio those outweigh the mother's own evidence.  So the rows are searched: of DISC_POOL rows
# simulated from a fixed seed, with trio 1's father exchanged with founder 10 and at the generating frequency, the first
# DISC_ERR rows that speak against the father alone (x_father <= -0.5, x_mother >= -0.1) and the first DISC_ROWS - DISC_ERR
# others with x_mother >= -0.1, in the pool's order.  Under the stated pedigree every child then has all three sums
# >= +5; with the child of trio 0 exchanged with founder 10 its LLR_BOTH is <= -5; with the father of trio 1 exchanged
# LLR_FATHER <= -5 and LLR_MOTHER >= +5 (tests/test_cpu_vcf_pedcheck.py).
DISC_FAMILIES = [TRIO, TRIO, QUAD_MOTHER_FIRST, PAIR]
DISC_POOL, DISC_ROWS, DISC_ERR, DISC_SEED = 2000, 300, 60, 29
DISC_CHILD, DISC_FOUNDER, DISC_FATHER, DISC_FATHER_CHILD = 2, 10, 3, 5
_DISC = {}


def discrimination_case(directory):
    """(ped, block, refalt, f): the discrimination data set and the frequencies its rows were generated at."""
    ped = write_pedigree(directory, DISC_FAMILIES)
    if "data" not in _DISC:
        block, refalt, f = simulate(ped.view, DISC_POOL, DISC_SEED)
        fams = PedcheckFamilies(ped.view)
        r = fams.solve(swap_columns(block, DISC_FATHER, DISC_FOUNDER), refalt, f, only=[DISC_FATHER_CHILD])
        x = r["x"][list(r["person"]).index(DISC_FATHER_CHILD)]
        err = (x[:, 0] <= -0.5) & (x[:, 1] >= -0.1)
        rest = ~err & (x[:, 1] >= -0.1)
        keep = np.sort(np.concatenate([np.flatnonzero(err)[:DISC_ERR], np.flatnonzero(rest)[:DISC_ROWS - DISC_ERR]]))
        assert len(keep) == DISC_ROWS
        block = np.ascontiguousarray(block[keep])
        block.setflags(write=False)
        _DISC["data"] = (block, refalt[keep].copy(), f[keep].copy())
    return (ped,) + _DISC["data"]


def example_records(src):
    """The records of a VCF the --in_vcf path computes on the autosomes (one-base REF and ALT, some sample with data, CHROM
    not X / Y / MT), as an engine block with the PL bytes placed as the host driver places them: (ped, block, refalt)."""
    ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
    person = {pid: p for p, pid in enumerate(ped.pids())}
    base = {"A": 1, "C": 2, "G": 3, "T": 4}
    rows, refalt, cols = [], [], None
    for l in (gzip.open(src, "rt") if src.endswith(".gz") else open(src)):
        if l.startswith("##"):
            continue
        c = l.rstrip("\n").split("\t")
        if l.startswith("#"):
            cols = [person[s] for s in c[9:]]
            continue
        if c[3] not in base or c[4] not in base or c[0] in ("X", "Y", "MT"):
            continue
        k = c[8].split(":").index("PL")
        pls = [[int(x) for x in v.split(":")[k].split(",")] for v in c[9:]]
        if not any(any(t) for t in pls):
            continue
        ra = base[c[3]] | base[c[4]] << 4
        row = np.zeros((ped.n_person, 10), np.uint8)
        for p, t in zip(cols, pls):
            row[p, three(ra)] = np.minimum(t, 255)
        rows.append(row)
        refalt.append(ra)
    return ped, np.stack(rows), np.array(refalt, np.uint8)
