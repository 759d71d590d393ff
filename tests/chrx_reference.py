"""An independent numpy reference for the sex-aware three-state chrX de novo model (pm_engine_set_vcf_denovo_chrx,
include/polymutt_engine.h) -- TEST INFRASTRUCTURE ONLY.

The CPU oracle cannot pin this model (its de novo objective uses the autosomal transmission on every chromosome), so the
family likelihood is formed here from the model's definition, without peeling: the joint sum over every member's three
states of founder priors x penetrances x one transmission per non-founder, as an einsum contraction.  Everything that
does not depend on the frequency is contracted once per site into a tensor over the founders' states; an evaluation
then contracts the founders' priors into it.  Which children do not mutate is read from the pedigree's peel steps (the
child of a type-3 step whose couple was the target of an earlier type-1 step: FamilyLikelihoodES.cpp:1391).  The
maximiser is a restatement of csrc/brent_core.h's OptimizeFrequency + Brent state machine.
"""
import math

import numpy as np

MALE = 1


def gi(b1, b2):
    b1, b2 = min(b1, b2), max(b1, b2)
    return (b1 - 1) * (10 - b1) // 2 + (b2 - b1)


def three(refalt):
    a1, a2 = int(refalt) & 15, int(refalt) >> 4
    return a1, a2, [gi(a1, a1), gi(a1, a2), gi(a2, a2)]


def allele_mut_matrix(mu, r):
    """A4 over (A, C, G, T): diagonal 1 - mu, a transition mu r / (1 + r), each transversion mu 0.5 / (1 + r)."""
    A = np.full((4, 4), mu * 0.5 / (1 + r))
    for a, b in ((0, 2), (2, 0), (1, 3), (3, 1)):
        A[a, b] = mu * r / (1 + r)
    A[np.diag_indices(4)] = 1 - mu
    return A


def chrx_transmissions():
    """T_F, T_M [father][mother][child] from the rules: a father is hemizygous (states 0, 2; a heterozygous father has no
    offspring), a daughter takes his allele and one of her mother's, a son one of his mother's alone."""
    mo = {0: (1.0, 0.0), 1: (0.5, 0.5), 2: (0.0, 1.0)}   # mother's state -> P(passes a1), P(passes a2)
    TF, TM = np.zeros((3, 3, 3)), np.zeros((3, 3, 3))
    for i in (0, 2):
        for j in range(3):
            p1, p2 = mo[j]
            if i == 0:
                TF[i, j, 0], TF[i, j, 1] = p1, p2
            else:
                TF[i, j, 1], TF[i, j, 2] = p1, p2
            TM[i, j, 0], TM[i, j, 2] = p1, p2
    return TF, TM


class Pedigree:
    """The arrays of a pm_pedigree view the model needs, and per family its non-founders with their mutation flag."""

    def __init__(self, view):
        nf, n = view.n_fam, view.n_person
        as_arr = np.ctypeslib.as_array
        self.n_fam, self.n_person = nf, n
        self.fam_start = as_arr(view.fam_start, shape=(nf + 1,)).copy()
        self.is_founder = as_arr(view.is_founder, shape=(n,)).copy()
        self.sex = as_arr(view.sex, shape=(n,)).copy()
        self.father = as_arr(view.father, shape=(n,)).copy()
        self.mother = as_arr(view.mother, shape=(n,)).copy()
        peel_start = as_arr(view.peel_start, shape=(nf + 1,)).copy()
        self.fams = []
        for f in range(nf):
            p0, p1 = int(self.fam_start[f]), int(self.fam_start[f + 1])
            couples, plain = set(), set()
            for k in range(int(peel_start[f]), int(peel_start[f + 1])):
                S = view.steps[k]
                if S.type == 1:
                    couples.add((S.to0, S.to1))
                elif S.type == 3 and (S.from0, S.from1) in couples:
                    plain.add(S.to0)
            founders = [i for i in range(p1 - p0) if self.is_founder[p0 + i]]
            kids = [(i, int(self.father[p0 + i]) - p0, int(self.mother[p0 + i]) - p0, int(self.sex[p0 + i]) == MALE, i not in plain)
                    for i in range(p1 - p0) if not self.is_founder[p0 + i]]
            for i, fa, mo, _, _ in kids:
                assert 0 <= fa < p1 - p0 and 0 <= mo < p1 - p0 and int(self.sex[p0 + fa]) == MALE, (f, i)
            self.fams.append((p0, p1 - p0, founders, kids))


class SiteModel:
    """One site: per family the frequency-independent tensor over its founders' states, for the de novo model (dn) and
    the standard one (both mutation matrices the identity)."""

    def __init__(self, ped, M10, A4, site_block, refalt):
        a1, a2, g = three(refalt)
        pen = np.power(10.0, -site_block[:, g].astype(np.float64) / 10.0)   # the vcf_mode table pow(10, -PL / 10)
        M3 = np.array([[M10[g[x] * 10 + g[y]] for y in range(3)] for x in range(3)])
        H3 = np.zeros((3, 3))
        al = (a1 - 1, a2 - 1)
        for x, ax in ((0, al[0]), (2, al[1])):
            for y, ay in ((0, al[0]), (2, al[1])):
                H3[x, y] = A4[ax, ay]
        TF, TM = chrx_transmissions()
        self.tables = {True: (np.einsum("ijm,mk->ijk", TF, M3), np.einsum("ijm,mk->ijk", TM, H3)), False: (TF, TM)}
        self.plain = (TF, TM)
        self.ped = ped
        self.K = {dn: [self._family(fam, pen, dn) for fam in ped.fams] for dn in (True, False)}

    def _family(self, fam, pen, dn):
        p0, n, founders, kids = fam
        ops = []
        for i in range(n):
            ops += [pen[p0 + i], [i]]
        for i, fa, mo, male, mutates in kids:
            T = (self.tables[dn] if mutates else self.plain)[1 if male else 0]
            ops += [T, [fa, mo, i]]
        return np.einsum(*ops, founders, optimize="greedy")

    def loglik(self, f, dn):
        """log10 of the objective at frequency f: the product over families of K contracted with the founders' priors."""
        hw = np.array([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)])
        hemi = np.array([f, 0.0, 1 - f])
        tot = 0.0
        for (p0, n, founders, kids), K in zip(self.ped.fams, self.K[dn]):
            v = K   # (founders only: K is the outer product of the penetrances, the family the product of its persons)
            for i in reversed(founders):   # contract the last axis: the founders are in axis order
                v = v @ (hemi if self.ped.sex[p0 + i] == MALE else hw)
            tot += math.log10(float(v))
        return tot


def _sign(a, b):
    return abs(a) if b >= 0 else -abs(a)


def brent_max(fun, tol=1e-4, itmax=200):
    """csrc/brent_core.h's PmBrent restated: maximise fun on [1e-4, 0.9999] from b = 0.9999.  Returns (max, maximiser,
    evaluation count as the engine counts it, converged)."""
    a, c, x = 0.0001, 0.5, 0.9999
    delta = d = 0.0
    nev, it = 1, 0
    phase1 = True
    mn = fmin = w = v = fw = fv = 0.0
    while True:
        fx = -fun(x)
        nev += 1
        if phase1:
            phase1 = False
            fmin = fx
            nev += 1
            mn = 0.9999
            w = v = mn
            fw = fv = fmin
        else:
            u, fu = x, fx
            if fu <= fmin:
                if u >= mn:
                    a = mn
                else:
                    c = mn
                v, w, mn = w, mn, u
                fv, fw, fmin = fw, fmin, fu
            else:
                if u < mn:
                    a = u
                else:
                    c = u
                if fu <= fw or w == mn:
                    v, w, fv, fw = w, u, fw, fu
                elif fu <= fv or v == mn or v == w:
                    v, fv = u, fu
        it += 1
        if it > itmax:
            return -fmin, mn, nev, False
        middle = 0.5 * (a + c)
        tol1 = tol * abs(mn) + 3.0e-10
        tol2 = 2.0 * tol1
        if abs(mn - middle) <= (tol2 - 0.5 * (c - a)):
            return -fmin, mn, nev, True
        golden = True
        if abs(delta) > tol1:
            rr = (mn - w) * (fmin - fv)
            q = (mn - v) * (fmin - fw)
            p = (mn - v) * q - (mn - w) * rr
            q = 2.0 * (q - rr)
            if q > 0.0:
                p = -p
            q = abs(q)
            temp = delta
            delta = d
            if not (abs(p) >= abs(0.5 * q * temp) or p <= q * (a - mn) or p >= q * (c - mn)):
                golden = False
                d = p / q
                u = mn + d
                if u - a < tol2 or c - u < tol2:
                    d = _sign(tol1, middle - mn)
        if golden:
            delta = a - mn if mn >= middle else c - mn
            d = 0.38196601 * delta
        x = mn + d if abs(d) >= tol1 else mn + _sign(tol1, d)


def reference_values(ped, M10, A4, block, refalt, tol=1e-4):
    """Per site (N, its maximiser, D_max = the standard chrX maximum, its maximiser) and the SiteModel list."""
    out = np.zeros((len(refalt), 4))
    models = []
    for i in range(len(refalt)):
        m = SiteModel(ped, M10, A4, np.asarray(block[i]), refalt[i])
        out[i, 0], out[i, 1], _, ok1 = brent_max(lambda f: m.loglik(f, True), tol)
        out[i, 2], out[i, 3], _, ok0 = brent_max(lambda f: m.loglik(f, False), tol)
        assert ok1 and ok0, i
        models.append(m)
    return out, models
