"""An independent numpy reference for the families and the children behind each DQ of a chrX section
(pm_engine_set_vcf_denovo_chrx_detail, include/polymutt_engine.h) -- TEST INFRASTRUCTURE ONLY.

It builds on chrx_reference: the same pedigree reading (which children do not mutate comes from the peel steps) and the
same definition of a family's likelihood -- the joint sum over every member's three states of founder priors x
penetrances x one transmission per non-founder, as an einsum contraction, no peeling.  Per family it gives the log10 of
that factor at a frequency; per child the joint K[a][b][s] over (father, mother, child) with everyone else summed out,
from which J_c(a, b, S) = Sum_{s in S} K[a][b][s], L_f = Sum K, the posterior and the event follow by the contract's
rules.

The transmission tables, the founder priors, the fathers' states and the states a child may carry are parameters
(Tables), so that tests/test_cpu_vcf_denovo_chrx_detail.py can substitute the autosomal ones and pin this code against
the CPU oracle before it judges the engine.
"""
import math

import numpy as np

from chrx_reference import MALE, chrx_transmissions, three


class Tables:
    """dn, plain: (to a daughter, to a son) [father][mother][child], with and without mutation; prior(f, male) the
    founder prior over the three states; father_states the states a father can carry; child_states(male) a child's."""

    def __init__(self, dn, plain, prior, father_states, child_states):
        self.dn, self.plain, self.prior, self.father_states, self.child_states = dn, plain, prior, father_states, child_states

    def nonmend(self, a, b, male):
        """The states the child may carry that the plain transmission from (a, b) gives probability 0."""
        T = self.plain[1 if male else 0]
        return [s for s in self.child_states(male) if T[a, b, s] == 0.0]


def m3_h3(M10, A4, refalt):
    a1, a2, g = three(refalt)
    M3 = np.array([[M10[g[x] * 10 + g[y]] for y in range(3)] for x in range(3)])
    H3 = np.zeros((3, 3))
    for x, ax in ((0, a1 - 1), (2, a2 - 1)):
        for y, ay in ((0, a1 - 1), (2, a2 - 1)):
            H3[x, y] = A4[ax, ay]
    return M3, H3


def chrx_tables(M10, A4, refalt):
    """The sex-aware model: T_F, T_M, Tdn_F = T_F M3, Tdn_M = T_M H3; a male founder (f, 0, 1 - f), everyone else
    Hardy-Weinberg; a father in states 0 and 2; a son in states 0 and 2, anyone else in all three."""
    M3, H3 = m3_h3(M10, A4, refalt)
    TF, TM = chrx_transmissions()
    dn = (np.einsum("ijm,mk->ijk", TF, M3), np.einsum("ijm,mk->ijk", TM, H3))
    prior = lambda f, male: np.array([f, 0.0, 1 - f]) if male else np.array([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)])
    return Tables(dn, (TF, TM), prior, (0, 2), lambda male: (0, 2) if male else (0, 1, 2))


def autosomal_transmission():
    p1 = {0: 1.0, 1: 0.5, 2: 0.0}   # a parent's state -> P(passes a1)
    T = np.zeros((3, 3, 3))
    for i in range(3):
        for j in range(3):
            T[i, j, 0] = p1[i] * p1[j]
            T[i, j, 2] = (1 - p1[i]) * (1 - p1[j])
            T[i, j, 1] = p1[i] * (1 - p1[j]) + (1 - p1[i]) * p1[j]
    return T


def autosomal_tables(M10, refalt):
    """The model of pm_engine_set_vcf_denovo_detail: one T, Tdn = T M3, Hardy-Weinberg for every founder, every person in
    all three states (the non-Mendelian sets are then the complement of the autosomal Mendelian ones)."""
    _, _, g = three(refalt)
    M3 = np.array([[M10[g[x] * 10 + g[y]] for y in range(3)] for x in range(3)])
    T = autosomal_transmission()
    Tdn = np.einsum("ijm,mk->ijk", T, M3)
    prior = lambda f, male: np.array([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)])
    return Tables((Tdn, Tdn), (T, T), prior, (0, 1, 2), lambda male: (0, 1, 2))


class SiteDetail:
    """One site: ped a chrx_reference.Pedigree, site_block [n_person][10] phred bytes, tables a Tables."""

    def __init__(self, ped, site_block, refalt, tables):
        _, _, g = three(refalt)
        self.g = g
        self.pen = np.power(10.0, -np.asarray(site_block)[:, g].astype(np.float64) / 10.0)
        self.ped, self.t = ped, tables

    def _ops(self, f, freq, dn):
        p0, n, founders, kids = self.ped.fams[f]
        ops = []
        for i in range(n):
            v = self.pen[p0 + i]
            if i in founders:
                v = v * self.t.prior(freq, int(self.ped.sex[p0 + i]) == MALE)
            ops += [v, [i]]
        for i, fa, mo, male, mutates in kids:
            T = (self.t.dn if (dn and mutates) else self.t.plain)[1 if male else 0]
            ops += [T, [fa, mo, i]]
        return ops

    def family_likelihood(self, f, freq, dn):
        return float(np.einsum(*self._ops(f, freq, dn), [], optimize="greedy"))

    def family_log10(self, f, freq, dn):
        return math.log10(self.family_likelihood(f, freq, dn))

    def family_terms(self, x_dn, x_std):
        """(D_f, |l_dn| + |l_std|) per family: D_f = log10 L_f^dn(x_dn) - log10 L_f^std(x_std)."""
        nf = self.ped.n_fam
        D, mag = np.zeros(nf), np.zeros(nf)
        for f in range(nf):
            l_dn, l_std = self.family_log10(f, x_dn, True), self.family_log10(f, x_std, False)
            D[f], mag[f] = l_dn - l_std, abs(l_dn) + abs(l_std)
        return D, mag

    def children(self, f):
        """The family's non-founders as (local index, father, mother, male)."""
        return [(i, fa, mo, male) for i, fa, mo, male, _ in self.ped.fams[f][3]]

    def child(self, f, c, freq):
        """The child with local index c of family f at freq in the de novo model: a dict with
        pp, event (a, b, s) in states or (-1, -1, -1), terms {(a, b): J}, singles {s: J_c(a*, b*, {s})} of the event's
        pair, L, and mag = |log10 L| + max |log10 J| over the positive terms (the scale of the comparison's bound)."""
        i, fa, mo, male = next(k for k in self.children(f) if k[0] == c)
        K = np.einsum(*self._ops(f, freq, True), [fa, mo, c], optimize="greedy")
        L = float(K.sum())
        terms = {}
        for a in self.t.father_states:   # (a, b) order
            for b in range(3):
                S = self.t.nonmend(a, b, male)
                if S:
                    terms[(a, b)] = float(sum(K[a, b, s] for s in S))
        num = 0.0
        for ab in sorted(terms):
            num += terms[ab]
        event, singles, best = (-1, -1, -1), {}, 0.0
        for ab in sorted(terms):
            if terms[ab] > best:
                best, pair = terms[ab], ab
        if best > 0.0:
            singles = {s: float(K[pair[0], pair[1], s]) for s in self.t.nonmend(pair[0], pair[1], male)}
            bv, bs = 0.0, -1
            for s in sorted(singles):
                if singles[s] > bv:
                    bv, bs = singles[s], s
            if bs >= 0:
                event = (pair[0], pair[1], bs)
        pos = [v for v in terms.values() if v > 0.0]
        mag = abs(math.log10(L)) + (max(abs(math.log10(v)) for v in pos) if pos else 0.0)
        return {"pp": min(num / L, 1.0) if L > 0.0 else 0.0, "event": event, "terms": terms, "singles": singles, "L": L,
                "mag": mag, "K": K}

    def event_glf(self, event):
        """The event as pm_person_dn reports it: GLF indices g[s] (a hemizygous state 0 / 2 is g11 / g22)."""
        return tuple(-1 if s < 0 else self.g[s] for s in event)
