"""A brute-force numpy reference for the joint call plane of the --in_vcf path (pm_engine_set_vcf_joint,
include/polymutt_engine.h) -- TEST INFRASTRUCTURE ONLY.

For one family of m members, one site and a frequency f of the reference allele, the full table over {0, 1, 2}^m of
    J(g) = Hardy-Weinberg founder priors (f^2, 2 f (1 - f), (1 - f)^2) at the founders' states
         x every member's likelihood 10^(-PL / 10) of its state
         x one autosomal Mendelian transmission T[g_fa][g_mo][g_c] per non-founder,
built from tests/vcf_posterior_reference.py's `three`, `transmission` and priors as an outer product (an einsum whose
output keeps every member's index).  No peeling, no max-product: the maximum, the set of assignments that reach it, the
runner-up and L = the table's sum are read off the table, and J at any given assignment is a look-up in it.

Like the posterior reference it covers autosomal sections of pedigrees with more than one family (Hardy-Weinberg priors
everywhere).  The table has 3^m entries per site: the sites go through in chunks so that a chunk stays within 2^24
entries, and the tests give families of more than 10 members at most 16 sites.
"""
import numpy as np

from vcf_posterior_reference import make_case, three, transmission  # noqa: F401  (make_case: re-exported for the tests)

CHUNK_ENTRIES = 1 << 24
NONE = 255   # pm_vcf_joint.g without an assignment


class JointFamilies:
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
        for f in range(nf):
            p0, p1 = int(fam_start[f]), int(fam_start[f + 1])
            m = p1 - p0
            assert m <= 16, "3^m entries per site"
            founders = [i for i in range(m) if self.is_founder[p0 + i]]
            kids = [(i, int(father[p0 + i]) - p0, int(mother[p0 + i]) - p0) for i in range(m) if not self.is_founder[p0 + i]]
            for i, fa, mo in kids:
                assert 0 <= fa < m and 0 <= mo < m and fa != mo, "a non-founder has both parents in its family"
            letters = [chr(ord("a") + i) for i in range(m)]
            subs = ",".join(["Z" + c for c in letters] + [letters[fa] + letters[mo] + letters[i] for i, fa, mo in kids])
            self.fams.append({"p0": p0, "m": m, "founders": founders, "kids": kids, "subs": subs + "->Z" + "".join(letters)})
        self.max_members = max(F["m"] for F in self.fams)

    def _vectors(self, block, refalt, af):
        g = np.array([three(r) for r in refalt])
        lk = 10.0 ** (-np.take_along_axis(np.asarray(block), g[:, None, :], axis=2).astype(np.float64) / 10.0)   # [n, np, 3]
        f = np.asarray(af, dtype=np.float64)
        prior = np.stack([f * f, 2 * f * (1 - f), (1 - f) * (1 - f)], axis=1)                                     # [n, 3]
        return lk, prior

    def tables(self, F, lk, prior):
        """Yields (slice of sites, J [sites, 3, ..., 3] with one axis per member of family F), chunk by chunk."""
        T = transmission()
        n = len(prior)
        step = max(1, CHUNK_ENTRIES // 3 ** F["m"])
        for s in range(0, n, step):
            sl = slice(s, min(n, s + step))
            vec = [lk[sl, F["p0"] + i] * (prior[sl] if i in F["founders"] else 1.0) for i in range(F["m"])]
            yield sl, np.einsum(F["subs"], *vec, *([T] * len(F["kids"])))

    @staticmethod
    def _lookup(J, gs):
        """J [sites, 3, ..., 3] at the assignments gs [sites, m]; nan where a member has no state (NONE)."""
        ok = (gs <= 2).all(axis=1)
        idx = np.where(ok[:, None], gs, 0)
        v = J[(np.arange(J.shape[0]),) + tuple(idx[:, i] for i in range(gs.shape[1]))]
        return np.where(ok, v, np.nan)

    def solve(self, block, refalt, af, g=None):
        """Per family a dict of per-site arrays: "max" = max J, "L" = sum J, "second" = the largest J of an assignment
        that does not reach the maximum (0 if there is none), "n_best" = how many assignments reach it, "argmax"
        [n, m] = the first of them in row-major order (all NONE where max J = 0), "marg" [n, m, 3] = the table's
        marginals over L (zeros where L = 0); with an assignment g [n, n_person] also "J_at" = evaluate()'s
        column of the family, from the same pass over the table."""
        lk, prior = self._vectors(block, refalt, af)
        n = len(refalt)
        out = []
        if g is not None:
            g = np.asarray(g).astype(np.int64)
        for F in self.fams:
            m = F["m"]
            r = {"max": np.zeros(n), "L": np.zeros(n), "second": np.zeros(n), "n_best": np.zeros(n, np.int64),
                 "argmax": np.full((n, m), NONE, np.int64), "marg": np.zeros((n, m, 3))}
            for sl, J in self.tables(F, lk, prior):
                flat = J.reshape(J.shape[0], -1)
                mx = flat.max(axis=1)
                r["max"][sl] = mx
                r["L"][sl] = flat.sum(axis=1)
                best = flat == mx[:, None]
                r["n_best"][sl] = best.sum(axis=1)
                r["second"][sl] = np.where(best, 0.0, flat).max(axis=1)
                first = np.stack(np.unravel_index(flat.argmax(axis=1), (3,) * m), axis=1)
                r["argmax"][sl] = np.where(mx[:, None] > 0, first, NONE)
                if g is not None:
                    r.setdefault("J_at", np.full(n, np.nan))[sl] = self._lookup(J, g[sl, F["p0"]:F["p0"] + m])
                L = r["L"][sl]
                for i in range(m):
                    mi = J.sum(axis=tuple(a for a in range(1, m + 1) if a != i + 1))
                    r["marg"][sl, i] = np.divide(mi, L[:, None], out=np.zeros_like(mi), where=L[:, None] != 0)
            out.append(r)
        return out

    def evaluate(self, block, refalt, af, g):
        """[n, n_fam]: J of every family at the assignment g [n, n_person] (states 0, 1, 2), looked up in the family's
        table; nan where a member of the family has no state (NONE)."""
        lk, prior = self._vectors(block, refalt, af)
        g = np.asarray(g).astype(np.int64)
        out = np.full((len(refalt), len(self.fams)), np.nan)
        for k, F in enumerate(self.fams):
            m = F["m"]
            for sl, J in self.tables(F, lk, prior):
                out[sl, k] = self._lookup(J, g[sl, F["p0"]:F["p0"] + m])
        return out

    def mendel_consistent(self, g):
        """[n, n_fam] bool: every father / mother / child trio of the family has T > 0 at the assignment g."""
        T = transmission()
        g = np.asarray(g).astype(np.int64)
        out = np.ones((g.shape[0], len(self.fams)), bool)
        for k, F in enumerate(self.fams):
            gs = g[:, F["p0"]:F["p0"] + F["m"]]
            out[:, k] &= (gs <= 2).all(axis=1)
            c = np.minimum(gs, 2)
            for i, fa, mo in F["kids"]:
                out[:, k] &= T[c[:, fa], c[:, mo], c[:, i]] > 0
        return out


# Hand-built trios, (PL11, PL12, PL22) of father, mother and child, whose marginal argmaxes no transmission allows while the
# joint optimum is unique with a runner-up of at most 0.8 of its mass.  Whether a trio does that depends on the frequency:
#   PLANTED_TRIO        at a reference frequency of 0.95: marginal calls (0/0, 0/0, 0/1), joint optimum (0/0, 0/1, 0/1) at
#                       posterior 0.475, runner-up 0.60 of it.  At 0.7 its marginal calls are the consistent (1/1, 0/0, 0/1).
#   PLANTED_TRIO_07     found by a random search over PLs in 0..39 for the same at 0.7: marginal calls (0/0, 0/0, 0/1), joint
#                       optimum (1/1, 0/0, 0/1), runner-up 0.74 of it.
#   PLANTED_TRIO_OWN_AF found by the same search for a trio that does it at the frequency the model itself estimates (0.80)
#                       when every family of an 8-trio pedigree carries it: marginal calls (0/0, 0/0, 0/1), joint optimum
#                       (0/0, 0/1, 0/1), runner-up 0.79 of it, every marginal argmax ahead by at least 0.13.  (With
#                       PLANTED_TRIO in every family the estimate is 0.54, where its marginal calls are consistent.)
PLANTED_TRIO = ((0, 23, 7), (0, 15, 22), (30, 0, 32))
PLANTED_TRIO_07 = ((0, 35, 7), (0, 12, 11), (29, 0, 28))
PLANTED_TRIO_OWN_AF = ((0, 22, 39), (0, 21, 33), (30, 0, 9))


def trio_block(fa, mo, kid, n_trios, n_sites=1):
    """(block [n_sites, 3 n_trios, 10], refalt): A ref, G alt, every trio the given (PL11, PL12, PL22) triples."""
    refalt = np.full(n_sites, 1 | 3 << 4, np.uint8)
    block = np.full((n_sites, 3 * n_trios, 10), 255, np.uint8)
    for t in range(n_trios):
        for j, tri in enumerate((fa, mo, kid)):
            block[:, 3 * t + j, three(refalt[0])] = tri
    block.setflags(write=False)
    return block, refalt
