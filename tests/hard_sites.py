"""Sites the synthetic generator (polymutt_amd/csrc/synth_core.h) never makes -- TEST INFRASTRUCTURE, pure numpy.

The generator writes one alt allele (the transition of the reference base), 255 in the other seven PL bytes of every
person, depth 8..29, mapQ 60, data for everybody, alt frequency <= 0.5 and a valid reference base.  hard_block() starts
from pm.synth_block_host() and rewrites every site as one of the classes below, interleaved site by site (PATTERN), so
that called, filtered and bad-ref sites alternate inside one k_prep block:

  tv          ref + tv1 or ref + tv2 segregate (the alt planes moved off the transition): maxidx 2 / 3
  nonref      nobody carries the reference base; ts + tv1, ts + tv2 or tv1 + tv2 segregate, the founders dealt as many
              homozygotes of one as of the other.  The two homozygote planes are made to weigh the same (_tie), so the
              two ref + alt configurations that each see one of them tie: var_post_prob < 0.99 after four
              configurations, n_cfg == 7, maxidx 4 / 5 / 6
  triallelic  even families segregate ref + ts, odd families ref + tv1
  dense       all ten bytes of every person U{0..255}, shifted so that the person's minimum is 0; or all ten in 0..3
  real        (3- and 4-person nuclear families only) records of tests/golden/example: family f takes example family
              f % 3, father / mother / k-th child by the pedigrees' own parent arrays (a trio takes the first child), the
              example site drawn from those with this site's reference base (the example holds one base only: a site
              with another takes the record's); every other one from the records where somebody is not plainly hom-ref;
              PL, depth and mapQ as they are
  highaf      ref + ts with alt frequency 0.8..1.0; or every person a confident hom-alt
  mendel      per family: founders confident hom-ref (0 / 255 / 255), the last non-founder confident hom-alt
              (255 / 255 0), the other non-founders ordinary hom-ref reads; seven planes 255.  At most the founders + 1
              persons of a family hold 0 / 255 triples (7 of 12 in the largest pedigree), so every likelihood stays far
              above the smallest double
  missing     persons with depth 0, mapQ 0 and ten zero bytes: a random 30 %; family 0 and the last 8 families; all but
              one family; every person whose parents are both founders (one whole non-founder generation); everybody
              (a site nobody has data for: num_samp_with_data == 0)
  stats       one person with depth 2^24 - 1 and mapQ 255 (dm == 0xFFFFFFFF); mapQ U{0..255}; depth 1; mapQ 60 with one
              person at 59 (an average just under 60, for filter_params)
  badref      ref 0 and 5..15

Sub-kinds rotate with each occurrence of the class.  Everything is drawn from np.random.default_rng(seed): same
arguments, same bytes; the block SHA-256 of the hard_* cases in tests/golden/synth/cases.json pins them.

write_glf_dataset() stores a block as one GLF v3 file per person (polymutt_amd/host/glf.h), next to the pedigree files
pm.synth_write_dataset() wrote, so that the reference reads the same bytes.  A GLF record holds the reference base as an
IUPAC nibble that the readers translate to 0..4, so `badref` values 5..15 cannot be stored: GOLDEN_CLASSES, the classes
of the reference-pinned hard_* cases, leaves `badref` out; the engine-versus-oracle runs keep it.
"""
import os

import numpy as np

import polymutt_amd as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example")

# `missing` twice: five sub-kinds in a 48-site block
PATTERN = ("tv", "missing", "nonref", "badref", "triallelic", "dense", "real", "highaf", "missing", "mendel", "stats")
ALL = tuple(dict.fromkeys(PATTERN))
EXTENDED_CLASSES = tuple(c for c in ALL if c != "real")
GOLDEN_CLASSES = tuple(c for c in ALL if c != "badref")
BAD_REFS = (0,) + tuple(range(5, 16))
TS, TV1, TV2 = (0, 3, 4, 1, 2), (0, 2, 1, 2, 1), (0, 4, 3, 4, 3)   # src/PedigreeGLF.h:14-53, by reference base 1..4


def gi(b1, b2):
    """glfHandler::GenotypeIndex: the PL byte of genotype b1/b2 (bases 1..4)."""
    b1, b2 = min(b1, b2), max(b1, b2)
    return (b1 - 1) * (10 - b1) // 2 + (b2 - b1)


class _Ped:
    """The arrays of a pm.Pedigree's view (global parent indices, -1 for founders)."""

    def __init__(self, ped):
        v = ped.view
        self.n_fam, self.n = v.n_fam, v.n_person
        self.start = np.ctypeslib.as_array(v.fam_start, shape=(v.n_fam + 1,)).copy()
        self.father = np.ctypeslib.as_array(v.father, shape=(v.n_person,)).copy()
        self.mother = np.ctypeslib.as_array(v.mother, shape=(v.n_person,)).copy()
        self.founder = self.father < 0
        self.fam_of = np.repeat(np.arange(self.n_fam), np.diff(self.start))

    def nuclear_roles(self, f):
        """(father, mother, [children]) of a 3- or 4-person nuclear family, as global person indices."""
        p = np.arange(self.start[f], self.start[f + 1])
        kids = [int(j) for j in p if not self.founder[j]]
        assert 1 <= len(kids) and len(p) == 2 + len(kids), "`real` needs nuclear families"
        fa, mo = int(self.father[kids[0]]), int(self.mother[kids[0]])
        assert all(self.father[k] == fa and self.mother[k] == mo for k in kids)
        return fa, mo, kids


def _triples(depth, nalt):
    """synth_core.h's PL(11, 12, 22) of (depth, alt reads) at 1 % error, capped at 255."""
    d, k = depth.astype(np.float64), nalt.astype(np.float64)
    e = 0.01
    L = np.stack([k * np.log10(e) + (d - k) * np.log10(1 - e), d * np.log10(0.5),
                  (d - k) * np.log10(e) + k * np.log10(1 - e)], axis=-1)
    return np.minimum(np.rint(-10.0 * (L - L.max(axis=-1, keepdims=True))), 255).astype(np.uint8)


def _gene_drop(P, af, rng, balanced):
    """Genotypes (alt allele count) [sites][persons]: founders Bernoulli(af[site]), non-founders one random haplotype
    of each parent (persons are in path order, parents first).  At the sites of `balanced` the founders are instead
    dealt aa, bb, ab, ba in turn, in random order: as many homozygotes of one allele as of the other, to within one."""
    n = len(af)
    u = rng.random((n, P.n, 2))
    h = np.zeros((n, P.n, 2), dtype=np.uint8)
    founders = np.nonzero(P.founder)[0]
    h[:, founders] = u[:, founders] < af[:, None, None]
    deal = np.array([[0, 0], [1, 1], [0, 1], [1, 0]], dtype=np.uint8)
    for s in np.nonzero(balanced)[0]:
        h[s, founders] = deal[rng.permutation(len(founders)) % 4]
    for j in np.nonzero(~P.founder)[0]:
        fa, mo = P.father[j], P.mother[j]
        h[:, j, 0] = np.where(u[:, j, 0] < 0.5, h[:, fa, 0], h[:, fa, 1])
        h[:, j, 1] = np.where(u[:, j, 1] < 0.5, h[:, mo, 0], h[:, mo, 1])
    return h.sum(axis=2)


def _put(pl, s, who, a, b, tri):
    """Persons `who` of site s: genotypes aa / ab / bb get tri[who], the other seven 255."""
    pl[s, who] = 255
    pl[s, who, gi(a, a)] = tri[who, 0]
    pl[s, who, gi(a, b)] = tri[who, 1]
    pl[s, who, gi(b, b)] = tri[who, 2]


def _tie(tri, founder):
    """The bytes of a `nonref` site, where each of two ref + alt configurations sees one of the two homozygote planes
    and 255 elsewhere: they tie when the planes weigh the same.  A non-founder's two homozygote bytes become the smaller
    of the two and that + 1, the heavier one on alternating sides from one non-founder to the next in the order of their
    bytes (a heterozygote stays
    one, a homozygote is one of either allele; equal bytes would leave a hemizygous son of a heterozygous mother with
    two exactly equal posteriors, and the best genotype to rounding); the founders, who alone carry the allele
    frequency, keep theirs, and bytes of their heavier plane are lowered (never below the person's heterozygote byte)
    until the two planes' sums over the founders are within 3, 0.3 log10 units."""
    tri = tri.astype(np.int64)
    kids = np.nonzero(~founder)[0]
    low = np.minimum(np.minimum(tri[kids, 0], tri[kids, 2]), 254)
    side = np.zeros(len(kids), dtype=np.int64)
    side[np.argsort(low, kind="stable")] = np.arange(len(kids)) % 2   # (in the order of the bytes: what a configuration
    # pays for a non-founder grows with the byte up to the price of a de novo mutation, so neighbours cancel)
    tri[kids, 0], tri[kids, 2] = low + side, low + 1 - side
    d = int(tri[founder, 0].sum() - tri[founder, 2].sum())
    col = 0 if d > 0 else 2
    d = abs(d)
    who = np.nonzero(founder)[0]
    for p in who[np.argsort(-tri[who, col], kind="stable")]:
        take = min(d - 3, int(tri[p, col] - tri[p, 1]))
        if take > 0:
            tri[p, col] -= take
            d -= take
    assert d <= 3, "nonref: the founders' homozygote planes cannot be balanced"
    return tri.astype(np.uint8)


_example = None


def _example_data():
    """tests/golden/example as dense blocks, and per example family its (father, mother, children) columns."""
    global _example
    if _example is None:
        ped = pm.Pedigree(os.path.join(EXAMPLE, "test.dat"), os.path.join(EXAMPLE, "test.ped"))
        cwd = os.getcwd()
        os.chdir(EXAMPLE)
        try:
            rd = pm.GlfReader(ped, "test.gif")
            parts = [rd.read(200000) for _ in rd.sections()]
            rd.close()
        finally:
            os.chdir(cwd)
        ref = np.concatenate([p[1] for p in parts])
        pl = np.concatenate([p[2] for p in parts])
        dm = np.concatenate([p[3] for p in parts])
        E = _Ped(ped)
        roles = [E.nuclear_roles(f) for f in range(E.n_fam)]
        ok = (ref >= 1) & (ref <= 4)
        homref = np.array([0] + [gi(b, b) for b in range(1, 5)])[np.where(ok, ref, 0)]
        variant = ok & (pl[np.arange(len(ref)), :, homref] > 0).any(axis=1)
        _example = (ref, pl, dm, roles, variant)
    return _example


def hard_block(ped, n_sites, seed, classes=ALL):
    """(pl [n][n_person][10] uint8, dm [n][n_person] uint32, ref [n] uint8, site_class [n] of str) -- module docstring."""
    P = _Ped(ped)
    rng = np.random.default_rng(seed)
    pl, dm, ref = pm.synth_block_host(ped.view, n_sites, seed)
    pattern = [c for c in PATTERN if c in classes]
    assert pattern and set(classes) <= set(ALL), classes
    site_class = np.array([pattern[s % len(pattern)] for s in range(n_sites)])
    af_range = {"tv": (0.15, 0.5), "highaf": (0.8, 1.0)}
    af = np.full(n_sites, 0.3)
    for s in range(n_sites):
        if site_class[s] in af_range:
            a, b = af_range[site_class[s]]
            af[s] = a + (b - a) * rng.random()
    G = _gene_drop(P, af, rng, site_class == "nonref")
    depth = rng.integers(8, 30, size=(n_sites, P.n))
    nalt = rng.binomial(depth, np.array([0.01, 0.5, 0.99])[G])
    tri = _triples(depth, nalt)
    dm[:] = depth.astype(np.uint32) | np.uint32(60 << 24)
    everyone = np.arange(P.n)
    seen = {}
    for s in range(n_sites):
        c = str(site_class[s])
        kind = seen.get(c, 0)
        seen[c] = kind + 1
        r = int(ref[s])
        ts, tv1, tv2 = TS[r], TV1[r], TV2[r]
        _put(pl, s, everyone, r, ts, tri[s])   # (the base every class but tv / nonref / ... keeps: ref + ts at af 0.3)
        if c == "tv":
            _put(pl, s, everyone, r, (tv1, tv2)[kind % 2], tri[s])
        elif c == "nonref":
            a, b = ((ts, tv1), (ts, tv2), (tv1, tv2))[kind % 3]
            _put(pl, s, everyone, a, b, _tie(tri[s], P.founder))
        elif c == "triallelic":
            odd = everyone[P.fam_of % 2 == 1]
            _put(pl, s, odd, r, tv1, tri[s])
        elif c == "dense":
            b = rng.integers(0, 256 if kind % 2 == 0 else 4, size=(P.n, 10))
            pl[s] = (b - b.min(axis=1, keepdims=True)).astype(np.uint8)
        elif c == "real":
            eref, epl, edm, roles, evar = _example_data()
            cand = np.nonzero(eref == r)[0]
            if not len(cand):   # (the example's section has one reference base: the site takes the record's)
                cand = np.arange(len(eref))
            if kind % 2 == 0:   # every other one from the records where somebody's best genotype is not hom-ref
                cand = cand[evar[cand]]
            e = int(cand[rng.integers(len(cand))])
            r = ref[s] = eref[e]
            for f in range(P.n_fam):
                fa, mo, kids = P.nuclear_roles(f)
                efa, emo, ekids = roles[f % 3]
                for dst, src in [(fa, efa), (mo, emo)] + list(zip(kids, ekids)):
                    pl[s, dst], dm[s, dst] = epl[e, src], edm[e, src]
        elif c == "highaf":
            if kind % 2 == 1:
                hom = _triples(depth[s], depth[s])
                _put(pl, s, everyone, r, ts, hom)
        elif c == "mendel":
            t = _triples(depth[s], np.zeros_like(depth[s]))
            t[P.founder] = (0, 255, 255)
            for f in range(P.n_fam):
                t[P.start[f + 1] - 1] = (255, 255, 0)   # (path order: the last person of a family is a non-founder)
            assert not P.founder[P.start[1:] - 1].any()
            _put(pl, s, everyone, r, ts, t)
        elif c == "missing":
            k = kind % 5
            if k == 0:
                gone = rng.random(P.n) < 0.3
            elif k == 1:
                gone = (P.fam_of == 0) | (P.fam_of >= P.n_fam - 8)
            elif k == 2:
                gone = P.fam_of != int(rng.integers(P.n_fam))
            elif k == 3:
                gone = ~P.founder & P.founder[np.maximum(P.father, 0)] & P.founder[np.maximum(P.mother, 0)]
            else:
                gone = np.ones(P.n, dtype=bool)
            pl[s, gone] = 0
            dm[s, gone] = 0
        elif c == "stats":
            k = kind % 4
            if k == 0:
                dm[s, int(rng.integers(P.n))] = 0xFFFFFFFF
            elif k == 1:
                dm[s] = depth[s].astype(np.uint32) | (rng.integers(0, 256, size=P.n).astype(np.uint32) << 24)
            elif k == 2:
                one = np.ones(P.n, dtype=np.int64)
                _put(pl, s, everyone, r, ts, _triples(one, rng.binomial(one, np.array([0.01, 0.5, 0.99])[G[s]])))
                dm[s] = np.uint32(1 | (60 << 24))
            else:
                dm[s, int(rng.integers(P.n))] -= np.uint32(1 << 24)
        elif c == "badref":
            ref[s] = BAD_REFS[kind % len(BAD_REFS)]
    assert int((dm & 0xFFFFFF).astype(np.int64).sum(axis=1).max()) < 2 ** 31
    return pl, dm, ref, site_class


def flat_configs(pl, ref):
    """[n][7] bool, from the bytes alone: configuration k of site s is Brent-minimised on an objective that does not
    depend on the allele frequency, because no person's reads tell its two alleles' three genotypes apart (the three
    bytes are equal in every person: 255 where nobody carries either allele, 0 where the person has no data).  Every
    founder term is then that byte's likelihood times (f + g)^2, 1 in real arithmetic, and Brent's path is decided by
    the last bit of the sum ("Exact mode and evaluation counts").  Configuration 0 has no minimisation."""
    n = len(ref)
    flat = np.zeros((n, 7), dtype=bool)
    for s in range(n):
        r = int(ref[s])
        if not 1 <= r <= 4:
            continue
        ts, tv1, tv2 = TS[r], TV1[r], TV2[r]
        for k, (a, b) in enumerate(((r, ts), (r, tv1), (r, tv2), (ts, tv1), (ts, tv2), (tv1, tv2)), start=1):
            x = pl[s][:, [gi(a, a), gi(a, b), gi(b, b)]]
            flat[s, k] = bool(((x[:, 0] == x[:, 1]) & (x[:, 1] == x[:, 2])).all())
    return flat


def site_kinds(site_class):
    """Per site, how many earlier sites have its class: hard_block's sub-kind is this count modulo the class's number
    of sub-kinds (tv 2, nonref 3, dense 2, real 2, highaf 2, missing 5, stats 4, badref 12)."""
    seen, out = {}, np.zeros(len(site_class), dtype=np.int64)
    for s, c in enumerate(site_class):
        out[s] = seen.get(str(c), 0)
        seen[str(c)] = out[s] + 1
    return out


def site_stats(dm):
    """CalcReadStats (NucFamGenotypeLikelihood.cpp:520-546) per site, in its arithmetic: total depth, samples with
    data, their share and the average mapping quality over them."""
    d = (dm & 0xFFFFFF).astype(np.int64)
    td, nsd = d.sum(axis=1), (d > 0).sum(axis=1)
    mq = (dm >> 24).astype(np.float64).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        avgmq = np.where(nsd > 0, mq / nsd, 0.0)
        ps = np.where(nsd > 0, nsd / float(dm.shape[1]), 0.0)
    return td, nsd, ps, avgmq


def filter_params(block, **kw):
    """(pm.Params, expected status per site) for a hard block: min_total_depth, max_total_depth, min_ps and
    min_map_quality read off the block's own sites so that for each filter one site sits exactly on the threshold (and
    passes: the reference filters with strict comparisons) and another lies just beyond it -- the neighbouring distinct
    value among the sites that reach the filter.  The expected statuses restate main.cpp's filter chain in numpy."""
    pl, dm, ref, _ = block
    td, nsd, ps, avgmq = site_stats(dm)
    ok = (ref >= 1) & (ref <= 4)
    u = np.unique(td[ok])
    assert len(u) >= 6
    min_td, max_td = int(u[2]), int(u[-3])
    reach = ok & (td >= min_td) & (td <= max_td)
    v = np.unique(ps[reach] * 100)
    assert len(v) >= 2
    min_ps = float(v[1])
    reach &= ps * 100 >= min_ps
    min_mq = 60
    assert (avgmq[reach] == 60.0).any() and ((avgmq[reach] < 60.0) & (avgmq[reach] > 59.0)).any()
    status = np.zeros(len(ref), dtype=np.int32)
    for s in range(len(ref)):
        if not ok[s]:
            status[s] = 5
        elif td[s] < min_td:
            status[s] = 1
        elif td[s] > max_td:
            status[s] = 2
        elif ps[s] * 100 < min_ps:
            status[s] = 3
        elif avgmq[s] < min_mq:
            status[s] = 4
    for code in (1, 2, 3, 4):
        assert (status == code).any(), code
    par = pm.Params.defaults(min_total_depth=min_td, max_total_depth=max_td, min_ps=min_ps, min_map_quality=min_mq, **kw)
    return par, status


def filter_flags(par):
    """The reference command line of filter_params' thresholds (repr: the shortest text that parses back exactly)."""
    return ["--minDepth", str(par.min_total_depth), "--maxDepth", str(par.max_total_depth),
            "--minPercSampleWithData", repr(par.min_ps), "--minMapQuality", str(par.min_map_quality)]


def load_pedigree(tmp_root, shape, families):
    """The pedigree pm.synth_write_dataset writes for (shape, families) -- a "+dn" suffix only plants sites."""
    import shutil
    d = os.path.join(str(tmp_root), f"ped_{shape}_{families}")
    pm.synth_write_dataset(d, shape.split("+")[0], families, 1, 1)
    ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
    shutil.rmtree(d)   # (one GLF file per person)
    return ped


def write_case(directory, shape, families, sites, seed, hard):
    """A hard_* case of tests/golden/synth/cases.json (`hard` = its "hard" entry: {"classes": [...]}): the pedigree
    files of pm.synth_write_dataset, the GLFs of hard_block(pedigree, sites, seed, classes).  Returns the block."""
    pm.synth_write_dataset(directory, shape, families, sites, seed)
    ped = pm.Pedigree(os.path.join(directory, "test.dat"), os.path.join(directory, "test.ped"))
    block = hard_block(ped, sites, seed, tuple(hard["classes"]))
    write_glf_dataset(directory, *block[:3])
    return block


_IUPAC = (0, 1, 2, 4, 8)


def write_glf_dataset(directory, pl, dm, ref, label="1"):
    """One GLF v3 file per person (p1.glf ... in person order, the names pm.synth_write_dataset put into test.gif),
    one section, one 20-byte SNP record per site and person:
      byte 0 = record type 1 << 4 | IUPAC nibble of the reference base, u32 offset 1, u32 depth (24 bits; min LLK 0),
      u8 mapQ, u8 lk[10].
    Header "GLF\\3" + u32 0 (no header text); section = i32 label length with NUL, label, i32 length; a 0 byte ends it."""
    n, n_person = dm.shape
    if ((ref < 0) | (ref > 4)).any():
        raise ValueError("a GLF record cannot hold a reference base outside 0..4")
    rec = np.zeros((n, n_person, 20), dtype=np.uint8)
    rec[:, :, 0] = (0x10 | np.asarray(_IUPAC, dtype=np.uint8)[ref])[:, None]
    rec[:, :, 1] = 1
    d = np.ascontiguousarray(dm & 0xFFFFFF, dtype="<u4")
    rec[:, :, 5:9] = d.view(np.uint8).reshape(n, n_person, 4)
    rec[:, :, 9] = dm >> 24
    rec[:, :, 10:] = pl
    lab = label.encode() + b"\0"
    head = b"GLF\x03" + np.uint32(0).tobytes() + np.int32(len(lab)).tobytes() + lab + np.int32(n).tobytes()
    for p in range(n_person):
        with open(os.path.join(directory, f"p{p + 1}.glf"), "wb") as fh:
            fh.write(head + rec[:, p].tobytes() + b"\0")
