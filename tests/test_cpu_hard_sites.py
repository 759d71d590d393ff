"""tests/hard_sites.py does what it says: on four small pedigrees, plain and --denovo, the CPU oracle gives every class
of hard_block() the outcome the class is built for.  These are conditions on the inputs -- if a class misses its
outcome, the class changes, not the assertion.  The oracle itself is pinned on the same builder by the reference: the
hard_* cases of tests/golden/synth run through test_cpu_oracle.py's parametrised tests, whose block SHA-256 also makes
any drift of the builder loud."""
import os

import numpy as np
import pytest

import hard_sites as hs
import polymutt_amd as pm
from fixtures import CASES, make_dataset, read_dataset
from oracle_binding import Oracle

# 12 rounds of the class pattern: every sub-kind of every class, every bad reference base
DATASETS = [("quad", 12, 132, hs.ALL), ("trio", 12, 132, hs.ALL), ("mixed", 13, 132, hs.ALL),
            ("extmix", 5, 120, hs.EXTENDED_CLASSES)]
SEED = 5
_blocks = {}


def _block(tmp_root, shape, n_fam, n_sites, classes):
    if shape not in _blocks:
        ped = hs.load_pedigree(tmp_root, shape, n_fam)
        b = hs.hard_block(ped, n_sites, SEED, classes)
        for a in b:
            a.setflags(write=False)
        _blocks[shape] = (ped,) + b
    return _blocks[shape]


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("hard_sites")


@pytest.mark.parametrize("denovo", [0, 1], ids=["plain", "denovo"])
@pytest.mark.parametrize("shape,n_fam,n_sites,classes", DATASETS, ids=[d[0] for d in DATASETS])
def test_every_class_reaches_its_outcome(built, tmp_root, shape, n_fam, n_sites, classes, denovo):
    ped, pl, dm, ref, cls = _block(tmp_root, shape, n_fam, n_sites, classes)
    kind = hs.site_kinds(cls)
    assert (cls[1:] != cls[:-1]).all(), "classes are interleaved site by site"
    ora = Oracle(ped.view, pm.Params.defaults(denovo=denovo, denovo_mut_rate=1e-5 if denovo else 1.5e-8))
    o, oc = ora.run(pl, dm, ref)
    called = o["status"] == 0
    is_ = {c: cls == c for c in classes}
    r = ref.astype(np.int64)

    assert (o["status"][is_["badref"]] == 5).all() and called[~is_["badref"]].all()
    assert sorted(set(ref[is_["badref"]].tolist())) == list(hs.BAD_REFS)
    assert (o["maxidx"][is_["tv"]] == 2 + kind[is_["tv"]] % 2).all()
    assert (o["n_cfg"][is_["nonref"]] == 7).all() and (o["maxidx"][is_["nonref"]] == 4 + kind[is_["nonref"]] % 3).all()
    # ... whose winning configuration is Brent-minimised on an objective that is not flat: parity.py excuses a minimiser
    # divergence where the likelihoods agree to FLAT_RTOL = 1e-12; here they differ by 1e-3 and more across the range
    for s in np.nonzero(is_["nonref"])[0]:
        pair = ((hs.TS, hs.TV1), (hs.TS, hs.TV2), (hs.TV1, hs.TV2))[kind[s] % 3]
        a, b = pair[0][r[s]], pair[1][r[s]]
        f = [ora.objective(pl[s], a, b, x, denovo) for x in (0.1, 0.5, 0.9)]
        assert min(f[0], f[2]) - f[1] > 1e-3 * abs(f[1]), (s, f)
    assert set(o["maxidx"][is_["triallelic"]].tolist()) == {1, 2}
    assert (o["maxidx"][is_["highaf"]] == 1).all() and (o["varfreq"][is_["highaf"], 1] < 0.3).all()
    everyone_hom_alt = is_["highaf"] & (kind % 2 == 1)
    assert (o["varfreq"][everyone_hom_alt, 1] < 1e-3).all() and everyone_hom_alt.any()
    if denovo:   # hom-ref parents, a hom-alt child in every family: a de novo record
        assert (o["emit"][is_["mendel"]] == 1).all() and (o["denovo_lr"][is_["mendel"]] > 0).all()
    if "real" in classes:
        assert (o["maxidx"][is_["real"]] > 0).any() and (o["maxidx"][is_["real"]] == 0).any()
    assert (o["n_cfg"][is_["dense"]] == 7).any()

    # read statistics, whoever is missing and whatever the depths and mapping qualities are
    td, nsd, ps, avgmq = hs.site_stats(dm)
    ok = ~is_["badref"]
    for f, want in (("total_depth", td), ("num_samp_with_data", nsd), ("perc_samp_with_data", ps), ("avg_map_qual", avgmq)):
        assert (o[f][ok] == want[ok]).all(), f
    nobody = is_["missing"] & (kind % 5 == 4)
    assert nobody.any() and (nsd[nobody] == 0).all()
    some = is_["missing"] & (kind % 5 != 4) & ((kind % 5 != 1) | (n_fam > 9))   # (family 0 + the last 8: all of <= 9)
    assert (nsd[some] > 0).all() and (nsd[some] < ped.n_person).all()
    assert (dm[is_["stats"] & (kind % 4 == 0)] == 0xFFFFFFFF).sum() == (is_["stats"] & (kind % 4 == 0)).sum() > 0
    assert ((dm[is_["stats"] & (kind % 4 == 2)] & 0xFFFFFF) == 1).all()

    c = ora.counters()
    assert c.transitions > 0 and c.transversions > 0 and c.tstvs1 > 0 and c.tstvs2 > 0 and c.tvs1tvs2 > 0 and c.homo_ref > 0
    # nothing a called site reports is NaN or infinite (the saturated `mendel` bytes included)
    for k in range(7):
        assert np.isfinite(o["varllk"][called & (o["n_cfg"] > k), k]).all(), k
    em = o["emit"] != 0
    assert em.any() and np.isfinite(o["af"][em]).all() and np.isfinite(o["denovo_lr"][em]).all()
    assert len(oc) == (o["emit"] == 1).sum() > 0 and np.isfinite(oc["dosage"]).all()


@pytest.mark.parametrize("shape,n_fam,n_sites,classes", DATASETS, ids=[d[0] for d in DATASETS])
def test_filter_params_put_sites_on_and_beyond_every_threshold(built, tmp_root, shape, n_fam, n_sites, classes):
    ped, pl, dm, ref, cls = _block(tmp_root, shape, n_fam, n_sites, classes)
    par, want = hs.filter_params((pl, dm, ref, cls))
    td, nsd, ps, avgmq = hs.site_stats(dm)
    ok = (ref >= 1) & (ref <= 4)
    reach_ps = ok & (td >= par.min_total_depth) & (td <= par.max_total_depth)
    reach_mq = reach_ps & (ps * 100 >= par.min_ps)
    for on, beyond in (((td == par.min_total_depth) & ok, want == 1), ((td == par.max_total_depth) & ok, want == 2),
                       ((ps * 100 == par.min_ps) & reach_ps, want == 3), ((avgmq == par.min_map_quality) & reach_mq, want == 4)):
        assert on.any() and beyond.any() and not (on & beyond).any()
    assert (avgmq[want == 4] > par.min_map_quality - 1).all()   # just beyond: one person's mapQ one lower
    ora = Oracle(ped.view, par)
    o, _ = ora.run(pl, dm, ref)
    assert (o["status"] == want).all()
    c = ora.counters()
    assert [c.min_total_depth_filter, c.max_total_depth_filter, c.min_ps_filter, c.min_map_qual_filter] == \
        [int((want == k).sum()) for k in (1, 2, 3, 4)]
    assert (want == 0).sum() > len(want) // 2   # the thresholds leave most sites to be called


def test_builder_is_deterministic(built, tmp_root):
    ped, pl, dm, ref, cls = _block(tmp_root, *DATASETS[0])
    again = hs.hard_block(ped, DATASETS[0][2], SEED, DATASETS[0][3])
    for a, b in zip((pl, dm, ref, cls), again):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    other = hs.hard_block(ped, DATASETS[0][2], SEED + 1, DATASETS[0][3])
    assert other[0].tobytes() != pl.tobytes()
    few = hs.hard_block(ped, 24, SEED, ("tv", "dense"))
    assert few[3].tolist() == ["tv", "dense"] * 12


def test_real_sites_are_the_example_records(built, tmp_root):
    """`real`: every family of a quad block holds the PL / depth / mapQ records of one example site and family, father,
    mother and children in the pedigree's roles; a trio takes father, mother and the first child."""
    eref, epl, edm, roles, _ = hs._example_data()
    erec = np.concatenate([epl, edm.view(np.uint8).reshape(edm.shape + (4,))], axis=2)
    for shape in ("quad", "trio"):
        ped, pl, dm, ref, cls = _block(tmp_root, *[d for d in DATASETS if d[0] == shape][0])
        rec = np.concatenate([pl, dm.view(np.uint8).reshape(dm.shape + (4,))], axis=2)
        size = 4 if shape == "quad" else 3
        for s in np.nonzero(cls == "real")[0][:4]:
            for f in range(ped.n_fam):
                efa, emo, ekids = roles[f % 3]
                cols = [efa, emo] + ekids[:size - 2]
                want = rec[s, f * size:(f + 1) * size]   # (synthetic nuclear families: father, mother, children)
                hit = (erec[:, cols] == want[None]).all(axis=(1, 2)) & (eref == ref[s])
                assert hit.any(), (shape, s, f)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if "hard" in c))
def test_glf_writer_round_trip(built, tmp_path, name):
    """write_glf_dataset -> pm.GlfReader returns the block bit for bit, at positions 2..n + 1 of section "1" (every record one past the last, as the generator writes them)."""
    case = CASES[name]
    assert case["sites"] <= 128 and case["families"] <= 13 and "badref" not in case["hard"]["classes"]
    make_dataset(name, str(tmp_path))
    ped, secs, sha = read_dataset(str(tmp_path))
    pl, dm, ref, cls = hs.hard_block(ped, case["sites"], case["seed"], tuple(case["hard"]["classes"]))
    (label, pos, gref, gpl, gdm), = secs
    assert label == "1" and pos.tolist() == list(range(2, case["sites"] + 2))
    for a, b in ((ref, gref), (pl, gpl), (dm, gdm)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert sha == case["block_sha256"]


def test_glf_writer_refuses_what_a_record_cannot_hold(tmp_path):
    pl, dm = np.zeros((2, 3, 10), np.uint8), np.zeros((2, 3), np.uint32)
    with pytest.raises(ValueError):
        hs.write_glf_dataset(str(tmp_path), pl, dm, np.array([1, 5], np.uint8))
    assert not os.listdir(tmp_path)
