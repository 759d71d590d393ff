"""The pipelined QUAD hoisting (hoist_quad_pipe_t, csrc/engine_dev.h: the next slot's ring dwords fetched under this
slot's arithmetic, the mutation-matrix rows loaded once per item, the DMA three slots ahead) computes the bytes the
earlier hoisting computed.  polymutt_amd/lib_exp/quad_hoist_v0.so is the same engine compiled with -DPM_QD_PIPE=0 (the
Makefile's `all` builds it next to lib/libpolymutt.so); each case runs the default library and quad_hoist_v0.so, each in
a fresh child process (POLYMUTT_LIB selects the library before anything is loaded), one after the other, on the same
synthetic quad sites under --denovo, and compares the site results and the genotype rows byte for byte.

Families (all multiples of 4, so n_person % 16 == 0 and the plan is a QUAD plan), 64 sites each, on the 64 x 16 lane plan
(the selection's own choice from 513 families on; PM_BRENT_TS=64,16 forces it for the small pedigrees, whose default
64 x 1 and 64 x 2 plans do not run the QUAD kernel):
     4   one slot row with 4 real lanes; every other row empty, every DMA window clamped
    64   exactly one full row
    68   one full row and a partial one
   960   15 full rows, the 16th all phantom
  1000   the headline: partial 16th row, clamped last window
  1024   every row full, no clamp
   300   the selection's 64 x 8 QUAD kernel (the other QUAD instantiation: the same loop at another unroll count),
         a partial 5th row and three empty ones
and for 68 and 1000 families one more run with LONG_SITES sites, at least as many as the persistent grid has blocks (8
per CU), so that every wave takes three or more items in turn: the hand-over of the ring from one item to the next
(the next item's first slots issued before this item's Brent loop), which 64 sites never reach.

Every case plants a de novo child (a ref/transition het call under two hom-ref parents, as synth.cpp's "+dn" does) at
a few sites, so that lists 1 and 2 (cfg 4-6 and the cfg-7 path) are not empty; the case asserts that records were
emitted for planted sites.  Each case asserts from brent_variants() that a QUAD (QD) kernel ran, in both libraries, and
records its S.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q0_LIB = os.path.join(ROOT, "polymutt_amd", "lib_exp", "quad_hoist_v0.so")
T_, S_, DN_, QD_ = 0, 1, 5, 8   # positions in a k_brent key (T, S, NUM, GEN, ES, DN, PF, EP, QD, NF, PD)
LONG_SITES = 2304   # >= 8 x 256 CUs

# name: (families, sites, S of the QUAD kernel, PM_BRENT_TS or None for the selection's own geometry)
CASES = {
    "f0004": (4, 64, 16, "64,16"),
    "f0064": (64, 64, 16, "64,16"),
    "f0068": (68, 64, 16, "64,16"),
    "f0960": (960, 64, 16, None),
    "f1000": (1000, 64, 16, None),
    "f1024": (1024, 64, 16, None),
    "f0300-s8": (300, 64, 8, None),
    "f0068-long": (68, LONG_SITES, 16, "64,16"),
    "f1000-long": (1000, LONG_SITES, 16, None),
}


def _pedigree(pm, n_fam):
    sys.path.insert(0, ROOT)
    import bench
    return bench.quad_pedigree(pm, n_fam, 2)


def _child(d, n_fam):
    """(child process) Run the sites of directory d on the library POLYMUTT_LIB names; results to d/out_<tag>.npz."""
    sys.path.insert(0, ROOT)
    import polymutt_amd as pm
    ped = _pedigree(pm, n_fam)
    pl, dm, ref = (np.load(os.path.join(d, f + ".npy")) for f in ("pl", "dm", "ref"))
    par = pm.Params.defaults(numerics=pm.NUM_POLY, denovo=1, denovo_mut_rate=1e-5)
    eng = pm.Engine(ped, par, max_batch=len(ref))
    try:
        res, calls = eng.run(pl, dm, ref)
        keys = np.array(eng.brent_variants(), dtype=np.int32).reshape(-1, 11)
    finally:
        eng.close()
    np.savez(os.path.join(d, "out_" + os.environ["PM_QD_TAG"] + ".npz"), res=res.view(np.uint8), calls=calls.view(np.uint8),
             keys=keys, lib=np.array(pm.LIB_PATH))


def _run_child(d, tag, lib, n_fam, ts):
    env = dict(os.environ, PM_QD_TAG=tag)
    env.pop("POLYMUTT_LIB", None)
    env.pop("PM_BRENT_TS", None)
    if ts:
        env["PM_BRENT_TS"] = ts
    if lib:
        env["POLYMUTT_LIB"] = lib
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), d, str(n_fam)], env=env, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    return np.load(os.path.join(d, "out_" + tag + ".npz"))


def _plant(pl, ref, n_fam, seed):
    """A de novo het call (ref / transition) in one kid of one family, under hom-ref parents, at every 16th site (and at
    site 1): synth.cpp's "+dn" records.  Returns the planted site indices."""
    gidx = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))
    rng = np.random.default_rng(seed)
    sites = sorted({1, *range(5, len(ref), 16)})
    for s in sites:
        r = int(ref[s])
        alt = {1: 3, 3: 1, 2: 4, 4: 2}[r]
        f = int(rng.integers(n_fam))
        kid = 4 * f + 2 + int(rng.integers(2))
        for p in (4 * f, 4 * f + 1):   # confident hom-ref parents
            pl[s, p, :] = 255
            pl[s, p, gidx[r - 1][r - 1]] = 0
            pl[s, p, gidx[r - 1][alt - 1]] = 60
        pl[s, kid, :] = 255
        pl[s, kid, gidx[r - 1][r - 1]] = 45
        pl[s, kid, gidx[r - 1][alt - 1]] = 0
        pl[s, kid, gidx[alt - 1][alt - 1]] = 90
    return np.array(sites)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_quad_hoist_pipe_is_byte_identical(built, tmp_path, name):
    import polymutt_amd as pm
    n_fam, n_sites, S, ts = CASES[name]
    assert os.path.exists(Q0_LIB), "lib_exp/quad_hoist_v0.so: built by `make -C polymutt_amd` (__graft_entry__.build())"
    d = str(tmp_path)
    ped = _pedigree(pm, n_fam)
    assert ped.n_person == 4 * n_fam and ped.n_person % 16 == 0
    pl, dm, ref = pm.synth_block_host(ped, n_sites, 1000 + n_fam)
    planted = _plant(pl, ref, n_fam, n_fam)
    for f, a in (("pl", pl), ("dm", dm), ("ref", ref)):
        np.save(os.path.join(d, f + ".npy"), a)
    new = _run_child(d, "new", None, n_fam, ts)
    old = _run_child(d, "q0", Q0_LIB, n_fam, ts)
    assert str(new["lib"]).endswith(os.path.join("lib", "libpolymutt.so")) and str(old["lib"]) == Q0_LIB
    # a QUAD kernel ran, in both libraries
    for z in (new, old):
        ks = [tuple(int(x) for x in k) for k in z["keys"]]
        qd = sorted({k[S_] for k in ks if k[QD_] and k[DN_] and k[T_] == 64})
        assert qd == [S], (name, ks)
    print(f"{name}: QUAD k_brent at 64 x S, S = {qd}")
    res = new["res"].view(pm.engine.SITE_DTYPE)
    assert (res["status"] == 0).sum() > 0 and (res["emit"] != 0).sum() > 0   # sites were called and records emitted
    assert (res["emit"][planted] != 0).any(), "no planted de novo site was emitted"
    assert new["res"].shape == old["res"].shape and new["calls"].shape == old["calls"].shape
    assert new["res"].tobytes() == old["res"].tobytes(), "site results differ"
    assert new["calls"].tobytes() == old["calls"].tobytes(), "genotype rows differ"
    assert (new["keys"] == old["keys"]).all()


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
