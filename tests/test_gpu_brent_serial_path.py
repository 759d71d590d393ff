"""The shortened serial path of the Brent evaluation (csrc/brent_core.h, engine_dev.h) computes the bytes the earlier
path computed.  polymutt_amd/lib_exp/serial_v0.so is the same engine compiled with -DPM_SERIAL_V0=1 (the Makefile's
`all` builds it next to lib/libpolymutt.so); each case runs the default library and serial_v0.so, each in a fresh
child process (POLYMUTT_LIB selects the library before anything is loaded), one after the other, on the same sites, and
compares the site results and the genotype rows byte for byte.

Cases, by the kernel and the reduction they reach (synthetic sites; "+dn" plants a de novo child):
  quad+dn 1024 x 64 --denovo   the QUAD kernel at 64 x 16, every slot row full
  quad+dn  300 x 128 --denovo  the QUAD kernel with a partial last slot row (phantom families)
  quad+dn 1100 x 32 --denovo   more families than one wave holds: block_logprod across waves
  trio+dn   40 x 200           plain trios: the lean kernel on prefetched planes (PF)
  ext10+dn   8 x 64            bi-allelic extended pedigrees: the run-time compiled ep_brent_jit, two items per wave
                               (wave_prod_pair, log10_mant_pair)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V0_LIB = os.path.join(ROOT, "polymutt_amd", "lib_exp", "serial_v0.so")
T_, S_, DN_, PF_, QD_ = 0, 1, 5, 6, 8   # positions in a k_brent key (T, S, NUM, GEN, ES, DN, PF, EP, QD, NF, PD)

# name: (shape, families, sites, --denovo, seed, check of the launched k_brent keys)
CASES = {
    "quad-full-rows": ("quad+dn", 1024, 64, 1, 21, lambda ks: any(k[T_] == 64 and k[S_] == 16 and k[QD_] for k in ks)),
    "quad-partial-row": ("quad+dn", 300, 128, 1, 21, lambda ks: any(k[T_] == 64 and k[QD_] for k in ks)),
    "quad-multi-wave": ("quad+dn", 1100, 32, 1, 21, lambda ks: any(k[T_] > 64 and k[DN_] for k in ks)),
    "trio-plain-pf": ("trio+dn", 40, 200, 0, 4, lambda ks: any(k[PF_] and not k[DN_] for k in ks)),
    "ext10-fused-pair": ("ext10+dn", 8, 64, 0, 34, lambda ks: ks == []),   # (the fused kernel: no k_brent launch)
}


def _child(d, denovo):
    """(child process) Run the sites of directory d on the library POLYMUTT_LIB names; results to d/out_<tag>.npz."""
    sys.path.insert(0, ROOT)
    import polymutt_amd as pm
    ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
    z = np.load(os.path.join(d, "sites.npz"))
    par = pm.Params.defaults(numerics=pm.NUM_POLY, denovo=denovo, denovo_mut_rate=1e-5 if denovo else 1.5e-8)
    eng = pm.Engine(ped.view, par, max_batch=len(z["ref"]))
    try:
        res, calls = eng.run(z["pl"], z["dm"], z["ref"])
        keys = np.array(eng.brent_variants(), dtype=np.int32).reshape(-1, 11)
    finally:
        eng.close()
    np.savez(os.path.join(d, "out_" + os.environ["PM_SERIAL_TAG"] + ".npz"), res=res.view(np.uint8), calls=calls.view(np.uint8),
             keys=keys, lib=np.array(pm.LIB_PATH))


def _run_child(d, tag, lib, denovo, extra_env):
    env = dict(os.environ, PM_SERIAL_TAG=tag, **extra_env)
    env.pop("POLYMUTT_LIB", None)
    if lib:
        env["POLYMUTT_LIB"] = lib
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__), d, str(denovo)], env=env, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    z = np.load(os.path.join(d, "out_" + tag + ".npz"))
    return z, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_serial_path_is_byte_identical(built, tmp_path, name):
    import polymutt_amd as pm
    shape, n_fam, n_sites, denovo, seed, keys_ok = CASES[name]
    assert os.path.exists(V0_LIB), "lib_exp/serial_v0.so: built by `make -C polymutt_amd` (__graft_entry__.build())"
    d = str(tmp_path)
    pm.synth_write_dataset(d, shape, n_fam, n_sites, seed)
    ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rd = pm.GlfReader(ped, "test.gif")
        (pos, ref, pl, dm), = [rd.read(1024) for _ in rd.sections()]
        rd.close()
    finally:
        os.chdir(cwd)
    assert len(ref) == n_sites and ped.n_fam == n_fam
    np.savez(os.path.join(d, "sites.npz"), pl=pl, dm=dm, ref=ref)
    for f in os.listdir(d):   # (one GLF file per person: the children read sites.npz)
        if f not in ("test.dat", "test.ped", "sites.npz"):
            os.unlink(os.path.join(d, f))
    fused = name == "ext10-fused-pair"
    extra = {"PM_JIT_LAYOUT": "1", "PM_FUSED_PAIR": "1"} if fused else {}
    new, err_new = _run_child(d, "new", None, denovo, extra)
    old, err_old = _run_child(d, "v0", V0_LIB, denovo, extra)
    assert str(new["lib"]).endswith(os.path.join("lib", "libpolymutt.so")) and str(old["lib"]) == V0_LIB
    # the case reached the kernel it is for, in both libraries
    for z, err in ((new, err_new), (old, err_old)):
        ks = [tuple(int(x) for x in k) for k in z["keys"]]
        assert keys_ok(ks), (name, ks)
        if fused:
            assert "ep_brent_jit" in err and "two items per wave" in err, err[-500:]
    res = new["res"].view(pm.engine.SITE_DTYPE)
    assert (res["status"] == 0).sum() > 0 and (res["emit"] != 0).sum() > 0   # sites were called and records emitted
    assert new["res"].shape == old["res"].shape and new["calls"].shape == old["calls"].shape
    assert new["res"].tobytes() == old["res"].tobytes(), "site results differ"
    assert new["calls"].tobytes() == old["calls"].tobytes(), "genotype rows differ"
    assert (new["keys"] == old["keys"]).all()


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]))
