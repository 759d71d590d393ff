#!/usr/bin/env python3
"""Cost of the joint call plane (pm_engine_set_vcf_joint) on vcf_mode engines: device-resident batches (pm_engine_synth,
(ref, alt = transition) per site as bench.py --vcf makes them), engines in flight as in bench.py --
tools/vcf_phase_cost.py's method.

Two geometries, each timed with the feature off, with it on, and with the phase plane on instead (the pass the joint one is
to be compared with on peeled families), in one session:
  config5  2000 mixed trio / quad families (BASELINE config 5): the standard posterior stage is k_posterior_lean<true>,
           the extra pass k_vcf_joint_lean;
  ext10    200 three-generation families of 10: the standard stage is the compiled schedule's posterior kernel, the extra
           pass k_vcf_joint_nuc (no work: every family is peeled) + k_vcf_joint_es, one sum peel and one max peel with its
           backtrack per family, where k_vcf_phase_es runs eight peels per child.
Per geometry: wall time per batch off, on and with the phase plane (each window ends in a device synchronise), `--repeats`
runs of each alternating with fresh engines, the medians' ratios (the figures DESIGN.md section 6 records) and the runs'
range, and, apart from the timed loop, the time to fetch one batch's plane to the host (pm_engine_vcf_joint: rows x
n_person x 8 bytes).  No threshold: nobody has measured this before.

Before anything is timed, the off case is shown to be the parent commit's: `--parent-root DIR` names a checkout of the
parent commit with its library built; a child process on that package and one on this tree each run one seeded batch per
geometry through pm_engine_run_vcf with every feature off and print a digest of the site results and genotype rows.  The
digests must be equal, or the tool stops.  Without --parent-root the profile records that the comparison was not made.

    python tools/vcf_joint_cost.py [--steps 200] [--repeats 3] [--parent-root DIR] [--out profiles/vcf_joint_cost.json]
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("PM_JOINT_COST_PACKAGE_ROOT") or ROOT)   # (the digest child of --parent-root: its package)

import polymutt_amd as pm  # noqa: E402

GEOMETRIES = (("config5", "mixed", 2000), ("ext10", "ext10", 200))
TS = np.array([0, 3, 4, 1, 2], np.uint8)   # base -> its transition


def pedigree(shape, families):
    d = tempfile.mkdtemp(prefix="pm_vj_cost_")
    pm.synth_write_dataset(d, shape, families, 1, 7)
    ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
    shutil.rmtree(d, ignore_errors=True)
    return ped


def synth_batch(eng, B, npers, seed, offset):
    """Device buffers (pl genotype-planar, ref with alt = the transition) of one seeded batch."""
    d_pl, d_dm, d_ref = eng.alloc(B * npers * 10), eng.alloc(B * npers * 4), eng.alloc(B)
    eng.synth(B, seed, offset, d_pl, d_dm, d_ref)
    href = np.empty(B, np.uint8)
    eng.to_host(href, d_ref, B)
    href = (href | (TS[href] << 4)).astype(np.uint8)
    eng.to_device(d_ref, href, B)
    eng.free(d_dm)
    return d_pl, d_ref, href


def digest(sites, seed):
    """sha256 of the site results and genotype rows of one seeded batch per geometry, every feature off."""
    out = {}
    for label, shape, fams in GEOMETRIES:
        ped = pedigree(shape, fams)
        eng = pm.Engine(ped.view, pm.Params.defaults(vcf_mode=1), max_batch=sites)
        npers = ped.n_person
        d_pl, d_ref, href = synth_batch(eng, sites, npers, seed, 0)
        planar = np.empty(sites * npers * 10, np.uint8)
        eng.to_host(planar, d_pl, planar.nbytes)
        block = np.ascontiguousarray(planar.reshape(sites, 10, npers).transpose(0, 2, 1))   # person-major, as the host path takes it
        res, calls = eng.run_vcf(block, href)
        h = hashlib.sha256()
        h.update(res.tobytes())
        h.update(calls.tobytes())
        out[label] = {"sites": sites, "rows": int(len(calls)), "sha256": h.hexdigest()}
        eng.free(d_pl)
        eng.free(d_ref)
        eng.close()
    return out


def digest_child(package_root, sites, seed):
    env = dict(os.environ)
    env.pop("POLYMUTT_LIB", None)
    env["PM_JOINT_COST_PACKAGE_ROOT"] = package_root
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", "--digest-sites", str(sites), "--seed", str(seed)],
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"digest child failed ({r.returncode}): {r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def measure(ped, B, pool, n_eng, steps, warmup, mode, seed):
    """mode: "off", "joint" (the feature) or "phase" (pm_engine_set_vcf_phase, for comparison)."""
    par = pm.Params.defaults(vcf_mode=1)
    engines = [pm.Engine(ped.view, par, max_batch=B) for _ in range(n_eng)]
    eng, npers = engines[0], ped.n_person
    bufs = []
    for p in range(pool):
        d_pl, d_ref, _ = synth_batch(eng, B, npers, seed, p * B)
        bufs.append((d_pl, None, d_ref))
    eng.sync()
    for e in engines:
        if mode == "joint":
            e.set_vcf_joint(True)
        elif mode == "phase":
            e.set_vcf_phase(True)
    pending = [False] * n_eng

    def step(i):
        k = i % n_eng
        if pending[k]:
            engines[k].sync()
        engines[k].run_device(B, *bufs[i % pool], None, None)
        pending[k] = True

    def drain():
        for k, e in enumerate(engines):
            if pending[k]:
                e.sync()
                pending[k] = False

    for i in range(warmup):
        step(i)
    drain()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    drain()
    dt = time.perf_counter() - t0
    out = {"seconds": dt, "sites_per_s": steps * B / dt, "ms_per_batch": 1e3 * dt / steps}
    if mode == "joint":   # one batch's plane to the host, apart from the timed loop (the second fetch: the buffers are touched)
        eng.run_device(B, *bufs[0], None, None)
        eng.sync()
        for _ in range(2):
            t1 = time.perf_counter()
            g, lp = eng.vcf_joint()
            out["plane_fetch_ms"] = 1e3 * (time.perf_counter() - t1)
        out["plane_rows"] = int(g.shape[0])
        out["plane_bytes"] = int(g.shape[0] * g.shape[1] * pm.VCF_JOINT_DTYPE.itemsize)
        out["plane_in_range"] = bool(np.isfinite(lp).all() and (lp <= 2.0 ** -23).all() and np.isin(g, (0, 1, 2, 255)).all())
        out["plane_share_assigned"] = float((g != 255).mean())
        out["plane_mean_lp"] = float(lp[g != 255].mean()) if (g != 255).any() else None
    for b in bufs:
        eng.free(b[0])
        eng.free(b[2])
    for e in engines:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="off / on pairs per geometry (the ratio is of the medians)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pool", type=int, default=2)
    ap.add_argument("--engines", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--digest", action="store_true", help="(child) print the feature-off digests and stop")
    ap.add_argument("--digest-sites", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_joint_cost.json"))
    a = ap.parse_args()
    if a.digest:
        print(json.dumps(digest(a.digest_sites, a.seed)))
        return
    out = {"config": {"batch": a.batch, "pool": a.pool, "engines": a.engines, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed},
           "kernels": {"config5": {"standard": "k_posterior_lean<true>", "extra_pass": "k_vcf_joint_lean", "phase_pass": "k_vcf_phase_lean"},
                       "ext10": {"standard": "compiled schedule's posterior kernel (es_post_jit)",
                                 "extra_pass": "k_vcf_joint_nuc (no work) + k_vcf_joint_es (one sum peel, one max peel and its backtrack per family)",
                                 "phase_pass": "k_vcf_phase_nuc (no work) + k_vcf_phase_es (eight generic reference-order peels per child)"}},
           "per_kernel_times": "unmeasured (no trace taken)"}
    if a.parent_root:   # the off case is the parent commit's, byte for byte, before anything is timed
        mine, parent = digest_child(ROOT, a.digest_sites, a.seed), digest_child(os.path.abspath(a.parent_root), a.digest_sites, a.seed)
        out["off_is_parent"] = {"this_tree": mine, "parent": parent, "identical": mine == parent}
        print("off_is_parent", json.dumps(out["off_is_parent"]), flush=True)
        if mine != parent:
            raise SystemExit("the feature-off output differs from the parent commit's: nothing timed")
    else:
        out["off_is_parent"] = {"identical": None, "note": "not compared: no --parent-root given"}
    for label, shape, fams in GEOMETRIES:
        ped = pedigree(shape, fams)
        modes = ("off", "joint", "phase")
        runs = {m: [] for m in modes}
        for _ in range(a.repeats):   # the three alternating, fresh engines each time
            for m in modes:
                runs[m].append(measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, m, a.seed))
        ms = {m: sorted(r["ms_per_batch"] for r in runs[m]) for m in modes}
        med = {m: ms[m][len(ms[m]) // 2] for m in modes}
        summary = lambda m: {"median": med[m], "min": ms[m][0], "max": ms[m][-1]}
        out[label] = {"shape": shape, "families": fams, "off": runs["off"], "on": runs["joint"], "phase_on": runs["phase"],
                      "ms_per_batch_off": summary("off"), "ms_per_batch_on": summary("joint"), "ms_per_batch_phase_on": summary("phase"),
                      "on_over_off_time": med["joint"] / med["off"], "phase_on_over_off_time": med["phase"] / med["off"],
                      "extra_pass_over_phase_pass": (med["joint"] - med["off"]) / (med["phase"] - med["off"])}
        print(label, json.dumps({k: out[label][k] for k in ("ms_per_batch_off", "ms_per_batch_on", "ms_per_batch_phase_on", "on_over_off_time",
                                                                "phase_on_over_off_time", "extra_pass_over_phase_pass")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
