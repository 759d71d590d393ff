#!/usr/bin/env python3
"""Cost of the transmission phase plane (pm_engine_set_vcf_phase) on vcf_mode engines: device-resident batches
(pm_engine_synth, (ref, alt = transition) per site as bench.py --vcf makes them), engines in flight as in bench.py --
tools/vcf_posteriors_cost.py's method.

Two geometries, each timed with the feature off and on in one session:
  config5  2000 mixed trio / quad families (BASELINE config 5): the standard posterior stage is k_posterior_lean<true>,
           the extra pass k_vcf_phase_lean -- expected: about one more lean posterior pass;
  ext10    200 three-generation families of 10: the standard stage is the compiled schedule's posterior kernel, the extra
           pass k_vcf_phase_nuc (no work: every family is peeled) + k_vcf_phase_es, eight generic peels per child where the
           posterior plane's k_vcf_post_es runs three per person.
Per geometry: wall time per batch off and on (each window ends in a device synchronise), `--repeats` runs of each
alternating with fresh engines, the medians' ratio (the figure DESIGN.md section 6 records) and the runs' range, and, apart
from the timed loop, the time to fetch one batch's plane to the host (pm_engine_vcf_phase: rows x n_person x 8 bytes).  No
threshold: nobody has measured this before.

Before anything is timed, the off case is shown to be the parent commit's: `--parent-root DIR` names a checkout of the
parent commit with its library built; a child process on that package and one on this tree each run one seeded batch per
geometry through pm_engine_run_vcf with every feature off and print a digest of the site results and genotype rows.  The
digests must be equal, or the tool stops.  Without --parent-root the profile records that the comparison was not made.

    python tools/vcf_phase_cost.py [--steps 200] [--repeats 3] [--parent-root DIR] [--out profiles/vcf_phase_cost.json]
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
sys.path.insert(0, os.environ.get("PM_PHASE_COST_PACKAGE_ROOT") or ROOT)   # (the digest child of --parent-root: its package)

import polymutt_amd as pm  # noqa: E402

GEOMETRIES = (("config5", "mixed", 2000), ("ext10", "ext10", 200))
TS = np.array([0, 3, 4, 1, 2], np.uint8)   # base -> its transition


def pedigree(shape, families):
    d = tempfile.mkdtemp(prefix="pm_vph_cost_")
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
    env["PM_PHASE_COST_PACKAGE_ROOT"] = package_root
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", "--digest-sites", str(sites), "--seed", str(seed)],
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"digest child failed ({r.returncode}): {r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def measure(ped, B, pool, n_eng, steps, warmup, on, seed):
    par = pm.Params.defaults(vcf_mode=1)
    engines = [pm.Engine(ped.view, par, max_batch=B) for _ in range(n_eng)]
    eng, npers = engines[0], ped.n_person
    bufs = []
    for p in range(pool):
        d_pl, d_ref, _ = synth_batch(eng, B, npers, seed, p * B)
        bufs.append((d_pl, None, d_ref))
    eng.sync()
    if on:
        for e in engines:
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
    if on:   # one batch's plane to the host, apart from the timed loop (the second fetch: the buffers are touched)
        eng.run_device(B, *bufs[0], None, None)
        eng.sync()
        for _ in range(2):
            t1 = time.perf_counter()
            ph = eng.vcf_phase()
            out["plane_fetch_ms"] = 1e3 * (time.perf_counter() - t1)
        out["plane_rows"] = int(ph.shape[0])
        out["plane_bytes"] = int(ph.nbytes)
        s = ph.astype(np.float64).sum(axis=-1)
        out["plane_in_range"] = bool(np.isfinite(ph).all() and (ph >= 0).all() and (s <= 1 + 2.0 ** -24).all())
        out["plane_share_nonzero"] = float((s > 0).mean())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_phase_cost.json"))
    a = ap.parse_args()
    if a.digest:
        print(json.dumps(digest(a.digest_sites, a.seed)))
        return
    out = {"config": {"batch": a.batch, "pool": a.pool, "engines": a.engines, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed},
           "kernels": {"config5": {"standard": "k_posterior_lean<true>", "extra_pass": "k_vcf_phase_lean"},
                       "ext10": {"standard": "compiled schedule's posterior kernel (es_post_jit)",
                                 "extra_pass": "k_vcf_phase_nuc (no work) + k_vcf_phase_es (eight generic reference-order peels per child)"}},
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
        runs = {False: [], True: []}
        for _ in range(a.repeats):   # off and on alternating, fresh engines each time
            for on in (False, True):
                runs[on].append(measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, on, a.seed))
        ms = {on: sorted(r["ms_per_batch"] for r in runs[on]) for on in runs}
        med = {on: ms[on][len(ms[on]) // 2] for on in ms}
        out[label] = {"shape": shape, "families": fams, "off": runs[False], "on": runs[True],
                      "ms_per_batch_off": {"median": med[False], "min": ms[False][0], "max": ms[False][-1]},
                      "ms_per_batch_on": {"median": med[True], "min": ms[True][0], "max": ms[True][-1]},
                      "on_over_off_time": med[True] / med[False]}
        print(label, json.dumps({k: out[label][k] for k in ("ms_per_batch_off", "ms_per_batch_on", "on_over_off_time")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
