#!/usr/bin/env python3
"""Cost of the per-person de novo posteriors (pm_engine_set_denovo_carriers) at bench.py's configuration: 1000 quads
under --denovo, 262 144-site device-resident batches (pm_engine_synth), 3 engines in flight, a pool of 4 batches.

Times the same steps with the feature off and with top_k = 4, and counts the written rows per batch (the kernel's
work is per written row).  The headline's synthetic sites hold no planted de novo mutation, so at the default
--minLLR_denovo almost no record is written; a second pair of timings with all_sites = 1 and minLLR 1e-300 (every site
with positive evidence is a row) shows the cost per row where there are rows.

--bench-lines FILE embeds the lines of a .jsonl file under "bench_feature_off": bench.py result lines of this tree and
of its parent commit taken in one session (each line a bench.py JSON object with a "tree" key added by whoever ran
them), the record that the feature left off costs nothing.

    python tools/denovo_carriers_cost.py [--steps 40] [--bench-lines FILE] [--out profiles/denovo_carriers_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import polymutt_amd as pm  # noqa: E402


def measure(ped, par, B, pool, n_eng, steps, warmup, top_k, seed):
    engines = [pm.Engine(ped, par, max_batch=B) for _ in range(n_eng)]
    eng, npers = engines[0], ped.n_person
    rsz = pm.engine.SITE_DTYPE.itemsize
    bufs = []
    for p in range(pool):
        b = (eng.alloc(B * npers * 10), eng.alloc(B * npers * 4), eng.alloc(B))
        eng.synth(B, seed, p * B, *b)
        bufs.append(b)
    eng.sync()
    if top_k:
        for e in engines:
            e.set_denovo_carriers(top_k)
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
    # rows per batch: one more pass over the pool on the first engine, results read back
    rows = []
    d_res = eng.alloc(B * rsz)
    for p in range(pool):
        eng.run_device(B, *bufs[p], d_res, None)
        eng.sync()
        r = np.zeros(B, pm.engine.SITE_DTYPE)
        eng.to_host(r, d_res, B * rsz)
        rows.append(int((r["call_row"] >= 0).sum()))
        if top_k:
            top, _ = eng.denovo_carriers()
            assert len(top) == rows[-1]
    eng.free(d_res)
    for b in bufs:
        for x in b:
            eng.free(x)
    for e in engines:
        e.close()
    return {"seconds": dt, "sites_per_s": steps * B / dt, "ms_per_batch": 1e3 * dt / steps, "rows_per_batch": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--families", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--engines", type=int, default=3)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denovo_carriers_cost.json"))
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    ped = bench.nuclear_pedigree(pm, a.families, 2)
    out = {"config": {"families": a.families, "shape": "quad", "denovo": 1, "batch": a.batch, "pool": a.pool,
                      "engines": a.engines, "steps": a.steps, "warmup": a.warmup, "top_k": a.top_k, "seed": a.seed}}
    for label, kw in (("default_minLLR", {}), ("every_positive_site_a_row", {"all_sites": 1, "denovo_min_llr": 1e-300})):
        par = pm.Params.defaults(denovo=1, **kw)
        off = measure(ped, par, a.batch, a.pool, a.engines, a.steps, a.warmup, 0, a.seed)
        on = measure(ped, par, a.batch, a.pool, a.engines, a.steps, a.warmup, a.top_k, a.seed)
        out[label] = {"off": off, "on": on, "on_over_off_time": on["seconds"] / off["seconds"]}
        print(label, json.dumps(out[label]), flush=True)
    if a.bench_lines:
        with open(a.bench_lines) as fh:
            out["bench_feature_off"] = [json.loads(l) for l in fh if l.strip()]
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
