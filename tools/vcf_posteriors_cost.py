#!/usr/bin/env python3
"""Cost of the genotype posterior plane (pm_engine_set_vcf_posteriors) on vcf_mode engines: device-resident batches
(pm_engine_synth, (ref, alt = transition) per site as bench.py --vcf makes them), engines in flight as in bench.py.

Two geometries, each timed with the feature off and on in one session:
  config5  2000 mixed trio / quad families (BASELINE config 5): the standard posterior stage is k_posterior_lean<true>,
           the extra pass k_vcf_post_lean;
  ext10    200 three-generation families of 10: the standard stage is the compiled schedule's posterior kernel, the extra
           pass k_vcf_post_nuc (no work: every family is peeled) + k_vcf_post_es (three generic peels per person).
Per geometry: wall time per batch off and on, `--repeats` runs of each alternating with fresh engines, the medians' ratio
(the figure DESIGN.md section 6 records) and the runs' range, and, apart from the timed loop, the time to fetch one
batch's plane to the host (pm_engine_vcf_posteriors: rows x n_person x 12 bytes, three times the bytes of the genotype
rows).

    python tools/vcf_posteriors_cost.py [--steps 200] [--repeats 3] [--out profiles/vcf_posteriors_cost.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import polymutt_amd as pm  # noqa: E402


def pedigree(shape, families):
    d = tempfile.mkdtemp(prefix="pm_vp_cost_")
    pm.synth_write_dataset(d, shape, families, 1, 7)
    ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
    shutil.rmtree(d, ignore_errors=True)
    return ped


def measure(ped, B, pool, n_eng, steps, warmup, on, seed):
    par = pm.Params.defaults(vcf_mode=1)
    engines = [pm.Engine(ped.view, par, max_batch=B) for _ in range(n_eng)]
    eng, npers = engines[0], ped.n_person
    ts = np.array([0, 3, 4, 1, 2], np.uint8)
    bufs = []
    for p in range(pool):
        d_pl, d_dm, d_ref = eng.alloc(B * npers * 10), eng.alloc(B * npers * 4), eng.alloc(B)
        eng.synth(B, seed, p * B, d_pl, d_dm, d_ref)
        href = np.empty(B, np.uint8)
        eng.to_host(href, d_ref, B)
        href = (href | (ts[href] << 4)).astype(np.uint8)
        eng.to_device(d_ref, href, B)
        eng.free(d_dm)
        bufs.append((d_pl, None, d_ref))
    eng.sync()
    if on:
        for e in engines:
            e.set_vcf_posteriors(True)
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
            post = eng.vcf_posteriors()
            out["plane_fetch_ms"] = 1e3 * (time.perf_counter() - t1)
        out["plane_rows"] = int(post.shape[0])
        out["plane_bytes"] = int(post.nbytes)
        s = post.astype(np.float64).sum(axis=-1)
        out["plane_rows_sum_to_one"] = bool((np.abs(s - 1) <= 3 * 2.0 ** -25).all())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_posteriors_cost.json"))
    a = ap.parse_args()
    out = {"config": {"batch": a.batch, "pool": a.pool, "engines": a.engines, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed},
           "kernels": {"config5": {"standard": "k_posterior_lean<true>", "extra_pass": "k_vcf_post_lean"},
                       "ext10": {"standard": "compiled schedule's posterior kernel (es_post_jit)",
                                 "extra_pass": "k_vcf_post_nuc (no work) + k_vcf_post_es (generic reference-order peels)"}}}
    for label, shape, fams in (("config5", "mixed", 2000), ("ext10", "ext10", 200)):
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
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
