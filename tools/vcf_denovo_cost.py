#!/usr/bin/env python3
"""Cost of de novo calling from VCF input (pm_engine_set_vcf_denovo) on vcf_mode engines: device-resident batches
(pm_engine_synth, (ref, alt = transition) per site as bench.py --vcf makes them), engines in flight as in bench.py.

Two geometries, each timed with the feature off and on in one session:
  config5  2000 mixed trio / quad families (BASELINE config 5): the standard item runs the lean split-plan k_brent, the
           de novo item k_vdn_brent<256> (nuclear families in closed form, coefficients in LDS);
  ext10    200 three-generation families of 10: the standard item runs the compiled peeling schedule (fused hoisting +
           Brent), the de novo item k_vdn_brent<256> with the reference-order three-state peel per evaluation.
Per run: wall time per batch and the summed Brent kernel time per batch (pm_kernel_stats.kernel_ms, which includes the de
novo Brent launch when the feature is on).

--bench-lines FILE embeds the lines of a .jsonl file under "bench_feature_off": bench.py result lines of this tree and
of its parent commit taken in one session (each line a bench.py JSON object with a "tree" key added by whoever ran
them), the record that the feature left off costs nothing.

    python tools/vcf_denovo_cost.py [--steps 24] [--bench-lines FILE] [--out profiles/vcf_denovo_cost.json]
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
    d = tempfile.mkdtemp(prefix="pm_vdn_cost_")
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
            e.set_vcf_denovo(True)
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
    for e in engines:
        e.kernel_stats(reset=True)
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    drain()
    dt = time.perf_counter() - t0
    st = [e.kernel_stats() for e in engines]
    brent_ms = sum(s.kernel_ms for s in st) + sum(s.es_hoist_ms for s in st)
    launches = sum(s.launches for s in st)
    # one batch's results: how many sites were called and carry a DQ
    rsz = pm.engine.SITE_DTYPE.itemsize
    d_res = eng.alloc(B * rsz)
    eng.run_device(B, *bufs[0], d_res, None)
    eng.sync()
    r = np.zeros(B, pm.engine.SITE_DTYPE)
    eng.to_host(r, d_res, B * rsz)
    eng.free(d_res)
    for b in bufs:
        eng.free(b[0])
        eng.free(b[2])
    for e in engines:
        e.close()
    return {"seconds": dt, "sites_per_s": steps * B / dt, "ms_per_batch": 1e3 * dt / steps,
            "brent_kernel_ms_per_batch": brent_ms / steps, "brent_launches_per_batch": launches / steps,
            "called_sites_per_batch": int((r["status"] == 0).sum()), "sites_with_dq_per_batch": int((r["evals"][:, 2] > 0).sum()),
            "mean_evals_standard": float(r["evals"][:, 1].mean()), "mean_evals_denovo": float(r["evals"][:, 2].mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pool", type=int, default=2)
    ap.add_argument("--engines", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_denovo_cost.json"))
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    out = {"config": {"batch": a.batch, "pool": a.pool, "engines": a.engines, "steps": a.steps, "warmup": a.warmup, "seed": a.seed},
           "kernels": {"config5": {"standard": "k_brent<128, 16, POLY, lean, PF, NF = 34> (split trio / quad plan)",
                                   "denovo": "k_vdn_brent<256> + k_finalize_vdn"},
                       "ext10": {"standard": "compiled peeling schedule (fused hoisting + Brent, ep_brent_jit)",
                                 "denovo": "k_vdn_brent<256> (generic reference-order three-state peel per evaluation, no "
                                           "run-time compiled kernel) + k_finalize_vdn"}}}
    for label, shape, fams in (("config5", "mixed", 2000), ("ext10", "ext10", 200)):
        ped = pedigree(shape, fams)
        off = measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, False, a.seed)
        on = measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, True, a.seed)
        out[label] = {"shape": shape, "families": fams, "off": off, "on": on,
                      "on_over_off_time": on["seconds"] / off["seconds"],
                      "on_over_off_brent_kernel_time": on["brent_kernel_ms_per_batch"] / off["brent_kernel_ms_per_batch"]}
        print(label, json.dumps(out[label]), flush=True)
    if a.bench_lines:
        with open(a.bench_lines) as fh:
            out["bench_feature_off"] = [json.loads(l) for l in fh if l.strip()]
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
