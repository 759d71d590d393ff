#!/usr/bin/env python3
"""Cost of naming the families and children behind each DQ (pm_engine_set_vcf_denovo_detail) on vcf_mode engines with
pm_engine_set_vcf_denovo on: the geometries and the device-resident batches of tools/vcf_denovo_cost.py.

  config5  2000 mixed trio / quad families (BASELINE config 5): k_vdn_who<256>, one lane per child, registers only;
  ext10    200 three-generation families of 10: k_vdn_who<256>, clamped three-state peels (up to 13 per child and row).
Each geometry at the default denovo_min_llr (0.01: the rows a CLI run has) and at 1e-300 (every site with positive de novo
evidence), --vcf_denovo alone against the detail on with fam_k = car_k = 4.  Per run: the rows per batch
(pm_engine_vcf_denovo_rows of one batch), the wall time per batch with the engines in flight, and the kernel time per
batch: k_vdn_rows + k_vdn_who have no timer of their own (pm_kernel_stats covers the Brent launches), so it is the
difference of the per-batch wall time of ONE engine, synchronised after every batch, with the detail on and off.  Every
figure is one timing, not a distribution.

--bench-lines FILE embeds the lines of a .jsonl file under "bench_feature_off": bench.py result lines of this tree and
of its parent commit taken alternately in one session, the record that the feature left off costs nothing.

    python tools/vcf_denovo_detail_cost.py [--steps 24] [--bench-lines FILE] [--out profiles/vcf_denovo_detail_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import polymutt_amd as pm  # noqa: E402
from vcf_denovo_cost import pedigree  # noqa: E402


def measure(ped, B, pool, n_eng, steps, warmup, detail, min_llr, seed):
    par = pm.Params.defaults(vcf_mode=1, denovo_min_llr=min_llr)
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
    for e in engines:
        e.set_vcf_denovo(True)
        if detail:
            e.set_vcf_denovo_detail(4, 4)
    pending = [False] * n_eng

    def timed(count, n_used):
        """count batches over the first n_used engines; a batch waits only for its engine's previous one"""
        for k in range(n_used):
            pending[k] = False
        t0 = time.perf_counter()
        for i in range(count):
            k = i % n_used
            if pending[k]:
                engines[k].sync()
            engines[k].run_device(B, *bufs[i % pool], None, None)
            pending[k] = True
        for k in range(n_used):
            if pending[k]:
                engines[k].sync()
                pending[k] = False
        return time.perf_counter() - t0

    timed(warmup, n_eng)
    for e in engines:
        e.kernel_stats(reset=True)
    dt = timed(steps, n_eng)
    st = [e.kernel_stats() for e in engines]
    brent_ms = sum(s.kernel_ms for s in st) + sum(s.es_hoist_ms for s in st)
    dt1 = timed(steps, 1)   # one engine: nothing overlaps, the batches' kernels run back to back
    eng.run_device(B, *bufs[0], None, None)
    eng.sync()
    rows = len(eng.vcf_denovo_rows()) if detail else None
    for b in bufs:
        eng.free(b[0])
        eng.free(b[2])
    for e in engines:
        e.close()
    return {"seconds": dt, "sites_per_s": steps * B / dt, "ms_per_batch": 1e3 * dt / steps,
            "brent_kernel_ms_per_batch": brent_ms / steps, "one_engine_ms_per_batch": 1e3 * dt1 / steps, "rows_per_batch": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pool", type=int, default=2)
    ap.add_argument("--engines", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_denovo_detail_cost.json"))
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    out = {"config": {"batch": a.batch, "pool": a.pool, "engines": a.engines, "steps": a.steps, "warmup": a.warmup, "seed": a.seed,
                      "fam_k": 4, "car_k": 4},
           "note": "each figure is one timing, not a distribution; detail_kernels_ms_per_batch = one_engine_ms_per_batch with "
                   "the detail on minus off (k_vdn_rows + k_vdn_who, plus their launch overhead)",
           "kernels": {"config5": "k_vdn_rows + k_vdn_who<256>: 2000 closed-form nuclear families, one lane per child",
                       "ext10": "k_vdn_rows + k_vdn_who<256>: 200 peeled families, clamped three-state peels"}}
    for label, shape, fams in (("config5", "mixed", 2000), ("ext10", "ext10", 200)):
        ped = pedigree(shape, fams)
        out[label] = {"shape": shape, "families": fams}
        for name, llr in (("min_llr_default", 0.01), ("min_llr_1e-300", 1e-300)):
            off = measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, False, llr, a.seed)
            on = measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, True, llr, a.seed)
            out[label][name] = {"denovo_min_llr": llr, "vcf_denovo_alone": off, "detail_on": on, "rows_per_batch": on["rows_per_batch"],
                                "on_over_off_time": on["seconds"] / off["seconds"],
                                "detail_kernels_ms_per_batch": on["one_engine_ms_per_batch"] - off["one_engine_ms_per_batch"]}
            print(label, name, json.dumps(out[label][name]), flush=True)
    if a.bench_lines:
        with open(a.bench_lines) as fh:
            out["bench_feature_off"] = [json.loads(l) for l in fh if l.strip()]
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
