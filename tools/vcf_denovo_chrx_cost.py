#!/usr/bin/env python3
"""Cost of de novo calling on chrX VCF records (pm_engine_set_vcf_denovo_chrx) at config 5's geometry: 2000 mixed trio /
quad families, device-resident batches (pm_engine_synth, (ref, alt = transition) per site as bench.py --vcf makes them),
one engine, every batch synchronised.

States, each timed as `runs` windows of `steps` batches after a warm-up, interleaved run by run, the median reported:
  x_off        a chrX section, no de novo feature (the parent commit's behaviour on chrX);
  x_vcf_denovo a chrX section, pm_engine_set_vcf_denovo alone (nothing runs on X);
  x_on         a chrX section with the X switch on: k_vdn_brent_x peels every family on every evaluation;
  x_detail     x_on plus the detail at fam_k = car_k = 2 and pm_engine_set_vcf_denovo_chrx_detail: k_vdn_rows and
               k_vdn_who_x per row (the row count of the last batch is reported beside the time);
  auto_off, auto_vcf_denovo  an autosomal section without and with pm_engine_set_vcf_denovo (k_vdn_brent's hoisted
               quartics), for comparison.
--min-llr X creates the engine with denovo_min_llr = X (the row threshold); --low-min-llr X also times x_on and x_detail
in a second process at that threshold, low enough that rows exist on the synthetic data.
--parent-lib FILE also times auto_vcf_denovo and x_on on another build of the library -- the parent commit's -- in
child processes alternated with this tree's (which of the two goes first alternates too), for the record that neither path
moved with the new switch off.

    python tools/vcf_denovo_chrx_cost.py [--runs 5] [--steps 4] [--parent-lib FILE] [--low-min-llr 1e-300]
                                         [--out profiles/vcf_denovo_chrx_detail_cost.json]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATES = {   # name -> (chromosome class, vcf_denovo, X switch, the detail and its X switch)
    "x_off": (1, False, False, False),
    "x_vcf_denovo": (1, True, False, False),
    "x_on": (1, True, True, False),
    "x_detail": (1, True, True, True),
    "auto_off": (0, False, False, False),
    "auto_vcf_denovo": (0, True, False, False),
}


def measure(states, families, B, runs, steps, warmup, seed, old_lib, min_llr=None):
    import polymutt_amd as pm
    if old_lib:   # a library from before the feature: it lacks the symbol
        pm.engine.EXPORTS.pop("pm_engine_set_vcf_denovo_chrx_detail", None)
    d = tempfile.mkdtemp(prefix="pm_vdnx_cost_")
    pm.synth_write_dataset(d, "mixed", families, 1, 7)
    ped = pm.Pedigree(os.path.join(d, "test.dat"), os.path.join(d, "test.ped"))
    shutil.rmtree(d, ignore_errors=True)
    par = pm.Params.defaults(vcf_mode=1) if min_llr is None else pm.Params.defaults(vcf_mode=1, denovo_min_llr=min_llr)
    eng = pm.Engine(ped.view, par, max_batch=B)
    npers = ped.n_person
    d_pl, d_dm, d_ref = eng.alloc(B * npers * 10), eng.alloc(B * npers * 4), eng.alloc(B)
    eng.synth(B, seed, 0, d_pl, d_dm, d_ref)
    href = np.empty(B, np.uint8)
    eng.to_host(href, d_ref, B)
    href = (href | (np.array([0, 3, 4, 1, 2], np.uint8)[href] << 4)).astype(np.uint8)
    eng.to_device(d_ref, href, B)
    eng.free(d_dm)
    rsz = pm.engine.SITE_DTYPE.itemsize
    d_res = eng.alloc(B * rsz)
    eng.sync()

    def enter(name):
        chrom, vdn, x, detail = STATES[name]
        eng.set_vcf_denovo_detail(0, 0)
        eng.set_vcf_denovo(vdn)
        if x:
            eng.set_vcf_denovo_chrx(True)
        if detail:
            eng.set_vcf_denovo_detail(2, 2)
            eng.set_vcf_denovo_chrx_detail(True)
        eng.begin_section(chrom)

    def window(n):
        t0 = time.perf_counter()
        for _ in range(n):
            eng.run_device(B, d_pl, None, d_ref, d_res, None)
            eng.sync()
        return (time.perf_counter() - t0) / n

    out = {s: {"ms_per_batch_runs": []} for s in states}
    for s in states:   # warm-up of every state: code objects, run-time compiled kernels
        enter(s)
        window(warmup)
        r = np.zeros(B, pm.engine.SITE_DTYPE)
        eng.to_host(r, d_res, B * rsz)
        out[s].update(called_sites_per_batch=int((r["status"] == 0).sum()), sites_with_dq_per_batch=int((r["evals"][:, 2] > 0).sum()),
                      mean_evals_standard=float(r["evals"][:, 1].mean()), mean_evals_denovo=float(r["evals"][:, 2].mean()),
                      detail_rows_per_batch=len(eng.vcf_denovo_rows()), denovo_min_llr=float(par.denovo_min_llr))
    for _ in range(runs):
        for s in states:
            enter(s)
            window(1)
            out[s]["ms_per_batch_runs"].append(1e3 * window(steps))
    for s in states:
        v = out[s]["ms_per_batch_runs"]
        out[s].update(ms_per_batch_median=statistics.median(v), ms_per_batch_min=min(v), ms_per_batch_max=max(v),
                      sites_per_s_median=B / statistics.median(v) * 1e3)
    for p in (d_pl, d_ref, d_res):
        eng.free(p)
    eng.close()
    return out


def child(lib, args, states, old_lib):
    env = dict(os.environ)
    env.pop("POLYMUTT_LIB", None)
    if lib:
        env["POLYMUTT_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(states), "--runs", str(args.runs), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--batch", str(args.batch), "--families", str(args.families), "--seed", str(args.seed)]
    if old_lib:
        cmd.append("--old-lib")
    if args.min_llr is not None:
        cmd += ["--min-llr", repr(args.min_llr)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child failed ({r.returncode}): {r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--families", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--revision", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcf_denovo_chrx_detail_cost.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--old-lib", action="store_true")
    ap.add_argument("--min-llr", type=float, default=None)
    ap.add_argument("--low-min-llr", type=float, default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child.split(","), a.families, a.batch, a.runs, a.steps, a.warmup, a.seed, a.old_lib, a.min_llr)))
        return
    rev = a.revision
    if rev is None and os.path.exists(os.path.join(ROOT, "REVISION")):
        rev = open(os.path.join(ROOT, "REVISION")).read().strip()
    out = {"revision": rev,
           "config": {"shape": "mixed", "families": a.families, "batch": a.batch, "runs": a.runs, "steps_per_run": a.steps,
                      "warmup_batches": a.warmup, "seed": a.seed, "engines": 1},
           "note": "ms per batch of one engine, each batch synchronised; median / min / max over the runs, the states "
                   "interleaved run by run in one process",
           "kernels": {"x_on": "k_vdn_brent_x<256> + k_finalize_vdn after the standard chrX item (plan 1)",
                       "x_detail": "x_on + k_vdn_rows + k_vdn_who_x<256> (fam_k = car_k = 2, no full matrices)",
                       "auto_vcf_denovo": "k_vdn_brent<256> + k_finalize_vdn after the lean split-plan k_brent"}}
    out["this_tree"] = child(None, a, list(STATES), False)
    t = out["this_tree"]
    out["x_on_over_x_off_time"] = t["x_on"]["ms_per_batch_median"] / t["x_off"]["ms_per_batch_median"]
    out["x_on_added_ms_per_batch"] = t["x_on"]["ms_per_batch_median"] - t["x_vcf_denovo"]["ms_per_batch_median"]
    out["x_detail_over_x_on_time"] = t["x_detail"]["ms_per_batch_median"] / t["x_on"]["ms_per_batch_median"]
    out["x_detail_rows_per_batch"] = t["x_detail"]["detail_rows_per_batch"]
    out["auto_added_ms_per_batch"] = t["auto_vcf_denovo"]["ms_per_batch_median"] - t["auto_off"]["ms_per_batch_median"]
    print(json.dumps(out["this_tree"]), flush=True)
    if a.low_min_llr is not None:   # the same two states where rows exist
        keep, a.min_llr = a.min_llr, a.low_min_llr
        low = child(None, a, ["x_on", "x_detail"], False)
        a.min_llr = keep
        out["this_tree_low_min_llr"] = low
        out["low_min_llr_x_detail_over_x_on_time"] = low["x_detail"]["ms_per_batch_median"] / low["x_on"]["ms_per_batch_median"]
        out["low_min_llr_x_detail_rows_per_batch"] = low["x_detail"]["detail_rows_per_batch"]
        print(json.dumps(low), flush=True)
    if a.parent_lib:   # alternate the two builds, a fresh process each
        pair = ["auto_vcf_denovo", "x_on"]
        rounds = []
        for k in range(4):   # which build goes first alternates, so that the order is not mistaken for the build
            r = {}
            for tree in (("this_tree", "parent") if k % 2 == 0 else ("parent", "this_tree")):
                r[tree] = child(None, a, pair, False) if tree == "this_tree" else child(a.parent_lib, a, pair, True)
            r["first"] = "this_tree" if k % 2 == 0 else "parent"
            rounds.append(r)
            print(json.dumps(r), flush=True)
        out["parent_ab"] = {"rounds": rounds}
        for s in pair:
            for tree in ("this_tree", "parent"):
                out["parent_ab"][f"{s}_{tree}_ms_per_batch_medians"] = [r[tree][s]["ms_per_batch_median"] for r in rounds]
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
