#!/usr/bin/env python3
"""Cost of one output plane of vcf_mode engines -- `--plane posteriors` (pm_engine_set_vcf_posteriors), `phase`
(pm_engine_set_vcf_phase) or `joint` (pm_engine_set_vcf_joint) -- or of the pedigree check, `--plane pedcheck`
(pm_engine_set_vcf_pedcheck: no plane, sums per non-founder; timed next to the phase and the joint plane): device-resident batches (pm_engine_synth, (ref, alt =
transition) per site as bench.py --vcf makes them), engines in flight as in bench.py.

Two geometries, each timed with the feature off and on in one session (the joint plane also with the phase plane on
instead, the pass it is to be compared with on peeled families):
  config5  2000 mixed trio / quad families (BASELINE config 5): the standard posterior stage is k_posterior_lean<true>,
           the extra pass the plane's lean kernel -- about one more lean posterior pass;
  ext10    200 three-generation families of 10: the standard stage is the compiled schedule's posterior kernel, the extra
           pass the plane's nuc kernel (no work: every family is peeled) + its es kernel: three generic peels per person
           (posteriors), eight per child (phase), one sum peel and one max peel with its backtrack per family (joint).
Per geometry: wall time per batch in each mode (each window ends in a device synchronise), `--repeats` runs of each
alternating with fresh engines, the medians' ratios (the figures DESIGN.md section 6 records) and the runs' range, and,
apart from the timed loop, the time to fetch one batch's plane to the host (rows x n_person x 12 or 8 bytes).  No
threshold.  The JSON keys are those of profiles/vcf_posteriors_cost.json, vcf_phase_cost.json and vcf_joint_cost.json.

Before anything is timed, the off case is shown to be the parent commit's: `--parent-root DIR` names a checkout of the
parent commit with its library built; a child process on that package and one on this tree each run one seeded batch per
geometry through pm_engine_run_vcf with every feature off and print a digest of the site results and genotype rows.  With
`--digest-planes` the children then turn the three planes on, run the batch again and add a sha256 of each plane's bytes.
The digests must be equal, or the tool stops.  Without --parent-root the profile records that the comparison was not made.

    python tools/vcf_plane_cost.py --plane phase [--steps 200] [--repeats 3] [--parent-root DIR [--digest-planes]] [--out FILE]
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
sys.path.insert(0, os.environ.get("PM_PLANE_COST_PACKAGE_ROOT") or ROOT)   # (the digest child of --parent-root: its package)

import polymutt_amd as pm  # noqa: E402

GEOMETRIES = (("config5", "mixed", 2000), ("ext10", "ext10", 200))
TS = np.array([0, 3, 4, 1, 2], np.uint8)   # base -> its transition
STANDARD = {"config5": "k_posterior_lean<true>", "ext10": "compiled schedule's posterior kernel (es_post_jit)"}


def post_stats(eng):
    post = eng.vcf_posteriors()
    s = post.astype(np.float64).sum(axis=-1)
    return post.shape[0], int(post.nbytes), {"plane_rows_sum_to_one": bool((np.abs(s - 1) <= 3 * 2.0 ** -25).all())}


def phase_stats(eng):
    ph = eng.vcf_phase()
    s = ph.astype(np.float64).sum(axis=-1)
    return ph.shape[0], int(ph.nbytes), {"plane_in_range": bool(np.isfinite(ph).all() and (ph >= 0).all() and (s <= 1 + 2.0 ** -24).all()),
                                         "plane_share_nonzero": float((s > 0).mean())}


def joint_stats(eng):
    g, lp = eng.vcf_joint()
    return g.shape[0], int(g.shape[0] * g.shape[1] * pm.VCF_JOINT_DTYPE.itemsize), {
        "plane_in_range": bool(np.isfinite(lp).all() and (lp <= 2.0 ** -23).all() and np.isin(g, (0, 1, 2, 255)).all()),
        "plane_share_assigned": float((g != 255).mean()),
        "plane_mean_lp": float(lp[g != 255].mean()) if (g != 255).any() else None}


def pedcheck_stats(eng):
    pc = eng.vcf_pedcheck()
    return int(pc.n.max(initial=0)), int(len(pc.person) * pm.VCF_PEDCHECK_DTYPE.itemsize), {
        "non_founders": int(len(pc.person)), "all_counted_alike": bool((pc.n == pc.n.max(initial=0)).all()),
        "share_all_links_supported": float((pc.llr > 0).all(axis=1).mean()) if len(pc.person) else None,
        "sums_sha256": hashlib.sha256(pc.n.tobytes() + pc.q.tobytes()).hexdigest()}


# per plane: the engine's setter, the plane's figures after a batch, the extra pass per geometry, what else is timed
# (mode -> the JSON prefix of its keys) and whether the profile carries the two keys the first tool did not write
PLANES = {
    "posteriors": {"setter": "set_vcf_posteriors", "stats": post_stats, "also": {}, "notes": False,
                   "extra_pass": {"config5": "k_vcf_post_lean", "ext10": "k_vcf_post_nuc (no work) + k_vcf_post_es (generic reference-order peels)"}},
    "phase": {"setter": "set_vcf_phase", "stats": phase_stats, "also": {}, "notes": True,
              "extra_pass": {"config5": "k_vcf_phase_lean",
                             "ext10": "k_vcf_phase_nuc (no work) + k_vcf_phase_es (eight generic reference-order peels per child)"}},
    "joint": {"setter": "set_vcf_joint", "stats": joint_stats, "also": {"phase": "phase_"}, "notes": True,
              "extra_pass": {"config5": "k_vcf_joint_lean",
                             "ext10": "k_vcf_joint_nuc (no work) + k_vcf_joint_es (one sum peel, one max peel and its backtrack per family)"}},
    "pedcheck": {"setter": "set_vcf_pedcheck", "stats": pedcheck_stats, "also": {"phase": "phase_", "joint": "joint_"}, "notes": True,
                 "extra_pass": {"config5": "k_vcf_pedcheck_lean",
                                "ext10": "k_vcf_pedcheck_es (four generic reference-order peels per child)"}},
}
OUTPUT_PLANES = ("posteriors", "phase", "joint")   # what --digest-planes covers (the parent commit's package has these)


def pedigree(shape, families):
    d = tempfile.mkdtemp(prefix="pm_plane_cost_")
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


def digest(sites, seed, planes):
    """sha256 of the site results and genotype rows of one seeded batch per geometry, every feature off; with `planes`
    also of each plane's bytes after the same batch with the three planes on."""
    sha = lambda *arrays: hashlib.sha256(b"".join(a.tobytes() for a in arrays)).hexdigest()
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
        out[label] = {"sites": sites, "rows": int(len(calls)), "sha256": sha(res, calls)}
        if planes:
            for k in OUTPUT_PLANES:
                getattr(eng, PLANES[k]["setter"])(True)
            res, calls = eng.run_vcf(block, href)
            out[label]["planes_on_sha256"] = sha(res, calls)
            out[label]["planes"] = {"posteriors": sha(eng.vcf_posteriors()), "phase": sha(eng.vcf_phase()), "joint": sha(*eng.vcf_joint())}
        eng.free(d_pl)
        eng.free(d_ref)
        eng.close()
    return out


def digest_child(package_root, sites, seed, planes):
    env = dict(os.environ)
    env.pop("POLYMUTT_LIB", None)
    env["PM_PLANE_COST_PACKAGE_ROOT"] = package_root
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--digest", "--digest-sites", str(sites), "--seed", str(seed)] +
                       (["--digest-planes"] if planes else []), env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"digest child failed ({r.returncode}): {r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def measure(ped, B, pool, n_eng, steps, warmup, plane, seed):
    """plane: a key of PLANES, or None for every feature off."""
    par = pm.Params.defaults(vcf_mode=1)
    engines = [pm.Engine(ped.view, par, max_batch=B) for _ in range(n_eng)]
    eng, npers = engines[0], ped.n_person
    bufs = []
    for p in range(pool):
        d_pl, d_ref, _ = synth_batch(eng, B, npers, seed, p * B)
        bufs.append((d_pl, None, d_ref))
    eng.sync()
    if plane:
        for e in engines:
            getattr(e, PLANES[plane]["setter"])(True)
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
    if plane:   # one batch's plane to the host, apart from the timed loop (the second fetch: the buffers are touched)
        eng.run_device(B, *bufs[0], None, None)
        eng.sync()
        for _ in range(2):
            t1 = time.perf_counter()
            rows, nbytes, more = PLANES[plane]["stats"](eng)
            out["plane_fetch_ms"] = 1e3 * (time.perf_counter() - t1)
        out.update({"plane_rows": int(rows), "plane_bytes": nbytes}, **more)
    for b in bufs:
        eng.free(b[0])
        eng.free(b[2])
    for e in engines:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plane", choices=sorted(PLANES), help="the plane to time (not needed with --digest)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3, help="off / on pairs per geometry (the ratio is of the medians)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pool", type=int, default=2)
    ap.add_argument("--engines", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--digest", action="store_true", help="(child) print the feature-off digests and stop")
    ap.add_argument("--digest-planes", action="store_true", help="the digests also cover the three planes' bytes")
    ap.add_argument("--digest-sites", type=int, default=1024)
    ap.add_argument("--out", default=None, help="default: profiles/vcf_<plane>_cost.json")
    a = ap.parse_args()
    if a.digest:
        print(json.dumps(digest(a.digest_sites, a.seed, a.digest_planes)))
        return
    if not a.plane:
        ap.error("--plane is required")
    P = PLANES[a.plane]
    out = {"config": {"batch": a.batch, "pool": a.pool, "engines": a.engines, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed},
           "kernels": {g: dict({"standard": STANDARD[g], "extra_pass": P["extra_pass"][g]},
                               **{pre + "pass": PLANES[m]["extra_pass"][g] for m, pre in P["also"].items()}) for g in STANDARD}}
    if P["notes"]:
        out["per_kernel_times"] = "unmeasured (no trace taken)"
    if a.parent_root:   # the off case is the parent commit's, byte for byte, before anything is timed
        mine = digest_child(ROOT, a.digest_sites, a.seed, a.digest_planes)
        parent = digest_child(os.path.abspath(a.parent_root), a.digest_sites, a.seed, a.digest_planes)
        out["off_is_parent"] = {"this_tree": mine, "parent": parent, "identical": mine == parent}
        print("off_is_parent", json.dumps(out["off_is_parent"]), flush=True)
        if mine != parent:
            raise SystemExit("the output differs from the parent commit's: nothing timed")
    elif P["notes"]:
        out["off_is_parent"] = {"identical": None, "note": "not compared: no --parent-root given"}
    modes = {"off": None, "on": a.plane, **{pre + "on": m for m, pre in P["also"].items()}}   # JSON name -> plane
    for label, shape, fams in GEOMETRIES:
        ped = pedigree(shape, fams)
        runs = {m: [] for m in modes}
        for _ in range(a.repeats):   # the modes alternating, fresh engines each time
            for m, plane in modes.items():
                runs[m].append(measure(ped, a.batch, a.pool, a.engines, a.steps, a.warmup, plane, a.seed))
        ms = {m: sorted(r["ms_per_batch"] for r in runs[m]) for m in modes}
        med = {m: ms[m][len(ms[m]) // 2] for m in modes}
        g = out[label] = dict({"shape": shape, "families": fams}, **runs)
        for m in modes:
            g["ms_per_batch_" + m] = {"median": med[m], "min": ms[m][0], "max": ms[m][-1]}
        for m in modes:
            if m != "off":
                g[m + "_over_off_time"] = med[m] / med["off"]
        for pre in P["also"].values():
            g["extra_pass_over_" + pre + "pass"] = (med["on"] - med["off"]) / (med[pre + "on"] - med["off"])
        print(label, json.dumps({k: v for k, v in g.items() if k.startswith("ms_per_batch_") or "_over_" in k}), flush=True)
    path = a.out or os.path.join(ROOT, "profiles", f"vcf_{a.plane}_cost.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
