"""The k_brent selection (polymutt_amd/csrc/brent_plan.h) agrees with the variant list (brent_variants.h, written by
tools/gen_brent_variants.py) and with the selection code of the commit before brent_plan.h, without a GPU.

tests/native/plan_check enumerates the selection over lane-plan geometries (forced with PM_BRENT_TS and by preference) x
numerics x --denovo x chromosome class x pedigree shape x persons x plane alignment x item list x switches, one line per
case.  tests/golden/brent_plan/selection_sha256.json holds each (numerics, denovo, class) slice's SHA-256 and line
count as recorded from the previous selection code (`recorded_from`, `how`), so a change that is meant to leave the
selection alone is checked to the last case.  A change MEANT to alter it (a new variant, another preference order)
re-records with

    python tests/test_cpu_brent_plan.py --record

after the GPU parity tests have passed on the new selection.  Never re-record to make a refactor pass."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "brent_plan", "selection_sha256.json")
EXE = os.path.join(ROOT, "tests", "native", "build", "plan_check")
SLICES = [f"{n}/{d}/{c}" for n in range(3) for d in range(2) for c in range(4)]   # pm_numerics / denovo / pm_chrom


def _run(*args):
    # (always through make, a no-op when up to date: a plan_check older than brent_plan.h would pass for the wrong reason)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "polymutt_amd"), "../tests/native/build/plan_check"], check=True)
    r = subprocess.run([EXE, *args], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-2000:]).decode()
    return r.stdout


def _slice(name):
    out = _run("cases", *name.split("/"))
    return {"sha256": hashlib.sha256(out).hexdigest(), "lines": out.count(b"\n"), "none": out.count(b"-> none\n")}


@pytest.mark.parametrize("name", SLICES)
def test_selection_is_unchanged(name):
    """Every case of the slice selects the recorded kernel and launch flavour, or `none` where the recorded code had
    no kernel either (the `none` cases are therefore exactly the recorded ones)."""
    golden = json.load(open(GOLDEN))
    assert sorted(golden["slices"]) == sorted(SLICES)
    assert _slice(name) == golden["slices"][name], f"selection differs from {golden['recorded_from']}"


def test_selection_and_variant_list_agree():
    """Every selected key is an instantiation, except keys only a PM_BRENT_TS geometry asks for (plan_check exits 1 when
    a preferred geometry has no kernel); those keys are the recorded ones; every instantiation is selected by a case."""
    golden = json.load(open(GOLDEN))
    lines = _run("summary").decode().splitlines()
    cases, variants = int(lines[0].split()[1]), int(lines[0].split()[3])
    assert cases == sum(s["lines"] for s in golden["slices"].values()) and variants == 157
    assert [l.split()[1] for l in lines if l.startswith("none ")] == golden["none_keys"]
    assert sum(int(l.split("(")[1].split()[0]) for l in lines if l.startswith("none ")) == sum(s["none"] for s in golden["slices"].values())
    assert [l.split()[1] for l in lines if l.startswith("unused ")] == golden["unused_variants"] == []


def test_generator_reproduces_the_committed_header(tmp_path):
    out = str(tmp_path / "brent_variants.h")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_brent_variants.py"), out], check=True, capture_output=True)
    assert open(out, "rb").read() == open(os.path.join(ROOT, "polymutt_amd", "csrc", "brent_variants.h"), "rb").read()


@pytest.mark.parametrize("n_fam,n_person,denovo,want", [(300, 1200, 1, (64, 8)), (512, 2048, 1, (64, 8)), (600, 2400, 1, (64, 16)),
                                                        (1000, 4000, 1, (64, 16)), (1024, 4096, 1, (64, 16)), (2000, 7000, 0, (128, 16))])
def test_choose_geometry_known_plans(n_fam, n_person, denovo, want):
    """The lane plans tests/test_gpu_engine.py asserts on hardware through eng.plan() (quads under --denovo; 2000 mixed
    trios and quads), from choose_geometry alone, POLY numerics."""
    assert tuple(int(x) for x in _run("geometry", str(n_fam), str(n_person), "4", str(denovo), "2").split()) == want


def _record():
    doc = json.load(open(GOLDEN))
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True, check=True).stdout.strip()
    doc["recorded_from"] = git("rev-parse", "HEAD") + (" + uncommitted changes" if git("status", "--porcelain", "--", "polymutt_amd/csrc") else "")
    doc["how"] = "python tests/test_cpu_brent_plan.py --record"
    doc["slices"] = {name: _slice(name) for name in SLICES}
    summary = _run("summary").decode().splitlines()
    doc["none_keys"] = [l.split()[1] for l in summary if l.startswith("none ")]
    doc["unused_variants"] = [l.split()[1] for l in summary if l.startswith("unused ")]
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{GOLDEN}: {len(SLICES)} slices from {doc['recorded_from']}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_cpu_brent_plan.py --record")
    _record()
