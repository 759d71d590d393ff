"""The schedule compiler's generated kernel text is pinned: for seven synthetic pedigrees and four switch settings,
every source polymutt_amd/csrc/es_jit.cpp generates (12 generate() runs: 4 chromosome classes x bi-allelic / --denovo
grouped / --denovo all, and the generate_fused() runs that yield a kernel) has the SHA-256 and the byte length recorded
in tests/golden/jit/source_sha256.json.  Byte-identical source under unchanged hipRTC flags gives identical code
objects, so a change to the generator that is meant to leave the kernels alone (a refactor) is checked here, on the
CPU, to the last byte.

Re-recording is a deliberate act that goes with a change MEANT to alter the generated kernels (then the GPU parity
tests are what checks the new kernels): build the tree whose output is to be pinned and run

    python tests/test_cpu_jit_source.py --record

which rewrites the JSON and notes the commit (and whether es_jit.cpp had uncommitted changes) it was made from.  Never
re-record to make a refactor pass."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jit", "source_sha256.json")
EXE = os.path.join(ROOT, "tests", "native", "build", "jit_check")

# pm.synth_write_dataset(dir, shape, families, 1, 3): test_schedule_compiler_builds_every_class's call; quadext with 257
# families has one extended family among nuclear ones
SHAPES = {"ext10": 5, "roof": 5, "roof2": 5, "ext12": 5, "ext11": 5, "extmix": 5, "quadext": 257}
ENVS = {"default": {}, "sp3_off": {"PM_ES_SP3": "0"}, "t3z_off": {"PM_ES_T3Z": "0"}, "prof": {"PM_ES_PROF": "1"}}


def _dump(shape, env_name, data_dir, out_dir):
    """jit_check --emit-all --no-compile on the shape's pedigree: {file: [sha256, bytes]} of the sources in out_dir."""
    import polymutt_amd as pm
    # (always through make, a no-op when up to date: a jit_check older than es_jit.cpp would pass for the wrong reason)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "polymutt_amd"), "../tests/native/build/jit_check"], check=True)
    if not os.path.exists(os.path.join(data_dir, "test.ped")):
        os.makedirs(data_dir, exist_ok=True)
        pm.synth_write_dataset(str(data_dir), shape, SHAPES[shape], 1, 3)
    os.makedirs(out_dir, exist_ok=True)
    # (only the switches of the case: none of the generator's PM_* knobs leaks in from the caller's environment)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PM_")}
    env.update(ENVS[env_name])
    r = subprocess.run([EXE, os.path.join(data_dir, "test.dat"), os.path.join(data_dir, "test.ped"), "--emit-all", str(out_dir),
                        "--no-compile"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for f in sorted(os.listdir(out_dir)):
        text = open(os.path.join(out_dir, f), "rb").read()
        got[f] = [hashlib.sha256(text).hexdigest(), len(text)]
    return got


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    return tmp_path_factory.mktemp("jit_source_data")


@pytest.mark.parametrize("env_name", list(ENVS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_generated_source_is_unchanged(tmp_path, datasets, shape, env_name):
    """Every generated source of the (pedigree, switches) case has the recorded SHA-256 and length.  On a mismatch the
    first differing file is named and the dump stays in tmp_path (diff it against a dump of the recorded commit)."""
    golden = json.load(open(GOLDEN))
    want = golden["cases"][f"{shape}/{env_name}"]
    got = _dump(shape, env_name, os.path.join(datasets, shape), tmp_path / "src")
    # 12 generate() runs and at least one fused kernel
    assert len(want) >= 13 and sum(f.startswith("class") for f in want) == 12, sorted(want)
    assert sorted(got) == sorted(want), f"generated files differ (dump kept in {tmp_path / 'src'})"
    for f in sorted(want):
        assert got[f] == want[f], (f"{f}: sha256/bytes {got[f]} but {want[f]} recorded from {golden['recorded_from']}; "
                                   f"dump kept in {tmp_path / 'src'}")


def _record():
    import tempfile
    sys.path.insert(0, ROOT)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "polymutt_amd"), "../tests/native/build/jit_check"], check=True)
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True, check=True).stdout.strip()
    commit = git("rev-parse", "HEAD")
    if git("status", "--porcelain", "--", "polymutt_amd/csrc/es_jit.cpp", "polymutt_amd/csrc/es_jit.h"):
        commit += " + uncommitted changes to es_jit"
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for shape in SHAPES:
            for env_name in ENVS:
                cases[f"{shape}/{env_name}"] = _dump(shape, env_name, os.path.join(tmp, shape), os.path.join(tmp, shape, env_name))
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as fh:
        json.dump({"what": "SHA-256 and byte length of the sources polymutt_amd/csrc/es_jit.cpp generates "
                           "(tests/test_cpu_jit_source.py; jit_check --emit-all --no-compile)",
                   "recorded_from": commit, "cases": cases}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{GOLDEN}: {len(cases)} cases from {commit}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_cpu_jit_source.py --record")
    _record()
