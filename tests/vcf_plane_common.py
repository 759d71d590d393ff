"""What the GPU tests of the three output planes of the --in_vcf path share (tests/test_gpu_vcf_posteriors.py,
test_gpu_vcf_phase.py, test_gpu_vcf_joint.py): the cached engine cases, the loop over a case's batches through one entry
point, and the CLI helpers.  Each test module keeps its own assertions and tolerances.
"""
import os
import subprocess

import numpy as np

import polymutt_amd as pm
from conftest import EXAMPLE
from vcf_phase_reference import large_nuclear_case, make_case

SRC = os.path.join(EXAMPLE, "testvcf.in.vcf.gz")

_DATA = {}


def dataset(tmp_path_factory, prefix, shape, nfam, nsites=96):
    """(owner of the pedigree, its view, block, refalt), generated once per case and left unchanged.  "nuclear": the
    pedigree with families of three and four children, which no synthetic shape reaches."""
    key = (prefix, shape, nfam, nsites)
    if key not in _DATA:
        if shape == "nuclear":
            ped, block, refalt = large_nuclear_case(nsites)
            _DATA[key] = (ped, ped, block, refalt)
        else:
            ped, block, refalt = make_case(str(tmp_path_factory.mktemp(f"{prefix}_{shape}_{nfam}")), shape, nfam, nsites)
            _DATA[key] = (ped, ped.view, block, refalt)
    return _DATA[key]


def run_batches(eng, block, refalt, batch, entry, fetch):
    """Every batch through one entry point ("run", "run_vcf" or submit and collect): (results, calls as (best, gq, label)
    int arrays, [fetch(the batch's genotype rows) per batch])."""
    res, calls, got = [], [], []
    zeros = np.zeros(block.shape[:2], np.uint32)
    for s in range(0, len(refalt), batch):
        sl = slice(s, s + batch)
        if entry == "run":
            r, c = eng.run(block[sl], zeros[sl], refalt[sl])
        elif entry == "run_vcf":
            r, c = eng.run_vcf(block[sl], refalt[sl])
        else:
            eng.submit(block[sl], zeros[sl], refalt[sl])
            r, c = eng.collect()
        res.append(r)
        calls.append(np.stack([c[f].astype(np.int16) for f in ("best", "gq", "label")], axis=-1))
        got.append(fetch(c))
    return np.concatenate(res), np.concatenate(calls), got


def cli(tmp_path, name, extra, src=None):
    """The example through the polymutt binary with `extra` options: the output's lines."""
    out = tmp_path / name
    r = subprocess.run([pm.BIN_PATH, "-p", "test.ped", "-d", "test.dat", "--in_vcf", src or SRC, "--out_vcf", str(out)] + extra,
                       cwd=EXAMPLE, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out.read_text().splitlines()


def strip_fields(lines, ids, placed, unphase=False):
    """The output without the header lines and sub-fields of the FORMAT keys `ids` (adjacent, in this order; placed(fmt, k)
    says whether the first may stand at index k of the record's FORMAT keys), and with `unphase` every phased GT unphased
    again."""
    n = len(ids)
    out = []
    for l in lines:
        if any(l.startswith(f"##FORMAT=<ID={i},") for i in ids):
            continue
        if l.startswith("#"):
            out.append(l)
            continue
        c = l.split("\t")
        fmt = c[8].split(":")
        k = fmt.index(ids[0])
        assert fmt[k:k + n] == list(ids) and placed(fmt, k), c[8]
        c[8] = ":".join(fmt[:k] + fmt[k + n:])
        for i in range(9, len(c)):
            v = c[i].split(":")
            if unphase and "|" in v[0]:
                assert v[0] in ("0|1", "1|0"), v[0]
                v[0] = "0/1"
            c[i] = ":".join(v[:k] + v[k + n:])
        out.append("\t".join(c))
    return out


def same(a, b):   # (the ##Polymutt= line records the command line)
    drop = lambda ls: [l for l in ls if not l.startswith("##Polymutt=")]
    return drop(a) == drop(b)
