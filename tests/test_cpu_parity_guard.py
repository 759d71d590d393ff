"""The comparisons themselves (parity.compare_results, fixtures.compare_to_dump) must fail on a non-finite value:
`|engine - oracle| > tol` is False for a NaN.  A real oracle result on hard sites (tests/hard_sites.py: every float field
is compared at some site) is doctored with NaN / +inf / -inf in each compared field in turn, on either side; every
doctored pair must raise, the undoctored pair and a pair holding the identical non-finite value on both sides must
pass."""
import numpy as np
import pytest

from fixtures import compare_to_dump, golden_dump, make_dataset, params_and_chrom, read_dataset
from oracle_binding import Oracle
from parity import compare_results

CASE = "hard_quad_denovo"
BAD = [np.nan, np.inf, -np.inf]


@pytest.fixture(scope="module")
def result(built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("guard"))
    case = make_dataset(CASE, d)
    ped, secs, _ = read_dataset(d)
    par, chrom = params_and_chrom(case["flags"])
    ora = Oracle(ped.view, par)
    ora.begin_section(chrom)
    (label, pos, ref, pl, dm), = secs
    res, calls = ora.run(pl, dm, ref)
    res.setflags(write=False)
    calls.setflags(write=False)
    return res, calls, golden_dump(CASE)


def _site(mask):
    assert mask.any()
    return int(np.nonzero(mask)[0][0])


def _site_fields(res, emitted):
    """(field, column or None, a site at which the comparison looks at it)."""
    called = res["status"] == 0
    out = [("varllk", k, _site(called & (res["n_cfg"] > k))) for k in range(7)]
    out += [("varfreq", k, _site(called & (res["n_cfg"] > k))) for k in range(1, 7)]
    out += [("var_post_prob", None, _site(called)), ("poly_qual", None, _site(called))]
    return out, _site(emitted)


def _poke(a, field, col, site, value):
    if isinstance(a, dict):   # (a reference dump: one array per field)
        b = dict(a)
        b[field] = a[field].copy()
    else:
        b = a.copy()
    if col is None:
        b[field][site] = value
    else:
        b[field][site, col] = value
    return b


def test_compare_results_rejects_non_finite_values(result):
    res, calls, _ = result
    assert compare_results(res, res.copy(), calls, calls.copy())["called"] > 0
    fields, em = _site_fields(res, res["emit"] != 0)
    fields += [(f, None, em) for f in ("af", "ab", "denovo_lr")]
    for field, col, site in fields:
        for v in BAD:
            bad = _poke(res, field, col, site, v)
            for e, o in ((bad, res), (res, bad)):
                with pytest.raises(AssertionError):
                    compare_results(e, o, calls, calls)
            compare_results(bad, bad.copy(), calls, calls)   # the identical non-finite value on both sides
        with pytest.raises(AssertionError):                  # ... but not two different ones
            compare_results(_poke(res, field, col, site, np.inf), _poke(res, field, col, site, np.nan), calls, calls)
    assert calls.size
    for v in BAD:
        bad = calls.copy()
        bad["dosage"][0, -1] = v
        for e, o in ((bad, calls), (calls, bad)):
            with pytest.raises(AssertionError):
                compare_results(res, res, e, o)
        compare_results(res, res, bad, bad.copy())
        compare_results(res, res, bad, calls, dosage=False)   # (vcf_mode rows carry no dosage: not compared)


def test_compare_to_dump_rejects_non_finite_values(result):
    res, _, dump = result
    assert compare_to_dump(res, dump)["called"] > 0
    fields, em = _site_fields(res, dump["emitted"] == 1)
    fields += [("denovo_lr", None, em)]
    for field, col, site in fields:
        for v in BAD:
            bad = _poke(res, field, col, site, v)
            with pytest.raises(AssertionError):
                compare_to_dump(bad, dump)
            dbad = _poke(dump, field, col, site, v)
            with pytest.raises(AssertionError):
                compare_to_dump(res, dbad)
            compare_to_dump(bad, dbad)
