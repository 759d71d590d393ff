"""Static accounting of the QUAD hoisting's slots in the headline k_brent instantiation (tools/isa_mix.py; cross-compiles
to gfx950 assembly, no GPU): what the pipelined hoisting (hoist_quad_pipe_t) is for.

Per hoisting slot, on the path a full slot row executes:
  - no scalar load belongs to the slot: the item's 30 mutation-matrix entries are loaded once, before slot 0 (the earlier
    hoisting, -DPM_QD_PIPE=0, re-loads them in every slot: 6 s_load);
  - the wait that retires the next slot's ring reads has the slot's 26 address shifts and more behind it (the earlier
    hoisting waits for its own ring reads with nothing behind them);
  - one exposed wait is left per slot where the earlier hoisting has two: the one for the slot's own lookups, with the
    DMA's three address instructions behind it (the last two slots, with no DMA outstanding, count their waits down
    between the FMAs instead).

"Exposed": fewer than EXPOSED_GAP VALU instructions between the last load a wait retires and the wait.  An LDS read
returns no sooner than about 64 cycles after its issue and a VALU instruction of a 64-lane wave issues in 4 (FP64: 4 or
more), so fewer than 8 instructions behind a wait leave over half of the shortest round trip uncovered.  The same
function applied to the -DPM_QD_PIPE=0 compile (the parent commit's code, byte for byte) reports two exposed waits in
every interior slot -- 0 instructions behind the wait for the ring reads, 3 (the DMA's address arithmetic) behind the
wait for the lookups and the scalar loads -- so the check is known to see what it looks for.

Figures of this toolchain, headline instantiation: executed VALU per full slot 132-133 in interior slots in both forms
(2 113 against 2 116 over the 16 slots); 256 VGPRs, no scratch, 106 SGPRs in both."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

EXPOSED_GAP = 8
S = 16
VALU_SLACK = 4   # bookkeeping instructions a slot may differ by from the earlier form's


@pytest.fixture(scope="module")
def mixes():
    import isa_mix
    assert os.path.exists(isa_mix.HIPCC), "hipcc: the build needs it as well"
    return {"pipe": isa_mix.account(isa_mix.NAMES["headline"], []),
            "v0": isa_mix.account(isa_mix.NAMES["headline"], ["PM_QD_PIPE=0"])}


def _exposed(slot):
    return [w for w in slot["lgkm_waits"] if w["retires"] and w["valu_gap"] < EXPOSED_GAP]


def test_resources(mixes):
    for m in mixes.values():
        assert m["markers_neutral"], "the PM_ISA_MARK markers changed the instruction mix"
        assert m["resources"]["scratch"] == 0 and m["resources"]["vgpr"] <= 256, m["resources"]
        assert m["hoist_slot"]["slots"] == S


def test_no_scalar_load_in_a_slot(mixes):
    new, old = (mixes[k]["hoist_slot"]["full_row"] for k in ("pipe", "v0"))
    # the earlier form: 3 x dwordx16 + 3 x dwordx4 per slot (the last slot's region also holds two loads of the code after it)
    assert [s["s_load"] for s in old[:S - 1]] == [6] * (S - 1) and old[S - 1]["s_load"] >= 6
    assert [s["s_load"] for s in new[:S - 1]] == [0] * (S - 1)
    assert new[S - 1]["s_load"] == old[S - 1]["s_load"] - 6


def test_ring_reads_are_not_waited_for_with_an_empty_pipe(mixes):
    new = mixes["pipe"]["hoist_slot"]["full_row"]
    for s in range(S - 1):   # every slot but the last fetches the next slot's ring dwords
        ring = [w for w in new[s]["lgkm_waits"] if w["ring_gap"] is not None]
        assert ring, (s, new[s])
        for w in ring:
            print(f"slot {s}: {w}")
            assert w["ring_gap"] >= 26, (s, w)   # the slot's own 26 lookup addresses, at the least
    for s in range(S):   # at most the wait for the slot's own lookups is exposed
        ex = _exposed(new[s])
        assert len(ex) <= 1 and all(w["last"] == "ds_read_b64" for w in ex), (s, new[s]["lgkm_waits"])


def test_the_check_sees_the_earlier_forms_waits(mixes):
    old = mixes["v0"]["hoist_slot"]["full_row"]
    for s in range(1, S - 1):
        ex = _exposed(old[s])
        print(f"slot {s}: {ex}")
        assert len(ex) == 2, (s, old[s]["lgkm_waits"])
        assert ex[0]["ring_gap"] == 0 and ex[0]["last"].startswith("ds_read"), ex[0]
        assert ex[1]["last"].startswith("s_load"), ex[1]
    for s in (0, S - 1):
        assert len(_exposed(old[s])) >= 2, (s, old[s]["lgkm_waits"])


def test_executed_valu_per_slot(mixes):
    new, old = ([s["valu"] for s in mixes[k]["hoist_slot"]["full_row"]] for k in ("pipe", "v0"))
    print("pipe", new, "v0", old)
    for s in range(S):
        assert abs(new[s] - old[s]) <= VALU_SLACK, (s, new[s], old[s])
