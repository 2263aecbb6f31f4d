"""What the compiler leaves in the task loop of the H = 1024 k_gru_steps_v6 instances the eval plan launches (tools/v6_loop_census.py,
one cross-compile to gfx950 assembly, no GPU): no clock read, no weight tuple copied out of an accumulator register per step -- the only
v_accvgpr_read_b32 of the loop are the reduction's, one per accumulator register (four f32x16 accumulators: 64) -- front-end weight
reads waited for with a COUNT while the next step's are in flight, and no scratch in any instance (profiles/v6_hot_loop_notes.md)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools")]
import v6_loop_census


@pytest.fixture(scope="module")
def census():
    return {r["key"]: r for r in v6_loop_census.run()}


def test_census_reads_every_instance(census):
    assert len(census) >= 22
    for key, r in census.items():
        assert "error" not in r, (key, r.get("error"))
        assert r["next_free_vgpr"] and r["scratch"] is not None, key


def test_no_v6_instance_uses_scratch(census):
    assert {k: r["scratch"] for k, r in census.items() if r["scratch"] != 0} == {}


@pytest.mark.parametrize("key,kfw", [("16,8,3,0,0", 8), ("16,6,3,0,0", 6)])
def test_headline_instances_carry_no_copies_and_no_clock(census, key, kfw):
    r = census[key]
    fe, rec, red = (r["stretch"][k] for k in v6_loop_census.STRETCHES)
    assert (fe["mfma"], rec["mfma"], red["mfma"]) == (6 * kfw, 96, 0)
    assert r["task_loop_clock"] == 0 and fe["clock"] == rec["clock"] == red["clock"] == 0
    assert fe["accvgpr_read"] == 0 and rec["accvgpr_read"] == 0           # weights are MFMA operands where they live
    assert red["accvgpr_read"] == 64                                        # one read per accumulator register (4 x f32x16)
    assert fe["accvgpr_write"] == 0 and rec["accvgpr_write"] == 0
    # front-end weights one 16-k step ahead: every step's three LDS reads are waited for with the next step's three (or some of
    # them) outstanding -- a counted wait -- and only the last step, with nothing behind it, drains the counter
    waits = {k: n for k, n in fe["waitcnt"].items() if k.startswith("lgkmcnt")}
    counted = sum(n for k, n in waits.items() if k not in ("lgkmcnt(0)", "lgkmcnt(1)", "lgkmcnt(2)"))
    assert counted >= kfw - 1, waits
    assert waits.get("lgkmcnt(0)", 0) <= 1, waits


def test_profiling_instances_keep_their_clock_reads(census):
    for key in ("16,8,3,0,1", "16,6,3,0,1"):
        assert census[key]["task_loop_clock"] == 5, key      # task start + one per phase: what tools/step_timing.py reports
