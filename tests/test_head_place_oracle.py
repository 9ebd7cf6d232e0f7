"""The inputs of the head-place GPU tests (tests/head_place_inputs.py), on
the CPU: the oracle alone shows that every case exercises the merge of the
exact replay's records with the parallel scan's -- at least one region comes
from the head (it is not in the list of the same tracks without the tags at
positions <= bw), and at least one region of that headless list is lost or
changed.  And capi binds the two entry points of the mode."""
import numpy as np
import pytest

from tests import head_place_inputs as hp


@pytest.mark.parametrize("case", hp.merge_cases(), ids=lambda c: c["name"])
def test_inputs_exercise_the_merge(oracle, case):
    ref, sums = hp.oracle_list(oracle, case)
    bare, _ = hp.oracle_list(oracle, hp.headless(case))
    assert len(ref) > 0 and len(sums) == len(ref)
    with_head, without = set(hp.keys(ref)), set(hp.keys(bare))
    assert with_head - without, "no region comes from the head"
    assert without - with_head, "no region of the headless variant is lost or changed"
    # unit-major, and within a unit left-ascending
    order = [(int(r["unit"]), int(r["left"])) for r in ref]
    assert order == sorted(order)


def test_long_region_input(oracle):
    """the capacity case: its first region is longer than 262,144 positions"""
    ref, _ = hp.oracle_list(oracle, hp.long_region())
    assert len(ref) >= 2
    assert int(ref["right"][0]) - int(ref["left"][0]) + 1 > 262_144
    assert int(ref["left"][0]) <= 50


def test_chain_case_layout():
    case = hp.chains()
    assert [u["buffer"] for u in case["units"]] == [0, 0, 0, 0, 0, 1, 1]
    bw = case["bw"]
    u = case["units"]
    assert u[0]["pos"].min() > bw and (u[1]["pos"] <= bw).any() and (u[1]["pos"] > bw).any()
    assert u[2]["pos"].max() <= bw and u[4]["pos"].size == 0
    assert (u[5]["pos"] <= bw).any() and u[6]["pos"].min() > bw


def test_no_heads_input():
    case = hp.no_heads()
    assert all((u["pos"] > case["bw"]).all() for u in case["units"])


def test_capi_binds_head_place():
    from unipeak_amd import capi
    assert "up_set_head_place" in capi.EXPORTS and "up_last_head_kind" in capi.EXPORTS
    for name in ("set_head_place", "last_head_kind"):
        assert callable(getattr(capi.Lib, name))
    header = open(capi.os.path.join(capi._HERE, "..", "include", "unipeak_hip.h")).read()
    assert "int up_set_head_place(up_ctx *ctx, int on);" in header
    assert "int up_last_head_kind(up_ctx *ctx);" in header
