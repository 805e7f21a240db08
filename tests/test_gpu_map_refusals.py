"""-m gpu: every refusal of the map-maintenance calls (tests/map_refusal_cases.py: the local map, the local keyframes, the covisibility calls,
keyframe culling, Fuse applied to the map, their `_stats` readers) answers the (rc, text) recorded in tests/golden/map_call_refusals.json, after
each refused call the entry point's smallest valid call returns its recorded outputs and statistics, and the valid synchronous calls with one
empty segment of the copy back return theirs, the untouched sentinel words included.  The recording was written by a build of commit 3c41255
("Apply Fuse to the map on the device"), the last one before the calls' host plumbing was shared - never by the tree under test."""
import json

import pytest

import map_refusal_cases as cases

pytestmark = pytest.mark.gpu
ENTRY_POINTS = cases.PAIRS + ["erase_connections_async", "connected_mask_async", "best_covisibles_async", "covisibility_copy", "map_points_scatter_async"]
EDGES = {"local_map_points": ["capacity_0"], "local_keyframes": ["entry_capacity_0"], "update_connections": ["n_update_0"],
         "cull_keyframes": ["n_cand_0_reparent_0"], "fuse_map": ["n_targets_0", "n_list_0", "log_cap_0"]}


@pytest.fixture(scope="module")
def recorded():
    with open(cases.GOLDEN) as f:
        return cases.unpack(json.load(f))      # (the valid call's result is stored once per entry point and form)


@pytest.fixture(scope="module")
def answered(orb):
    return json.loads(json.dumps(cases.run()))      # (through JSON: tuples and lists compare as the recording holds them)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_refusals_answer_as_recorded(recorded, answered, name):
    rec, got = recorded[name], answered[name]
    assert sorted(got) == sorted(rec)                # the same rows: none dropped, none new without a recording
    for row in rec:
        assert got[row]["refusal"] == rec[row]["refusal"], (row, got[row]["refusal"], rec[row]["refusal"])
        assert (got[row]["refusal"][0] == 0) == row.startswith("edge/"), row
        assert got[row]["after"] == rec[row]["after"], (row, got[row]["after"], rec[row]["after"])
        assert got[row]["after"]["call"] == [0, ""], row


@pytest.mark.parametrize("name", cases.PAIRS)
def test_the_earlier_of_two_violated_checks_answers(recorded, name):
    rec = recorded[name]
    pairs = [row for row in rec if rec[row]["same_as"]]
    assert len(pairs) >= 6, pairs
    for row in pairs:
        assert rec[row]["refusal"] == rec[rec[row]["same_as"]]["refusal"], row


@pytest.mark.parametrize("name", cases.PAIRS)
def test_the_empty_segments_are_rows(recorded, name):
    for edge in EDGES[name]:
        row = recorded[name]["edge/" + edge]
        assert row["refusal"] == [0, ""] and row["form"] == "sync", edge
        assert row["after"] != recorded[name]["sync/null_owner"]["after"], edge      # (not the valid call's result again)


def test_the_quirks_of_check_order_are_rows(recorded):
    ck, uc = recorded["cull_keyframes"], recorded["update_connections"]
    # culling checks the graph's slots before it looks at the covisibility state, and does not ask for first_connection
    assert ck["async/slots+differ"]["refusal"] == ck["async/slots"]["refusal"]
    assert ck["edge/first_connection_null"]["refusal"] == [0, ""]
    assert uc["async/first_connection_null"]["refusal"] == uc["async/cov_array_null"]["refusal"]
    # the synchronous fuse_map answers negative sizes with a text of its own
    fm = recorded["fuse_map"]
    assert fm["sync/n_list_neg"]["refusal"] == fm["sync/sizes"]["refusal"] != fm["async/n_list_neg"]["refusal"]
