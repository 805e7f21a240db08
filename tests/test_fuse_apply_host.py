"""CPU: the contract of jsorb_fuse_map (include/jsorb.h) restated over the device arrays (tests/fuse_apply_cases.py) against the reference's own
ORBmatcher.cpp runs stored in tests/golden/ref_matcher_fuse.npz and ref_matcher_fuse_sim3.npz, and against the immediate recomputation on
fuse_replay.LiveMap for the constructed cases.  tests/test_gpu_fuse_apply.py holds the device to the restatement."""
import ctypes

import numpy as np
import pytest

import fuse_apply_cases as fa
import fuse_replay
import ref_matcher_cases as cases

PERMUTATION_SEED = 5


@pytest.fixture(scope="module")
def stored():
    return {name: fa.stored(name) for name in fa.FILES}


@pytest.mark.parametrize("name", fa.FILES)
def test_every_stored_case_gives_the_references_own_run(po, stored, name):
    """no case is left out: every one is expressible in the device arrays, and steps 0-5 with the descriptors deferred to the end of a target give
    the reference's map, counts and event log, with the identity and with a seeded slot permutation"""
    n_replace = n_add = 0
    for cname, c in stored[name].items():
        ev = c["out"]["events"]
        ev = ev[np.isin(ev[:, 0], (fa.EV_REPLACE, fa.EV_ADD_MAP_POINT))]
        searched = fuse_replay.replay(c, cases.fuse_search(po, c, "restatement"), "sequential")[2][0]
        for seed in (None, PERMUTATION_SEED):
            W = fa.to_world(c, fa.permutation(c, seed))
            res = fa.restate(po, W)
            try:
                fuse_replay.same_map(fa.as_reference(W, res), c["out"], fa.REFERENCE_KEYS)
                assert np.array_equal(fa.events_as_reference(W, res["events"]), ev), "log"
                assert np.array_equal(res["best_idx"], searched), "best_idx"
                assert res["counts"][1] == (ev[:, 0] == fa.EV_REPLACE).sum() and res["counts"][2] == (ev[:, 0] == fa.EV_ADD_MAP_POINT).sum()
            except AssertionError as e:
                raise AssertionError("%s / %s / permutation %s" % (name, cname, seed)) from e
        n_replace += int((ev[:, 0] == fa.EV_REPLACE).sum())
        n_add += int((ev[:, 0] == fa.EV_ADD_MAP_POINT).sum())
    assert n_replace >= 500 and n_add >= 300      # not vacuous: the stored logs hold 534 / 364 and 574 / 396


def test_four_scw_cases_list_a_row_twice(stored):
    twice = [k for k, c in stored["fuse_sim3"].items() if len(set(c["list"].tolist())) < len(c["list"])]
    assert len(twice) >= 4


EXPECT = {      # name -> (n_fused per target, Replace calls, AddMapPoint calls) by hand
    "a_survivor_inherits_twice": ([2], 2, 0), "a_survivor_is_replaced_later": ([2], 2, 0), "equal_observations": ([1], 1, 0),
    "a_stereo_observation_flips_it": ([1], 1, 0), "a_bad_point_in_the_slot": ([1], 0, 0), "an_unregistered_entry_holds_the_point_at_hand": ([2], 0, 1),
    "an_observation_in_a_bad_keyframe": ([1], 1, 0), "a_duplicate_list_row_overload_1": ([1], 0, 1), "a_duplicate_list_row_overload_2": ([2], 0, 1),
    "a_null_list_entry": ([1], 0, 1), "the_replace_loop": ([1], 1, 0), "a_skipped_target_between_two": ([1, 0, 1], 0, 2),
    "log_cap_smaller_than_the_log": ([3], 1, 2), "visible_and_found_sums": ([1], 1, 0)}


@pytest.mark.parametrize("name", list(EXPECT))
def test_constructed_cases_equal_the_immediate_recomputation(po, name):
    c = fa.constructed()[name]
    for perm in (None, fa.reversed_slots(c)):
        W = fa.to_world(c, perm)
        res = fa.restate(po, W)
        fa.check_against_live(po, c, W, res)
        assert (res["n_fused"].tolist(), int(res["counts"][1]), int(res["counts"][2])) == EXPECT[name]
    # what each case is about
    W = fa.to_world(c)
    res = fa.restate(po, W)
    if name == "a_survivor_inherits_twice":
        assert res["log"][:2].tolist() == [[2, 0, 2, -1], [2, 1, 2, -1]] and (res["point_pool"] == 2).sum() == 5 and res["counts"][5] == 1
    if name == "a_survivor_is_replaced_later":
        assert res["log"][:2].tolist() == [[2, 2, 0, -1], [2, 0, 1, -1]] and res["bad"].tolist() == [1, 0, 1] and np.array_equal(res["tdesc"][0], W["tdesc"][0])
    if name == "equal_observations":
        assert res["replaced"].tolist() == [-1, 0]
    if name == "a_stereo_observation_flips_it":
        assert res["replaced"].tolist() == [1, -1]
    if name == "a_bad_point_in_the_slot":
        assert res["counts"][3] == 1 and np.array_equal(res["point_pool"], W["point_pool"])
    if name == "an_observation_in_a_bad_keyframe":
        assert res["point_pool"][0] == 0 and res["registered"][0] == 1 and np.unpackbits(res["tdesc"][0]).sum() == 10
    if name == "a_skipped_target_between_two":
        assert (res["best_idx"][1] == -1).all() and res["counts"][6] == 1
    if name == "log_cap_smaller_than_the_log":
        assert res["log"].shape == (1, 4) and res["counts"][8] == 3 and res["counts"][9] == 1 and len(res["events"]) == 3
    if name in ("the_replace_loop", "visible_and_found_sums"):
        p, q = res["events"][0][1:3]
        assert res["found"][q] == W["found"][q] + W["found"][p] and res["visible"][q] == W["visible"][q] + W["visible"][p]


@pytest.mark.parametrize("mutant", fa.MUTANTS)
def test_every_mutant_of_the_restatement_fails_its_case(po, mutant):
    c = fa.constructed()[fa.MUTANT_CASES[mutant]]
    W = fa.to_world(c, fa.reversed_slots(c) if mutant == "descriptor_by_slot" else None)
    fa.check_against_live(po, c, W, fa.restate(po, W))
    with pytest.raises(AssertionError):
        fa.check_against_live(po, c, W, fa.restate(po, W, mutant))


def test_the_permuted_stored_runs_catch_a_descriptor_order_by_slot(po, stored):
    caught = 0
    for name in fa.FILES:
        for cname, c in stored[name].items():
            if not (c["out"]["events"][:, 0] == fa.EV_REPLACE).any():
                continue
            W = fa.to_world(c, fa.permutation(c, PERMUTATION_SEED))
            try:
                fuse_replay.same_map(fa.as_reference(W, fa.restate(po, W, "descriptor_by_slot")), c["out"], fa.REFERENCE_KEYS)
            except AssertionError:
                caught += 1
    assert caught >= 4


def test_the_padded_world_crosses_the_index_builds_blocks(po):
    W = fa.padded_world(po, 3, S=60, run=120, n_rows=4000, n_targets=3)
    res = fa.restate(po, W)
    assert res["counts"][1] >= 5 and res["counts"][2] >= 5 and (W["state"] == 2).any()
    # Replace moved entries of the extra keyframes, bad ones included
    moved = np.nonzero(res["point_pool"] != W["point_pool"])[0]
    assert (moved >= W["case"]["obs"].shape[0]).any() and len(set(fa.entry_slots(W)[moved].tolist())) > 3


def test_the_variant_and_the_library_report_their_chunk():
    from jetson_slam_amd import build as jb
    assert jb.VARIANTS["tiny_fuse_apply"] == (["-DFA_CHUNK=%d" % fa.CHUNKS[1]], ["k_fuse_apply.hip"])
    for path, want in ((jb.build_lib(), fa.CHUNKS[0]), (jb.build_variant("tiny_fuse_apply", *jb.VARIANTS["tiny_fuse_apply"]), fa.CHUNKS[1])):
        got = ctypes.c_int()
        assert ctypes.CDLL(path).jsorb_fuse_map_build_caps(ctypes.byref(got)) == 0 and got.value == want
