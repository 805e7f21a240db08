"""-m "not gpu": the yardsticks of tests/local_kf_cases.py and tests/local_map_cases.py - the two transcriptions and the two numpy forms - against the
front half of the reference's own Tracking::TrackLocalMap: src/Tracking.cpp, src/KeyFrame.cpp and src/MapPoint.cpp compiled unmodified
(tools/ref_tracking), recorded in tests/golden/ref_matcher_tracking.npz (tools/ref_tracking_goldens.py) and, where the reference tree is present,
rebuilt and compared live.  Every mutant of a transcription must fail a named world against the STORED reference output."""
import functools
import zlib

import numpy as np
import pytest

import local_kf_cases as kc
import local_map_cases as lc
import tracking_cases as tc

WORLDS = tc.worlds()
GOLDEN = tc.load_golden()
f32 = np.float32


@functools.lru_cache(maxsize=None)
def recorded(name, host=False):
    T = tc.host_variant(WORLDS[name]) if host else WORLDS[name]
    return T, tc.unpack(T, GOLDEN[T["name"]]["raw"])


def test_the_file_holds_the_worlds_and_nothing_else():
    names = [n for T in WORLDS.values() for n in (T["name"], T["name"] + ".host")]
    assert list(GOLDEN) == names
    # no named case and no seeded world is left out
    assert all(n in WORLDS for n in kc.CASES) and len(kc.CASES) == 40 and sum(n.startswith("seed_") for n in WORLDS) == 12
    assert all("lm_" + n in WORLDS for n in ("six", "empty_first_middle_last", "zero_keyframes", "only_empty_keyframes", "no_frame", "edge_64_63", "edge_64_64",
                                              "edge_64_65", "edge_64_129", "edge_1024_1025"))
    for seed in tc.SEEDS:
        T = WORLDS["seed_%d" % seed]
        assert all((fr["G"]["state"][64:] == 0).all() for fr in T["frames"])
    for T in WORLDS.values():
        for V in (T, tc.host_variant(T)):
            assert GOLDEN[V["name"]]["raw"].dtype == np.int32 and int(GOLDEN[V["name"]]["crc"]) == zlib.crc32(tc.world_bytes(V)), V["name"]


def test_the_sequences_show_what_they_are_named_for():
    seqs = {n: T for n, T in WORLDS.items() if n.startswith("seq_")}
    assert len(seqs) >= 6 and all(len(T["frames"]) >= 3 for T in seqs.values())
    rec = lambda n: recorded(n)[1]
    r = rec("seq_empty_counter_in_the_middle")
    pred = tc.predicted(WORLDS["seq_empty_counter_in_the_middle"])
    assert [p["kept"] for p in pred] == [False, True, True, False, False] and r[1]["local_kf_slot"].tolist() == r[0]["local_kf_slot"].tolist() == r[2]["local_kf_slot"].tolist()
    assert r[1]["ref_slot"] == r[0]["ref_slot"] and len(r[1]["local_point_row"]) > 50
    r = rec("seq_every_voter_bad")
    assert len(r[1]["local_kf_slot"]) == 0 and r[1]["ref_slot"] == r[0]["ref_slot"] >= 0 and int(r[1]["n_launches"]) == 1 and r[1]["launch_floats"].shape == (9, 0)
    assert len(r[0]["local_kf_slot"]) > 3 and len(r[2]["local_kf_slot"]) > 3
    T, r = recorded("seq_a_point_turns_bad")
    turned = np.nonzero(T["frames"][1]["bad"] & ~T["frames"][0]["bad"].astype(bool))[0]
    assert set(turned) & set(r[0]["local_point_row"]) and not set(turned) & set(r[1]["local_point_row"])
    assert set(turned) & set(T["frames"][1]["frame_rows"]) and not set(turned) & set(r[1]["frame_after"])          # NULL in the frame, too
    T, r = recorded("seq_the_same_point_at_two_keypoints")
    assert all(len(set(fr["frame_rows"].tolist())) < len(fr["frame_rows"]) for fr in T["frames"]) and r[1]["visible"].max() >= 3
    r = rec("seq_a_frame_sees_the_whole_local_map")
    assert len(r[1]["local_point_row"]) > 100 and int(r[1]["n_launches"]) == 1 and r[1]["launch_floats"].shape == (9, 0) and not int(r[1]["matcher_called"])
    assert int(r[0]["matcher_called"]) and int(r[2]["matcher_called"])
    # 1; 3 for RGB-D; 5 one frame after a relocalisation; 5 beats 3; two frames after it (mnId == mnLastRelocFrameId + 2) 1 again
    assert [float(x["th"]) for x in rec("seq_the_three_th")] == [1.0, 3.0, 5.0, 5.0, 1.0]
    # the host path asks Frame::isInFrustum about exactly the points the launcher is handed, in the same order
    for n in seqs:
        for a, b in zip(tc.predicted(WORLDS[n]), recorded(n, host=True)[1]):
            assert np.array_equal(a["map_points"], b["asked"]) and not int(b["n_launches"])


@pytest.mark.parametrize("name", list(WORLDS))
def test_every_yardstick_reproduces_the_reference(name):
    """the transcriptions and the numpy forms: every recorded array of every frame, with use_gpu_ = 1 and 0, bit for bit"""
    for host in (False, True):
        T, rec = recorded(name, host)
        for kf_fn, lm_fn in ((kc.update_local_keyframes_restated, lc.update_local_points_restated), (kc.update_local_keyframes_numpy, lc.update_local_points_numpy)):
            assert tc.same_where_recorded(T, tc.predicted(T, kf_fn, lm_fn), rec) == [], (T["name"], kf_fn.__name__)
        for p, r in zip(tc.predicted(T), rec):   # the launcher's nine arrays are the table's rows, gathered in list order
            if not host:
                assert np.array_equal(tc.bits(r["launch_floats"]), tc.bits(T["table"]["floats"][:, p["map_points"]]))


def test_the_table_columns_are_built_forward():
    for table in (tc.kf_table(), tc.lm_table()):
        F = table["floats"]
        assert np.array_equal(F[6], table["maxd"]) and np.array_equal(F[7], f32(1.2) * table["maxd"]) and np.array_equal(F[8], f32(0.8) * table["mind"])
        assert F.dtype == f32 and (F[7] != (1.2 * table["maxd"].astype(np.float64)).astype(f32)).any()      # (1.2f is not 1.2: the float product shows)
    W = lc.world()
    assert (tc.lm_table()["floats"][:6] == W["floats"][:6]).all()


def test_track_proj_xr_is_two_roundings():
    """mTrackProjXR = u - mbf * invz (Tracking.cpp:1617) in float32 without contraction: the product rounded, then the difference"""
    n = n_fused_differs = 0
    for name in WORLDS:
        T, rec = recorded(name)
        for fr, p, r in zip(T["frames"], tc.predicted(T), rec):
            if not int(r["matcher_called"]):
                continue
            v = r["in_view"] != 0
            invz = np.zeros(len(v), f32)
            pos = {int(row): k for k, row in enumerate(p["map_points"])}
            at = np.array([pos.get(int(row), 0) for row in r["local_point_row"]], np.int64)
            if len(p["map_points"]):
                invz = p["k16"][0][0][at]
            bf = f32(fr["cam"]["bf"])
            two = (r["proj_x"] - (bf * invz).astype(f32)).astype(f32)
            fused = (r["proj_x"].astype(np.float64) - np.float64(bf) * invz.astype(np.float64)).astype(f32)
            assert np.array_equal(tc.bits(r["proj_xr"][v]), tc.bits(two[v])), name
            n, n_fused_differs = n + int(v.sum()), n_fused_differs + int((fused[v] != two[v]).sum())
    assert n > 5000 and n_fused_differs > 50         # a contracted product would have shown


def test_changed_for_the_reference_is_complete():
    assert {n: T["kinds"] for n, T in WORLDS.items() if T["kinds"]} == tc.CHANGED_FOR_THE_REFERENCE
    assert all(set(k) <= set(tc.KINDS) for k in tc.CHANGED_FOR_THE_REFERENCE.values())
    assert all(set(WORLDS["seed_%d" % s]["kinds"]) <= {"capacity_raised"} for s in tc.SEEDS)      # drawn expressible from the start
    assert WORLDS["first_list_over_capacity"]["kf_capacity"] == 128 and WORLDS["first_list_over_capacity"]["original_capacity"][0] == 84


def test_the_driver_rebuilt_gives_the_recorded_arrays(tmp_path):
    ref = tc.reference_tree()
    if ref is None:
        pytest.skip("the reference tree is not here")
    tc.build_driver(ref)
    for T in WORLDS.values():
        for V in (T, tc.host_variant(T)):
            rec = tc.run_driver(V, str(tmp_path))
            for k in ("raw", "crc"):
                assert np.array_equal(rec[k], GOLDEN[V["name"]][k]), (V["name"], k)


# ---- sensitivity: one decision of a transcription flipped at a time; each must fail a named world against the STORED reference output ----
KF_MUTANTS = {                                   # mutant of update_local_keyframes_restated -> the world it must fail
    "votes_at_least": "order_keys_against_slots",             # votes >= max: the last of the largest instead of the first
    "end_reevaluated": "seq_the_graph_changes",               # the loop end re-evaluated: appended elements are walked, too
    "size_at_least_80": "limit_80",                           # size() >= 80
    "parent_bad_tested": "parent_bad",                        # isBad() tested on the parent
    "parent_break_inner": "parent_ends_the_loop",             # the parent's break leaving only the inner scope
    "bad_voters_not_counted": "all_voters_bad",               # a counter that holds only bad voters no longer clears the list
    "children_slot_order": "children_key_order",              # the child run in slot order instead of key order
}
LM_MUTANTS = {                                   # mutant of update_local_points_restated -> the world it must fail
    "filter_dropped": "lm_six",                               # the map_points filter dropped: the launcher sees points the frame has seen
    "marks_for_bad_frame_points": "lm_six",                   # a bad frame point keeps its pointer, its mark and its IncreaseVisible
    "list_by_row": "lm_empty_first_middle_last",              # the list ordered by row
}
NO_OUTPUT = {                                    # mutant -> why no recorded array can show it
    "duplicate_after_bad": "only a point that passed isBad() is marked (:1834-1837) and the flags do not move inside a call, so no bad point ever meets "
                           "the duplicate test with this frame's mark: the order of :1832 and :1834 decides nothing, not even n_duplicates / n_bad",
}


def test_the_mutant_lists_are_whole():
    assert set(KF_MUTANTS) == set(kc.MUTANTS) and set(LM_MUTANTS) | set(NO_OUTPUT) == set(lc.MUTANTS)
    assert all(w in WORLDS for w in list(KF_MUTANTS.values()) + list(LM_MUTANTS.values()))


@pytest.mark.parametrize("mutant", list(KF_MUTANTS) + list(LM_MUTANTS))
def test_each_mutant_fails_its_world_against_the_reference(mutant):
    T, rec = recorded((KF_MUTANTS if mutant in KF_MUTANTS else LM_MUTANTS)[mutant])
    kf_fn = functools.partial(kc.update_local_keyframes_restated, mutant=mutant) if mutant in KF_MUTANTS else None
    lm_fn = functools.partial(lc.update_local_points_restated, mutant=mutant) if mutant in LM_MUTANTS else None
    assert tc.same_where_recorded(T, tc.predicted(T), rec) == []
    assert tc.same_where_recorded(T, tc.predicted(T, kf_fn, lm_fn), rec) != [], mutant


def test_mutants_that_change_no_output():
    for mutant, why in NO_OUTPUT.items():
        lm_fn, moved = functools.partial(lc.update_local_points_restated, mutant=mutant), 0
        for name in WORLDS:
            T, rec = recorded(name)
            pred = tc.predicted(T, None, lm_fn)
            assert tc.same_where_recorded(T, pred, rec) == [], (mutant, name, why)
            moved += sum(p["lm_stats"] != q["lm_stats"] for p, q in zip(pred, tc.predicted(T)))
        assert moved == 0, (mutant, why)             # ... nor do the statistics
