"""-m "not gpu": the restatements and cases of tests/local_kf_cases.py, and the product boundary of jsorb_local_keyframes - the ABI, the ctypes
signatures, the build variant, the shim and the example.  No compute call is made."""
import ctypes
import os
import re

import numpy as np
import pytest

import local_kf_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsorb_local_keyframes_async", "jsorb_local_keyframes", "jsorb_local_keyframes_stats", "jsorb_local_keyframes_build_caps")


def both(case):
    a, b = kc.run_steps(kc.update_local_keyframes_restated, case), kc.run_steps(kc.update_local_keyframes_numpy, case)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["stats"] == y["stats"] and x["ref_slot"] == y["ref_slot"], (case["name"], i, x["stats"], y["stats"])
        for k in ("list", "local_kf_start", "local_point_row", "counts"):
            assert x[k].dtype == y[k].dtype == np.int32 and np.array_equal(x[k], y[k]), (case["name"], i, k)
    return a


@pytest.mark.parametrize("name", list(kc.CASES))
def test_the_two_restatements_agree_and_the_case_takes_its_exit(name):
    case = kc.CASES[name]
    r = both(case)[case["check_step"]]
    for k, v in case["expect"].items():
        assert r["stats"][k] == v, (name, k, r["stats"])
    if case["expect_list"] is not None:
        assert r["list"].tolist() == case["expect_list"]
    if case["expect_ref"] is not None:
        assert r["ref_slot"] == case["expect_ref"]
    assert len(r["local_kf_start"]) == case["kf_capacity"] + 1 and len(r["local_point_row"]) == case["entry_capacity"]
    for step in case["steps"]:                                               # the shapes the cases promise
        G = step["G"]
        assert len(G["state"]) == kc.S and len(step["bad"]) == kc.N_ROWS and (step["frame_rows"] is None or len(step["frame_rows"]) <= 64)
        ok = [s for s in range(kc.S) if G["state"][s] and kc.run_ok(int(G["point_off"][s]), int(G["point_len"][s]), kc.POOL)]
        assert all(G["point_len"][s] <= 40 for s in ok)
        for s in range(kc.S):                                                # the child runs are in std::set's order: by key among the usable ones
            if kc.run_ok(int(G["child_off"][s]), int(G["child_len"][s]), kc.CHILD_POOL):
                c = [int(x) for x in G["child_pool"][G["child_off"][s]:G["child_off"][s] + G["child_len"][s]] if 0 <= x < kc.S and G["state"][x]]
                assert c == sorted(c, key=lambda x: (int(G["order_key"][x]), x)), (name, s)


def test_seeded_random_graphs():
    reasons, kept, overflow = set(), 0, 0
    for seed in range(300):
        for r in both(kc.random_case(seed)):
            reasons.add(r["stats"]["end_reason"])
            kept += int(r["counts"][7])
            overflow += int(r["counts"][6])
    assert reasons == {0, 1, 2} and kept > 20 and overflow > 20


def test_the_cases_cover_what_the_contract_names():
    C = kc.CASES
    stats = {n: kc.run_steps(kc.update_local_keyframes_restated, c)[c["check_step"]] for n, c in C.items()}
    assert [stats["limit_%d" % n]["stats"]["n_local"] for n in (78, 79, 80, 81)] == [81, 82, 83, 81]
    assert stats["first_list_over_capacity"]["counts"].tolist()[5] == 1 and C["capacity_128"]["kf_capacity"] == 128
    e = int(stats["entries_exact"]["counts"][4])
    assert [C["entries_" + k]["entry_capacity"] for k in ("one_short", "exact", "seven_more", "zero")] == [e - 1, e, e + 7, 0] and e > 40
    assert [int(stats["entries_" + k]["counts"][6]) for k in ("one_short", "exact", "seven_more", "zero")] == [1, 0, 0, 1]
    assert (stats["entries_seven_more"]["local_point_row"][e:] == -1).all() and np.array_equal(stats["entries_one_short"]["local_point_row"],
                                                                                                 stats["entries_exact"]["local_point_row"][:e - 1])
    assert C["frame_null"]["steps"][0]["frame_rows"] is None and len(C["frame_empty"]["steps"][0]["frame_rows"]) == 0
    assert C["registered"]["steps"][0]["G"]["registered"] is not None and C["frame_row_twice"]["steps"][0]["G"]["registered"] is None
    kept = kc.run_steps(kc.update_local_keyframes_restated, C["empty_counter_keeps_the_list"])
    assert [int(r["counts"][7]) for r in kept] == [0, 1, 0] and kept[1]["list"].tolist() == kept[0]["list"].tolist()
    assert not np.array_equal(kept[1]["local_point_row"], kept[0]["local_point_row"]) and kept[1]["counts"][4] < kept[0]["counts"][4]
    zero = stats["zero_length_run_in_the_middle"]["local_kf_start"]
    assert zero[2] == zero[3] and zero[3] < zero[4]                          # the third of four keyframes has no entries
    # more voters than every cap of the tiny build: membership bits beyond slot 64, child runs beyond 16 candidates, both kinds appended
    tiny, G = stats["tiny_caps"], C["tiny_caps"]["steps"][0]["G"]
    member_lds, child_lds = kc.CAPS[1]
    first = tiny["list"][:tiny["stats"]["n_first"]]
    assert (first >= member_lds).sum() > 10 and (tiny["list"][len(first):] >= member_lds).any() and (tiny["list"][len(first):] < member_lds).any()
    assert int(G["child_len"][first[:4]].sum()) > child_lds and tiny["stats"]["n_children"] >= 2
    assert C["long_child_run"]["steps"][0]["G"]["child_len"].max() > 64          # a child run longer than a wave


def test_abi_bindings_and_build():
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb, orb
    lib = ctypes.CDLL(g.build())
    hdr = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    src = open(os.path.join(ROOT, "jetson_slam_amd", "orb.py")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
    for cite in ("src/Tracking.cpp:1844-1952", ":1848-1864", ":1866", ":1876-1891", ":1895-1945", ":1947-1951", "src/LocalMapping.cpp:158"):
        assert cite in hdr, cite
    assert "What stays on the host: UpdateLocalKeyFrames" not in hdr and "jsorb_local_keyframes_async below" in hdr
    l = orb.load_library()
    assert len(l.jsorb_local_keyframes_async.argtypes) == 12 and len(l.jsorb_local_keyframes.argtypes) == 15
    assert len(l.jsorb_local_keyframes_stats.argtypes) == 9 and len(l.jsorb_local_keyframes_build_caps.argtypes) == 2
    # the struct as the header lays it out (x86-64: three ints, padding, eleven pointers)
    assert ctypes.sizeof(orb.JsorbKeyframeGraph) == 104 and orb.JsorbKeyframeGraph.state.offset == 16 and orb.JsorbKeyframeGraph.parent.offset == 96
    assert [f[0] for f in orb.JsorbKeyframeGraph._fields_[3:]] == list(orb.KeyframeGraph.ARRAYS)
    assert orb.local_keyframes_build_caps() == kc.CAPS[0] and orb.LOCAL_KF_COUNTS == kc.COUNTS and orb.LOCAL_KF_MIN_CAPACITY == 84
    assert "k_local_keyframes.hip" in jb.SOURCES and "jsorb_localkf.hip" in jb.SOURCES and "update_local_keyframes" in jb.EXAMPLES
    assert jb.VARIANTS["tiny_local_kf"] == (["-DLK_MEMBER_LDS=%d" % kc.CAPS[1][0], "-DLK_CHILD_LDS=%d" % kc.CAPS[1][1]], ["k_local_keyframes.hip"])
    m, c = ctypes.c_int(), ctypes.c_int()
    tiny = ctypes.CDLL(jb.build_variant("tiny_local_kf", *jb.VARIANTS["tiny_local_kf"]))
    assert tiny.jsorb_local_keyframes_build_caps(ctypes.byref(m), ctypes.byref(c)) == 0 and (m.value, c.value) == kc.CAPS[1]
    assert tiny.jsorb_local_keyframes_build_caps(None, None) == 0
    # the refusals that need no device: a NULL handle
    assert l.jsorb_local_keyframes_async(None, None, None, None, 0, 84, 0, *([None] * 5)) == -1
    assert l.jsorb_local_keyframes(None, None, None, None, 0, 84, 0, *([None] * 8)) == -1 and l.jsorb_local_keyframes_stats(*([None] * 9)) == -1


def test_the_shim_and_the_example_compile(tmp_path):
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb
    g.build()
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    assert "class KeyframeGraph" in shim and "struct LocalKeyFrames" in shim and "UpdateLocalKeyFrames(" in shim
    assert re.search(r"UpdateLocalPoints\(ORBExtractor &ex, const jsorb::MapPointTable &table, const jsorb_frustum_params &frustum, jsorb::LocalKeyFrames &local", shim)
    exe = jb.build_example("update_local_keyframes", str(tmp_path / "update_local_keyframes"))
    assert os.path.getsize(exe) > 0
