"""-m "not gpu": the two yardsticks of tests/covis_cases.py against each other on the named cases and on seeded random worlds, the mutants, and the
product boundary of jsorb_update_connections - the ABI, the ctypes signatures, the build variant, the shim and the example.  No compute call is
made."""
import ctypes
import os
import re

import numpy as np
import pytest

import covis_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsorb_update_connections_async", "jsorb_update_connections", "jsorb_update_connections_stats", "jsorb_erase_connections_async",
       "jsorb_connected_mask_async", "jsorb_best_covisibles_async", "jsorb_covisibility_copy", "jsorb_covisibility_build_caps",
       "jsorb_update_connections_scratch")


def both(world):
    """the restatement's results; the literal transcription agrees wherever no map went over its capacity"""
    r = cc.run_restated(world)
    if not cc.overflowed(r):
        cc.same(cc.run_literal(world), r, world["name"])
    for res in r:                                # what holds past capacity too: lengths within C, maps in key order, lists in theirs
        st, G, C = res["state"], world["G"], world["C"]
        assert st["conn_slot"].shape[1] == C and (st["conn_len"] <= C).all() and (st["ord_len"] <= C).all()
        for s in np.nonzero(st["conn_len"])[0]:
            k = [(int(G["order_key"][o]), int(o)) for o in st["conn_slot"][s, :st["conn_len"][s]]]
            assert k == sorted(set(k)), (world["name"], s)
        for s in np.nonzero(st["ord_len"])[0]:
            k = [(int(w), int(G["order_key"][o]), int(o)) for o, w in zip(st["ord_slot"][s, :st["ord_len"][s]], st["ord_weight"][s, :st["ord_len"][s]])]
            assert k == sorted(set(k), reverse=True), (world["name"], s)
    return r


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_two_yardsticks_agree_and_the_case_shows_what_it_is_named_for(name):
    world, expect = cc.build_case(name)
    r = both(world)
    cc.check_expect(r, expect)
    G = world["G"]                               # the shapes the cases promise
    assert len(G["state"]) == cc.S and len(world["bad"]) == cc.N_ROWS and len(G["point_pool"]) == cc.POOL
    assert all(len(arg) <= cc.MAX_UPDATE for kind, arg in world["script"] if kind == "update")
    if "overflow" not in name and "c_plus_one" not in name:
        assert not cc.overflowed(r)


def test_the_literal_form_alone_shows_the_early_return():
    world, expect = cc.build_case("unchanged_weight_keeps_the_list")
    r = cc.run_literal(world)
    cc.check_expect(r, expect)
    assert r[-1]["n_early"] == 1


def test_seeded_random_worlds():
    n_fallback = n_overflow = n_early = n_compared = n_erase = 0
    for seed in range(300):
        world = cc.random_world(seed)
        r = both(world)
        n_compared += not cc.overflowed(r)
        for res in r:
            if "parent_out" in res:
                n_fallback += int(res["counts"][5])
                n_overflow += int(res["counts"][6])
                n_early += res["n_early"]
            else:
                n_erase += int(res["counts"][1])
    assert n_fallback > 100 and n_overflow > 100 and n_early > 1000 and n_compared >= 225 and n_erase > 50, (n_fallback, n_overflow, n_early, n_compared, n_erase)


@pytest.mark.parametrize("mutant", list(cc.MUTANTS))
def test_each_mutant_fails_its_case(mutant):
    world, expect = cc.build_case(cc.MUTANTS[mutant])
    good = cc.run_restated(world)
    cc.check_expect(good, expect)
    bad = cc.run_restated(world, mutant)
    with pytest.raises(AssertionError):
        cc.same(good, bad)
    with pytest.raises(AssertionError):
        cc.check_expect(bad, expect)


def test_the_cases_cover_what_the_contract_names():
    worlds = {n: cc.build_case(n)[0] for n in cc.CASES}
    res = {n: cc.run_restated(w) for n, w in worlds.items()}
    assert res["map_of_exactly_c"][-1]["state"]["conn_len"][0] == worlds["map_of_exactly_c"]["C"] == 16
    assert [int(res[n][-1]["counts"][6]) for n in ("map_of_exactly_c", "map_of_c_plus_one_by_its_own_update", "map_of_c_plus_one_by_an_incoming_connection")] == [0, 1, 1]
    assert worlds["registered_bytes"]["G"]["registered"] is not None and worlds["counts_14_15_16"]["G"]["registered"] is None
    assert worlds["run_longer_than_a_wave"]["G"]["point_len"].max() > 64 and res["more_than_64_connected"][0]["state"]["conn_len"][0] > 64
    assert [len(worlds[n]["script"][0][1]) for n in ("n_update_0", "repeated_member", "n_update_32")] == [0, 3, 32]
    tiny = [n for n, w in worlds.items() if w["C"] <= cc.CAPS[1][1]]
    assert len(tiny) >= 3 and all(cc.CAPS[0][0] <= w["C"] <= cc.CAPS[0][1] for w in worlds.values())
    # the neighbours rows: rewritten for the slots whose list was, untouched elsewhere
    st = res["counts_14_15_16"][-1]["state"]
    assert st["neighbours"][0].tolist() == [3, 2] + [-1] * 8 and st["neighbours"][2].tolist() == [0] + [-1] * 9 and (st["neighbours"][1] == cc.UNTOUCHED).all()
    snap = res["counts_14_15_16"][-1]["snapshot"]
    assert snap == [[(1, 14), (2, 15), (3, 16)]]


def test_abi_bindings_and_build():
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb, orb
    lib = ctypes.CDLL(g.build())
    hdr = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    src = open(os.path.join(ROOT, "jetson_slam_amd", "orb.py")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
    for cite in ("src/KeyFrame.cpp:293-383", ":127-161", ":557-571", ":306-314", ":316-323", ":327", ":338-344", ":352-356", ":358-365", ":375-380",
                 ":127-140", ":470-471", ":480-481", "src/LoopClosing.cpp:560", ":163-170", ":178-186"):
        assert cite in hdr, cite
    l = orb.load_library()
    assert len(l.jsorb_update_connections_async.argtypes) == 10 and len(l.jsorb_update_connections.argtypes) == 12
    assert len(l.jsorb_update_connections_stats.argtypes) == 8 and len(l.jsorb_erase_connections_async.argtypes) == 6
    assert len(l.jsorb_connected_mask_async.argtypes) == 4 and len(l.jsorb_best_covisibles_async.argtypes) == 7
    assert len(l.jsorb_covisibility_copy.argtypes) == 7 and len(l.jsorb_covisibility_build_caps.argtypes) == 2
    # the structs as the header lays them out (x86-64: two ints, seven pointers; three pointers)
    assert ctypes.sizeof(orb.JsorbCovisibility) == 64 and orb.JsorbCovisibility.conn_len.offset == 8 and orb.JsorbCovisibility.first_connection.offset == 56
    assert ctypes.sizeof(orb.JsorbConnSnapshot) == 24
    assert orb.covisibility_build_caps() == cc.CAPS[0] and orb.UPDATE_CONNECTIONS_COUNTS == cc.COUNTS and orb.UPDATE_CONNECTIONS_MAX == cc.MAX_UPDATE
    assert "k_covisibility.hip" in jb.SOURCES and "jsorb_covis.hip" in jb.SOURCES and "update_connections" in jb.EXAMPLES
    assert jb.VARIANTS["tiny_covis"] == (["-DCV_CAP_MAX=%d" % cc.CAPS[1][1]], ["k_covisibility.hip"])
    lo, hi = ctypes.c_int(), ctypes.c_int()
    tiny = ctypes.CDLL(jb.build_variant("tiny_covis", *jb.VARIANTS["tiny_covis"]))
    assert tiny.jsorb_covisibility_build_caps(ctypes.byref(lo), ctypes.byref(hi)) == 0 and (lo.value, hi.value) == cc.CAPS[1]
    assert tiny.jsorb_covisibility_build_caps(None, None) == 0
    # the refusals that need no device: a NULL matcher, a NULL state
    assert l.jsorb_update_connections_async(None, None, None, None, 0, *([None] * 5)) == -1
    assert l.jsorb_update_connections(None, None, None, None, 0, *([None] * 7)) == -1 and l.jsorb_update_connections_stats(*([None] * 8)) == -1 and l.jsorb_update_connections_scratch(None, None, None) == -1
    assert l.jsorb_erase_connections_async(None, None, None, 0, None, None) == -1 and l.jsorb_connected_mask_async(None, None, 0, None) == -1
    assert l.jsorb_best_covisibles_async(None, None, 0, None, 1, None, None) == -1 and l.jsorb_covisibility_copy(None, 0, *([None] * 5)) == -1


def test_the_shim_and_the_example_compile(tmp_path):
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb
    g.build()
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    for text in ("class Covisibility", "UpdateConnections(", "EraseConnections(", "GetConnectedKeyFrames(", "GetBestCovisibilityKeyFrames(",
                 "GetCovisiblesByWeight(", "GetWeight("):
        assert text in shim, text
    exe = jb.build_example("update_connections", str(tmp_path / "update_connections"))
    assert os.path.getsize(exe) > 0
