"""-m "not gpu": the two yardsticks of tests/kf_culling_cases.py against each other on the named cases and on 300 seeded random worlds, the
mutants, the coverage floors, and the product boundary of jsorb_cull_keyframes - the ABI, the ctypes signatures, the source list.  No compute
call is made."""
import ctypes
import os
import re

import numpy as np
import pytest

import kf_culling_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsorb_cull_keyframes_async", "jsorb_cull_keyframes", "jsorb_cull_keyframes_stats", "jsorb_cull_keyframes_build_caps")


@pytest.fixture(scope="module")
def worlds():
    out = []
    for seed in range(300):
        W = kc.random_world(seed)
        out.append((W, kc.run_restated(W)))
    return out


@pytest.mark.parametrize("name", list(kc.CASES))
def test_the_two_yardsticks_agree_and_the_case_shows_what_it_is_named_for(name):
    world, expect = kc.build_case(name)
    r = kc.run_restated(world)
    kc.same(kc.run_literal(world), r, name)
    kc.check_expect(r, expect, world)


def test_seeded_random_worlds_bit_for_bit(worlds):
    assert len(worlds) == 300
    for W, r in worlds:                          # every world: none is left out
        G = W["G"]
        assert len(G["state"]) <= 24 and G["point_len"].max() <= 48 and W["views"]["octave"].max() <= 7
        kc.same(kc.run_literal(W), r, W["name"])


def test_coverage_floors(worlds):
    n_cull = n_two = n_bad = n_changed = n_tree = 0
    for W, r in worlds:
        c = r["counts"]
        n_cull += c[2] > 0
        n_two += c[2] >= 2
        n_bad += c[5] > 0
        n_changed += kc.verdict_changed_by_a_cull(W)
        culled = {int(s): int(W["G"]["parent"][s]) for s in r["culled_slot"] if s >= 0}
        # a record that is not the fallback: the new parent is not the culled keyframe's own parent
        recs = r["reparent_out"][:min(int(c[8]), W["cap"])]
        n_tree += any(int(W["G"]["parent"][ch]) in culled and p != culled[int(W["G"]["parent"][ch])] for ch, p in recs.tolist())
    assert n_cull >= 100 and n_two >= 40 and n_bad >= 40 and n_changed >= 20 and n_tree >= 20, (n_cull, n_two, n_bad, n_changed, n_tree)


@pytest.mark.parametrize("mutant", list(kc.MUTANTS))
def test_each_mutant_fails_its_case(mutant):
    world, expect = kc.build_case(kc.MUTANTS[mutant])
    good = kc.run_restated(world)
    kc.check_expect(good, expect, world)
    bad = kc.run_restated(world, mutant)
    with pytest.raises(AssertionError):
        kc.same(good, bad)
    with pytest.raises(AssertionError):
        kc.check_expect(bad, expect, world)


@pytest.mark.parametrize("run", [kc.run_literal, kc.run_restated])
def test_max_cull_1_repeated_equals_one_call_of_16(worlds, run):
    n = 0
    for W, _ in worlds[:120]:
        one = run(dict(W, max_cull=kc.MAX_CULL))
        cand = [int(a) for a in W["cand"] if a >= 0]
        if one["counts"][2] < 2 or len(set(cand)) != len(cand):      # (the list holds a slot once: a call that continues sees only its own part of it)
            continue
        n += 1
        last, total, culled, recs, tail = kc.continued(W, run, 1)
        for k in ("decision", "n_mps", "n_redundant"):
            assert np.array_equal(total[k], one[k]), (W["name"], k)
        assert culled == [int(s) for s in one["culled_slot"] if s >= 0]
        assert recs[:W["cap"]] == [tuple(x) for x in one["reparent_out"][:int(one["counts"][8])].tolist()]
        assert tail[:8].tolist() == one["counts"][1:9].tolist()
        for k in kc.WRITTEN + ("bad", "ref_slot", "to_be_erased"):
            assert (last[k] is None and one[k] is None) or np.array_equal(last[k], one[k]), (W["name"], k)
        for k in one["cov"]:
            assert np.array_equal(last["cov"][k], one["cov"][k]), (W["name"], k)
    assert n >= 15


def test_the_double_comparison_is_the_integer_one():
    # (double)n_redundant > 0.9 * (double)n_mps against 10 * n_redundant > 9 * n_mps at and next to every multiple of 10 and at large counts
    for n_mps in list(range(0, 2000)) + [2 ** 31 - 1 - k for k in range(40)] + [10 ** 9 + k for k in range(40)]:
        lo = 9 * n_mps // 10
        for n_red in (lo - 1, lo, lo + 1, lo + 2):
            if n_red >= 0:
                assert (float(n_red) > 0.9 * float(n_mps)) == (10 * n_red > 9 * n_mps), (n_mps, n_red)


def test_abi_bindings_and_build():
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb, orb
    lib = ctypes.CDLL(g.build())
    hdr = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    src = open(os.path.join(ROOT, "jetson_slam_amd", "orb.py")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
    for cite in ("src/LocalMapping.cpp:638-702", "src/KeyFrame.cpp:457-549", "src/MapPoint.cpp:142-168", ":182-199", ":129-140", ":649", ":666", ":671-689",
                 ":699", ":463-467", ":483-541", ":473-475"):
        assert cite in hdr, cite
    l = orb.load_library()
    assert len(l.jsorb_cull_keyframes_async.argtypes) == 19 and len(l.jsorb_cull_keyframes.argtypes) == 25
    # the structs as the header lays them out (x86-64: an int and four pointers; eight pointers)
    assert ctypes.sizeof(orb.JsorbKeyframeViews) == 40 and orb.JsorbKeyframeViews.octave.offset == 8 and ctypes.sizeof(orb.JsorbCullingState) == 64
    assert orb.cull_keyframes_build_caps() == (4096, kc.MAX_CULL) and orb.CULL_COUNTS == kc.COUNTS and orb.CULL_MAX == kc.MAX_CULL
    assert (orb.CULL_KEPT, orb.CULL_CULLED, orb.CULL_DEFERRED, orb.CULL_SKIPPED, orb.CULL_NOT_REACHED) == (kc.KEPT, kc.CULLED, kc.DEFERRED, kc.SKIPPED, kc.NOT_REACHED)
    assert "k_kf_culling.hip" in jb.SOURCES and "jsorb_culling.hip" in jb.SOURCES
    # the refusals that need no device: a NULL matcher
    assert l.jsorb_cull_keyframes_async(None, None, None, None, None, None, 0, -1, 0, None, 1, None, 0, *([None] * 6)) == -1
    assert l.jsorb_cull_keyframes(None, None, None, None, None, None, 0, -1, 0, None, 1, None, 0, *([None] * 12)) == -1
    assert l.jsorb_cull_keyframes_stats(None, None) == -1 and l.jsorb_cull_keyframes_build_caps(None, None) == 0


def test_the_shim_and_the_example_compile(tmp_path):
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb
    g.build()
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    for text in ("class KeyframeViews", "class CullingState", "struct CulledKeyFrames", "KeyFrameCulling(", "set_keyframe_views("):
        assert text in shim, text
    assert "keyframe_culling" in jb.EXAMPLES
    exe = jb.build_example("keyframe_culling", str(tmp_path / "keyframe_culling"))
    assert os.path.getsize(exe) > 0
