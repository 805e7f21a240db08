"""-m "not gpu": the restatements and cases of tests/local_map_cases.py, and the product boundary of jsorb_local_map_points - the ABI, the ctypes
signatures, the build variant, the shim and the example.  No compute call is made."""
import ctypes
import os
import re

import numpy as np
import pytest

import local_map_cases as lc
from test_tracking_edges import k16_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsorb_local_map_points_async", "jsorb_local_map_points", "jsorb_local_map_stats", "jsorb_local_map_build_caps", "jsorb_map_points_scatter_async")


def lists_of(name):
    W, c = lc.world(), lc.build_case(name)
    return W, c, lc.update_local_points_restated(W["bad"], c["keyframes"], c["frame_rows"])


@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_two_restatements_agree(name):
    W, c, a = lists_of(name)
    b = lc.update_local_points_numpy(W["bad"], c["keyframes"], c["frame_rows"])
    assert a["stats"] == b["stats"]
    for k in ("blocked_in", "local", "map_points"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert len(np.unique(a["local"])) == len(a["local"]) and not W["bad"][a["local"]].any()
    assert len(c["entries"]) == c["kf_start"][-1] == a["stats"]["n_entries"] == sum(lc.CASES[name][0])


@pytest.mark.parametrize("name", list(lc.CASES))
def test_every_case_is_non_vacuous(name):
    """at least one entry dropped for each reason the case claims, points inside the frustum left over, and what the case is named for is in it"""
    W, c, a = lists_of(name)
    for reason in c["claims"]:
        assert a["stats"][reason] >= 1, reason
    if name in lc.EMPTY:
        assert c["claims"] == () and len(a["local"]) == 0 and c["frame_rows"] is not None
        return
    assert set(c["claims"]) >= set(lc.REASONS[:-1])
    inside = k16_restated(lc.frustum_block(W, a["map_points"]), W["n_levels"], lambda x: np.log(x).astype(np.float32))[2]
    assert inside.sum() >= 2 and (inside == 0).any()                     # counts[2] > 0, and capacity counts[2] - 1 still keeps a point
    e, kfs = c["entries"], c["keyframes"]
    assert sum(c["shared"] in k for k in kfs) >= min(3, sum(len(k) >= 30 for k in kfs)) and (e == c["shared"]).sum() >= 3      # a row in three keyframes
    assert any((k == c["twice"]).sum() >= 2 for k in kfs)                 # a row twice in one keyframe
    assert (e == -1).any() and (e == lc.N_ROWS).any() and (e < -1).any() and W["bad"][e[(e >= 0) & (e < lc.N_ROWS)]].any()
    if c["frame_rows"] is not None:
        first = np.nonzero(e == c["seen_first"])[0]
        assert len(first) >= 2 and c["seen_first"] in a["local"] and c["seen_first"] not in a["map_points"]      # seen, its first occurrence kept in the list
        f = c["frame_rows"]
        assert (f == -1).any() and (f >= lc.N_ROWS).any() and (f < -1).any() and W["bad"][f[(f >= 0) & (f < lc.N_ROWS)]].any()
        assert a["blocked_in"].any() and not a["blocked_in"].all()
    else:
        assert a["stats"]["n_seen"] == 0 and len(a["blocked_in"]) == 0


def test_the_cases_cover_what_the_contract_names():
    sizes = {n: s for n, (s, _) in lc.CASES.items()}
    assert sizes["empty_first_middle_last"][0] == 0 and sizes["empty_first_middle_last"][-1] == 0 and 0 in sizes["empty_first_middle_last"][1:-1]
    assert sizes["zero_keyframes"] == [] and sum(sizes["only_empty_keyframes"]) == 0 and not lc.CASES["no_frame"][1]
    for chunk in lc.CHUNKS:
        assert sorted(sum(sizes[n]) for n in lc.edge_cases(chunk)) == [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    assert all(len(s) <= 6 for s in sizes.values())
    assert lc.capacities(5) == [0, 4, 5, 6] and lc.capacities(0) == [0, 1]


def test_the_world_takes_every_exit_of_k16():
    W = lc.world()
    rows = np.arange(lc.N_ROWS)
    f, level, inside = k16_restated(lc.frustum_block(W, rows), W["n_levels"], lambda x: np.log(x).astype(np.float32))
    for kind in range(1, 6):
        assert (W["kind"] == kind).sum() >= 50 and not inside[W["kind"] == kind].any(), kind      # behind, outside the image, too far, too near, view angle
    assert inside[W["kind"] == 0].mean() > 0.95 and W["bad"].sum() >= 20
    assert len(set(level[inside == 1].tolist())) == W["n_levels"]


def test_abi_bindings_and_build():
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb, orb
    lib = ctypes.CDLL(g.build())
    hdr = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    src = open(os.path.join(ROOT, "jetson_slam_amd", "orb.py")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
    for cite in ("src/Tracking.cpp:1818-1841", ":1352-1367", ":1410-1420", "src/cuda/tracking_isinfrustum.cu:19-117", "src/ORBmatcher.cpp:43-47"):
        assert cite in hdr, cite
    l = orb.load_library()
    assert len(l.jsorb_local_map_points_async.argtypes) == 19 and len(l.jsorb_local_map_points.argtypes) == 21
    assert len(l.jsorb_local_map_stats.argtypes) == 7 and len(l.jsorb_map_points_scatter_async.argtypes) == 15
    # the structs as the header lays them out (x86-64: one int, padding, eleven pointers; 19 floats, 5 ints, 2 floats; 9 floats, a byte, padding)
    assert ctypes.sizeof(orb.JsorbMapPointTable) == 96 and orb.JsorbMapPointTable.Px.offset == 8
    assert ctypes.sizeof(orb.JsorbFrustumParams) == 104 and orb.JsorbFrustumParams.minX.offset == 76
    assert orb.MAP_POINT_RECORD_DTYPE.itemsize == 40 and orb.MAP_POINT_RECORD_DTYPE.fields["bad"][1] == 36
    assert orb.local_map_build_caps() == lc.CHUNKS[0]
    p = orb.make_frustum_params(np.eye(3), [1, 2, 3], [4, 5, 6], (7, 8, 9, 10), (0, 320, 0, 240), 3, 0.18, 0.5)
    assert list(p.tcw) == [1, 2, 3] and list(p.Ow) == [4, 5, 6] and (p.fx, p.cy, p.maxX, p.maxY, p.nScaleLevels) == (7, 10, 320, 240, 3)
    assert "k_local_map.hip" in jb.SOURCES and "jsorb_localmap.hip" in jb.SOURCES
    assert jb.VARIANTS["tiny_local_map"] == (["-DLM_CHUNK=%d" % lc.CHUNKS[1]], ["k_local_map.hip"])
    caps = ctypes.c_int()
    tiny = ctypes.CDLL(jb.build_variant("tiny_local_map", *jb.VARIANTS["tiny_local_map"]))
    assert tiny.jsorb_local_map_build_caps(ctypes.byref(caps)) == 0 and caps.value == lc.CHUNKS[1]
    # the refusals that need no device: a NULL handle, the scatter's sizes and arrays
    assert l.jsorb_local_map_points_async(None, 0, None, None, 0, None, None, None, 0, *([None] * 10)) == -1 and l.jsorb_local_map_stats(*([None] * 7)) == -1
    assert l.jsorb_map_points_scatter_async(None, -1, *([None] * 10), 0, None, None) == -1
    assert l.jsorb_map_points_scatter_async(None, 4, *([None] * 10), 3, None, None) == -1
    assert l.jsorb_map_points_scatter_async(None, 4, *([None] * 10), 0, None, None) == 0


def test_the_shim_and_the_example_compile(tmp_path):
    import __graft_entry__ as g
    from jetson_slam_amd import build as jb
    g.build()
    assert "track_local_map" in jb.EXAMPLES
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    assert "class MapPointTable" in shim and "UpdateLocalPoints(" in shim
    exe = jb.build_example("track_local_map", str(tmp_path / "track_local_map"))
    assert os.path.getsize(exe) > 0
