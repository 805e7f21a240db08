"""The two host statements of MapPoint::ComputeDistinctiveDescriptors (tests/distinct_cases.py) against each other: the sequential transcription of
src/MapPoint.cpp:273-338 and the numpy restatement of k_distinct.hip's method, on the constructed cases (one per decision) and on the random blocks,
whose coverage counters must all be non-zero; then the declarations of the new entry points.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import distinct_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dc.constructed()


@pytest.fixture(scope="module")
def blocks():
    """seed -> (world, the transcription's (descriptors, best_obs, best_median) from zeroed descriptors): computed once, never changed"""
    out = {}
    for seed in dc.BLOCK_SEEDS:
        w = dc.block(seed)
        out[seed] = (w, dc.world_reference(w))
    return out


def test_constructed_cases_decide_what_they_name():
    for name, (obs, bi, bm) in CASES.items():
        old = np.full(32, 0x5a, np.uint8)
        desc, got_i, got_m = dc.reference_point(obs, old)
        kept = [d for d, bad in obs if not bad]
        if bi is not None:
            assert (got_i, got_m) == (bi, bm), name
        if got_i < 0:
            assert np.array_equal(desc, old), name                   # rule 1: the old descriptor stays
        else:
            assert np.array_equal(desc, kept[got_i]), name
            assert dc.point_by_keys(np.stack(kept)) == (got_i, got_m), name
    ref = lambda n: dc.reference_point(CASES[n][0], None)
    # index 0 for N = 1 and 2 whatever the descriptors stand there
    assert ref("n2")[1] == ref("n2_swapped")[1] == 0 and not np.array_equal(ref("n2")[0], ref("n2_swapped")[0])
    # a tie on the best median: the first row; the two swapped: the other descriptor
    assert ref("tie_pair")[1:] == ref("tie_pair_swapped")[1:] and not np.array_equal(ref("tie_pair")[0], ref("tie_pair_swapped")[0])
    # no tie on the best median: a permutation gives the same bytes at another index
    a, b = ref("permute_a"), ref("permute_b")
    assert np.array_equal(a[0], b[0]) and a[1] != b[1] and a[2] == b[2]
    assert (ref("complements")[0] == 255).all() and ref("max_median")[2] == 0


def test_restatement_equals_transcription_on_the_constructed_world():
    names, w = dc.constructed_world(CASES)
    start, row = dc.csr(w)
    old = np.full((len(names), 32), 0x5a, np.uint8)
    want, bo, bm = dc.world_reference(w, old)
    for caps in (dc.SHIPPED, dc.TINY):
        r = dc.restatement(start, row, w["kf_desc"], desc_out=old, want_changed=True, caps=caps)
        assert np.array_equal(r["best_obs"], bo) and np.array_equal(r["best_median"], bm)
        assert np.array_equal(r["desc_out"], want) and np.array_equal(r["changed"], (want != old).any(axis=1))
    for p, n in enumerate(names):
        if CASES[n][1] is not None:
            assert (bo[p], bm[p]) == CASES[n][1:], n


def test_blocks_cover_every_decision(blocks):
    for seed, (w, (_, bo, _)) in blocks.items():
        c = dc.coverage(w, bo)
        assert all(v > 0 for v in c.values()), (seed, c)
        assert {"n_16", "n_17", "n_64", "n_65", "n_1024", "n_1025", "n_4", "n_5", "n_8", "n_9"} <= set(c)


def test_restatement_equals_transcription_on_the_blocks(blocks):
    for seed, (w, (want, bo, bm)) in blocks.items():
        start, row = dc.csr(w)
        for caps in (dc.SHIPPED, dc.TINY):
            r = dc.restatement(start, row, w["kf_desc"], desc_out=np.zeros_like(want), want_changed=True, caps=caps)
            assert np.array_equal(r["best_obs"], bo) and np.array_equal(r["best_median"], bm) and np.array_equal(r["desc_out"], want), seed
            N = np.diff(start)
            assert r["stats"][:3] == tuple(int(((N > a) & (N <= b)).sum()) for a, b in ((0, caps[0]), (caps[0], caps[1]), (caps[1], 1 << 30)))
            assert r["stats"][3:6] == (int((N > caps[2]).sum()), int((N == 0).sum()), 0) and r["stats"][7] == N.max()
            assert r["stats"][6] == int(r["changed"].sum()) == int((want != 0).any(axis=1).sum())


def test_restatement_defines_the_invalid_inputs():
    """obs_start out of range or descending, obs_row out of range, out_row out of range: -1 / -1, the row untouched, one more invalid each"""
    kf = dc.clustered(np.random.default_rng(3), 40)
    start = np.array([0, 3, 6, 9, 12, 15, 18], np.int32)
    row = np.arange(18, dtype=np.int32)
    old = np.full((6, 32), 7, np.uint8)
    good = dc.restatement(start, row, kf, desc_out=old, want_changed=True)
    assert (good["best_obs"] >= 0).all() and good["stats"][5] == 0
    for bad_start, bad_row, out_row, hit in (([0, 3, 6, 9, 12, 15, 19], row, None, [5]), ([0, 3, -1, 9, 12, 15, 18], row, None, [1, 2]),
                                             ([0, 3, 9, 6, 12, 15, 18], row, None, [2]), (start, np.where(row == 4, 40, row), None, [1]),
                                             (start, np.where(row == 17, -1, row), None, [5]), (start, row, [0, 1, 2, 6, 4, -1], [3, 5])):
        r = dc.restatement(bad_start, bad_row, kf, out_row=out_row, desc_out=old, want_changed=True, n_obs=18)
        ok = np.setdiff1d(np.arange(6), hit)
        assert (r["best_obs"][hit] == -1).all() and (r["best_median"][hit] == -1).all() and r["stats"][5] == len(hit) and not r["changed"][hit].any()
        dst = ok if out_row is None else np.array(out_row)[ok]
        same = np.array([p for p in ok if bad_start[p] == start[p] and bad_start[p + 1] == start[p + 1]])      # (a moved offset makes another point)
        assert np.array_equal(r["best_obs"][same], good["best_obs"][same])
        assert (r["best_obs"][ok] >= 0).all() and np.array_equal(r["desc_out"][dst][np.isin(ok, same)], good["desc_out"][same])
        rest = np.setdiff1d(np.arange(6), dst)
        assert (r["desc_out"][rest] == 7).all()


NAMES = ("jsorb_distinctive_descriptors_async", "jsorb_distinctive_descriptors", "jsorb_distinctive_descriptors_stats", "jsorb_distinct_build_caps")


def test_header_binding_and_build_declare_the_new_entry_points(orb):
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    bound = orb.load_library()
    raw = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(orb.__file__).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in orb.EXPORTS and '"%s": (' % n in src, n
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert decl, n
        n_args = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(getattr(bound, n).argtypes), (n, n_args)
    assert "MapPoint.cpp:273-338" in raw and "LocalMapping.cpp:158-159" in raw
    for m in ("distinctive_descriptors", "distinctive_descriptors_stats"):
        assert callable(getattr(orb.KeyframeMatcher, m))
    assert orb.distinct_build_caps() == dc.SHIPPED
    from jetson_slam_amd import build as jb
    assert "k_distinct.hip" in jb.SOURCES and "jsorb_mappoints.hip" in jb.SOURCES and "update_map_points" in jb.EXAMPLES
    assert jb.VARIANTS["tiny_distinct"] == (["-DDD_GROUP_LANES=%d" % dc.TINY[0], "-DDD_WAVE_LANES=%d" % dc.TINY[1], "-DDD_LDS_DESC=%d" % dc.TINY[2]], ["k_distinct.hip"])
    ksrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_distinct.hip")).read()
    for name, val in zip(("DD_GROUP_LANES", "DD_WAVE_LANES", "DD_LDS_DESC"), dc.SHIPPED):
        assert re.search(r"#define %s %d\b" % (name, val), ksrc), name


def test_refusals_without_a_device(orb):
    """a NULL matcher is refused by every entry point; the binding refuses what it can see without a device"""
    import torch
    from kf_refusal_cases import FakeTensor
    lib = orb.load_library()
    assert lib.jsorb_distinctive_descriptors_async(None, 0, None, 0, None, None, 0, None, 0, None, None, None, None) == -1
    assert lib.jsorb_distinctive_descriptors(None, 0, None, 0, None, None, 0, None, 0, None, None, None, None) == -1
    assert lib.jsorb_distinctive_descriptors_stats(None, *[None] * 8) == -1
    assert lib.jsorb_distinct_build_caps(None, None, None) == 0
    K = orb.KeyframeMatcher
    st, row, kf = FakeTensor(torch.int32, (4,)), FakeTensor(torch.int32, (9,)), FakeTensor(torch.uint8, (20, 32))

    def refused(*a):
        with pytest.raises(orb.JsorbError) as e:
            K._distinct_args(*a)
        return str(e.value)
    assert K._distinct_args(st, row, kf, None, None, False)[1] == 3
    assert "must be a device tensor" in refused(np.zeros(4, np.int32), row, kf, None, None, False)
    assert "n_points + 1 offsets" in refused(FakeTensor(torch.int64, (4,)), row, kf, None, None, False)
    assert "must be a contiguous" in refused(st, FakeTensor(torch.int64, (9,)), kf, None, None, False)
    assert "must be a contiguous" in refused(st, row, FakeTensor(torch.uint8, (20, 16)), None, None, False)
    assert "must be a contiguous" in refused(st, row, kf, FakeTensor(torch.int32, (4,)), FakeTensor(torch.uint8, (3, 32)), False)
    assert "changed needs desc_out" in refused(st, row, kf, None, None, True)
