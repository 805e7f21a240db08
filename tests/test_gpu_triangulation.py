"""-m gpu: jsorb_search_for_triangulation* (k_bow_group + k_tri_match + k_tri_resolve) on a jsorb_keyframe_matcher against the sequential
transcription of ORBmatcher::SearchForTriangulation and the kernels' restatement of tests/test_triangulation_host.py - match12, counts and
statistics, bit for bit."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import REAL_SEED, both_transforms, frame_side, sampled_voc
from test_gpu_search_local import _dev, _mk
from test_triangulation_host import (ROTATION_KEPT, CONSTRUCTED, F_LINE, FAR, TR_KF_CHUNK, agree, default_params, geometry, random_case, scale_tables,
                                     search_for_triangulation_reference, search_for_triangulation_restated, sides)

pytestmark = pytest.mark.gpu
KF1_DT = dict(node=np.int32, free=np.uint8, stereo=np.uint8, x=np.float32, y=np.float32, angle=np.float32, desc=np.uint8)
KF2_DT = dict(KF1_DT, octave=np.int32)
NONE = (0, 0, 0, 0, (-1, -1, -1))


def tri_params(orb, prm):
    return orb.make_triangulation_params(prm["scale_factor"][:prm["n_levels"]], prm["level_sigma2"][:prm["n_levels"]], th_low=prm["th_low"],
                                         check_orientation=prm["check_orientation"], only_stereo=prm["only_stereo"])


def host_both(KF1, KF2, geom, prm):
    """the transcription and the restatement (which must agree): (match12, nmatches, (node pairs, distances, line tests, largest node, ind))"""
    ref = search_for_triangulation_reference(KF1, KF2, geom, prm)
    st = agree(ref, search_for_triangulation_restated(KF1, KF2, geom, prm))
    return ref[0], ref[1], st


def dev_side(kf, dts):
    return {k: _dev(np.asarray(kf[k], dt).reshape((-1, 32) if k == "desc" else (-1,))) for k, dt in dts.items()}


def concat(kf2s):
    """the KF2s as the concatenated arrays of jsorb_search_for_triangulation_async"""
    start = np.cumsum([0] + [len(k["node"]) for k in kf2s]).astype(np.int32)
    cat = {k: np.concatenate([np.zeros((0, 32) if k == "desc" else (0,), dt)] + [np.asarray(kf[k], dt).reshape((-1, 32) if k == "desc" else (-1,)) for kf in kf2s])
           for k, dt in KF2_DT.items()}
    return start, cat


def check_search(orb, m, KF1, kf2s, geoms, prm, sync=False, hosts=None):
    """one device call of KF1 against the KF2s, held to both host functions, statistics included; returns the host's results per keyframe"""
    start, cat = concat(kf2s)
    F = np.stack([g["F12"] for g in geoms]) if geoms else np.zeros((0, 9), np.float32)
    E = np.array([[g["ex"], g["ey"]] for g in geoms], np.float32).reshape(-1, 2)
    d1, d2 = dev_side(KF1, KF1_DT), dev_side(cat, KF2_DT)
    if sync:
        mk, cnt = m.search_for_triangulation_host(d1, start, d2, F, E, tri_params(orb, prm))
    else:
        mk, cnt = m.search_for_triangulation(d1, start, d2, F, E, tri_params(orb, prm))      # (waits for its own work)
        mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
    n1 = len(KF1["node"])
    if hosts is None:
        hosts = [host_both(KF1, K2, g, prm) if len(K2["node"]) and n1 else (np.full(n1, -1), 0, NONE) for K2, g in zip(kf2s, geoms)]
    assert mk.shape == (len(kf2s), n1)
    for i, h in enumerate(hosts):
        assert np.array_equal(mk[i], h[0]) and int(cnt[i]) == h[1], (i, int(cnt[i]), h[1])
    want = (sum(h[2][0] for h in hosts), sum(h[2][1] for h in hosts), sum(h[2][2] for h in hosts), max([h[2][3] for h in hosts] + [0]),
            hosts[0][2][4] if hosts else (-1, -1, -1))
    assert m.stats() == want, (m.stats(), want)
    return hosts


@pytest.fixture(scope="module")
def matcher(orb):
    m = orb.KeyframeMatcher()
    yield m
    m.close()


def observe(rng, KF1, n2, i=0):
    """a KF2 of n2 keypoints that observes KF1's keypoints (their descriptors and nodes), most of them on the line x2 = 0 of F_LINE; every
    second keyframe keeps the geometry of its own random cloud, which few candidates pass"""
    _, KF2, geom, _ = random_case(rng, 0, n2, 6, forward=bool(i % 4 == 1))
    n1 = len(KF1["node"])
    if n1 and n2:
        src = rng.integers(0, n1, n2)
        KF2["desc"], KF2["node"] = KF1["desc"][src].copy(), KF1["node"][src].copy()
    if i % 2 == 0:
        KF2["x"] = np.where(rng.random(n2) < 0.7, 0.0, 5.0).astype(np.float32)
        geom = geometry(F_LINE, *FAR)
    return KF2, geom


EMPTY2 = {k: np.zeros((0, 32) if k == "desc" else (0,), dt) for k, dt in KF2_DT.items()}


# ---- every constructed case of the host test, both forms ----
def test_constructed_cases_through_the_device(orb, matcher):
    for name in sorted(CONSTRUCTED):
        KF1, KF2, geom, prm, want, count = CONSTRUCTED[name]
        for sync in (False, True):
            h = check_search(orb, matcher, KF1, [KF2], [geom], prm, sync=sync)
            assert list(h[0][0]) == want and h[0][1] == count, name
            assert name not in ROTATION_KEPT or matcher.stats()[4] == ROTATION_KEPT[name], name      # the rotation check's edges: kept_bins


# ---- the group, wave and workgroup edges: KF2 node runs of 1, 15, 16, 17 and 33 entries, KF1 of 1, 15, 16, 17 and 257 sorted positions ----
@pytest.mark.parametrize("n1", [1, 15, 16, 17, 257])
def test_run_and_position_edges(orb, matcher, n1):
    rng = np.random.default_rng(n1)
    g = geometry(F_LINE, *FAR)
    for run in (1, 15, 16, 17, 33):
        # one node of `run` KF2 entries with distances in 0..60 (ties likely), some off the line, some with a map point; KF1: n1 keypoints of that
        # node plus a second node that only KF1 has
        d2 = rng.integers(0, 61, run)
        KF1, KF2 = sides(list(d2), kf1_n=n1, x2=np.where(rng.random(run) < 0.3, 5.0, 0.0), free2=(rng.random(run) < 0.8), octave=rng.integers(0, 8, run),
                         angle2=rng.uniform(0, 360, run))
        KF1["desc"] = np.stack([np.packbits((rng.random(256) < 0.04).astype(np.uint8)) for _ in range(n1)])
        KF1["node"] = np.where(np.arange(n1) % 5 == 4, 9, 0).astype(np.int32)
        KF1["angle"] = rng.uniform(0, 360, n1).astype(np.float32)
        for rot in (0, 1):
            h = check_search(orb, matcher, KF1, [KF2], [g], default_params(check_orientation=rot), sync=bool(rot))
            assert h[0][2][3] == run
    # the last sorted position alone in its node: KF1 of n1 nodes against KF2 with all of them
    KF1, KF2 = sides([10] * n1, kf1_n=n1, node1=np.arange(n1)[::-1], node2=np.arange(n1))
    h = check_search(orb, matcher, KF1, [KF2], [g], default_params(check_orientation=0))
    assert h[0][1] == n1 and list(h[0][0]) == list(range(n1))[::-1]


# ---- 0, 1, 3 and 256 keyframes, an empty one in the middle; more than one launch chunk ----
@pytest.mark.parametrize("n_kf", [0, 1, 3, 256])
def test_keyframe_counts(orb, matcher, n_kf):
    rng = np.random.default_rng(100 + n_kf)
    KF1 = random_case(rng, 40, 0, 4)[0]
    kf2s, geoms, prm = [], [], default_params()
    for i in range(n_kf):
        KF2, geom = observe(rng, KF1, 0 if i == 1 else int(rng.integers(1, 12)), i)
        kf2s.append(KF2)
        geoms.append(geom)
    assert n_kf <= TR_KF_CHUNK or n_kf > 2 * TR_KF_CHUNK
    for sync in (False, True):
        h = check_search(orb, matcher, KF1, kf2s, geoms, prm, sync=sync)
    if n_kf >= 3:
        assert h[1][1] == 0 and sum(x[1] for x in h) > 0


# ---- real frames: two extracts of a synthetic stereo pair through the BoW transform with a sampled vocabulary ----
def test_real_frames(orb, configs, matcher):
    c = configs["c1"]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    rng = np.random.default_rng(12)
    frames = []
    for img in (left, right):
        g.extract(img)
        kp = g.keypoints()
        s = frame_side(kp, g.descriptors())
        n = len(s["angle"])
        s.update(x=kp[:n].astype(np.float32), y=kp[n:2 * n].astype(np.float32), octave=kp[4 * n:5 * n].astype(np.int32),
                 free=(rng.random(n) < 0.8).astype(np.uint8), stereo=(rng.random(n) < 0.5).astype(np.uint8))
        frames.append(s)
    L, R = frames
    tree = sampled_voc(L["desc"])
    voc = orb.Vocabulary(tree, levels_up=1)
    for s in frames:
        s["node"] = orb.bow_transform_descriptors(voc, _dev(s["desc"]))[1].cpu().numpy()
        assert np.array_equal(s["node"], both_transforms(tree, s["desc"], 1)[1])
    # a rectified pair: x1^T F12 x2 = y2 - y1 (the epipolar lines are the rows), the epipole at infinity
    geom = geometry([0, 0, 0, 0, 0, -1, 0, 1, 0], 1e9, float(c["h"]) / 2)
    s, s2 = scale_tables(c["L"])
    for rot, only in ((1, 0), (0, 0), (1, 1)):
        prm = default_params(check_orientation=rot, only_stereo=only, n_levels=c["L"], scale_factor=s, level_sigma2=s2)
        h = check_search(orb, matcher, L, [R, EMPTY2, L], [geom, geom, geom], prm, sync=bool(rot))
        assert h[0][1] >= (1 if only else 15) and h[2][1] > h[0][1] and h[0][2][0] > 20, (rot, only, h[0][1])


# ---- twenty calls back to back on one matcher with changing sizes: scratch reuse leaks no state ----
def test_twenty_calls_with_changing_sizes(orb):
    m = orb.KeyframeMatcher()
    rng = np.random.default_rng(77)
    for call in range(20):
        n1, n_kf = int(rng.choice([0, 3, 60, 200])), int(rng.choice([1, 2, 5]))
        KF1, _, _, prm = random_case(rng, n1, 0, 6, check_orientation=call % 2)
        kf2s, geoms = [], []
        for i in range(n_kf):
            KF2, geom = observe(rng, KF1, int(rng.choice([0, 7, 90])), i)
            kf2s.append(KF2)
            geoms.append(geom)
        check_search(orb, m, KF1, kf2s, geoms, prm, sync=call % 3 == 0)
    m.close()


# ---- the async form on an external stream ----
def test_async_on_an_external_stream(orb):
    import torch
    m = orb.KeyframeMatcher()
    own = m.get_stream()
    assert own
    st = torch.cuda.Stream()
    m.set_stream(st.cuda_stream)
    assert m.get_stream() == st.cuda_stream
    rng = np.random.default_rng(5)
    KF1, KF2, geom, prm = random_case(rng, 120, 150, 5)
    start, cat = concat([KF2])
    with torch.cuda.stream(st):
        d1, d2 = dev_side(KF1, KF1_DT), dev_side(cat, KF2_DT)     # uploaded on the stream the matcher runs on: ordered without a wait
        mk, cnt = m.search_for_triangulation(d1, start, d2, geom["F12"][None], np.array([[geom["ex"], geom["ey"]]], np.float32), tri_params(orb, prm), wait=False)
        mk, cnt = mk.cpu(), cnt.cpu()
    st.synchronize()
    h = host_both(KF1, KF2, geom, prm)
    assert np.array_equal(mk.numpy()[0], h[0]) and int(cnt[0]) == h[1] > 0 and m.stats() == h[2]
    m.set_stream(None)
    assert m.get_stream() == own
    check_search(orb, m, KF1, [KF2], [geom], prm)
    m.close()


# ---- a second matcher on a second thread while an extractor handle extracts ----
def test_matcher_thread_beside_an_extractor(orb, configs):
    c = configs["c1"]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    alone_kp, alone_desc = g.keypoints().copy(), g.descriptors().copy()
    rng = np.random.default_rng(9)
    KF1, KF2, geom, prm = random_case(rng, 200, 220, 8)
    hosts = [host_both(KF1, KF2, geom, prm)]
    m = orb.KeyframeMatcher()
    check_search(orb, m, KF1, [KF2], [geom], prm, hosts=hosts)
    errors = []

    def matching():
        try:
            for i in range(10):
                check_search(orb, m, KF1, [KF2], [geom], prm, sync=bool(i % 2), hosts=hosts)
        except BaseException as e:      # noqa: BLE001 - reported on the main thread
            errors.append(e)

    t = threading.Thread(target=matching)
    t.start()
    for i in range(10):
        g.extract(right if i % 2 else left)
        if i % 2 == 0:
            assert np.array_equal(g.keypoints(), alone_kp) and np.array_equal(g.descriptors(), alone_desc)
    t.join()
    assert not errors, errors
    m.close()


# ---- validation ----
def test_edges_and_validation(orb, matcher):
    import torch
    lib = orb.load_library()
    fresh = orb.KeyframeMatcher()
    assert lib.jsorb_search_for_triangulation_stats(fresh.handle, None, None, None, None, None) == -4      # before any call
    fresh.close()
    rng = np.random.default_rng(3)
    KF1, KF2, geom, prm = random_case(rng, 50, 60, 3)
    p = tri_params(orb, prm)
    d1, (start, cat) = dev_side(KF1, KF1_DT), concat([KF2])
    d2 = dev_side(cat, KF2_DT)
    F, E = np.ascontiguousarray(geom["F12"]), np.array([geom["ex"], geom["ey"]], np.float32)
    mk = torch.zeros(2 * 50 + 8, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    p1 = [d1[k].data_ptr() for k in orb.KeyframeMatcher.KF1_KEYS]
    p2 = [d2[k].data_ptr() for k in orb.KeyframeMatcher.KF2_KEYS]

    def call(prm_=p, n1=50, a1=p1, nk=1, ks=start, a2=p2, f=F, e=E, o=(mk.data_ptr(), cnt.data_ptr())):
        return lib.jsorb_search_for_triangulation_async(matcher.handle, ctypes.byref(prm_) if prm_ is not None else None, n1, *a1, nk,
                                                        ks.ctypes.data if ks is not None else None, *a2, f.ctypes.data if f is not None else None,
                                                        e.ctypes.data if e is not None else None, *o)
    assert call() == 0
    matcher.sync()
    assert np.array_equal(mk.cpu().numpy()[:50], host_both(KF1, KF2, geom, prm)[0])
    assert call(prm_=None) == -1 and call(nk=-1) == -1 and call(nk=257) == -1 and call(ks=None) == -1 and call(f=None) == -1 and call(e=None) == -1
    assert call(n1=-1) == -1 and call(n1=1 << 18) == -1
    for j in range(7):
        assert call(a1=p1[:j] + [None] + p1[j + 1:]) == -1, j
    for j in range(8):
        assert call(a2=p2[:j] + [None] + p2[j + 1:]) == -1, j
    assert call(a1=p1[:6] + [p1[6] + 8]) == -1 and call(a2=p2[:7] + [p2[7] + 8]) == -1        # misaligned descriptors
    assert call(o=(None, cnt.data_ptr())) == -1 and call(o=(mk.data_ptr(), None)) == -1
    assert call(ks=np.array([5, 2], np.int32)) == -1 and call(ks=np.array([-1, 2], np.int32)) == -1 and call(ks=np.array([0, 1 << 18], np.int32)) == -1
    for bad in (0, 17):
        q = tri_params(orb, prm)
        q.n_levels = bad
        assert call(prm_=q) == -1
    assert b"n_levels" in lib.jsorb_keyframe_matcher_last_error(matcher.handle)
    two = np.array([30, 30, 60], np.int32)                               # offsets that do not start at 0: an empty keyframe, then the second half
    FF, EE = np.concatenate([F, F]), np.concatenate([E, E])
    assert call(nk=2, ks=two, f=FF, e=EE) == 0
    matcher.sync()
    half = {k: v[30:] for k, v in KF2.items()}
    got = mk.cpu().numpy()
    assert np.array_equal(got[50:100], host_both(KF1, half, geom, prm)[0]) and (got[:50] == -1).all() and cnt.cpu().numpy()[0] == 0
    with pytest.raises(orb.JsorbError):
        matcher.search_for_triangulation(dict(d1, node=d1["node"].long()), start, d2, F[None], E[None], p)
    with pytest.raises(orb.JsorbError):
        matcher.search_for_triangulation(d1, start, d2, F[None], E[None], orb.make_bow_params())


# ---- the C++ example through the compat shim: one keyframe against three neighbours, checked against its own sequential loop and the Python path ----
@pytest.mark.parametrize("rot", [0, 1])
def test_create_new_map_points_example(orb, configs, tmp_path, matcher, rot):
    from jetson_slam_amd import build as jb
    c = configs["c1"]
    exe = jb.build_example("create_new_map_points", str(tmp_path / "create_new_map_points"))
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    other = synth_stereo_pair(REAL_SEED + 1, c["h"], c["w"])[1]
    images = [left, right, left, other]
    g = _mk(orb, c)
    g.extract(left)
    tree = sampled_voc(frame_side(g.keypoints(), g.descriptors())["desc"])
    paths = [str(tmp_path / ("kf%d.raw" % i)) for i in range(4)]
    for img, p in zip(images, paths):
        img.tofile(p)
    vp, op = str(tmp_path / "vocabulary.bin"), str(tmp_path / "out.bin")
    with open(vp, "wb") as f:
        f.write(np.array([tree["n_nodes"], tree["depth_L"], 1], np.int32).tobytes())
        for key in ("child_start", "children", "descriptors", "word_id", "weight"):
            f.write(np.ascontiguousarray(tree[key]).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), str(rot)] + paths + [vp, op], timeout=300,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    # the same keyframes through the Python path
    sides_ = []
    for img in images:
        g.extract(img)
        kp = g.keypoints()
        s = frame_side(kp, g.descriptors())
        n = len(s["angle"])
        s.update(x=kp[:n].astype(np.float32), y=kp[n:2 * n].astype(np.float32), octave=kp[4 * n:5 * n].astype(np.int32),
                 free=(np.arange(n) % 5 != 4).astype(np.uint8), stereo=(np.arange(n) % 2).astype(np.uint8), node=both_transforms(tree, s["desc"], 1)[1])
        sides_.append(s)
    geom = geometry([0, 0, 0, 0, 0, -1, 0, 1, 0], 1e9, float(c["h"]) / 2)
    s, s2 = scale_tables(c["L"])
    prm = default_params(check_orientation=rot, n_levels=c["L"], scale_factor=s, level_sigma2=s2)
    h = check_search(orb, matcher, sides_[0], sides_[1:], [geom] * 3, prm, sync=True)
    blob = np.fromfile(op, np.int32)
    n1 = len(sides_[0]["node"])
    assert int(blob[0]) == n1 and list(blob[1:4]) == [x[1] for x in h] and h[0][1] >= 15 and h[1][1] > h[0][1]
    for k in range(3):
        assert np.array_equal(blob[4 + k * n1:4 + (k + 1) * n1], h[k][0]), k
    assert ("nmatches=%d,%d,%d" % tuple(x[1] for x in h)) in out.stdout and "host_sequential_us=" in out.stdout
