"""-m gpu: jsorb_search_for_initialization (k_assign_grid + k_init_candidates + k_init_resolve) and the kept initial frame on real extracted frames
against the sequential transcription of ORBmatcher::SearchForInitialization and the kernels' restatement of tests/test_search_init_host.py -
matches12, matches21, the count, prev_matched and the statistics, bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair
from test_gpu_search_local import EUROC, _dev, _mk
from test_search_init_host import (SI_CAP, default_params, f1_drawn_from, f1_from_frame, frame_from_extract, search_for_initialization,
                                   search_init_restated)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NP_MIN = 50                                      # Tracking's np_min: the fewest correspondences MonocularInitialization goes on with


def frame_of(g, c, bounds=None, image=0):
    xu, yu = g.keypoints_undistorted(image)
    return frame_from_extract(g.keypoints(image), g.descriptors(image), xu, yu, c["w"], c["h"], bounds=bounds)


def init_params(orb, F2, prm):
    return orb.make_init_params((float(F2["min_x"]), float(F2["min_y"]), float(F2["inv_w"]), float(F2["inv_h"])), window=float(prm["window"]),
                                nn_ratio=float(prm["nn_ratio"]), th_low=prm["th_low"], check_orientation=prm["check_orientation"],
                                cols=F2["cols"], rows=F2["rows"])


def host_both(F1, F2, prev, prm, cap=SI_CAP):
    """the transcription and the restatement (which must agree), as (matches12, matches21, count, prev_matched, stats, trace)"""
    ref = search_for_initialization(F1, F2, prev, prm)
    res = search_init_restated(F1, F2, prev, prm, cap=cap)
    assert np.array_equal(ref[0], res[0]) and np.array_equal(ref[1], res[1]) and ref[2] == res[2]
    assert np.array_equal(ref[3].view(np.uint32), res[3].view(np.uint32))
    assert (ref[4]["candidates"], ref[4]["displaced"], ref[4]["ind"]) == (res[4][1], res[4][3], res[4][4])
    return ref[0], ref[1], ref[2], ref[3], res[4], ref[4]


def check_raw(orb, g, F1, F2, prev, prm, cap=SI_CAP, image=0):
    """the raw-pointer entry on device tensors against both host functions; returns the host's results"""
    import torch
    pm = _dev(prev)
    m12, m21, cnt = g.search_for_initialization(_dev(F1["octave"]), _dev(F1["angle"]), _dev(F1["desc"]), pm, init_params(orb, F2, prm), image=image)
    torch.cuda.synchronize()
    h = host_both(F1, F2, prev, prm, cap)
    assert np.array_equal(m12.cpu().numpy(), h[0]) and np.array_equal(m21.cpu().numpy(), h[1]) and int(cnt.item()) == h[2]
    assert np.array_equal(pm.cpu().numpy().view(np.uint32), h[3].view(np.uint32))
    assert g.search_for_initialization_stats() == h[4]
    return h


def check_kept(orb, g, F1, F2, prev, prm, cap=SI_CAP, image=0):
    """the kept initial frame against the current extract; returns the host's results (prev_matched to feed the next call)"""
    m12, pm, cnt = g.search_initial_frame(init_params(orb, F2, prm), image=image)
    h = host_both(F1, F2, prev, prm, cap)
    assert np.array_equal(m12, h[0]) and cnt == h[2] and np.array_equal(pm.view(np.uint32), h[3].view(np.uint32))
    assert g.search_for_initialization_stats() == h[4]
    return h


# ---- the kept initial frame: left view kept, right view matched, then two more frames; the copy survives the extracts ----
@pytest.mark.parametrize("name", ["c1", "c2"])
@pytest.mark.parametrize("rot", [1, 0])
def test_kept_initial_frame_over_consecutive_frames(orb, configs, name, rot):
    c = configs[name]
    left, right = synth_stereo_pair(41, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    n1 = g.set_initial_frame()
    Fl = frame_of(g, c)
    F1, prev = f1_from_frame(Fl)
    assert n1 == len(F1["octave"]) == g.initial_frame_n() > 100
    prm = default_params(check_orientation=rot)
    g.extract(right)
    Fr = frame_of(g, c)
    h = check_kept(orb, g, F1, Fr, prev, prm)
    assert h[2] >= NP_MIN and h[4][1] > h[2]
    # the second call consumes the first one's prev_matched (the matched points moved to the right view's keypoints)
    assert not np.array_equal(h[3], prev)
    g.extract(left)
    h2 = check_kept(orb, g, F1, Fl, h[3], prm)
    assert h2[2] >= NP_MIN
    # three further extracts of other images: the kept arrays are the handle's own
    other = [synth_stereo_pair(90 + i, c["h"], c["w"])[0] for i in range(3)]
    for img in other:
        g.extract(img)
    Fo = frame_of(g, c)
    h3 = check_kept(orb, g, F1, Fo, h2[3], prm)
    g.extract(right)
    h4 = check_kept(orb, g, F1, Fr, h3[3], prm)
    assert h4[2] >= NP_MIN and g.initial_frame_n() == n1
    g.clear_initial_frame()
    assert g.initial_frame_n() == -1
    with pytest.raises(orb.JsorbError):
        g.search_initial_frame(init_params(orb, Fr, prm))


# ---- the raw-pointer entry: F1 drawn from F2's own keypoints with replacement: displaced claims and hidden candidates ----
@pytest.mark.parametrize("name", ["c1", "c2"])
@pytest.mark.parametrize("rot", [1, 0])
def test_drawn_arrays_displace_and_hide(orb, configs, name, rot):
    c = configs[name]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(41, c["h"], c["w"])[1])
    F2 = frame_of(g, c)
    F1, prev = f1_drawn_from(np.random.default_rng(1), F2, 2 * int((F2["octave"] == 0).sum()))
    h = check_raw(orb, g, F1, F2, prev, default_params(check_orientation=rot))
    tr = h[5]
    assert h[2] >= NP_MIN and tr["displaced"] > 0 and tr["hidden"] > 0 and (tr["culled"] > 0) == bool(rot), (h[2], tr)
    assert (F1["octave"] < 0).any() and (F1["octave"] > 0).any()


# ---- monocular with a camera: F2's mvKeysUn from k_undistort bin the grid and update prev_matched; kept frame and raw entry ----
def test_with_camera(orb, configs):
    c = configs["c2"]
    (fx, fy, cx, cy), dist, _ = EUROC
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    g = _mk(orb, c)
    g.set_camera(K, dist)
    left, right = synth_stereo_pair(5, c["h"], c["w"])
    b = orb.image_bounds(K, dist, c["w"], c["h"])
    bounds = (b[0], b[1], b[2], b[3])
    g.extract(left)
    g.set_initial_frame()
    Fl = frame_of(g, c, bounds=bounds)
    assert not np.array_equal(Fl["kx"], g.keypoints(0)[:len(Fl["kx"])].astype(np.float32))      # the undistorted coordinates
    F1, prev = f1_from_frame(Fl)
    g.extract(right)
    Fr = frame_of(g, c, bounds=bounds)
    h = check_kept(orb, g, F1, Fr, prev, default_params())
    assert h[2] >= NP_MIN
    D1, dprev = f1_drawn_from(np.random.default_rng(2), Fr, 1500)
    h = check_raw(orb, g, D1, Fr, dprev, default_params())
    assert h[2] >= NP_MIN and h[5]["displaced"] > 0 and h[5]["hidden"] > 0


# ---- a window that covers the whole grid: every octave-0 keypoint is a candidate of every octave-0 point ----
def test_window_over_the_whole_grid(orb, configs):
    c = configs["c1"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(41, c["h"], c["w"])[1])
    F2 = frame_of(g, c)
    F1, prev = f1_drawn_from(np.random.default_rng(3), F2, 150)
    h = check_raw(orb, g, F1, F2, prev, default_params(window=f32(1000)))
    n0 = int((F2["octave"] == 0).sum())
    assert h[4][1] >= n0 * int((F1["octave"] == 0).sum()) and h[2] > 10
    # a negative F1 octave switches the level check off: all N keypoints are its candidates, more than the list holds
    assert len(F2["kx"]) > SI_CAP and h[4][2] >= int((F1["octave"] < 0).sum()) > 0


# ---- the rotation check at its edges: four equal bins, a lone match at and below a tenth, an angle outside [0, 360), the check off ----
def test_rotation_cull_cases(orb, configs):
    from test_gpu_search_kf import constructed_on_device
    from test_search_kf_host import lattice_case
    from test_search_last_frame_host import ROTATION_CULL, rotation_cull_expected
    for name, rots in sorted(ROTATION_CULL.items()):
        F0, _, _ = lattice_case(rots)
        g, F2 = constructed_on_device(orb, configs["c1"], F0)
        n, own = len(rots), np.arange(len(rots))
        F1 = dict(octave=np.zeros(n, np.int32), angle=np.asarray(rots, np.float32), desc=F0["desc"].copy())
        prev = np.stack([F0["kx"], F0["ky"]]).astype(np.float32)
        for on in (1, 0):
            ind, kept = rotation_cull_expected(rots, on)
            h = check_raw(orb, g, F1, F2, prev, default_params(window=f32(5), check_orientation=on))
            assert np.array_equal(h[0], np.where(kept, own, -1)) and h[2] == kept.sum() and tuple(h[4][4]) == ind, (name, on)


# ---- the shared compaction at a group's width and at the list's end: 15, 16, 17 and (on the small build) cap + 1 survivors in one window, the points
# in the first and last group of a wave, the first of the next wave and the last of the block ----
@pytest.mark.parametrize("variant", [None, "tiny_init_cap"])
def test_survivor_counts_at_the_group_and_list_edges(orb, configs, monkeypatch, variant):
    from jetson_slam_amd import build as jb
    from test_gpu_search_kf import constructed_on_device
    from test_search_kf_host import COMPACTION_AT, compaction_case
    if variant:
        monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant(variant, *jb.VARIANTS[variant])))
    cap = 2 if variant else SI_CAP
    F0, Pk, _ = compaction_case()
    g, F2 = constructed_on_device(orb, configs["c1"], F0)
    u = [40.0 if i in (0, 15) else 120.0 if i == 3 else 200.0 if i == 4 else 280.0 for i in range(16)]
    v = [140.0 if i == 15 else 40.0 if i in COMPACTION_AT else 100.0 for i in range(16)]
    F1 = dict(octave=np.zeros(16, np.int32), angle=np.zeros(16, np.float32), desc=np.zeros((16, 32), np.uint8))
    h = check_raw(orb, g, F1, F2, np.array([u, v], np.float32), default_params(window=f32(5)), cap=cap)
    rounds, n_cand, n_over = h[4][:3]
    assert n_cand == sum(COMPACTION_AT.values()) and n_over == sum(k > cap for k in COMPACTION_AT.values()) == (4 if variant else 0)
    assert h[2] == 4 and sorted(np.nonzero(h[0] >= 0)[0]) == sorted(COMPACTION_AT)


# ---- the build with 2 candidates per point: most points take the resolver's rescan of the grid ----
def test_candidate_overflow_build(orb, configs, monkeypatch):
    from jetson_slam_amd import build as jb
    c = configs["c2"]
    lib = orb.load_library(jb.build_variant("tiny_init_cap", *jb.VARIANTS["tiny_init_cap"]))
    monkeypatch.setattr(orb, "_lib", lib)
    left, right = synth_stereo_pair(41, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    g.set_initial_frame()
    F1, prev = f1_from_frame(frame_of(g, c))
    g.extract(right)
    F2 = frame_of(g, c)
    h = check_kept(orb, g, F1, F2, prev, default_params(), cap=2)
    assert h[4][2] > 100 and h[2] >= NP_MIN
    D1, dprev = f1_drawn_from(np.random.default_rng(4), F2, 1200)
    h = check_raw(orb, g, D1, F2, dprev, default_params(), cap=2)
    assert h[4][2] > 100 and h[5]["displaced"] > 0 and h[5]["hidden"] > 0


# ---- image 5 of an 8-image device batch equals that image extracted alone ----
def test_batch_image_equals_single(orb, configs):
    import torch
    c = configs["c2"]
    imgs = [synth_stereo_pair(80 + i, c["h"], c["w"])[0] for i in range(8)]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=8)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], 8, keep=dev)
    g.sync()
    s = _mk(orb, c)
    s.extract(imgs[5])
    F2 = frame_of(s, c)
    assert np.array_equal(g.keypoints(5), s.keypoints(0))
    F1, prev = f1_drawn_from(np.random.default_rng(5), F2, 1000)
    h = check_raw(orb, g, F1, F2, prev, default_params(), image=5)
    check_raw(orb, s, F1, F2, prev, default_params())
    assert h[2] >= NP_MIN
    # image 2 of the batch kept as the initial frame, image 5 matched against it
    g.set_initial_frame(image=2)
    K1, kprev = f1_from_frame(frame_of(g, c, image=2))
    check_kept(orb, g, K1, F2, kprev, default_params(), image=5)


# ---- edges and validation ----
def test_edges_and_validation(orb, configs):
    import torch
    c = configs["c1"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(41, c["h"], c["w"])[1])
    F2 = frame_of(g, c)
    N = len(F2["kx"])
    prm = default_params()
    p = init_params(orb, F2, prm)
    lib = orb.load_library()
    assert lib.jsorb_search_for_initialization_stats(g.handle, None, None, None, None, None) != 0      # before any call
    F1, prev = f1_drawn_from(np.random.default_rng(6), F2, 300)
    # n1 = 0
    e = torch.empty(0, device="cuda")
    m12, m21, cnt = g.search_for_initialization(e.int(), e.float(), torch.empty((0, 32), dtype=torch.uint8, device="cuda"),
                                                torch.empty((2, 0), dtype=torch.float32, device="cuda"), p)
    assert len(m12) == 0 and len(m21) == N and (m21.cpu().numpy() == -1).all() and int(cnt.item()) == 0
    assert g.search_for_initialization_stats() == (0, 0, 0, 0, (-1, -1, -1))
    # every F1 octave > 0: nothing matches, prev_matched untouched
    high = dict(F1, octave=np.full(300, 2, np.int32))
    h = check_raw(orb, g, high, F2, prev, prm)
    assert h[2] == 0 and np.array_equal(h[3], prev)
    # far windows, NaN positions
    odd = prev.copy()
    odd[0, :10] = np.nan
    odd[1, 10:20] = f32(3e38)
    odd[0, 20:30] = f32(-1e6)
    h = check_raw(orb, g, F1, F2, odd, prm)
    assert (h[0][:30] == -1).all() and h[2] > 10
    # N = 0: a flat image has no keypoints
    flat = _mk(orb, c)
    flat.extract(np.full((c["h"], c["w"]), 128, np.uint8))
    assert flat.n_keypoints(0) == 0
    Fz = frame_of(flat, c)
    h = check_raw(orb, flat, F1, Fz, prev, prm)
    assert h[2] == 0 and np.array_equal(h[3], prev)
    assert flat.set_initial_frame() == 0
    m12, pm, n = flat.search_initial_frame(p)
    assert len(m12) == 0 and n == 0
    # validation
    ins = [_dev(F1["octave"]), _dev(F1["angle"]), _dev(F1["desc"]), _dev(prev)]
    outs = [torch.zeros(max(N, 300) + 64, dtype=torch.int32, device="cuda") for _ in range(3)]
    ip, op = [t.data_ptr() for t in ins], [t.data_ptr() for t in outs]
    call = lambda prm_, n=300, image=0, i=ip, o=op: lib.jsorb_search_for_initialization_async(g.handle, image, ctypes.byref(prm_), n, *i, *o)
    assert call(p) == 0
    assert call(p, o=[op[0], None, op[2]]) == 0                      # matches21 may be NULL
    assert call(p, n=-1) == -1 and call(p, image=3) != 0
    for j in range(4):
        assert call(p, i=ip[:j] + [None] + ip[j + 1:]) == -1, j
    assert call(p, o=[None, op[1], op[2]]) == -1 and call(p, o=[op[0], op[1], None]) == -1
    assert call(p, i=ip[:2] + [ip[2] + 8, ip[3]]) == -1              # misaligned descriptors
    for bad in (dict(cols=200, rows=100), dict(cols=0), dict(rows=-1)):
        q = init_params(orb, F2, prm)
        for k, v in bad.items():
            setattr(q, k, v)
        assert call(q) == -1, bad
    fresh = _mk(orb, c)
    assert lib.jsorb_search_for_initialization_async(fresh.handle, 0, ctypes.byref(p), 0, *([None] * 4), *op) != 0      # no extract yet
    assert lib.jsorb_init_reference_set(fresh.handle, 0) != 0 and fresh.initial_frame_n() == -1
    with pytest.raises(orb.JsorbError):
        g.search_for_initialization(_dev(F1["octave"].astype(np.int64)), ins[1], ins[2], ins[3], p)
    # the synchronous C entry: matches12 and prev_matched on the host with the count
    pm = _dev(prev)
    m12_h, prev_h, n_out = np.zeros(300, np.int32), np.zeros((2, 300), np.float32), ctypes.c_int()
    assert lib.jsorb_search_for_initialization(g.handle, 0, ctypes.byref(p), 300, ip[0], ip[1], ip[2], pm.data_ptr(), m12_h.ctypes.data,
                                               prev_h.ctypes.data, ctypes.byref(n_out)) == 0
    h = host_both(F1, F2, prev, prm)
    assert np.array_equal(m12_h, h[0]) and n_out.value == h[2] and np.array_equal(prev_h.view(np.uint32), h[3].view(np.uint32))
    assert np.array_equal(pm.cpu().numpy().view(np.uint32), h[3].view(np.uint32))


# ---- the C++ example through the compat shim gives the count the Python path gives ----
def test_search_for_initialization_example(orb, configs, tmp_path):
    from jetson_slam_amd import build as jb
    c = configs["c2"]
    exe = jb.build_example("search_for_initialization", str(tmp_path / "search_for_initialization"))
    left, right = synth_stereo_pair(91, c["h"], c["w"])
    lp, rp, op = (str(tmp_path / s) for s in ("first.raw", "second.raw", "out.bin"))
    left.tofile(lp)
    right.tofile(rp)
    subprocess.check_call([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, op], timeout=300)
    g = _mk(orb, c)
    g.extract(left)
    n1 = g.set_initial_frame()
    F1, prev = f1_from_frame(frame_of(g, c))
    g.extract(right)
    h = check_kept(orb, g, F1, frame_of(g, c), prev, default_params())
    blob = np.fromfile(op, np.int32)
    assert int(blob[1]) == n1 and int(blob[0]) == h[2] >= NP_MIN
    assert np.array_equal(blob[2:2 + n1], h[0].astype(np.int32))
    assert np.array_equal(blob[2 + n1:2 + 3 * n1].view(np.uint32), h[3].reshape(-1).view(np.uint32))
