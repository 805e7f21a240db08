"""-m gpu: jsorb_search_by_projection_kf (k_assign_grid + k_kf_candidates + k_kf_resolve) on real extracted frames and on constructed ones against
the sequential transcription of ORBmatcher::SearchByProjection(CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) and the kernels' restatement of
tests/test_search_kf_host.py - match_kp, match_dist, kp_match, the count and the statistics (rounds, candidates, overflowed points, kept bins), bit
for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_gpu_call_order as order
from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import REAL_SEED, both_transforms, default_params, sampled_voc
from test_gpu_bow import check_search, side_of
from test_gpu_call_order import world  # noqa: F401  (the module-scoped fixture)
from test_gpu_search_last_frame import last_frame_of
from test_gpu_search_local import EUROC, _dev, _mk
from test_search_kf_host import (COMPACTION_AT, camera_centre, chain_case, compaction_case, culled_keypoint_case, distance_ranges, lattice_case,
                                 make_frame, search_by_projection_kf, search_kf_restated)
from test_search_last_frame_host import ROTATION_CULL, rotation_cull_expected

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def kf_params(c, F, th, orb_dist, bounds=None, cam=None, check_orientation=1, seed=0):
    """a current pose a little off the one the points are made with (points_of): K14 lands them next to their keypoints"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 0.002, 3)
    R = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]], np.float32)
    t = rng.normal(0, 0.01, 3).astype(np.float32)
    fx, fy, cx, cy = cam if cam is not None else (f32(c["fx"]), f32(c["fx"]), f32(c["w"] / 2), f32(c["h"] / 2))
    b = bounds if bounds is not None else (f32(0), f32(c["w"]), f32(0), f32(c["h"]))
    return dict(th=f32(th), orb_dist=orb_dist, check_orientation=check_orientation, fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), min_x=f32(b[0]),
                max_x=f32(b[1]), min_y=f32(b[2]), max_y=f32(b[3]), Rcw=R, tcw=t, Ow=camera_centre(R, t), log_sf=f32(np.log(f32(1.2))))


def points_of(rng, F, prm, n, n_levels, outliers=0.3):
    """a keyframe's map points: keypoints of this frame (drawn with replacement: several points want one keypoint) back-projected through the pose of
    prm, descriptors a few bits off, distance ranges that predict the keypoint's octave +-1 (some out of range), angles offset by one rotation plus
    ~30 % outliers, some points behind the camera"""
    N = len(F["kx"])
    src = rng.integers(0, N, n)
    z = rng.uniform(1.0, 15.0, n)
    Pc = np.stack([(F["kx"][src] + rng.normal(0, 1.0, n) - prm["cx"]) * z / prm["fx"], (F["ky"][src] + rng.normal(0, 1.0, n) - prm["cy"]) * z / prm["fy"], z])
    Pw = np.linalg.solve(prm["Rcw"].astype(np.float64), Pc - prm["tcw"].astype(np.float64)[:, None]).astype(np.float32)
    Pw[:, rng.random(n) < 0.03] *= -1
    desc = F["desc"][src].copy()
    flip = rng.random((n, 32)) < 0.03
    desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    off = np.where(rng.random(n) < outliers, rng.uniform(0, 360, n), f32(12.0)).astype(np.float32)
    P = dict(Px=Pw[0].copy(), Py=Pw[1].copy(), Pz=Pw[2].copy(), angle=np.mod(F["angle"][src] + off, f32(360)).astype(np.float32), desc=desc)
    level = np.clip(F["octave"][src] + rng.integers(-1, 2, n), 0, n_levels - 1)
    P["maxd"], P["maxdi"], P["mindi"] = distance_ranges(rng, P, prm["Ow"], F["scale"], level)
    return P, src


def c_params(orb, F, prm):
    return orb.make_kf_projection_params(prm["Rcw"], prm["tcw"], (prm["fx"], prm["fy"], prm["cx"], prm["cy"]),
                                         (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]), (F["inv_w"], F["inv_h"]), float(prm["log_sf"]),
                                         th=float(prm["th"]), orb_dist=prm["orb_dist"], check_orientation=prm["check_orientation"], cols=F["cols"],
                                         rows=F["rows"], Ow=prm["Ow"])


POINT_KEYS = ("Px", "Py", "Pz", "maxd", "maxdi", "mindi", "angle", "desc")


def run_device(orb, g, F, P, prm, image=0):
    import torch
    blocked = None if F["blocked"] is None else _dev(np.asarray(F["blocked"], np.uint8))
    mk, md, km, cnt = g.search_by_projection_kf(*[_dev(P[k]) for k in POINT_KEYS], c_params(orb, F, prm), blocked=blocked, image=image)
    torch.cuda.synchronize()
    return mk.cpu().numpy(), md.cpu().numpy(), km.cpu().numpy(), int(cnt.cpu().numpy()[0])


def check(po, orb, g, F, P, prm, image=0):
    """the device against the transcription and the restatement, statistics included; returns (match_kp, kp_match, count, (rounds, candidates, overflow, ind))"""
    m, d, km, cnt = run_device(orb, g, F, P, prm, image)
    ref = search_by_projection_kf(po, F, P, prm)
    res = search_kf_restated(po, F, P, prm, cap=orb.search_kf_build_caps()[0])
    for r in (ref, res):
        assert np.array_equal(m, r[0]) and np.array_equal(d, r[1]) and np.array_equal(km, r[2]) and cnt == r[3], (cnt, r[3])
    st = g.search_by_projection_kf_stats()
    assert st == (res[6], res[4], res[7], tuple(res[5])) and st[1] == ref[4] and st[3] == tuple(ref[5]), (st, res[4:], ref[4:])
    return m, km, cnt, st


def poke_keypoints(orb, g, kx, ky, octave, angle, desc, image=0):
    """overwrite the handle's extract result on the device with a constructed frame of the same keypoint count: x, y (SoA rows 0, 1), angle (row 3,
    float bits), octave (row 4) and the descriptors"""
    lib = orb.load_library()
    N = g.n_keypoints(image)
    assert len(kx) == len(ky) == len(octave) == len(angle) == len(desc) == N
    kp, dp = lib.jsorb_keypoints_device(g.handle, image), lib.jsorb_descriptors_device(g.handle, image)
    rows = {0: np.asarray(kx, np.int32), 1: np.asarray(ky, np.int32), 3: np.asarray(angle, np.float32), 4: np.asarray(octave, np.int32)}
    for r, a in rows.items():
        a = np.ascontiguousarray(a)
        assert lib.jsorb_mem_h2d(ctypes.c_void_p(kp + 4 * r * N), ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0
    d = np.ascontiguousarray(desc, np.uint8)
    assert lib.jsorb_mem_h2d(ctypes.c_void_p(dp), ctypes.c_void_p(d.ctypes.data), ctypes.c_size_t(d.nbytes)) == 0
    lib.jsorb_mem_device_sync()


def constructed_on_device(orb, c, F0, seed=2):
    """a handle whose first keypoints are the constructed frame F0 (integer coordinates); the rest lie in a far corner on an octave no point predicts"""
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(seed, c["h"], c["w"])[0])
    N, n0 = g.n_keypoints(0), len(F0["kx"])
    assert N > n0
    pad = N - n0
    kx = np.concatenate([F0["kx"], np.full(pad, c["w"] - 3.0)]).astype(np.float32)
    ky = np.concatenate([F0["ky"], np.full(pad, c["h"] - 3.0)]).astype(np.float32)
    octave = np.concatenate([F0["octave"], np.full(pad, 2)])
    angle = np.concatenate([F0["angle"], np.zeros(pad, np.float32)])
    desc = np.concatenate([F0["desc"], np.full((pad, 32), 255, np.uint8)])
    assert (kx == np.round(kx)).all() and (ky == np.round(ky)).all()
    poke_keypoints(orb, g, kx, ky, octave, angle, desc)
    return g, make_frame(kx, ky, octave, angle, desc, n_levels=c["L"], W=c["w"], H=c["h"])


# ---- stereo C1 / C2 frames: th 10 / ORBdist 100, then th 3 / 64 with the first pass's matches as blocked_in ----
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_extracted_frames_match_the_reference(po, orb, configs, name):
    c = configs[name]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(11, c["h"], c["w"])[0])
    F = dict(last_frame_of(g, c), blocked=None)
    rng = np.random.default_rng(3)
    prm = kf_params(c, F, 10, 100, seed=1)
    P, src = points_of(rng, F, prm, 1000 if name == "c2" else 400, c["L"])
    P["desc"][1::50] = P["desc"][0::50][:len(P["desc"][1::50])]              # identical descriptors: exact-tie distances
    m, km, cnt, (rounds, n_cand, n_over, ind) = check(po, orb, g, F, P, prm)
    assert cnt > len(m) // 4 and n_cand > 2 * cnt and rounds >= 3 and ind[0] >= 0
    assert (m >= 0).sum() > cnt                                              # something was culled
    # :2075-2079: every map point of the frame is in sFound and on a keypoint; the others again in the narrow window
    left = np.ones(len(m), bool)
    left[km[km >= 0]] = False
    P2 = {k: v[left] for k, v in P.items()}
    F2 = dict(F, blocked=(km >= 0).astype(np.uint8))
    m2, km2, cnt2, st2 = check(po, orb, g, F2, P2, dict(prm, th=f32(3), orb_dist=64))
    assert left.sum() > 50 and not (km2[km >= 0] >= 0).any()                # no blocked keypoint is matched again
    assert st2[1] > 0


# ---- monocular with a camera: mvKeysUn from k_undistort is what the grid bins and the window tests ----
def test_monocular_with_camera(po, orb, configs):
    c = configs["c2"]
    (fx, fy, cx, cy), dist, _ = EUROC
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    g = _mk(orb, c)
    g.set_camera(K, dist)
    g.extract(synth_stereo_pair(5, c["h"], c["w"])[0])
    b = orb.image_bounds(K, dist, c["w"], c["h"])
    F = dict(last_frame_of(g, c, bounds=(b[0], b[1], b[2], b[3])), blocked=None)
    assert not np.array_equal(F["kx"], g.keypoints(0)[:len(F["kx"])].astype(np.float32))
    prm = kf_params(c, F, 10, 100, bounds=b, cam=(fx, fy, cx, cy), seed=9)
    P, _ = points_of(np.random.default_rng(9), F, prm, 600, c["L"])
    _, _, cnt, _ = check(po, orb, g, F, P, prm)
    assert cnt > 100


# ---- image 5 of an 8-image device batch ----
def test_batch_image(po, orb, configs):
    import torch
    c = configs["c1"]
    imgs = [synth_stereo_pair(80 + i, c["h"], c["w"])[0] for i in range(8)]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=8)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], 8, keep=dev)
    s = _mk(orb, c)
    s.extract(imgs[5])
    F = dict(last_frame_of(s, c), blocked=None)
    prm = kf_params(c, F, 10, 100, seed=5)
    P, _ = points_of(np.random.default_rng(5), F, prm, 300, c["L"])
    _, _, cnt, _ = check(po, orb, g, F, P, prm, image=5)
    assert cnt > 50


# ---- group and block edges of 16 lanes x 16 points per workgroup ----
@pytest.mark.parametrize("n", [1, 15, 17, 257])
def test_point_counts_at_group_and_block_edges(po, orb, configs, n):
    c = configs["c1"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(12, c["h"], c["w"])[0])
    rng = np.random.default_rng(n)
    F = dict(last_frame_of(g, c), blocked=(rng.random(g.n_keypoints(0)) < 0.1).astype(np.uint8))
    prm = kf_params(c, F, 10, 100, seed=n)
    P, _ = points_of(rng, F, prm, n, c["L"], outliers=0.0)
    P["Pz"][:1] = np.abs(P["Pz"][:1])
    m, _, cnt, _ = check(po, orb, g, F, P, prm)
    assert (m >= 0).sum() >= min(n, 8) // 2 or n == 1


# ---- constructed frames written into a handle: the chain of 40 (one round per link), the hidden culled keypoint ----
def test_claim_chain_of_40_on_the_device(po, orb, configs):
    c = configs["c1"]
    F0, P, prm = chain_case(40)
    F0 = dict(F0, kx=f32(100) + np.arange(41, dtype=np.float32) % 3, ky=f32(100) + np.arange(41, dtype=np.float32) // 3)      # integer coordinates, one window
    g, F = constructed_on_device(orb, c, F0)
    prm = dict(prm, max_x=f32(c["w"]), max_y=f32(c["h"]), th=f32(20))
    m, km, cnt, (rounds, n_cand, n_over, _) = check(po, orb, g, F, P, prm)
    assert rounds >= 40 and cnt == 40 and n_cand == 40 * 41 and n_over == 0
    d = np.unpackbits(F["desc"][m], axis=1).sum(1)
    assert np.array_equal(d, np.arange(40))                                  # point i ends on the keypoint at distance i


def test_culled_keypoint_stays_hidden_on_the_device(po, orb, configs):
    c = configs["c1"]
    F0, P, prm = culled_keypoint_case()
    g, F = constructed_on_device(orb, c, F0)
    prm = dict(prm, max_x=f32(c["w"]), max_y=f32(c["h"]))
    m, km, cnt, (_, _, _, ind) = check(po, orb, g, F, P, prm)
    assert m[12] == 12 and m[13] == 13 and km[12] == -1 and cnt == 13 and ind == (0, -1, -1)


# ---- the rotation check at its edges: four equal bins, a lone match at and below a tenth, an angle outside [0, 360), the check off ----
def test_rotation_cull_cases(po, orb, configs):
    c = configs["c1"]
    for name, rots in sorted(ROTATION_CULL.items()):
        F0, P, prm = lattice_case(rots)
        g, F = constructed_on_device(orb, c, F0)
        n, own = len(rots), np.arange(len(rots))
        for on in (1, 0):
            ind, kept = rotation_cull_expected(rots, on)
            m, km, cnt, st = check(po, orb, g, F, P, dict(prm, max_x=f32(c["w"]), max_y=f32(c["h"]), check_orientation=on))
            assert np.array_equal(m, own) and np.array_equal(km[:n], np.where(kept, own, -1)) and (km[n:] == -1).all(), (name, on)
            assert cnt == kept.sum() and st[3] == ind, (name, on)


# ---- the shared compaction at a group's width and at the list's end: 15, 16, 17 and (on the small build) cap + 1 survivors in one window, the points
# in the first and last group of a wave, the first of the next wave and the last of the block ----
@pytest.mark.parametrize("variant", [None, "tiny_kf_cap"])
def test_survivor_counts_at_the_group_and_list_edges(po, orb, configs, monkeypatch, variant):
    from jetson_slam_amd import build as jb
    if variant:
        monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant(variant, *jb.VARIANTS[variant])))
    cap = orb.search_kf_build_caps()[0]
    assert cap == (2 if variant else 128)
    F0, P, prm = compaction_case()
    g, F = constructed_on_device(orb, configs["c1"], F0)
    m, km, cnt, (rounds, n_cand, n_over, _) = check(po, orb, g, F, P, dict(prm, max_x=f32(configs["c1"]["w"]), max_y=f32(configs["c1"]["h"])))
    assert n_cand == sum(COMPACTION_AT.values()) and n_over == sum(v > cap for v in COMPACTION_AT.values()) == (4 if variant else 0)
    assert cnt == 4 and sorted(np.nonzero(m >= 0)[0]) == sorted(COMPACTION_AT)


# ---- a 1 x 1 grid and a window over the whole image: one point sees every keypoint (more than the shipped list holds: the resolver walks again) ----
def test_one_cell_grid_and_a_window_over_everything(po, orb, configs):
    c = configs["c2"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(14, c["h"], c["w"])[0])
    F = dict(last_frame_of(g, c), blocked=None)
    F = dict(F, cols=1, rows=1, inv_w=f32(1) / f32(c["w"]), inv_h=f32(1) / f32(c["h"]))
    from test_search_local_host import build_grid
    F["grid"], F["start"], F["items"] = build_grid(F["kx"], F["ky"], F["min_x"], F["min_y"], F["inv_w"], F["inv_h"], 1, 1)
    prm = kf_params(c, F, 1000, 100, seed=14)
    P, _ = points_of(np.random.default_rng(14), F, prm, 12, c["L"], outliers=0.0)
    P["maxdi"][:] = f32(1e30)
    P["mindi"][:] = f32(0)
    m, _, cnt, (rounds, n_cand, n_over, _) = check(po, orb, g, F, P, prm)
    N = len(F["kx"])
    cap = orb.search_kf_build_caps()[0]
    assert N > cap and n_over >= 10 and n_cand > n_over * cap and cnt > 3      # nearly every point sees more keypoints than the list holds


# ---- the tiny_kf_cap build: 2 keys per point (most points overflow), claims in LDS up to 64 keypoints (an ordinary frame's live in global memory) ----
def test_tiny_caps_take_the_rescan_and_the_global_claims(po, orb, configs, monkeypatch):
    from jetson_slam_amd import build as jb
    lib = orb.load_library(jb.build_variant("tiny_kf_cap", *jb.VARIANTS["tiny_kf_cap"]))
    monkeypatch.setattr(orb, "_lib", lib)
    assert orb.search_kf_build_caps() == (2, 64)
    c = configs["c1"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(11, c["h"], c["w"])[0])
    N = g.n_keypoints(0)
    assert N > 64                                                            # claim[] is kp_match in global memory
    rng = np.random.default_rng(21)
    F = dict(last_frame_of(g, c), blocked=(rng.random(N) < 0.05).astype(np.uint8))
    prm = kf_params(c, F, 10, 100, seed=21)
    P, _ = points_of(rng, F, prm, 400, c["L"])
    m, _, cnt, (rounds, n_cand, n_over, _) = check(po, orb, g, F, P, prm)
    assert cnt > 100 and n_over > len(P["Px"]) // 2 and rounds >= 3
    # the chain on the same build: every point's list overflows, 40 rounds of walking the window again
    F0, Pc, prmc = chain_case(40)
    F0 = dict(F0, kx=f32(100) + np.arange(41, dtype=np.float32) % 3, ky=f32(100) + np.arange(41, dtype=np.float32) // 3)
    g2, F2 = constructed_on_device(orb, c, F0)
    _, _, cnt2, (rounds2, _, n_over2, _) = check(po, orb, g2, F2, Pc, dict(prmc, max_x=f32(c["w"]), max_y=f32(c["h"]), th=f32(20)))
    assert cnt2 == 40 and rounds2 >= 40 and n_over2 == 40


# ---- empty sides, no blocked array, everything blocked, no orientation check, validation, kernel timing ----
def test_edges_and_validation(po, orb, configs):
    import torch
    c = configs["c1"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(71, c["h"], c["w"])[0])
    N = g.n_keypoints(0)
    F = dict(last_frame_of(g, c), blocked=None)
    rng = np.random.default_rng(71)
    prm = kf_params(c, F, 10, 100, seed=71)
    P, _ = points_of(rng, F, prm, 300, c["L"])
    P["Px"][20:25] = np.nan
    P["Pz"][25:30] = f32(3e38)
    P["maxd"][30:35] = np.inf
    P["maxd"][35:40] = np.nan
    P["maxdi"][40:45] = np.nan
    _, _, cnt, _ = check(po, orb, g, F, P, prm)                              # blocked_in = NULL
    assert cnt > 50
    _, _, _, st = check(po, orb, g, F, P, dict(prm, check_orientation=0))
    assert st[3] == (-1, -1, -1)
    m, km, cnt, st = check(po, orb, g, dict(F, blocked=np.ones(N, np.uint8)), P, prm)
    assert cnt == 0 and (m == -1).all() and (km == -1).all() and st[1] == 0
    # n_points = 0
    p = c_params(orb, F, prm)
    e = torch.empty(0, device="cuda")
    mk, md, km, cnt = g.search_by_projection_kf(*[e.float()] * 7, torch.empty((0, 32), dtype=torch.uint8, device="cuda"), p)
    assert len(mk) == 0 and int(cnt.item()) == 0 and len(km) == N and (km.cpu().numpy() == -1).all()
    assert g.search_by_projection_kf_stats() == (1, 0, 0, (-1, -1, -1))
    km_host, n_host = g.search_by_projection_kf_host(*[_dev(P[k]) for k in POINT_KEYS], p)
    ref = search_by_projection_kf(po, F, P, prm)
    assert np.array_equal(km_host, ref[2]) and n_host == ref[3]
    # N = 0: an image without a corner
    blank = _mk(orb, c)
    blank.extract(np.full((c["h"], c["w"]), 128, np.uint8))
    assert blank.n_keypoints(0) == 0
    mk, md, km, cnt = blank.search_by_projection_kf(*[_dev(P[k]) for k in POINT_KEYS], p)
    assert int(cnt.item()) == 0 and len(km) == 0 and (mk.cpu().numpy() == -1).all()
    # validation
    lib = orb.load_library()
    fv = torch.zeros(2, dtype=torch.float32, device="cuda")
    desc = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    o = [torch.zeros(N + 64, dtype=torch.int32, device="cuda") for _ in range(4)]
    outs = [t.data_ptr() for t in o]
    ins = [fv.data_ptr()] * 7 + [desc.data_ptr(), None]
    call = lambda prm_, n=2, image=0, i=ins, out=outs: lib.jsorb_search_by_projection_kf_async(g.handle, image, ctypes.byref(prm_), n, *i, *out)
    assert call(p) == 0
    assert call(p, n=-1) == -1
    assert call(p, image=3) != 0
    for j in range(8):                                                       # NULL arrays
        assert call(p, i=ins[:j] + [None] + ins[j + 1:]) == -1, j
    for j in range(4):
        assert call(p, out=outs[:j] + [None] + outs[j + 1:]) == -1, j
    assert call(p, i=ins[:7] + [desc.data_ptr() + 8, None]) == -1           # misaligned descriptors
    for bad in (dict(cols=200, rows=100), dict(cols=0), dict(rows=-1)):
        q = c_params(orb, F, prm)
        for k, v in bad.items():
            setattr(q, k, v)
        assert call(q) == -1, bad
    fresh = _mk(orb, c)
    assert lib.jsorb_search_by_projection_kf_async(fresh.handle, 0, ctypes.byref(p), 0, *([None] * 9), *outs) != 0      # no extract yet
    assert lib.jsorb_search_by_projection_kf_stats(fresh.handle, None, None, None, None) != 0
    with pytest.raises(orb.JsorbError):
        g.search_by_projection_kf(*[_dev(P[k].astype(np.float64)) if k == "maxd" else _dev(P[k]) for k in POINT_KEYS], p)
    g.enable_kernel_timing(True)
    g.reset_kernel_timing()
    run_device(orb, g, F, P, prm)
    t = g.search_by_projection_kf_kernel_times()
    assert all(t[k][1] == 1 and t[k][0] > 0 for k in ("k_assign_grid", "k_kf_candidates", "k_kf_resolve"))


# ---- the call followed, with no host wait, by a multi-lane batch on a handle with its own stream: tests/test_gpu_call_order.py's sequence ----
class KfProjection:
    """jsorb_search_by_projection_kf_async as a reader of tests/test_gpu_call_order.py"""

    def __init__(self, W, s, i):
        import torch
        self.W, self.s, self.i = W, s, i
        F = self.F = dict(W.frames[s, i]["last"], blocked=None)
        self.prm = kf_params(order.C, F, 10, 100, seed=5)
        self.P = W.memo(("kf_P", s, i), lambda: points_of(np.random.default_rng(6), F, self.prm, order.N_POINTS, order.C["L"])[0])
        self.inp = [_dev(self.P[k]) for k in POINT_KEYS]
        N = len(F["kx"])
        full = lambda n, v: torch.full((n,), v, dtype=torch.int32, device="cuda")
        self.out = [full(order.N_POINTS, -1), full(order.N_POINTS, -1), full(N, -1), full(1, 0)]
        self.p = c_params(W.orb, F, self.prm)

    def enqueue(self, g, image):
        rc = g._lib.jsorb_search_by_projection_kf_async(g.handle, image, ctypes.byref(self.p), order.N_POINTS, *[t.data_ptr() for t in self.inp], None,
                                                        *[t.data_ptr() for t in self.out])
        assert rc == 0, (rc, g._lib.jsorb_last_error(g.handle))

    def check(self, g=None):
        ref = self.W.memo(("kf_ref", self.s, self.i), lambda: search_by_projection_kf(self.W.po, self.F, self.P, self.prm))
        m, d, km, cnt = (t.cpu().numpy() for t in self.out)
        assert int(cnt[0]) == ref[3] > 0, ("KfProjection", self.s, self.i, int(cnt[0]), ref[3])
        assert np.array_equal(m, ref[0]) and np.array_equal(d, ref[1]) and np.array_equal(km, ref[2]), ("KfProjection", self.s, self.i)


@pytest.mark.parametrize("lanes,first", [(4, "batch_last"), (2, "single")])
def test_reader_is_ordered_before_the_next_batch(world, monkeypatch, lanes, first):  # noqa: F811
    monkeypatch.setitem(order.READERS, "kf_projection", KfProjection)
    order.run_sequence(world, monkeypatch, "kf_projection", lanes, first, "own")


# ---- the C++ example through the compat shim gives the counts the Python path gives ----
def test_relocalization_example(po, orb, configs, tmp_path):
    from jetson_slam_amd import build as jb
    c = configs["c1"]
    exe = jb.build_example("relocalization", str(tmp_path / "relocalization"))
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    KF = side_of(g)
    kf_frame = last_frame_of(g, c)
    tree = sampled_voc(KF["desc"])
    n_kf = len(KF["angle"])
    # the keyframe's map points: its keypoints at the depth of the pair's disparity d(y) = 6 + floor(24 y / H) (jetson_slam_amd/synth.py), in the
    # keyframe's camera; the current (right) camera sits one baseline to the right, so a point projects onto its keypoint in the right image
    fx, cx, cy = float(c["fx"]), c["w"] / 2.0, c["h"] / 2.0
    z = c["bf"] / (6 + (24 * kf_frame["ky"].astype(np.int64)) // c["h"])
    Pw = np.stack([(kf_frame["kx"] - cx) * z / fx, (kf_frame["ky"] - cy) * z / fx, z]).astype(np.float32)
    F_scale = kf_frame["scale"]
    prm = dict(th=f32(10), orb_dist=100, check_orientation=1, fx=f32(fx), fy=f32(fx), cx=f32(cx), cy=f32(cy), min_x=f32(0), max_x=f32(c["w"]), min_y=f32(0),
               max_y=f32(c["h"]), Rcw=np.eye(3, dtype=np.float32), tcw=np.array([-c["bf"] / fx, 0, 0], np.float32), log_sf=f32(np.log(f32(1.2))))
    prm["Ow"] = camera_centre(prm["Rcw"], prm["tcw"])
    Pd = dict(Px=Pw[0], Py=Pw[1], Pz=Pw[2])
    maxd, maxdi, mindi = distance_ranges(np.random.default_rng(1), Pd, prm["Ow"], F_scale, kf_frame["octave"])
    lp, rp, vp, pp, op = (str(tmp_path / s) for s in ("keyframe.raw", "current.raw", "vocabulary.bin", "points.bin", "out.bin"))
    left.tofile(lp)
    right.tofile(rp)
    with open(vp, "wb") as f:
        f.write(np.array([tree["n_nodes"], tree["depth_L"], 1], np.int32).tobytes())
        for key in ("child_start", "children", "descriptors", "word_id", "weight"):
            f.write(np.ascontiguousarray(tree[key]).tobytes())
    with open(pp, "wb") as f:
        f.write(np.int32(n_kf).tobytes())
        for a in (Pw[0], Pw[1], Pw[2], maxd, maxdi, mindi, prm["Rcw"].ravel(), prm["tcw"], prm["Ow"], np.array([fx, fx, cx, cy, prm["log_sf"]], np.float32)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, vp, pp, op], timeout=300, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    # the Python path: SearchByBoW -> inliers as blocked_in -> the matcher at (10, 100) -> again at (3, 64)
    KF["node"] = both_transforms(tree, KF["desc"], 1)[1]
    KF["valid"] = np.ones(n_kf, np.uint8)
    g.extract(right)
    R = side_of(g)
    R["node"] = both_transforms(tree, R["desc"], 1)[1]
    match_kf, n_bow, _ = check_search(orb, g, [KF], R, default_params(nn_ratio=f32(0.75)))[0]
    F = dict(last_frame_of(g, c), blocked=None)
    N = len(F["kx"])
    mvp = np.full(N, -1, np.int64)
    hit = np.nonzero(match_kf >= 0)[0][::2]
    mvp[hit] = match_kf[hit]
    counts = []
    for th, orb_dist in ((10, 100), (3, 64)):
        slot = np.setdiff1d(np.arange(n_kf), mvp[mvp >= 0])
        P = dict(Px=Pw[0][slot], Py=Pw[1][slot], Pz=Pw[2][slot], maxd=maxd[slot], maxdi=maxdi[slot], mindi=mindi[slot], angle=KF["angle"][slot],
                 desc=KF["desc"][slot])
        _, km, cnt, _ = check(po, orb, g, dict(F, blocked=(mvp >= 0).astype(np.uint8)), P, dict(prm, th=f32(th), orb_dist=orb_dist))
        mvp[km >= 0] = slot[km[km >= 0]]
        counts.append(cnt)
    blob = np.fromfile(op, np.int32)
    assert blob[:5].tolist() == [n_bow, len(hit), counts[0], counts[1], N] and np.array_equal(blob[5:5 + N], mvp.astype(np.int32))
    assert ("bow=%d inliers=%d first=%d second=%d" % (n_bow, len(hit), counts[0], counts[1])) in out.stdout
    assert n_bow >= 15 and counts[0] > 10
