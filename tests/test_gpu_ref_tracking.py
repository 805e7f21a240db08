"""-m gpu: jsorb_local_keyframes then jsorb_local_map_points (ONE keyframe over local_point_row, the hand-over of DESIGN section 26) on every world and
frame of tests/tracking_cases.py, against what the reference's own Tracking.cpp recorded for it in tests/golden/ref_matcher_tracking.npz: the list of
local keyframes and the reference keyframe, the local map points, the points the K16 launcher was handed and left in view with the fields the
matcher then read, the frame's pointers after the call.  A world's frames go one after the other on ONE handle, graph and table - the marks persist
by frame id in the reference and are restored by k_lk_gather / k_lm_write here.  Synchronous and asynchronous form; the shipped library and the
tiny_local_kf / tiny_local_map builds.  Every comparison is np.array_equal on bit patterns.

The frame: the handle holds the extracted frame of local_map_cases.world(); a world's frame rows are padded with -1 (no map point at that keypoint)
to its keypoint count, so no world needs keypoints of its own poked in."""
import functools

import numpy as np
import pytest

import local_map_cases as lc
import tracking_cases as tc
from test_gpu_local_map import _dev, bits

pytestmark = pytest.mark.gpu
WORLDS = tc.worlds()
GOLDEN = tc.load_golden()
f32 = np.float32


@functools.lru_cache(maxsize=None)
def recorded(name):
    return tc.unpack(WORLDS[name], GOLDEN[name]["raw"]), tc.predicted(WORLDS[name])


def make_handle(orb):
    W = lc.world()
    c = W["c"]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    g.extract(W["left"])
    assert g.n_keypoints(0) == W["N"]
    return g


@pytest.fixture(scope="module")
def handle(orb):
    return make_handle(orb)


class Device:
    """a world's graph and table on the device; load(frame) writes a frame's arrays behind the same pointers"""

    def __init__(self, orb, T, N):
        G, F = T["frames"][0]["G"], T["table"]["floats"]
        self.orb, self.N, self.n_rows = orb, N, F.shape[1]
        self.graph = orb.KeyframeGraph(len(G["state"]), len(G["point_pool"]), len(G["child_pool"]))
        self.table = orb.MapPointTable(self.n_rows)
        rec = np.zeros(self.n_rows, orb.MAP_POINT_RECORD_DTYPE)
        rec["P"], rec["Pn"] = F[0:3].T, F[3:6].T
        rec["MaxDistance"], rec["invariance_maxDistance"], rec["invariance_minDistance"] = F[6], F[7], F[8]
        self.table.scatter(np.arange(self.n_rows, dtype=np.int32), rec)
        assert np.array_equal(bits(self.table.floats.cpu().numpy()[:, :self.n_rows]), bits(F))

    def load(self, fr):
        self.graph.load(**fr["G"])
        self.table.bad[:self.n_rows].copy_(_dev(fr["bad"]))
        if fr["frame_rows"] is None:
            return None
        rows = np.full(self.N, -1, np.int32)
        assert len(fr["frame_rows"]) <= self.N
        rows[:len(fr["frame_rows"])] = fr["frame_rows"]
        return _dev(rows)


def start_state(T):
    slot = np.zeros(T["kf_capacity"], np.int32)
    slot[:len(T["prev_list"])] = T["prev_list"]
    return _dev(slot), _dev(np.array([len(T["prev_list"]), T["prev_ref"]], np.int32))


def run_world(orb, g, name, sync):
    """every frame of the world on the one handle, each against the reference's record (and the yardstick's counters beside it)"""
    T = WORLDS[name]
    rec, pred = recorded(name)
    dev = Device(orb, T, g.n_keypoints(0))
    state, kc_, ec = start_state(T), T["kf_capacity"], T["entry_capacity"]
    for i, (fr, r, p) in enumerate(zip(T["frames"], rec, pred)):
        label, cam = (name, i, sync), fr["cam"]
        rows = dev.load(fr)
        lk = g.local_keyframes(dev.graph, dev.table, rows, kc_, ec, state=state, sync=sync)
        state = lk["state"]
        h = {k: v.cpu().numpy() for k, v in lk.items() if hasattr(v, "cpu")}
        n = len(r["local_kf_slot"])
        # ---- jsorb_local_keyframes against mvpLocalKeyFrames, mpReferenceKF and the rows UpdateLocalPoints walked
        assert np.array_equal(h["local_kf_slot"][:n], r["local_kf_slot"]), label
        assert h["state_io"].tolist() == [n, int(r["ref_slot"])], label
        assert np.array_equal(h["local_kf_start"], p["local_kf_start"]) and h["local_kf_start"][n] == len(p["entries"]), label
        assert h["local_point_row"].dtype == np.int32 and np.array_equal(h["local_point_row"], p["gathered"]), label
        assert np.array_equal(h["local_point_row"][:len(p["entries"])], p["entries"]) and (h["local_point_row"][len(p["entries"]):] == -1).all(), label
        assert h["counts"].tolist() == p["counts"].tolist() and h["counts"][2] == n and h["counts"][3] == int(r["ref_slot"]) and h["counts"][5:7].tolist() == [0, 0], label
        assert g.local_keyframes_stats() == p["stats"], label
        if sync:
            assert np.array_equal(lk["local_kf_slot_host"][:n], r["local_kf_slot"]) and lk["state_host"].tolist() == [n, int(r["ref_slot"])], label
            assert lk["counts_host"].tolist() == p["counts"].tolist(), label
        # ---- jsorb_local_map_points over local_point_row against mvpLocalMapPoints, the launcher's points and the fields the matcher read
        view = r["in_view"] != 0 if int(r["matcher_called"]) else np.zeros(len(r["local_point_row"]), bool)
        n_in = int(view.sum())
        assert n_in == int(r["n_to_match"])
        capacity = n_in + 2
        frustum = orb.make_frustum_params(cam["R"], cam["t"], cam["Ow"], cam["cam"], cam["bounds"], cam["n_levels"], cam["logsf"], 0.5)
        lm = g.local_map_points(dev.table, frustum, [0, ec], lk["local_point_row"], rows, capacity, sync=sync)
        o = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in lm.items()}
        n_launched = r["launch_floats"].shape[1]
        assert o["counts"].tolist() == [len(r["local_point_row"]), n_launched, n_in, n_in, 0], (label, o["counts"].tolist())
        pad = lambda v, fill=0: np.concatenate([v, np.full(capacity - n_in, fill, v.dtype)])
        assert np.array_equal(o["point_row"], pad(r["local_point_row"][view], -1)), label
        assert np.array_equal(o["in_frustum"], pad(np.ones(n_in, np.uint8))), label
        if n_in:
            assert np.array_equal(bits(o["u"]), bits(pad(r["proj_x"][view]))) and np.array_equal(bits(o["v"]), bits(pad(r["proj_y"][view]))), label
            assert np.array_equal(o["predicted_level"], pad(r["level"][view])) and np.array_equal(bits(o["view_cos"]), bits(pad(r["view_cos"][view]))), label
            # invz: the reference keeps u - mbf * invz; K16's own invz is the restated one (pinned to the PTX elsewhere)
            invz = p["k16"][0][0][p["inside"]]
            assert np.array_equal(bits(o["invz"]), bits(pad(invz))), label
            xr = (o["u"][:n_in] - (f32(cam["bf"]) * o["invz"][:n_in]).astype(f32)).astype(f32)
            assert np.array_equal(bits(xr), bits(r["proj_xr"][view])), label
        blocked = np.zeros(dev.N, np.uint8)
        blocked[:len(r["frame_after"])] = r["frame_after"] >= 0
        assert np.array_equal(o["blocked_in"], blocked), label
        stats = dict(p["lm_stats"], n_entries=ec, n_null=p["lm_stats"]["n_null"] + ec - len(p["entries"]))      # (the padding of local_point_row: NULL entries)
        assert g.local_map_stats() == stats, (label, g.local_map_stats(), stats)
        if sync:
            assert np.array_equal(o["point_row_host"], o["point_row"]) and o["counts_host"].tolist() == o["counts"].tolist(), label


@pytest.mark.parametrize("name", list(WORLDS))
def test_the_device_gives_what_the_reference_recorded(orb, handle, name):
    assert orb.local_keyframes_build_caps() == tc.kc.CAPS[0] and orb.local_map_build_caps() == lc.CHUNKS[0]
    for sync in (False, True):
        run_world(orb, handle, name, sync)


def test_the_build_with_tiny_local_keyframe_caps(orb, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_local_kf", *jb.VARIANTS["tiny_local_kf"])))
    assert orb.local_keyframes_build_caps() == tc.kc.CAPS[1]
    g = make_handle(orb)
    for name in WORLDS:
        run_world(orb, g, name, False)


def test_the_build_with_chunks_of_64_entries(orb, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_local_map", *jb.VARIANTS["tiny_local_map"])))
    assert orb.local_map_build_caps() == lc.CHUNKS[1]
    g = make_handle(orb)
    for name in WORLDS:
        run_world(orb, g, name, False)


@pytest.mark.parametrize("name", [n for n, k in tc.CHANGED_FOR_THE_REFERENCE.items() if "capacity_raised" in k])
def test_the_original_capacity_keeps_the_prefix(orb, handle, name):
    """the worlds whose capacity was raised for the reference, at the capacity the case names: a prefix of what the reference produced"""
    T = WORLDS[name]
    rec, pred = recorded(name)
    kc_, ec = T["original_capacity"]
    assert (kc_, ec) != (T["kf_capacity"], T["entry_capacity"])
    dev = Device(orb, T, handle.n_keypoints(0))
    fr, r, p = T["frames"][0], rec[0], pred[0]
    lk = handle.local_keyframes(dev.graph, dev.table, dev.load(fr), kc_, ec, state=None)
    h = {k: v.cpu().numpy() for k, v in lk.items() if hasattr(v, "cpu")}
    n = int(h["state_io"][0])
    if kc_ < int(p["stats"]["n_first"]):                                     # the first list is cut, and the expansion walks the cut list
        assert h["counts"][5] == 1 and n >= kc_ and np.array_equal(h["local_kf_slot"][:kc_], r["local_kf_slot"][:kc_])
    else:
        e = p["entries"]
        m = min(ec, len(e))
        assert h["counts"][5] == 0 and np.array_equal(h["local_kf_slot"][:n], r["local_kf_slot"]) and h["counts"][4] == len(e)
        assert h["counts"][6] == int(len(e) > ec) and np.array_equal(h["local_point_row"][:m], e[:m]) and (h["local_point_row"][m:] == -1).all()
