"""-m gpu: jsorb_local_map_points (k_lm_marks, k_lm_list, k_lm_scan, k_lm_write) on the cases of tests/local_map_cases.py against the composition it
replaces - the restated lists, a numpy gather, the existing jsorb_is_in_frustum on the gathered arrays, the points inside compacted - and its
outputs through the existing matcher.  Every comparison is np.array_equal on bit patterns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import local_map_cases as lc
from frame_builders import frame_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FLOATS = ("u", "v", "invz", "view_cos")
_composed = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def make_frame(orb):
    """the world's stereo frame on the device, through the library `orb` currently holds: (left handle, right handle, uRight tensor)"""
    import torch
    W = lc.world()
    c = W["c"]
    gl, gr = (orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"]) for _ in range(2))
    gl.extract(W["left"])
    gr.extract(W["right"])
    assert np.array_equal(gl.keypoints(0), W["kp"])                      # the oracle's frame, bit for bit: the cases' frame rows fit it
    u, _, _ = orb.compute_stereo_matches(gl, gr, c["bf"] / c["fx"], c["bf"])
    assert np.array_equal(u.view(np.uint32), W["u_right"].view(np.uint32))
    ur = torch.empty(len(u), dtype=torch.float32, device="cuda")
    assert orb.load_library().jsorb_mem_d2d(ctypes.c_void_p(ur.data_ptr()), ctypes.c_void_p(orb.load_library().jsorb_stereo_uright_device(gl.handle, 0)),
                                            ctypes.c_size_t(4 * len(u))) == 0
    return gl, gr, ur


def make_table(orb, W=None):
    """the world's table on the device: every row through scatter, the descriptors copied"""
    W = W or lc.world()
    t = orb.MapPointTable(lc.N_ROWS)
    rec = np.zeros(lc.N_ROWS, orb.MAP_POINT_RECORD_DTYPE)
    F = W["floats"]
    rec["P"], rec["Pn"] = F[0:3].T, F[3:6].T
    rec["MaxDistance"], rec["invariance_maxDistance"], rec["invariance_minDistance"], rec["bad"] = F[6], F[7], F[8], W["bad"]
    t.scatter(np.arange(lc.N_ROWS, dtype=np.int32), rec)
    t.desc.copy_(_dev(W["desc"]))
    return t


def frustum_of(orb, W):
    return orb.make_frustum_params(W["R"], W["t"], W["Ow"], W["cam"], W["bounds"], W["n_levels"], W["logsf"], W["vca"])


@pytest.fixture(scope="module")
def env(orb):
    gl, gr, ur = make_frame(orb)
    return dict(gl=gl, gr=gr, ur=ur, table=make_table(orb), frustum=frustum_of(orb, lc.world()))


def composed(orb, name, W=None, case=None):
    """The composition the call replaces, once per case: the restated lists, the gather, the existing jsorb_is_in_frustum on the device."""
    import torch
    if name in _composed and W is None:
        return _composed[name]
    key, W, c = W is None, W or lc.world(), case or lc.build_case(name)
    a = lc.update_local_points_restated(W["bad"], c["keyframes"], c["frame_rows"])
    rows = a["map_points"]
    n = len(rows)
    G = _dev(W["floats"][:, rows]) if n else torch.zeros((9, 1), dtype=torch.float32, device="cuda")
    R, t, Ow = _dev(W["R"].ravel()), _dev(W["t"]), _dev(W["Ow"])
    zz, uu, vv, vc = (torch.full((max(n, 1),), -7.0, dtype=torch.float32, device="cuda") for _ in range(4))
    lvl = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    inside = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert orb.load_library().jsorb_is_in_frustum(None, n, *[G[i].data_ptr() for i in range(9)], R.data_ptr(), t.data_ptr(), Ow.data_ptr(), *W["cam"], *W["bounds"],
                                                  W["n_levels"], W["logsf"], W["vca"], zz.data_ptr(), uu.data_ptr(), vv.data_ptr(), lvl.data_ptr(), vc.data_ptr(),
                                                  inside.data_ptr()) == 0
    full = dict(u=uu[:n], v=vv[:n], invz=zz[:n], predicted_level=lvl[:n], view_cos=vc[:n], in_frustum=inside[:n], mp_descriptors=_dev(W["desc"][rows].reshape(n, 32)))
    ins = inside[:n].cpu().numpy() == 1
    k16 = tuple(x[:n].cpu().numpy()[ins] for x in (uu, vv, zz, lvl, vc))
    r = dict(lists=a, rows_inside=rows[ins], inside=ins, k16=k16, full=full, case=c)
    if key:
        _composed[name] = r
    return r


def run_new(g, table, frustum, c, capacity, **kw):
    fr = None if c["frame_rows"] is None else _dev(c["frame_rows"])
    out = g.local_map_points(table, frustum, c["kf_start"], _dev(c["entries"]), fr, capacity, **kw)
    return out, {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def check_case(orb, g, table, frustum, name, W=None, case=None, sync_at=None):
    ref = composed(orb, name, W, case)
    W = W or lc.world()
    a, c, n_in = ref["lists"], ref["case"], len(ref["rows_inside"])
    assert n_in > 0 or name in lc.EMPTY
    for capacity in lc.capacities(n_in):
        _, h = run_new(g, table, frustum, c, capacity, sync=capacity == sync_at)
        exp = lc.expected_outputs(ref["rows_inside"], ref["k16"], W["desc"], capacity)
        for k, v in exp.items():
            assert h[k].dtype == v.dtype and np.array_equal(bits(h[k]), bits(v)), (name, capacity, k)
        assert np.array_equal(h["blocked_in"], a["blocked_in"] if c["frame_rows"] is not None else np.zeros(W["N"], np.uint8)), (name, capacity)
        counts = [len(a["local"]), len(a["map_points"]), n_in, min(n_in, capacity), int(n_in > capacity)]
        assert h["counts"].tolist() == counts, (name, capacity, h["counts"].tolist(), counts)
        assert g.local_map_stats() == a["stats"], (name, capacity)
        if capacity == sync_at:
            assert np.array_equal(h["point_row_host"], exp["point_row"]) and h["counts_host"].tolist() == counts
    return n_in


# ---- composition: every case, at capacities one short of nToMatch (a prefix is kept), exact, one more (a padding slot) and 0 ----
@pytest.mark.parametrize("name", list(lc.CASES))
def test_the_call_equals_the_composition_it_replaces(orb, env, name):
    ref = composed(orb, name)
    n_in = len(ref["rows_inside"])
    if name not in lc.EMPTY:
        assert n_in >= 2 and (~ref["inside"]).any()                       # points outside the frustum were compacted away
    check_case(orb, env["gl"], env["table"], env["frustum"], name, sync_at=lc.capacities(n_in)[-1])      # (the synchronous form once per case)


# ---- the outputs through the existing matcher, against the existing path: jsorb_is_in_frustum over ALL map_points with the exact n ----
@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("th", [1.0, 5.0])
def test_the_matcher_sees_the_same_points(orb, env, th, stereo):
    W, g = lc.world(), env["gl"]
    ref = composed(orb, "six")
    c, n_in = ref["case"], len(ref["rows_inside"])
    capacity = n_in + 3
    out, h = run_new(g, env["table"], env["frustum"], c, capacity)
    F = frame_of(g, W["c"])
    grid = (0.0, 0.0, float(F["inv_w"]), float(F["inv_h"]))
    ur = env["ur"] if stereo else None
    mk, md, km, cnt = g.search_local_points(out["u"], out["v"], out["invz"], out["predicted_level"], out["view_cos"], out["in_frustum"], out["mp_descriptors"],
                                            grid, th=th, mbf=W["c"]["bf"], u_right=ur, blocked=out["blocked_in"])
    new = [x.cpu().numpy() for x in (mk, md, km, cnt)]
    o = ref["full"]
    mk, md, km, cnt = g.search_local_points(o["u"], o["v"], o["invz"], o["predicted_level"], o["view_cos"], o["in_frustum"], o["mp_descriptors"], grid, th=th,
                                            mbf=W["c"]["bf"], u_right=ur, blocked=_dev(ref["lists"]["blocked_in"]))
    old = [x.cpu().numpy() for x in (mk, md, km, cnt)]
    assert int(new[3][0]) == int(old[3][0]) > 20
    rows = ref["lists"]["map_points"]
    assert np.array_equal(np.where(new[2] >= 0, h["point_row"][np.maximum(new[2], 0)], -1), np.where(old[2] >= 0, rows[np.maximum(old[2], 0)], -1))      # kp_match, as rows
    assert np.array_equal(new[0][:n_in], old[0][ref["inside"]]) and np.array_equal(new[1][:n_in], old[1][ref["inside"]])      # match_kp[i] belongs to point_row[i]
    assert (new[0][n_in:] == -1).all() and (old[0][~ref["inside"]] == -1).all()
    assert (W["bad"][h["point_row"][:n_in]] == 0).all() and (new[0] >= 0).sum() == int(new[3][0])


# ---- the scratch is restored: another frame and other keyframes first, then the call - as on a fresh handle ----
def test_a_second_call_sees_clean_scratch(orb, env):
    from jetson_slam_amd.synth import synth_stereo_pair
    W = lc.world()
    c = W["c"]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    other, _ = synth_stereo_pair(5, c["h"], c["w"])
    g.extract(other)
    first = dict(lc.build_case("edge_1024_2049"))
    rng = np.random.default_rng(1)
    first["frame_rows"] = rng.integers(-1, lc.N_ROWS, g.n_keypoints(0)).astype(np.int32)      # marks nearly every row it names
    _, h1 = run_new(g, env["table"], env["frustum"], first, 700)
    assert h1["counts"][0] > 500 and g.local_map_stats()["n_seen"] > 50
    g.extract(W["left"])
    for name in ("six", "no_frame"):                                     # (the second of them leaves no marks of its own)
        check_case(orb, g, env["table"], env["frustum"], name)


# ---- captured once under a HIP graph, replayed on new table contents, keyframes and frame rows ----
def test_the_call_is_capturable(orb, env):
    import torch
    W = lc.world()
    c = W["c"]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    s = torch.cuda.Stream()
    g.set_stream(s.cuda_stream)
    g.extract(W["left"])
    table, frustum = make_table(orb), env["frustum"]
    case = lc.build_case("six")
    entries, frame_rows = _dev(case["entries"]), _dev(case["frame_rows"])
    capacity = 300
    out = g.local_map_points(table, frustum, case["kf_start"], entries, frame_rows, capacity)      # the scratch takes its size
    before = {k: v.cpu().numpy() for k, v in out.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.local_map_points(table, frustum, case["kf_start"], entries, frame_rows, capacity, out=out, wait=False)
    # new contents behind the same pointers: other rows bad, a moved point, the keyframes' rows reversed, the frame's marks shifted
    W2 = dict(W, bad=W["bad"].copy(), floats=W["floats"].copy())
    flip = np.arange(0, lc.N_ROWS, 7)
    W2["bad"][flip] ^= 1
    W2["floats"][2, flip] *= f32(1.01)
    rec = np.zeros(len(flip), orb.MAP_POINT_RECORD_DTYPE)
    F = W2["floats"][:, flip]
    rec["P"], rec["Pn"] = F[0:3].T, F[3:6].T
    rec["MaxDistance"], rec["invariance_maxDistance"], rec["invariance_minDistance"], rec["bad"] = F[6], F[7], F[8], W2["bad"][flip]
    table.scatter(flip.astype(np.int32), rec)
    kfs = [k[::-1].copy() for k in case["keyframes"]]
    case2 = dict(case, keyframes=kfs, entries=np.concatenate(kfs), frame_rows=np.roll(case["frame_rows"], 3))
    entries.copy_(_dev(case2["entries"]))
    frame_rows.copy_(_dev(case2["frame_rows"]))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    after = {k: v.cpu().numpy() for k, v in out.items()}
    ref = composed(orb, "six (replayed)", W2, case2)
    n_in = len(ref["rows_inside"])
    exp = lc.expected_outputs(ref["rows_inside"], ref["k16"], W2["desc"], capacity)
    for k, v in exp.items():
        assert np.array_equal(bits(after[k]), bits(v)), k
    a = ref["lists"]
    assert after["counts"].tolist() == [len(a["local"]), len(a["map_points"]), n_in, min(n_in, capacity), int(n_in > capacity)]
    assert np.array_equal(after["blocked_in"], a["blocked_in"]) and g.local_map_stats() == a["stats"]
    assert not np.array_equal(after["point_row"], before["point_row"]) and after["counts"].tolist() != before["counts"].tolist()
    graph.replay()                                                       # ... and the replay left clean scratch behind
    torch.cuda.synchronize()
    assert np.array_equal(out["point_row"].cpu().numpy(), after["point_row"]) and out["counts"].cpu().numpy().tolist() == after["counts"].tolist()


# ---- the build with chunks of 64 entries: its own chunk edges, and the larger cases across many chunks ----
def test_chunks_of_64_entries(orb, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_local_map", *jb.VARIANTS["tiny_local_map"])))
    assert orb.local_map_build_caps() == lc.CHUNKS[1]
    gl, gr, _ = make_frame(orb)
    table, frustum = make_table(orb), frustum_of(orb, lc.world())
    for name in lc.edge_cases(lc.CHUNKS[1]) + ["six", "empty_first_middle_last", "edge_1024_2049", "zero_keyframes"]:
        check_case(orb, gl, table, frustum, name)


# ---- scatter: changed rows equal, untouched rows untouched, rows outside the table skipped ----
def test_scatter_writes_the_rows_it_names(orb):
    import torch
    rng = np.random.default_rng(2)
    n = 300
    t = orb.MapPointTable(n)
    t.floats.copy_(_dev(rng.normal(size=(9, n)).astype(f32)))
    t.bad.copy_(_dev((rng.random(n) < 0.3).astype(np.uint8)))
    t.desc.copy_(_dev(rng.integers(0, 256, (n, 32), dtype=np.uint8)))
    f0, b0, d0 = t.floats.cpu().numpy(), t.bad.cpu().numpy(), t.desc.cpu().numpy()
    rows = np.array([3, 299, n, -1, 0, 5000, 150, -2 ** 31, 2 ** 31 - 1] + list(range(20, 280, 1)), np.int32)
    rec = np.zeros(len(rows), orb.MAP_POINT_RECORD_DTYPE)
    rec["P"], rec["Pn"] = rng.normal(size=(len(rows), 3)), rng.normal(size=(len(rows), 3))
    rec["MaxDistance"], rec["invariance_maxDistance"], rec["invariance_minDistance"] = (rng.normal(size=len(rows)) for _ in range(3))
    rec["bad"] = rng.integers(0, 2, len(rows))
    rec[list(rows).index(150)] = rec[list(rows[9:]).index(150) + 9]      # the one row named twice carries one record
    t.scatter(rows, rec)
    f1, b1 = t.floats.cpu().numpy(), t.bad.cpu().numpy()
    ok = (rows >= 0) & (rows < n)
    touched = np.zeros(n, bool)
    touched[rows[ok]] = True
    assert touched.sum() == 263 and (~ok).sum() == 5
    got = np.concatenate([rec["P"].T, rec["Pn"].T, rec["MaxDistance"][None], rec["invariance_maxDistance"][None], rec["invariance_minDistance"][None]]).astype(f32)
    assert np.array_equal(bits(f1[:, rows[ok]]), bits(got[:, ok])) and np.array_equal(b1[rows[ok]], rec["bad"][ok])
    assert np.array_equal(bits(f1[:, ~touched]), bits(f0[:, ~touched])) and np.array_equal(b1[~touched], b0[~touched]) and (~touched).sum() == 37
    assert np.array_equal(t.desc.cpu().numpy(), d0)                      # descriptors are not the scatter's
    t.scatter(np.zeros(0, np.int32), np.zeros(0, orb.MAP_POINT_RECORD_DTYPE))      # nothing to do
    assert np.array_equal(bits(t.floats.cpu().numpy()), bits(f1))
    lib = orb.load_library()
    assert lib.jsorb_map_points_scatter_async(None, n, *[t.floats[i].data_ptr() for i in range(9)], t.bad.data_ptr(), -1, None, None) == -1
    assert lib.jsorb_map_points_scatter_async(None, n, *[t.floats[i].data_ptr() for i in range(9)], None, 2, _dev(rows).data_ptr(), _dev(rows).data_ptr()) == -1


# ---- every refusal of the contract: the code, the text, and nothing launched ----
def test_refusals(orb, env):
    import torch
    g, lib, W = env["gl"], orb.load_library(), lc.world()
    case = lc.build_case("six")
    entries, frame_rows = _dev(case["entries"]), _dev(case["frame_rows"])
    cap = 64
    out = g.local_map_points(env["table"], env["frustum"], case["kf_start"], entries, frame_rows, cap)
    torch.cuda.synchronize()
    stats = g.local_map_stats()
    for v in out.values():
        v.fill_(77)
    torch.cuda.synchronize()
    tb, fp, ks = env["table"].struct(), env["frustum"], np.ascontiguousarray(case["kf_start"], np.int32)
    names = ("point_row", "u", "v", "invz", "predicted_level", "view_cos", "in_frustum", "mp_descriptors", "blocked_in", "counts")

    def call(table=tb, prm=fp, n_kf=len(ks) - 1, kf_start=ks, rows=entries.data_ptr(), image=0, capacity=cap, **ptr):
        p = [ptr.get(k, out[k].data_ptr()) for k in names]
        rc = lib.jsorb_local_map_points_async(g.handle, image, ctypes.byref(table) if table is not None else None, ctypes.byref(prm) if prm is not None else None, n_kf,
                                              kf_start.ctypes.data if kf_start is not None else None, rows, frame_rows.data_ptr(), capacity, *p)
        return rc, lib.jsorb_last_error(g.handle).decode()

    def table_with(**kw):
        t = env["table"].struct()
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    big = np.array([0, 1 << 24], np.int32)
    refusals = [
        (dict(table=None), "NULL table, prm or counts_dev"), (dict(prm=None), "NULL table, prm or counts_dev"), (dict(counts=None), "NULL table, prm or counts_dev"),
        (dict(kf_start=None), "NULL kf_start"), (dict(rows=None), "NULL kf_point_row"), (dict(u=None), "NULL output"), (dict(mp_descriptors=None), "NULL output"),
        (dict(point_row=None), "NULL output"), (dict(table=table_with(Pnz=None)), "NULL table array"), (dict(table=table_with(bad=None)), "NULL table array"),
        (dict(kf_start=np.array([-1, 5, 9], np.int32), n_kf=2), "kf_start must be ascending offsets"),
        (dict(kf_start=np.array([0, 9, 5], np.int32), n_kf=2), "kf_start must be ascending offsets"),
        (dict(table=table_with(desc=env["table"].desc.data_ptr() + 8)), "16-byte aligned"), (dict(mp_descriptors=out["mp_descriptors"].data_ptr() + 4), "16-byte aligned"),
        (dict(capacity=-1), "must not be negative"), (dict(n_kf=-1), "must not be negative"), (dict(table=table_with(n_rows=-1)), "must not be negative"),
        (dict(kf_start=big, n_kf=1), "more than 16777215 entries"),
    ]
    for kw, text in refusals:
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("local_map_points: ") and text in err, (kw, rc, err)
    rc, err = call(image=3)
    assert rc not in (0, -1) and "no extract result" in err
    rows_h, counts_h = np.zeros(cap, np.int32), np.zeros(5, np.int32)
    p = [out[k].data_ptr() for k in names]
    sync_args = [g.handle, 0, ctypes.byref(tb), ctypes.byref(fp), len(ks) - 1, ks.ctypes.data, entries.data_ptr(), frame_rows.data_ptr(), cap] + p
    assert lib.jsorb_local_map_points(*sync_args, rows_h.ctypes.data, None) == -1 and "NULL host output" in lib.jsorb_last_error(g.handle).decode()
    assert lib.jsorb_local_map_points(*sync_args, None, counts_h.ctypes.data) == -1
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in out.values()) and g.local_map_stats() == stats      # nothing was launched
    # E == 0 with a NULL kf_point_row, and n_keyframes == 0 with a NULL kf_start, are valid calls
    assert call(kf_start=np.array([4, 4], np.int32), n_kf=1, rows=None)[0] == 0 and call(kf_start=None, n_kf=0, rows=None)[0] == 0
    g.sync()
    assert out["counts"].cpu().numpy().tolist() == [0, 0, 0, 0, 0] and bool((out["point_row"] == -1).all()) and bool((out["in_frustum"] == 0).all())
    fresh = orb.ORBExtractor(W["c"]["h"], W["c"]["w"], 1.2, W["c"]["L"], 9, 14, 7, W["c"]["th"], None, W["c"]["tile"], W["c"]["tile"])
    with pytest.raises(orb.JsorbError):
        fresh.local_map_stats()


# ---- the C++ example through the compat shim: one TrackLocalMap step both ways, checked by the example itself ----
def test_track_local_map_example(orb, tmp_path):
    from jetson_slam_amd import build as jb
    W = lc.world()
    c, case = W["c"], lc.build_case("six")
    exe = jb.build_example("track_local_map", str(tmp_path / "track_local_map"))
    lp, rp, ip = (str(tmp_path / s) for s in ("l.raw", "r.raw", "in.bin"))
    W["left"].tofile(lp)
    W["right"].tofile(rp)
    with open(ip, "wb") as f:
        f.write(np.int32(lc.N_ROWS).tobytes() + W["floats"].tobytes() + W["desc"].tobytes() + W["bad"].tobytes())
        f.write(np.int32(len(case["kf_start"]) - 1).tobytes() + case["kf_start"].tobytes() + case["entries"].tobytes())
        f.write(np.int32(len(case["frame_rows"])).tobytes() + case["frame_rows"].tobytes())
        for a in (W["R"].ravel(), W["t"], W["Ow"], np.array(W["cam"], f32), np.array([W["logsf"], c["bf"], 1.0], f32)):
            f.write(np.ascontiguousarray(a, f32).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, ip], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.returncode, out.stdout, out.stderr)
