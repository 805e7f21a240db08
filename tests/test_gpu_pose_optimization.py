"""-m gpu: jsorb_pose_optimization (k_pose_optimize) and jsorb_apply_matches_async against tests/pose_optimization_cases.py, in the shipped build
and in tiny_pose (a workgroup of one wave, one edge per thread in registers).

What is compared, per world: counts, outlier and point_row_out EXACTLY (the worlds are conditioned on a classification margin >= 1e-4, which the
host test checks on the transcription alone, so no case and no edge is left out); pose_out within TOL = DEVICE_FACTOR x PERMUTATION_SPREAD =
64 x 1.7e-10 (max |dR| and |dt| / (1 + |t|_inf)) - the spread is the largest the TRANSCRIPTION shows under eight permutations of its edge order
(tests/test_pose_optimization_host.py measures and asserts it), the factor is there because the device differs from the transcription in its
summation tree AND in sin / cos / pow and the quaternion's rounding, not in order alone; Tcw_out within one float step of
the rounded transcription (2^-23 on R, 2^-23 max(1, |t|_inf) on t: the double spread is far below 2^-24), its last row exact; with fewer than 3
edges Tcw_out equal to Tcw_in bit for bit.  Iteration and trial counts are diagnostics and are not compared."""
import ctypes

import numpy as np
import pytest

import pose_optimization_cases as pc

pytestmark = pytest.mark.gpu
f32 = np.float32
TOL = pc.DEVICE_FACTOR * pc.PERMUTATION_SPREAD
STEP = 2.0 ** -23


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_env(orb):
    """the two frames on the device through the library `orb` currently holds: {kind: handle}"""
    env = {}
    for kind in ("main", "blank"):
        F = pc.frame(kind)
        c = F["c"]
        g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
        g.extract(F["image"])
        assert np.array_equal(g.keypoints(0), F["kp"])        # the oracle's frame, bit for bit: the worlds' rows fit it
        env[kind] = g
    return env


@pytest.fixture(scope="module")
def env(orb):
    return make_env(orb)


def table_of(orb, P, bad=None):
    t = orb.MapPointTable(len(P))
    if len(P):
        t.floats[0:3, :len(P)].copy_(_dev(np.ascontiguousarray(np.asarray(P, f32).T)))
        if bad is not None:
            t.bad[:len(P)].copy_(_dev(bad))
    return t


def params_of(orb, W):
    p = W["prm"]
    return orb.make_pose_params((p["fx"], p["fy"], p["cx"], p["cy"]), p["bf"], p["inv_level_sigma2"])


def run(orb, env, W, rows=None, Tcw=None, table=None, **kw):
    """the call on world W (rows / Tcw: several problems over it); everything back on the host"""
    g = env[W["kind"]]
    table = table or table_of(orb, W["P"], W["bad"])
    rows = W["rows"][None] if rows is None else rows
    Tcw = W["Tcw"][None] if Tcw is None else Tcw
    ur = None if W["u_right"] is None else _dev(W["u_right"])
    sync = kw.get("sync", False)
    out = g.pose_optimization(table, params_of(orb, W), _dev(np.asarray(rows, np.int32)), np.asarray(Tcw, f32) if sync else _dev(np.asarray(Tcw, f32)), ur, **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}, g


def check(h, p, W, ref, what):
    """problem p of the outputs h against the transcription's result"""
    N = W["N"]
    assert h["counts"][p].tolist() == ref["counts"].tolist(), (what, h["counts"][p].tolist(), ref["counts"].tolist())
    assert np.array_equal(h["outlier"][p].reshape(-1)[:N], ref["outlier"]), (what, int((h["outlier"][p].reshape(-1)[:N] != ref["outlier"]).sum()))
    assert np.array_equal(h["point_row_out"][p].reshape(-1)[:N], ref["row_out"]), what
    T = h["Tcw_out"][p].reshape(16)
    if ref["counts"][0] < 3:
        assert np.array_equal(T.view(np.uint32), np.asarray(W["Tcw"], f32).reshape(16).view(np.uint32)), what
        assert np.array_equal(h["pose"][p], ref["pose"]), what
        return
    dR, dt = pc.pose_difference(h["pose"][p], ref["pose"])
    print("%s: dR %.3g dt %.3g (tolerance %.3g)" % (what, dR, dt, TOL))
    assert dR <= TOL and dt <= TOL, (what, dR, dt, TOL)
    E = ref["Tcw_out"].reshape(4, 4)
    D = np.abs(T.reshape(4, 4).astype(np.float64) - E.astype(np.float64))
    assert D[:3, :3].max() <= STEP and D[:3, 3].max() <= STEP * max(1.0, float(np.abs(E[:3, 3]).max())), (what, D)
    assert np.array_equal(T[12:].view(np.uint32), np.array([0, 0, 0, 1], f32).view(np.uint32)), what


def check_world(orb, env, name, **kw):
    W, ref = pc.world(name), pc.expected(name)
    assert ref["class_margin"] >= pc.MARGIN, (name, ref["class_margin"])          # the condition on the world (held on the CPU by the host test)
    h, g = run(orb, env, W, **kw)
    check(h, 0, W, ref, name)
    s, d = g.pose_optimization_stats(), ref["diag"]
    assert (s["n_outside_rows"], s["n_mono"], s["n_stereo"]) == (d["n_outside_rows"], d["n_mono"], d["n_stereo"]), (name, s)
    return h


# ---- every named and seeded world in the shipped build, through both call forms ----
@pytest.mark.parametrize("name", pc.WORLDS)
def test_the_worlds_in_the_shipped_build(orb, env, name):
    assert orb.pose_optimization_build_caps() == (256, 4)
    a = check_world(orb, env, name)
    b = check_world(orb, env, name, sync=True)
    for k in ("Tcw_out", "pose", "outlier", "counts"):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (name, k)


# ---- the same worlds in tiny_pose: edges beyond threads x registers from 65 edges on, the wave's butterfly alone ----
def test_the_worlds_in_the_tiny_pose_build(orb, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_pose", *jb.VARIANTS["tiny_pose"])))
    assert orb.pose_optimization_build_caps() == (64, 1)
    tiny = make_env(orb)
    for name in pc.WORLDS:
        check_world(orb, tiny, name)


# ---- determinism: the same bits twice, and as problem 5 of 8 ----
def test_a_problem_does_not_depend_on_the_run_or_on_its_place_in_the_batch(orb, env):
    name = "mixed"
    W, ref = pc.world(name), pc.expected(name)
    one, _ = run(orb, env, W)
    two, _ = run(orb, env, W)
    rng = np.random.default_rng(5)
    rows, Tcw, worlds = [], [], []
    for p in range(8):
        r, T = W["rows"].copy(), W["Tcw"].copy()
        if p != 5:
            r[rng.choice(W["kps"], 20 + 10 * p, replace=False)] = -1
            T[:3, 3] += rng.normal(0, 0.02, 3).astype(f32)
        rows.append(r)
        Tcw.append(T)
        worlds.append(dict(W, rows=r, Tcw=T))
    batch, _ = run(orb, env, W, rows=np.stack(rows), Tcw=np.stack(Tcw))
    for k in ("Tcw_out", "pose", "outlier", "point_row_out", "counts"):
        bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
        assert np.array_equal(bits(one[k]), bits(two[k])), k
        assert np.array_equal(bits(one[k][0]), bits(batch[k][5])), k
    check(batch, 5, W, ref, "mixed as problem 5 of 8")
    for p in (0, 7):
        r = pc.reference(worlds[p])
        assert r["class_margin"] >= pc.MARGIN
        check(batch, p, worlds[p], r, "problem %d of 8" % p)


# ---- the asynchronous form through a captured graph (one stream), replayed on another initial pose ----
def test_the_call_is_capturable(orb):
    import torch
    W = pc.world("e257")
    F = pc.frame("main")
    c = F["c"]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    s = torch.cuda.Stream()
    g.set_stream(s.cuda_stream)
    g.extract(F["image"])
    table, prm = table_of(orb, W["P"], W["bad"]), params_of(orb, W)
    rows, Tcw, ur = _dev(W["rows"][None]), _dev(W["Tcw"][None]), _dev(W["u_right"])
    direct = g.pose_optimization(table, prm, rows, Tcw, ur)                    # the scratch takes its size
    want = {k: v.cpu().numpy() for k, v in direct.items()}
    out = {k: torch.zeros_like(v) for k, v in direct.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.pose_optimization(table, prm, rows, Tcw, ur, out=out, wait=False)
    graph.replay()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert np.array_equal(out[k].cpu().numpy().view(np.uint8), v.view(np.uint8)), k
    T2 = W["Tcw"].copy()
    T2[:3, 3] += f32(0.01)
    Tcw.copy_(_dev(T2[None]))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    again = g.pose_optimization(table, prm, rows, Tcw, ur)
    for k, v in again.items():
        assert np.array_equal(out[k].cpu().numpy().view(np.uint8), v.cpu().numpy().view(np.uint8)), k
    assert not np.array_equal(out["pose"].cpu().numpy(), want["pose"])


# ---- jsorb_apply_matches_async against numpy ----
def test_apply_matches(orb):
    import torch
    rng = np.random.default_rng(3)
    N, n = 700, 1000
    frame = rng.integers(-1, 500, N).astype(np.int32)
    kp = np.full(n, -1, np.int32)
    hit = rng.choice(n, 400, replace=False)
    kp[hit] = rng.choice(N, 400, replace=False)                   # distinct keypoints, as the matchers give them
    kp[rng.choice(np.setdiff1d(np.arange(n), hit), 30, replace=False)] = rng.choice(np.array([N, N + 5, 2 ** 31 - 1, -7]), 30)
    row = rng.integers(0, 5000, n).astype(np.int32)
    row[rng.choice(n, 100, replace=False)] = -1
    want = pc.apply_matches(frame, row, kp)
    assert (want != frame).sum() > 200
    d = _dev(frame)
    orb.apply_matches(_dev(row), _dev(kp), d)
    assert np.array_equal(d.cpu().numpy(), want)
    # nothing to do: no point, no keypoint
    e = _dev(frame)
    orb.apply_matches(_dev(row[:0]), _dev(kp[:0]), e)
    assert np.array_equal(e.cpu().numpy(), frame)
    lib = orb.load_library()
    assert lib.jsorb_apply_matches_async(None, -1, None, None, N, ctypes.c_void_p(e.data_ptr())) == -1
    assert lib.jsorb_apply_matches_async(None, 4, None, None, N, ctypes.c_void_p(e.data_ptr())) == -1
    torch.cuda.synchronize()
    assert np.array_equal(e.cpu().numpy(), frame)


# ---- local map -> search -> apply -> optimise on one small frame: the device's apply against the host's, bit for bit ----
def test_the_four_call_chain_has_no_host_hop(orb):
    import local_map_cases as lc
    from test_gpu_local_map import frustum_of, make_frame, make_table
    W = lc.world()
    c = W["c"]
    gl, gr, ur = make_frame(orb)
    table, frustum = make_table(orb), frustum_of(orb, W)
    case = lc.build_case("six")
    frame_rows = np.full(W["N"], -1, np.int32)
    capacity = 600
    lm = gl.local_map_points(table, frustum, case["kf_start"], _dev(case["entries"]), _dev(frame_rows), capacity)
    grid = (0.0, 0.0, 64.0 / c["w"], 48.0 / c["h"])
    match_kp, _, _, n = gl.search_local_points(lm["u"], lm["v"], lm["invz"], lm["predicted_level"], lm["view_cos"], lm["in_frustum"], lm["mp_descriptors"],
                                               grid, th=3.0, mbf=c["bf"], u_right=ur, blocked=lm["blocked_in"])
    assert int(n.cpu()[0]) >= 20
    on_device = _dev(frame_rows)
    orb.apply_matches(lm["point_row"], match_kp, on_device)
    on_host = pc.apply_matches(frame_rows, lm["point_row"].cpu().numpy(), match_kp.cpu().numpy())
    assert np.array_equal(on_device.cpu().numpy(), on_host) and (on_host >= 0).sum() == int(n.cpu()[0])
    scale = gl.get_scale_factors()[:c["L"]].astype(f32)
    prm = orb.make_pose_params(W["cam"], c["bf"], (f32(1.0) / (scale * scale)).astype(f32))
    Tcw = np.eye(4, dtype=f32)
    Tcw[:3, :3], Tcw[:3, 3] = W["R"], W["t"]
    a = gl.pose_optimization(table, prm, on_device, _dev(Tcw[None]), ur)
    b = gl.pose_optimization(table, prm, _dev(on_host), _dev(Tcw[None]), ur)
    assert int(a["counts"][0, 0]) == (on_host >= 0).sum() and int(a["counts"][0, 3]) == 4 and int(a["counts"][0, 2]) >= 10
    for k in a:
        assert np.array_equal(a[k].cpu().numpy().view(np.uint8), b[k].cpu().numpy().view(np.uint8)), k


# ---- argument errors: their codes, and nothing launched ----
def test_refusals(orb, env):
    import torch
    W = pc.world("e63")
    g, N = env["main"], W["N"]
    lib = orb.load_library()
    table, prm = table_of(orb, W["P"], W["bad"]), params_of(orb, W)
    rows, Tcw = _dev(W["rows"][None]), _dev(W["Tcw"][None])
    Tout = torch.full((1, 16), 7.0, dtype=torch.float32, device="cuda")
    pose = torch.full((1, 12), 7.0, dtype=torch.float64, device="cuda")
    flags = torch.full((1, N), 7, dtype=torch.uint8, device="cuda")
    rout = torch.full((1, N), 7, dtype=torch.int32, device="cuda")
    counts = torch.full((1, 4), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(h=g.handle, image=0, prm=prm, tb=None, n=1, **ptr):
        tb = tb or table.struct()
        p = dict(rows=rows.data_ptr(), ur=None, Tin=Tcw.data_ptr(), Tout=Tout.data_ptr(), pose=pose.data_ptr(), flags=flags.data_ptr(), rout=rout.data_ptr(),
                 counts=counts.data_ptr())
        p.update(ptr)
        return lib.jsorb_pose_optimization_async(h, image, None if prm is None else ctypes.byref(prm), None if tb is None else ctypes.byref(tb), n, p["rows"],
                                                 p["ur"], p["Tin"], p["Tout"], p["pose"], p["flags"], p["rout"], p["counts"])

    def table_with(**kw):
        t = table.struct()
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    INVALID, UNSUPPORTED, STATE = -1, -3, -4
    assert call(h=None) == INVALID
    assert call(prm=None) == INVALID
    assert lib.jsorb_pose_optimization_async(g.handle, 0, ctypes.byref(prm), None, 1, rows.data_ptr(), None, Tcw.data_ptr(), Tout.data_ptr(), pose.data_ptr(),
                                             flags.data_ptr(), rout.data_ptr(), counts.data_ptr()) == INVALID
    assert call(n=-1) == INVALID
    assert call(tb=table_with(n_rows=-1)) == INVALID
    assert call(tb=table_with(Px=None)) == INVALID
    assert call(tb=table_with(desc=table.desc.data_ptr() + 4)) == INVALID
    for k in ("rows", "Tin", "Tout", "flags", "counts"):
        assert call(**{k: None}) == INVALID, k
    assert call(pose=pose.data_ptr() + 4) == INVALID
    assert call(image=1) == STATE and call(image=-1) == STATE
    c = pc.frame("main")["c"]
    fresh = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    assert call(h=fresh.handle) == STATE
    stats = np.zeros(8, np.int32)
    assert lib.jsorb_pose_optimization_stats(fresh.handle, stats.ctypes.data) == STATE
    assert lib.jsorb_pose_optimization_stats(g.handle, None) == INVALID
    assert call(n=2 ** 31 // N + 1) == UNSUPPORTED
    g.sync()
    torch.cuda.synchronize()
    for t in (Tout, pose, flags, rout, counts):
        assert bool((t == 7).all())                           # nothing was launched
    assert call() == 0
    g.sync()
    assert counts.cpu().numpy()[0].tolist() == pc.expected("e63")["counts"].tolist()


# ---- the C++ example through the compat shim: one TrackLocalMap tail with no host hop, checked by the example against its own C++ double loop ----
def test_pose_optimization_example(orb, tmp_path):
    import subprocess
    import local_map_cases as lc
    from jetson_slam_amd import build as jb
    W = lc.world()
    c, case = W["c"], lc.build_case("six")
    exe = jb.build_example("pose_optimization", str(tmp_path / "pose_optimization"))
    lp, rp, ip = (str(tmp_path / s) for s in ("l.raw", "r.raw", "in.bin"))
    W["left"].tofile(lp)
    W["right"].tofile(rp)
    with open(ip, "wb") as f:
        f.write(np.int32(lc.N_ROWS).tobytes() + W["floats"].tobytes() + W["desc"].tobytes() + W["bad"].tobytes())
        f.write(np.int32(len(case["kf_start"]) - 1).tobytes() + case["kf_start"].tobytes() + case["entries"].tobytes())
        f.write(np.int32(-1).tobytes())
        for a in (W["R"].ravel(), W["t"], W["Ow"], np.array(W["cam"], f32), np.array([W["logsf"], c["bf"], 3.0], f32)):
            f.write(np.ascontiguousarray(a, f32).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, ip], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.returncode, out.stdout, out.stderr)
