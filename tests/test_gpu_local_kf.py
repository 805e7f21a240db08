"""-m gpu: jsorb_local_keyframes (k_lk_marks, k_lk_votes, k_lk_rank, k_lk_expand, k_lk_gather) on the cases of tests/local_kf_cases.py against the
literal transcription of Tracking::UpdateLocalKeyFrames there, and its hand-over to jsorb_local_map_points and the matcher.  Integer work: every
comparison is np.array_equal."""
import ctypes
import subprocess

import numpy as np
import pytest

import local_kf_cases as kc
import local_map_cases as lc
from frame_builders import frame_of
from test_gpu_local_map import _dev, bits, frustum_of, make_frame, make_table

pytestmark = pytest.mark.gpu
OUT = ("point_row", "u", "v", "invz", "predicted_level", "view_cos", "in_frustum", "mp_descriptors", "blocked_in")


def small_handle(orb):
    return orb.ORBExtractor(240, 320, 1.2, 3, 9, 14, 7, 20, None, 15, 15)


@pytest.fixture(scope="module")
def handle(orb):
    return small_handle(orb)


class DeviceCase:
    """a graph and a table on the device for the cases' shapes; load(step) writes a step's arrays behind the same pointers"""

    def __init__(self, orb):
        import torch
        self.orb = orb
        self.graph = orb.KeyframeGraph(kc.S, kc.POOL, kc.CHILD_POOL)
        self.registered = self.graph.registered
        self.table = orb.MapPointTable(kc.N_ROWS)
        self.frame = torch.zeros(64, dtype=torch.int32, device="cuda")

    def load(self, step):
        G = step["G"]
        self.graph.registered = None if G["registered"] is None else self.registered
        self.graph.load(**{k: v for k, v in G.items() if v is not None})
        self.table.bad.copy_(_dev(step["bad"]))
        fr = step["frame_rows"]
        if fr is None:
            return None
        assert len(fr) <= 64
        self.frame[:len(fr)] = _dev(fr)
        return self.frame[:len(fr)]


def check_result(g, out, ref, label):
    h = {k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")}
    n = len(ref["list"])
    assert h["counts"].tolist() == ref["counts"].tolist(), (label, h["counts"].tolist(), ref["counts"].tolist())
    assert np.array_equal(h["local_kf_slot"][:n], ref["list"]), (label, h["local_kf_slot"][:n], ref["list"])
    assert h["state_io"].tolist() == [n, ref["ref_slot"]], label
    assert np.array_equal(h["local_kf_start"], ref["local_kf_start"]), label
    assert h["local_point_row"].dtype == np.int32 and np.array_equal(h["local_point_row"], ref["local_point_row"]), label
    assert g.local_keyframes_stats() == ref["stats"], (label, g.local_keyframes_stats(), ref["stats"])
    return h


def run_case(g, dc, case, sync=False):
    """the case's steps on the device with the persistent state, each against the restated form"""
    refs = kc.run_steps(kc.update_local_keyframes_restated, case)
    state = None
    for i, (step, ref) in enumerate(zip(case["steps"], refs)):
        fr = dc.load(step)
        out = g.local_keyframes(dc.graph, dc.table, fr, case["kf_capacity"], case["entry_capacity"], state=state, sync=sync)
        state = out["state"]
        check_result(g, out, ref, (case["name"], i))
        if sync:
            n = len(ref["list"])
            assert np.array_equal(out["local_kf_slot_host"][:n], ref["list"]) and out["state_host"].tolist() == [n, ref["ref_slot"]]
            assert out["counts_host"].tolist() == ref["counts"].tolist()
    return refs


# ---- every case, every step, every output, the stats ----
@pytest.mark.parametrize("name", list(kc.CASES))
def test_the_call_equals_the_reference_loops(orb, handle, name):
    assert orb.local_keyframes_build_caps() == kc.CAPS[0]
    run_case(handle, DeviceCase(orb), kc.CASES[name])


def test_seeded_random_graphs(orb, handle):
    dc = DeviceCase(orb)
    for seed in range(40):
        run_case(handle, dc, kc.random_case(seed))


# ---- the build whose LDS membership bits end at slot 64 and whose LDS child candidates end at 16 ----
def test_the_tiny_build(orb, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_local_kf", *jb.VARIANTS["tiny_local_kf"])))
    assert orb.local_keyframes_build_caps() == kc.CAPS[1]
    g, dc = small_handle(orb), DeviceCase(orb)
    for case in kc.CASES.values():
        run_case(g, dc, case)
    for seed in range(0, 40, 3):
        run_case(g, dc, kc.random_case(seed))


# ---- call, empty-counter call, call: the persistent state through the synchronous form ----
def test_call_empty_counter_call(orb, handle):
    case = kc.CASES["empty_counter_keeps_the_list"]
    refs = run_case(handle, DeviceCase(orb), case, sync=True)
    assert [int(r["counts"][7]) for r in refs] == [0, 1, 0] and refs[1]["list"].tolist() == refs[0]["list"].tolist() != refs[2]["list"].tolist()
    assert not np.array_equal(refs[1]["local_point_row"], refs[0]["local_point_row"])      # gathered again from the changed pool


# ---- the Python graph's setters lay out the same map ----
def test_the_graph_setters(orb, handle):
    import torch
    step = kc.CASES["tiny_caps"]["steps"][0]
    G = step["G"]
    graph = orb.KeyframeGraph(kc.S, kc.POOL, kc.CHILD_POOL)
    for s in range(kc.S):
        if G["state"][s]:
            graph.set_keyframe(s, G["point_pool"][G["point_off"][s]:G["point_off"][s] + G["point_len"][s]], int(G["order_key"][s]), int(G["state"][s]))
            graph.set_neighbours(s, G["neighbours"][s])
            graph.set_children(s, G["child_pool"][G["child_off"][s]:G["child_off"][s] + G["child_len"][s]])
            graph.set_parent(s, int(G["parent"][s]))
    graph.set_keyframe(126, [1, 2, 3], 5)
    graph.erase(126)
    graph.set_state(0, orb.KF_BAD)
    G2 = {k: getattr(graph, k).cpu().numpy() for k in graph.ARRAYS}
    table = orb.MapPointTable(kc.N_ROWS)
    table.bad.copy_(_dev(step["bad"]))
    ref = kc.update_local_keyframes_restated(G2, step["bad"], step["frame_rows"], 84, 900)
    want = kc.update_local_keyframes_restated(G, step["bad"], step["frame_rows"], 84, 900)
    assert ref["list"].tolist() == want["list"].tolist() and G2["state"][126] == 0 and G2["state"][0] == 2
    out = handle.local_keyframes(graph, table, _dev(step["frame_rows"]), 84, 900)
    check_result(handle, out, ref, "setters")
    with pytest.raises(orb.JsorbError):
        graph.set_keyframe(kc.S, [1], 0)


# ---- the hand-over: local keyframes, then the local map with ONE keyframe over local_point_row, then the matcher ----
def local_map_graph(orb, case, n_rows):
    """the keyframes of a tests/local_map_cases.py case as a graph: slot 3 + 2 i for keyframe i, keys against the slots, a chain of neighbours"""
    runs = case["keyframes"]
    graph = orb.KeyframeGraph(32, sum(len(r) for r in runs) + len(runs[0]) + 8, 16)
    slots = [3 + 2 * i for i in range(len(runs))]
    for i, (s, r) in enumerate(zip(slots, runs)):
        graph.set_keyframe(s, np.where((r >= 0) & (r < n_rows), r, -1), 1000 - 10 * i)      # (rows outside the table: the local map drops them either way)
        graph.set_neighbours(s, [slots[(i + 1) % len(slots)], 30])
    # a keyframe LocalMapping has not processed yet: in no point's observations, so no vote; it comes in as a neighbour, its rows all duplicates
    graph.set_keyframe(30, runs[0][::-1].copy(), 5000, registered=np.zeros(len(runs[0]), np.uint8))
    return graph


def test_the_hand_over_to_the_local_map_and_the_matcher(orb):
    import torch
    W = lc.world()
    gl, gr, ur = make_frame(orb)
    table, frustum = make_table(orb), frustum_of(orb, W)
    case = lc.build_case("six")
    graph = local_map_graph(orb, case, lc.N_ROWS)
    G = {k: getattr(graph, k).cpu().numpy() for k in graph.ARRAYS}
    frame_rows = _dev(case["frame_rows"])
    ref = kc.update_local_keyframes_restated(G, W["bad"], case["frame_rows"], 84, 0)
    assert ref["stats"]["n_first"] >= 4 and ref["stats"]["n_neighbours"] >= 1 and len(ref["list"]) == len(case["keyframes"]) + 1
    runs = [G["point_pool"][G["point_off"][s]:G["point_off"][s] + G["point_len"][s]] for s in ref["list"]]
    kf_start = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int32)
    e_total, capacity = int(kf_start[-1]), 700
    F = frame_of(gl, W["c"])
    grid = (0.0, 0.0, float(F["inv_w"]), float(F["inv_h"]))

    def search(g, o):
        r = g.search_local_points(o["u"], o["v"], o["invz"], o["predicted_level"], o["view_cos"], o["in_frustum"], o["mp_descriptors"], grid, th=1.0,
                                   mbf=W["c"]["bf"], u_right=ur, blocked=o["blocked_in"])
        return [x.cpu().numpy() for x in r]

    old = gl.local_map_points(table, frustum, kf_start, _dev(np.concatenate(runs)), frame_rows, capacity)
    old_h, old_m = {k: old[k].cpu().numpy() for k in OUT + ("counts",)}, search(gl, old)
    assert old_h["counts"][2] > 50 and old_m[3][0] > 20
    entry_capacity = e_total + 9
    fresh = orb.ORBExtractor(W["c"]["h"], W["c"]["w"], 1.2, W["c"]["L"], 9, 14, 7, W["c"]["th"], None, W["c"]["tile"], W["c"]["tile"])
    fresh.extract(W["left"])
    # gl: the local map has used the row words and set them back; fresh: the local keyframes are the first to touch them, the local map follows
    for order, g in (("local map first", gl), ("local keyframes first", fresh)):
        lk = g.local_keyframes(graph, table, frame_rows, 84, entry_capacity)
        assert int(lk["counts"][4]) == e_total and np.array_equal(lk["local_kf_slot"].cpu().numpy()[:len(ref["list"])], ref["list"])
        new = g.local_map_points(table, frustum, [0, entry_capacity], lk["local_point_row"], frame_rows, capacity)
        new_h = {k: new[k].cpu().numpy() for k in OUT + ("counts",)}
        for k in OUT:
            assert np.array_equal(bits(new_h[k]), bits(old_h[k])), (order, k)
        assert new_h["counts"][:4].tolist() == old_h["counts"][:4].tolist()
        assert g.local_map_stats()["n_null"] >= 9                            # the padding, dropped as NULL entries
        for a, b in zip(search(g, new), old_m):
            assert np.array_equal(a, b), order


# ---- (local keyframes, local map, search) captured once, replayed after the graph's arrays changed ----
def test_the_step_is_capturable(orb):
    import torch
    W = lc.world()
    c = W["c"]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    s = torch.cuda.Stream()
    g.set_stream(s.cuda_stream)
    g.extract(W["left"])
    table, frustum = make_table(orb), frustum_of(orb, W)
    case = lc.build_case("six")
    graph = local_map_graph(orb, case, lc.N_ROWS)
    frame_rows = _dev(case["frame_rows"])
    entry_capacity, capacity = int(graph.point_len.sum()) + 4, 600
    F = frame_of(g, c)
    grid = (0.0, 0.0, float(F["inv_w"]), float(F["inv_h"]))

    sprm = orb.JsorbSearchParams(1.0, 0.8, orb.TH_HIGH, c["bf"], *grid, 64, 48)
    N, lib = g.n_keypoints(0), orb.load_library()

    def step(lk=None, lm=None, wait=True):
        lk = g.local_keyframes(graph, table, frame_rows, 84, entry_capacity, out=lk, wait=wait)
        lm = g.local_map_points(table, frustum, [0, entry_capacity], lk["local_point_row"], frame_rows, capacity, out=lm, wait=wait)
        if "match_kp" not in lm:
            lm.update(match_kp=torch.empty(capacity, dtype=torch.int32, device="cuda"), match_dist=torch.empty(capacity, dtype=torch.int32, device="cuda"),
                      kp_match=torch.empty(N, dtype=torch.int32, device="cuda"), n_matches=torch.empty(1, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
        assert lib.jsorb_search_local_points_async(g.handle, 0, ctypes.byref(sprm), capacity, *[lm[k].data_ptr() for k in
                                                   ("u", "v", "invz", "predicted_level", "view_cos", "in_frustum", "mp_descriptors")], None,
                                                   lm["blocked_in"].data_ptr(), *[lm[k].data_ptr() for k in ("match_kp", "match_dist", "kp_match", "n_matches")]) == 0
        if wait:
            g.sync()
        return lk, lm

    def snapshot(lk, lm):
        return {k: v.cpu().numpy() for k, v in list(lk.items()) + list(lm.items()) if hasattr(v, "cpu")}

    lk, lm = step()                                                           # the scratch takes its size
    before = snapshot(lk, lm)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=s):
        step(lk, lm, wait=False)
    # the map changes behind the same pointers: a keyframe goes bad, another loses its neighbours, a run's rows are reversed, the frame's rows shift
    graph.set_state(5, orb.KF_BAD)
    graph.set_neighbours(3, [])
    off, ln = int(graph.point_off[7]), int(graph.point_len[7])
    graph.point_pool[off:off + ln] = graph.point_pool[off:off + ln].flip(0)
    frame_rows.copy_(_dev(np.roll(case["frame_rows"], 5)))
    lk["state_io"].copy_(_dev(np.array([0, -1], np.int32)))
    torch.cuda.synchronize()
    graph_.replay()
    torch.cuda.synchronize()
    replayed = snapshot(lk, lm)
    lk["state_io"].copy_(_dev(np.array([0, -1], np.int32)))
    lk2, lm2 = step()                                                         # uncaptured, on the same inputs
    plain = snapshot(lk2, lm2)
    n_local = int(plain["state_io"][0])
    for k in plain:                                                           # (local_kf_slot is IN/OUT: what lies behind n_local is the caller's)
        a, b = (replayed[k][:n_local], plain[k][:n_local]) if k == "local_kf_slot" else (replayed[k], plain[k])
        assert np.array_equal(bits(a), bits(b)), k
    G = {k: getattr(graph, k).cpu().numpy() for k in graph.ARRAYS}
    ref = kc.update_local_keyframes_restated(G, W["bad"], np.roll(case["frame_rows"], 5), 84, entry_capacity)
    assert replayed["counts"][:8].tolist() != before["counts"][:8].tolist() and np.array_equal(replayed["local_point_row"], ref["local_point_row"])
    assert not np.array_equal(replayed["local_kf_slot"], before["local_kf_slot"])


# ---- every refusal of the contract: the code, the text, and nothing launched ----
def test_refusals(orb, handle):
    import torch
    g, lib = handle, orb.load_library()
    dc = DeviceCase(orb)
    fr = dc.load(kc.CASES["tiny_caps"]["steps"][0])
    out = g.local_keyframes(dc.graph, dc.table, fr, 84, 500)
    stats = g.local_keyframes_stats()
    keep = {k: out[k].clone() for k in ("local_kf_slot", "state_io", "local_kf_start", "local_point_row", "counts")}
    names = ("local_kf_slot", "state_io", "local_kf_start", "local_point_row", "counts")

    def call(graph=None, table=None, n_frame=len(fr), kf_capacity=84, entry_capacity=500, no_graph=False, no_table=False, **ptr):
        gs, tb = graph or dc.graph.struct(), table or dc.table.struct()
        p = [ptr.get(k, out[k].data_ptr()) for k in names]
        rc = lib.jsorb_local_keyframes_async(g.handle, None if no_graph else ctypes.byref(gs), None if no_table else ctypes.byref(tb), fr.data_ptr(), n_frame,
                                             kf_capacity, entry_capacity, *p)
        return rc, lib.jsorb_last_error(g.handle).decode()

    def graph_with(**kw):
        s = dc.graph.struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def table_with(**kw):
        t = dc.table.struct()
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    refusals = [(dict(no_graph=True), "NULL graph"), (dict(no_table=True), "NULL graph"), (dict(counts=None), "NULL graph"), (dict(state_io=None), "NULL graph"),
                (dict(local_kf_slot=None), "NULL graph"), (dict(local_kf_start=None), "NULL graph"), (dict(local_point_row=None), "NULL local_point_row"),
                (dict(table=table_with(bad=None)), "NULL table array"), (dict(kf_capacity=83), "at least 84"), (dict(kf_capacity=-1), "at least 84"),
                (dict(entry_capacity=-1), "must not be negative"), (dict(entry_capacity=1 << 24), "more than 16777215 entries"),
                (dict(n_frame=-1), "must not be negative"), (dict(table=table_with(n_rows=-1)), "must not be negative"),
                (dict(graph=graph_with(max_keyframes=-1)), "must not be negative"), (dict(graph=graph_with(pool_entries=-1)), "must not be negative"),
                (dict(graph=graph_with(child_entries=-1)), "must not be negative"), (dict(graph=graph_with(max_keyframes=1 << 24)), "more than 16777215 keyframe slots")]
    refusals += [(dict(graph=graph_with(**{k: None})), "NULL graph array") for k in dc.graph.ARRAYS if k != "registered"]
    for kw, text in refusals:
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("local_keyframes: ") and text in err, (kw, rc, err)
    slot_h, state_h, counts_h = np.zeros(84, np.int32), np.zeros(2, np.int32), np.zeros(8, np.int32)
    gs, tb = dc.graph.struct(), dc.table.struct()
    args = [g.handle, ctypes.byref(gs), ctypes.byref(tb), fr.data_ptr(), len(fr), 84, 500] + [out[k].data_ptr() for k in names]
    assert lib.jsorb_local_keyframes(*args, None, state_h.ctypes.data, counts_h.ctypes.data) == -1 and "NULL host output" in lib.jsorb_last_error(g.handle).decode()
    assert lib.jsorb_local_keyframes(*args, slot_h.ctypes.data, None, counts_h.ctypes.data) == -1
    assert lib.jsorb_local_keyframes(*args, slot_h.ctypes.data, state_h.ctypes.data, None) == -1
    torch.cuda.synchronize()
    assert all(bool((out[k] == keep[k]).all()) for k in names) and g.local_keyframes_stats() == stats      # nothing was launched
    # valid edge calls: no slots at all, no entries wanted, registered NULL
    assert call(graph=graph_with(max_keyframes=0, **{k: None for k in dc.graph.ARRAYS}), entry_capacity=0, local_point_row=None)[0] == 0
    g.sync()
    assert out["counts"].cpu().numpy().tolist()[:3] == [0, 0, int(keep["state_io"][0])] and int(out["counts"][7]) == 1
    assert call(graph=graph_with(registered=None))[0] == 0
    g.sync()
    with pytest.raises(orb.JsorbError):
        small_handle(orb).local_keyframes_stats()


# ---- the C++ example through the compat shim: one TrackLocalMap step both ways, checked by the example itself ----
def test_update_local_keyframes_example(orb, tmp_path):
    from jetson_slam_amd import build as jb
    exe = jb.build_example("update_local_keyframes", str(tmp_path / "update_local_keyframes"))
    out = subprocess.run([exe], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.returncode, out.stdout, out.stderr)
