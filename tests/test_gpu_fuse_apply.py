"""-m gpu: jsorb_fuse_map (k_fa_index, k_fa_snapshot, k_fa_grid, k_fa_head, k_fuse_match_run, k_fa_apply, k_fa_csr, k_distinct_*, k_fa_finish) on the
worlds of tests/fuse_apply_cases.py against the restatement there, and through it against the reference's own runs (tests/test_fuse_apply_host.py).
Every comparison is np.array_equal over ALL the arrays the call writes, all its outputs and all its counts."""
import numpy as np
import pytest

import fuse_apply_cases as fa
import ref_matcher_cases as cases

pytestmark = pytest.mark.gpu
FORMS = ("async", "sync")
PERMUTATION_SEED = 5


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse_params(orb, prm):
    return orb.make_fuse_params((prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]),
                                (prm["inv_w"], prm["inv_h"]), float(prm["log_sf"]), prm["scale"], prm["inv_sigma2"], th=float(prm["th"]),
                                th_low=prm["th_low"], check_reprojection=prm["check"], bf=float(prm["bf"]), cols=prm["cols"], rows=prm["rows"])


class DeviceWorld:
    """a world's graph, table, keypoints and fuse state on the device"""

    def __init__(self, orb, W):
        import torch
        self.W, self.S, self.n_rows, self.pool = W, W["S"], W["n_rows"], W["pool"]
        self.graph = orb.KeyframeGraph(self.S, self.pool, 1)
        self.table = orb.MapPointTable(self.n_rows)
        self.kp = orb.KeyframeKeypoints(self.graph)
        self.kp.load(**{k: W[k] for k in self.kp.ARRAYS})
        self.table.floats[:, :self.n_rows].copy_(_dev(W["floats"]))
        n = max(self.n_rows, 1)
        self.replaced = torch.empty(n, dtype=torch.int32, device="cuda")
        self.visible, self.found = (None if W[k] is None else torch.empty(n, dtype=torch.int32, device="cuda") for k in ("visible", "found"))
        self.state = orb.fuse_state(self.graph, self.table, self.replaced, self.visible, self.found)
        self.params = fuse_params(orb, cases.fuse_prm(W["case"]))
        self.load()

    def load(self, W=None):
        """everything the call writes, as the world (or another of the same sizes) has it, into the same device arrays"""
        W = self.W if W is None else W
        self.graph.load(**{k: W[k] for k in ("state", "order_key", "point_off", "point_len", "point_pool", "registered")})
        self.table.bad[:self.n_rows].copy_(_dev(W["bad"]))
        self.table.desc[:self.n_rows].copy_(_dev(W["tdesc"]))
        self.replaced.fill_(-1)
        for k in ("visible", "found"):
            if W[k] is not None:
                getattr(self, k)[:self.n_rows].copy_(_dev(W[k]))

    def args(self, list_row=None):
        W = self.W
        return (self.params, self.graph, self.table, self.kp, self.state, [int(r) for r in W["list"]] if list_row is None else list_row, W["targets"], W["Rcw"],
                W["tcw"], W["Ow"])

    def fuse(self, m, form="async", **kw):
        W = self.W
        out = m.fuse_map(*self.args(), replace_loop=W["replace_loop"], log_cap=W["log_cap"], sync=form == "sync", **kw)
        if form == "sync":
            for k in fa.OUTPUTS:
                assert np.array_equal(out[k + "_host"], out[k].cpu().numpy()), k
        stats = m.fuse_map_stats()
        assert [stats[k] for k in fa.COUNTS] == out["counts"].cpu().numpy().tolist()
        return self.result(out)

    def result(self, out):
        import torch
        torch.cuda.synchronize()
        g, n = self.graph, self.n_rows
        res = dict(point_pool=g.point_pool[:self.pool], registered=g.registered[:self.pool], bad=self.table.bad[:n], tdesc=self.table.desc[:n],
                   replaced=self.replaced[:n], visible=None if self.visible is None else self.visible[:n], found=None if self.found is None else self.found[:n])
        res = {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}
        res.update({k: out[k].cpu().numpy() for k in fa.OUTPUTS})
        return res


@pytest.fixture(scope="module")
def matcher(orb):
    return orb.KeyframeMatcher()


_WORLDS = {}


def worlds():
    """(name, world, restated) of every stored case of both files and every constructed case, with the identity and with permuted slots: made once"""
    if not _WORLDS:
        from oracle import pyoracle as po
        po.build()
        every = [(f, k, c) for f in fa.FILES for k, c in fa.stored(f).items()] + [("constructed", k, c) for k, c in fa.constructed().items()]
        for f, k, c in every:
            for seed in (None, PERMUTATION_SEED):
                W = fa.to_world(c, fa.permutation(c, seed))
                _WORLDS[(f, k, seed)] = (W, fa.restate(po, W))
    return _WORLDS


def run_all(orb, m, group):
    n_replace = n_add = 0
    for (f, k, seed), (W, want) in worlds().items():
        if f != group:
            continue
        assert W["S"] <= 36 and W["n_rows"] <= 973 and max(W["point_len"]) <= 300 and len(W["targets"]) <= 33
        dw = DeviceWorld(orb, W)
        for form in FORMS:
            if form != FORMS[0]:
                dw.load()
            fa.same(want, dw.fuse(m, form), (f, k, seed, form))
        n_replace, n_add = n_replace + int(want["counts"][1]), n_add + int(want["counts"][2])
    return n_replace, n_add


@pytest.mark.parametrize("group", fa.FILES + ("constructed",))
def test_every_case_equals_the_restatement(orb, matcher, group):
    n_replace, n_add = run_all(orb, matcher, group)
    assert group == "constructed" or (n_replace >= 1000 and n_add >= 600)      # both permutations of 534 / 364 and 574 / 396


@pytest.mark.parametrize("group", fa.FILES + ("constructed",))
def test_the_tiny_build(orb, monkeypatch, group):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_fuse_apply", *jb.VARIANTS["tiny_fuse_apply"])))
    assert orb.fuse_map_build_caps() == fa.CHUNKS[1]
    # lists longer than the chunk are walked: the survivors of the stored runs end with more than twenty observers, those of the constructed cases with five
    longest = max(np.bincount(r["point_pool"][(r["point_pool"] >= 0) & (r["registered"] != 0)]).max(initial=0) for (f, _, _), (_, r) in worlds().items() if f == group)
    assert longest > (fa.CHUNKS[1] if group == "constructed" else 4 * fa.CHUNKS[1])
    run_all(orb, orb.KeyframeMatcher(), group)


def test_a_map_that_crosses_the_index_builds_block_edges(orb, matcher, po):
    # 70 000 rows, 200 slots of 400 entries: more slots than a block of k_fa_index strides over in one step would need, runs longer than its 256 threads
    W = fa.padded_world(po, 3)
    want = fa.restate(po, W)
    assert want["counts"][1] >= 20 and want["counts"][2] >= 20 and want["counts"][5] >= 5
    fa.same(want, DeviceWorld(orb, W).fuse(matcher), W["name"])


def _direction_b(W, res):
    """the second direction of SearchInNeighbors after the first: the first target as the keyframe the points go into, the rows the other targets hold as the list"""
    off, ln = W["point_off"], W["point_len"]
    rows = []
    for s in W["targets"][1:]:
        for r in res["point_pool"][off[s]:off[s] + ln[s]]:
            if r >= 0 and not res["bad"][r] and r not in rows:
                rows.append(int(r))
    return rows


def test_two_calls_in_a_row_then_update_connections_and_culling(orb, po):
    """direction A, then B with the candidates built from A's result, update_connections and cull_keyframes directly behind on the same matcher:
    their results equal those from the restatement's arrays uploaded afresh"""
    import torch
    c = fa.stored("fuse")["random0.00"]
    W = fa.to_world(c, fa.permutation(c, PERMUTATION_SEED))
    wantA = fa.restate(po, W)
    WB = dict(W, point_pool=wantA["point_pool"], registered=wantA["registered"], bad=wantA["bad"], tdesc=wantA["tdesc"])
    WB["list"] = np.array(_direction_b(W, wantA), np.int32)
    WB["targets"], WB["Rcw"], WB["tcw"], WB["Ow"] = W["targets"][:1], W["Rcw"][:1], W["tcw"][:1], W["Ow"][:1]
    WB["log_cap"] = len(WB["list"])
    cB = dict(c, list=WB["list"], targets=c["targets"][:1])
    cB["P"] = dict(c["P"], bad=wantA["bad"], desc=wantA["tdesc"])
    WB["case"] = cB
    wantB = fa.restate(po, WB)
    assert wantB["counts"][0] >= 3 and len(WB["list"]) >= 50
    m, dw = orb.KeyframeMatcher(), DeviceWorld(orb, W)
    fa.same(wantA, dw.fuse(m), "A")
    dw.W = WB
    gotB = dw.fuse(m)
    for k in fa.WRITTEN[:4] + fa.OUTPUTS:
        assert np.array_equal(gotB[k], wantB[k]), ("B", k)
    # the covisibility graph and a culling round read the new state
    slots = [int(s) for s in W["targets"][:4]]

    def behind(dw_, matcher_):
        cov = orb.Covisibility(dw_.S, 16)
        views = orb.KeyframeViews(dw_.graph, depth=False)
        views.load(octave=W["octave"].astype(np.uint8), stereo=(W["uright"] >= 0).astype(np.uint8))
        up = matcher_.update_connections(dw_.graph, dw_.table, cov, slots, neighbours=dw_.graph.neighbours)
        cull = matcher_.cull_keyframes(dw_.graph, dw_.table, cov, views, orb.culling_state(dw_.graph, dw_.table), slots, monocular=True,
                                       neighbours=dw_.graph.neighbours)
        torch.cuda.synchronize()
        out = {k: v for k, v in cov.arrays().items()}
        out.update(parent_out=up["parent_out"].cpu().numpy(), up_counts=up["counts"].cpu().numpy(),
                   **{k: cull[k].cpu().numpy() for k in ("decision", "n_mps", "n_redundant", "culled_slot", "counts")})
        return out
    got = behind(dw, m)
    fresh = DeviceWorld(orb, dict(WB, point_pool=wantB["point_pool"], registered=wantB["registered"], bad=wantB["bad"], tdesc=wantB["tdesc"]))
    want = behind(fresh, orb.KeyframeMatcher())
    assert want["up_counts"][0] == len(slots) and want["conn_len"].sum() > 0
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_the_call_is_capturable(orb, po):
    """captured behind a warm-up call, replayed on a fresh copy of another world of the same sizes (the list the other way round, other descriptors)"""
    import torch
    c = fa.stored("fuse")["random0.01"]
    W = fa.to_world(c)
    c2 = dict(c, list=c["list"][::-1].copy())
    other = np.array(c["P"]["desc"], np.uint8).reshape(-1, 32).copy()
    other[:, 0] ^= 0x0f                          # (a few bits: other distances, still matches)
    c2["P"] = dict(c["P"], desc=other)
    W2 = fa.to_world(c2)
    want = fa.restate(po, W2)
    assert want["counts"][1] >= 3 and want["log"].tolist() != fa.restate(po, W)["log"].tolist()
    m, dw = orb.KeyframeMatcher(), DeviceWorld(orb, W)
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    lst = _dev(W["list"])
    kw = dict(replace_loop=W["replace_loop"], log_cap=W["log_cap"])
    out = m.fuse_map(*dw.args(lst), **kw)      # the scratch and the statistics words take their size
    graph_ = torch.cuda.CUDAGraph()
    dw.load()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph_, stream=s):
        m.fuse_map(*dw.args(lst), out=out, wait=False, **kw)
    dw.load(W2)                                  # (what the capture enqueued has not run)
    lst.copy_(_dev(W2["list"]))
    for k in fa.OUTPUTS:
        out[k].fill_(-9)
    torch.cuda.synchronize()
    graph_.replay()
    torch.cuda.synchronize()
    fa.same(want, dw.result(out), "replayed")
    stats = m.fuse_map_stats()
    assert [stats[k] for k in fa.COUNTS] == want["counts"].tolist()


def test_refusals(orb, matcher, po):
    import torch
    c = fa.constructed()["equal_observations"]
    W = fa.to_world(c)
    dw = DeviceWorld(orb, W)
    fresh = orb.KeyframeMatcher()
    with pytest.raises(orb.JsorbError, match="before"):
        fresh.fuse_map_stats()
    a = dw.args()
    call = lambda *args, **kw: matcher.fuse_map(*args, **dict(dict(log_cap=4), **kw))
    # a state pointer that is not the graph's or the table's
    other = orb.KeyframeGraph(dw.S, dw.pool, 1)
    with pytest.raises(orb.JsorbError, match="not the graph's"):
        call(a[0], other, *a[2:])
    with pytest.raises(orb.JsorbError, match="not the graph's"):
        call(*a[:2], orb.MapPointTable(dw.n_rows), *a[3:])
    # kp->pool_entries != graph->pool_entries
    with pytest.raises(orb.JsorbError, match="pool_entries"):
        call(*a[:3], orb.KeyframeKeypoints(orb.KeyframeGraph(dw.S, dw.pool + 1, 1)), *a[4:])
    # n_targets outside [0, 256]
    with pytest.raises(orb.JsorbError, match="n_targets"):
        call(*a[:6], np.zeros(257, np.int32), np.zeros((257, 9), np.float32), np.zeros((257, 3), np.float32), np.zeros((257, 3), np.float32))
    # unaligned descriptors
    kp = orb.KeyframeKeypoints(dw.graph)
    kp.desc = torch.zeros(32 * (dw.pool + 1) + 1, dtype=torch.uint8, device="cuda")[1:1 + 32 * dw.pool].reshape(dw.pool, 32)
    with pytest.raises(orb.JsorbError, match="aligned"):
        call(*a[:3], kp, *a[4:])
    # visible without found
    with pytest.raises(orb.JsorbError, match="visible"):
        orb.fuse_state(dw.graph, dw.table, visible=dw.replaced)
    st = orb.fuse_state(dw.graph, dw.table)
    st.visible = dw.replaced.data_ptr()
    with pytest.raises(orb.JsorbError, match="visible"):
        call(*a[:4], st, *a[5:])
    # negative sizes, a graph without registered bytes
    with pytest.raises(orb.JsorbError, match="negative"):
        call(*a, log_cap=-1)
    other.registered = None
    with pytest.raises(orb.JsorbError, match="registered"):
        orb.fuse_state(other, dw.table)
    # nothing was changed by the refused calls; an empty list and no targets are valid calls
    for k, v in dw.result(matcher.fuse_map(*a[:5], [], *a[6:], log_cap=2)).items():
        if k in fa.WRITTEN[:4]:
            assert np.array_equal(v, W[k]), k
    out = matcher.fuse_map(*a[:5], [], *a[6:], log_cap=2, sync=True)
    assert out["counts_host"].tolist() == [0] * 10 and out["n_fused_host"].tolist() == [0] and (out["log_host"] == -1).all()
    out = matcher.fuse_map(*a[:6], [], np.zeros((0, 9)), np.zeros((0, 3)), np.zeros((0, 3)), log_cap=0, sync=True)
    assert out["counts_host"].tolist() == [0] * 10 and out["best_idx_host"].shape == (0, 1)
    fa.same(fa.restate(po, W), dw.fuse(matcher), "after the refusals")


def test_refusals_the_binding_cannot_reach(orb, matcher):
    """at the C ABI: the overload with Scw without replace_point, a graph without registered bytes, more pairs than an int holds - and nothing written"""
    import ctypes as C
    import torch
    c = fa.constructed()["the_replace_loop"]
    W = fa.to_world(c)
    dw = DeviceWorld(orb, W)
    lib = orb.load_library()
    T, n = len(W["targets"]), len(W["list"])
    lst = _dev(W["list"])
    out = [torch.full((max(T * n, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    nf, lg, cn = (torch.full((k,), -7, dtype=torch.int32, device="cuda") for k in (T, 4, 10))
    R, t, O = (np.ascontiguousarray(W[k], np.float32) for k in ("Rcw", "tcw", "Ow"))
    ts = np.ascontiguousarray(W["targets"], np.int32)
    torch.cuda.synchronize()

    def call(graph=None, replace_point=out[2].data_ptr(), n_list=n, n_targets=T):
        gs, tb, ks = (graph or dw.graph.struct()), dw.table.struct(), dw.kp.struct()
        rc = lib.jsorb_fuse_map_async(matcher._m, C.byref(dw.params), 1, C.byref(gs), C.byref(tb), C.byref(ks), C.byref(dw.state), n_list, lst.data_ptr(), n_targets,
                                      ts.ctypes.data, R.ctypes.data, t.ctypes.data, O.ctypes.data, out[0].data_ptr(), out[1].data_ptr(), replace_point,
                                      nf.data_ptr(), 1, lg.data_ptr(), cn.data_ptr())
        return rc, lib.jsorb_keyframe_matcher_last_error(matcher._m).decode()
    rc, err = call(replace_point=None)
    assert rc == -1 and "replace_point" in err
    bare = dw.graph.struct()
    bare.registered = None
    rc, err = call(graph=bare)
    assert rc == -1 and "registered" in err
    rc, err = call(n_list=1 << 24, n_targets=256)
    assert rc == -3 and "too large" in err
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in out + [nf, lg, cn])
    for k, v in dw.result(dict(zip(fa.OUTPUTS, out + [nf, lg, cn]))).items():
        if k in fa.WRITTEN[:4]:
            assert np.array_equal(v, W[k]), k
    assert call()[0] == 0
    matcher.sync()
    assert cn.cpu().numpy()[1] == 1                  # the accepted call ran the Replace loop


def test_the_example_fuses_both_directions_like_the_host_loop(orb, tmp_path):
    import subprocess
    from jetson_slam_amd import build as jb
    exe = jb.build_example("fuse_map", str(tmp_path / "fuse_map"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
