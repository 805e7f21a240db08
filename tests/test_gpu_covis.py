"""-m gpu: jsorb_update_connections (k_cv_marks, k_cv_counts, k_cv_select, k_cv_apply, k_cv_reset), jsorb_erase_connections, jsorb_connected_mask and
jsorb_best_covisibles on the worlds of tests/covis_cases.py, against the restated parallel form there and against the arrays recorded from the
reference's own src/KeyFrame.cpp (tests/golden/ref_matcher_covis.npz).  Integer work: every comparison is np.array_equal, over ALL slots."""
import ctypes
import subprocess

import numpy as np
import pytest

import covis_cases as cc
import local_kf_cases as kc

pytestmark = pytest.mark.gpu
FORMS = ("c_entry", "binding_sync", "async_back_to_back")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class DeviceWorld:
    """a graph, a table and a covisibility state on the device for the worlds' shapes"""

    def __init__(self, orb, C):
        self.orb = orb
        self.graph = orb.KeyframeGraph(cc.S, cc.POOL, 1)
        self.registered = self.graph.registered
        self.table = orb.MapPointTable(cc.N_ROWS)
        self.cov = orb.Covisibility(cc.S, C)

    def load(self, world):
        G, st = world["G"], world["state"]
        assert self.cov.conn_capacity == world["C"]
        self.graph.registered = None if G["registered"] is None else self.registered
        self.graph.load(**{k: v for k, v in G.items() if v is not None})
        self.graph.load(neighbours=st["neighbours"])
        self.table.bad.copy_(_dev(world["bad"]))
        self.cov.load(**{k: st[k] for k in self.cov.ARRAYS})

    def state(self):
        import torch
        torch.cuda.synchronize()
        st = self.cov.arrays()
        st["neighbours"] = self.graph.neighbours.cpu().numpy()
        return cc.normalised(st)


def device_results(orb, m, dw, world, form):
    """the world's script on the device -> results in the yardsticks' form.  async_back_to_back enqueues every step without a wait in between
    and reads the state once, behind the last step: its intermediate states are None."""
    import torch
    dw.load(world)
    lib, results = orb.load_library(), []
    for kind, arg in world["script"]:
        wait = form != "async_back_to_back"
        if kind == "erase":
            counts = m.erase_connections(dw.graph, dw.cov, arg, neighbours=dw.graph.neighbours, wait=wait)
            results.append(dict(counts_dev=counts))
        elif form == "c_entry":
            n, C = len(arg), dw.cov.conn_capacity
            slots = _dev(np.array(arg, np.int32).reshape(-1))
            parent, counts = torch.full((max(n, 1),), -9, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
            snap = [torch.zeros((max(n, 1), C), dtype=torch.int32, device="cuda"), torch.zeros((max(n, 1), C), dtype=torch.int32, device="cuda"),
                    torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")]
            sn = orb.JsorbConnSnapshot(*[t.data_ptr() for t in snap])
            gs, tb, cs = dw.graph.struct(), dw.table.struct(), dw.cov.struct()
            torch.cuda.synchronize()
            rc = lib.jsorb_update_connections_async(m.handle, ctypes.byref(gs), ctypes.byref(tb), ctypes.byref(cs), n, slots.data_ptr() if n else None,
                                                    dw.graph.neighbours.data_ptr(), parent.data_ptr(), ctypes.byref(sn), counts.data_ptr())
            assert rc == 0, lib.jsorb_keyframe_matcher_last_error(m.handle)
            m.sync()
            results.append(dict(parent_out=parent[:n], counts_dev=counts, snap_slot=snap[0][:n], snap_weight=snap[1][:n], snap_len=snap[2][:n]))
        else:
            out = m.update_connections(dw.graph, dw.table, dw.cov, arg, neighbours=dw.graph.neighbours, snapshot=True, sync=form == "binding_sync", wait=wait)
            if form == "binding_sync":
                assert np.array_equal(out["parent_host"], out["parent_out"].cpu().numpy()) and np.array_equal(out["counts_host"], out["counts"].cpu().numpy())
            results.append(dict(out, counts_dev=out["counts"]))
        if wait:
            results[-1]["state"] = dw.state()
            if kind == "update":
                stats = m.update_connections_stats()
                assert [stats[k] for k in cc.COUNTS] == results[-1]["counts_dev"].cpu().numpy()[:7].tolist()
            n_words, n_nonzero = m.update_connections_scratch() if any(k == "update" for k, _ in world["script"][:len(results)]) else (cc.N_ROWS, 0)
            assert n_words >= cc.N_ROWS and n_nonzero == 0, (world["name"], len(results), n_nonzero)
    if form == "async_back_to_back":
        m.sync()
        for r in results:
            r["state"] = None
        if results:
            results[-1]["state"] = dw.state()
    for r in results:
        r["counts"] = r["counts_dev"].cpu().numpy()
        if "parent_out" in r:
            r["parent_out"] = r["parent_out"].cpu().numpy()
            ln = r["snap_len"].cpu().numpy()
            ss, sw = r["snap_slot"].cpu().numpy(), r["snap_weight"].cpu().numpy()
            r["snapshot"] = [None if ln[i] < 0 else list(zip(ss[i, :ln[i]].tolist(), sw[i, :ln[i]].tolist())) for i in range(len(ln))]
    return results


def check(world, got, want, label):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        if "parent_out" in w:
            assert g["counts"].tolist() == w["counts"].tolist(), (label, t, g["counts"].tolist(), w["counts"].tolist())
            assert np.array_equal(g["parent_out"], w["parent_out"]), (label, t, g["parent_out"], w["parent_out"])
            assert g["snapshot"] == w["snapshot"], (label, t, "snapshot")
        else:
            assert g["counts"].tolist() == w["counts"].tolist(), (label, t, "erase counts", g["counts"].tolist(), w["counts"].tolist())
        if g["state"] is not None:
            for k, v in w["state"].items():
                assert g["state"][k].dtype == v.dtype and np.array_equal(g["state"][k], v), (label, t, k, np.argwhere(g["state"][k] != v)[:4].tolist())


@pytest.fixture(scope="module")
def matcher(orb):
    return orb.KeyframeMatcher()


@pytest.fixture(scope="module")
def device_worlds(orb):
    cache = {}

    def get(C):
        if C not in cache:
            cache[C] = DeviceWorld(orb, C)
        return cache[C]
    return get


# ---- every case through the three forms: all slots' arrays, the neighbours rows, parent_out, the snapshot, counts, stats, the scratch ----
@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_cases_equal_the_restatement(orb, matcher, device_worlds, name):
    assert orb.covisibility_build_caps() == cc.CAPS[0]
    world, expect = cc.build_case(name)
    want = cc.run_restated(world)
    for form in FORMS:
        got = device_results(orb, matcher, device_worlds(world["C"]), world, form)
        check(world, got, want, (name, form))
    cc.check_expect(device_results(orb, matcher, device_worlds(world["C"]), world, "c_entry"), expect)


# ---- the recorded worlds: the device against the reference's own KeyFrame.cpp ----
@pytest.mark.parametrize("form", FORMS)
def test_the_recorded_worlds_equal_the_reference(orb, matcher, device_worlds, form):
    golden = cc.load_golden()
    for world in cc.golden_worlds():
        got = device_results(orb, matcher, device_worlds(world["C"]), world, form)
        check(world, got, cc.run_restated(world), (world["name"], form))
        if form != "async_back_to_back":
            cc.same_as_recorded(world, got, golden[world["name"]])


def test_seeded_random_worlds_with_overflow(orb, matcher, device_worlds):
    n_overflow = 0
    for seed in range(0, 120, 4):                # the worlds of C = 16
        world = cc.random_world(seed)
        want = cc.run_restated(world)
        n_overflow += sum(int(r["counts"][6]) for r in want if "parent_out" in r)
        check(world, device_results(orb, matcher, device_worlds(world["C"]), world, "binding_sync"), want, world["name"])
    assert n_overflow > 10


# ---- the build whose LDS buffers end at 24 + 32 entries ----
def test_the_tiny_build(orb, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_covis", *jb.VARIANTS["tiny_covis"])))
    assert orb.covisibility_build_caps() == cc.CAPS[1]
    with pytest.raises(orb.JsorbError):
        orb.Covisibility(cc.S, cc.CAPS[1][1] + 1)
    m, worlds, n = orb.KeyframeMatcher(), {}, 0
    for world in [cc.build_case(name)[0] for name in cc.CASES] + [cc.random_world(seed) for seed in range(0, 40, 4)]:
        if world["C"] > cc.CAPS[1][1]:
            continue
        dw = worlds.setdefault(world["C"], DeviceWorld(orb, world["C"]))
        check(world, device_results(orb, m, dw, world, "binding_sync"), cc.run_restated(world), ("tiny", world["name"]))
        n += 1
    assert n >= 25


# ---- the getters: the mask, the best lists, one slot's copy ----
def test_connected_mask_best_covisibles_and_the_copies(orb, matcher, device_worlds):
    world = cc.random_world(5)
    dw = device_worlds(world["C"])
    want = cc.run_restated(world)[-1]["state"]
    device_results(orb, matcher, dw, world, "binding_sync")
    busy = [int(s) for s in np.argsort(-want["ord_len"])[:6]] + [int(np.argmin(want["conn_len"]))]
    for s in busy:
        mask = matcher.connected_mask(dw.cov, s).cpu().numpy()
        ref = np.zeros(cc.S, np.uint8)
        ref[want["conn_slot"][s, :want["conn_len"][s]]] = 1
        assert mask.dtype == np.uint8 and np.array_equal(mask, ref), s
        assert dw.cov.connected(s).tolist() == want["conn_slot"][s, :want["conn_len"][s]].tolist()
        assert dw.cov.ordered(s).tolist() == want["ord_slot"][s, :want["ord_len"][s]].tolist()
        assert dw.cov.weights(s).tolist() == want["ord_weight"][s, :want["ord_len"][s]].tolist()
        assert dw.cov.best(s, 5).tolist() == want["ord_slot"][s, :min(5, want["ord_len"][s])].tolist()
        ow = want["ord_weight"][s, :want["ord_len"][s]]
        for w in sorted(set(ow.tolist() + [0, 15, 10 ** 6])):
            n = int((ow >= w).sum())             # GetCovisiblesByWeight's upper_bound: empty when EVERY weight is at or above w
            assert dw.cov.by_weight(s, w).tolist() == ([] if n == len(ow) else want["ord_slot"][s, :n].tolist()), (s, w)
        if want["conn_len"][s]:
            o = int(want["conn_slot"][s, 0])
            assert dw.cov.weight(s, o) == want["conn_weight"][s, 0]
        assert dw.cov.weight(s, s) == 0
    assert want["ord_len"][busy[0]] > 3
    slots = busy + [-1, cc.S]
    for N in (1, 5, 10, 40):
        out, out_len = (t.cpu().numpy() for t in matcher.best_covisibles(dw.cov, slots, N))
        for i, s in enumerate(slots):
            lst = want["ord_slot"][s, :min(N, want["ord_len"][s])].tolist() if 0 <= s < cc.S else []
            assert out[i].tolist() == lst + [-1] * (N - len(lst)) and out_len[i] == len(lst), (N, s)


# ---- the chain: the device-maintained neighbours table feeds jsorb_local_keyframes ----
def test_the_maintained_neighbours_feed_the_local_keyframes(orb, matcher):
    import torch
    world = cc.random_world(13)
    G = dict(world["G"])
    slots = [int(s) for s in np.nonzero(G["state"])[0]]
    world["script"] = [("update", slots[i:i + 32]) for i in range(0, len(slots), 32)]
    world["state"]["neighbours"][:] = -1
    dw = DeviceWorld(orb, world["C"])
    device_results(orb, matcher, dw, world, "binding_sync")
    host = cc.run_literal(world)[-1]["state"]["neighbours"]      # the table a host loop over the reference's lists would upload
    assert np.array_equal(dw.graph.neighbours.cpu().numpy(), host) and (host[slots] >= 0).sum() > 3 * len(slots)
    voters = slots[:1]
    frame_rows = np.concatenate([cc.run_of(G, s)[:8] for s in voters]).astype(np.int32)
    Gk = dict(G, neighbours=host, child_off=np.zeros(cc.S, np.int32), child_len=np.zeros(cc.S, np.int32), child_pool=np.full(1, -1, np.int32),
              parent=np.full(cc.S, -1, np.int32))
    ref = kc.update_local_keyframes_restated(Gk, world["bad"], frame_rows, 84, 0)
    g = orb.ORBExtractor(240, 320, 1.2, 3, 9, 14, 7, 20, None, 15, 15)
    out = g.local_keyframes(dw.graph, dw.table, _dev(frame_rows), 84, 0)
    n = len(ref["list"])
    assert ref["stats"]["n_neighbours"] >= 1 and out["counts"].cpu().numpy().tolist() == ref["counts"].tolist()
    assert np.array_equal(out["local_kf_slot"].cpu().numpy()[:n], ref["list"])


# ---- captured once, replayed on another state ----
def test_the_call_is_capturable(orb):
    import torch
    world = cc.random_world(13)
    upd = [arg for kind, arg in world["script"] if kind == "update" and len(arg) > 1][0]
    world["script"] = [("update", upd)]
    m, dw = orb.KeyframeMatcher(), DeviceWorld(orb, world["C"])
    s = torch.cuda.Stream()
    m.set_stream(s.cuda_stream)
    dw.load(world)
    out = m.update_connections(dw.graph, dw.table, dw.cov, upd, neighbours=dw.graph.neighbours, snapshot=True)      # the scratch takes its size
    graph_ = torch.cuda.CUDAGraph()
    dw.load(world)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph_, stream=s):
        m.update_connections(dw.graph, dw.table, dw.cov, out["slots"], neighbours=dw.graph.neighbours, out=out, wait=False)
    dw.load(world)                               # (what the capture enqueued has not run)
    out["slots"].copy_(out["slots"].flip(0))     # the same keyframes the other way round, behind the same pointers
    torch.cuda.synchronize()
    graph_.replay()
    torch.cuda.synchronize()
    world["script"] = [("update", upd[::-1])]
    want = cc.run_restated(world)[-1]
    got = dw.state()
    for k, v in want["state"].items():
        assert np.array_equal(got[k], v), k
    assert out["counts"].cpu().numpy().tolist() == want["counts"].tolist() and np.array_equal(out["parent_out"].cpu().numpy(), want["parent_out"])
    assert m.update_connections_scratch()[1] == 0


# ---- the refusals of the contract: the code, the text, and nothing launched ----
def test_refusals(orb, matcher, device_worlds):
    import torch
    lib, m = orb.load_library(), matcher
    world, _ = cc.build_case("counts_14_15_16")
    dw = device_worlds(world["C"])
    device_results(orb, m, dw, world, "binding_sync")
    before = dw.state()
    slots, parent, counts = _dev(np.array([0, 1], np.int32)), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.full((8,), -5, dtype=torch.int32, device="cuda")

    def call(graph=None, table=None, cov=None, n=2, slots_p=slots.data_ptr(), counts_p=counts.data_ptr(), snap=None, no=()):
        gs, tb, cs = graph or dw.graph.struct(), table or dw.table.struct(), cov or dw.cov.struct()
        ref = lambda x, k: None if k in no else ctypes.byref(x)
        rc = lib.jsorb_update_connections_async(m.handle, ref(gs, "graph"), ref(tb, "table"), ref(cs, "cov"), n, slots_p, None, parent.data_ptr(),
                                                None if snap is None else ctypes.byref(snap), counts_p)
        return rc, lib.jsorb_keyframe_matcher_last_error(m.handle).decode()

    def with_(s, **kw):
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    lo, hi = orb.covisibility_build_caps()
    refusals = [(dict(no=("graph",)), "NULL graph"), (dict(no=("table",)), "NULL graph"), (dict(no=("cov",)), "NULL cov"), (dict(counts_p=None), "NULL graph"),
                (dict(n=-1), "n_update must be in [0, 32]"), (dict(n=33), "n_update must be in [0, 32]"), (dict(slots_p=None), "NULL update_slot"),
                (dict(cov=with_(dw.cov.struct(), conn_capacity=lo - 1)), "conn_capacity outside"), (dict(cov=with_(dw.cov.struct(), conn_capacity=hi + 1)), "conn_capacity outside"),
                (dict(cov=with_(dw.cov.struct(), max_keyframes=cc.S - 1)), "differ in max_keyframes"), (dict(cov=with_(dw.cov.struct(), max_keyframes=-1)), "must not be negative"),
                (dict(graph=with_(dw.graph.struct(), pool_entries=-1)), "must not be negative"), (dict(table=with_(dw.table.struct(), n_rows=-1)), "must not be negative"),
                (dict(table=with_(dw.table.struct(), bad=None)), "NULL table array"), (dict(snap=orb.JsorbConnSnapshot(None, None, None)), "NULL snapshot array")]
    refusals += [(dict(graph=with_(dw.graph.struct(), **{k: None})), "NULL graph array") for k in ("state", "order_key", "point_off", "point_len", "point_pool")]
    refusals += [(dict(cov=with_(dw.cov.struct(), **{k: None})), "NULL covisibility array") for k in dw.cov.ARRAYS]
    for kw, text in refusals:
        rc, err = call(**kw)
        assert rc == -1 and err.startswith("update_connections: ") and text in err, (kw, rc, err)
    cs, gs = dw.cov.struct(), dw.graph.struct()
    for slot in (-1, cc.S):
        assert lib.jsorb_erase_connections_async(m.handle, ctypes.byref(gs), ctypes.byref(cs), slot, None, counts.data_ptr()) == -1
        assert lib.jsorb_connected_mask_async(m.handle, ctypes.byref(cs), slot, counts.data_ptr()) == -1
    assert lib.jsorb_best_covisibles_async(m.handle, ctypes.byref(cs), 1, slots.data_ptr(), 0, counts.data_ptr(), None) == -1
    assert lib.jsorb_covisibility_copy(ctypes.byref(cs), cc.S, *([None] * 5)) == -1
    after = dw.state()
    assert all(np.array_equal(before[k], after[k]) for k in before) and (counts.cpu().numpy() == -5).all()      # nothing was launched
    # a valid edge call: no slots at all - both members are skipped and say so
    rc, err = call(graph=with_(dw.graph.struct(), max_keyframes=0), cov=with_(dw.cov.struct(), max_keyframes=0))
    m.sync()
    assert rc == 0 and parent.cpu().numpy().tolist() == [-1, -1] and counts.cpu().numpy().tolist() == [0, 2, 0, 0, 0, 0, 0, 0], (rc, err)
    after = dw.state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    with pytest.raises(orb.JsorbError):
        orb.KeyframeMatcher().update_connections_stats()
    with pytest.raises(orb.JsorbError):
        orb.Covisibility(cc.S, hi + 1)


# ---- the C++ example through the compat shim: ProcessNewKeyFrame, a CorrectLoop-shaped run and a SetBadFlag, checked by the example itself ----
def test_update_connections_example(orb, tmp_path):
    from jetson_slam_amd import build as jb
    exe = jb.build_example("update_connections", str(tmp_path / "update_connections"))
    out = subprocess.run([exe], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.returncode, out.stdout, out.stderr)
