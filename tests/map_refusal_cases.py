"""The refusals of the map-maintenance calls (include/jsorb.h) as calls on the C ABI: both forms of jsorb_local_map_points, jsorb_local_keyframes,
jsorb_update_connections, jsorb_cull_keyframes and jsorb_fuse_map, the single calls jsorb_erase_connections_async, jsorb_connected_mask_async,
jsorb_best_covisibles_async, jsorb_covisibility_copy and jsorb_map_points_scatter_async, the five `_stats` readers and
jsorb_update_connections_scratch before any call.  In the manner of tests/kf_refusal_cases.py: one row per refusing line with the (rc, text) it
answers, rows that violate two consecutive checks at once (the earlier one answers), after every refused call the entry point's smallest valid
call with its outputs and statistics, and valid synchronous calls in which each segment of the copy back is empty in turn (the words no call may
touch stay at the -7 they were set to, so they are absent from the recording).  tests/test_gpu_map_refusals.py holds the loaded library to the
recording in tests/golden/map_call_refusals.json; running this module writes that file with whichever library JSORB_LIBRARY selects.

The shapes are the smallest at which every line is reachable: a graph of 2 slots with 2 pool entries, a table of 2 rows, conn_capacity at the
build's minimum, one candidate, one target and one list point on a 1x1 grid, kf_capacity 84, one extracted 320x240 three-level frame.  Every
pointer a row passes is NULL or a live buffer of the valid call, so a row that is (wrongly) not refused still runs on valid memory; the sizes
that would not are refused by a range check of their own."""
import ctypes as C
import json
import os
import sys

import numpy as np

from kf_refusal_cases import unpack, write  # noqa: F401  (the recording's form is the keyframe matchers')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_call_refusals.json")
WORDS = 2048                 # of the device and of the host output buffer
BIG = 1 << 24
A, S, B = "async", "sync", "both"


class Context:
    """a matcher, an extractor with one frame, the device state of every valid call and its host copy (put back before each valid call)"""

    def __init__(self):
        import torch
        from jetson_slam_amd import orb
        from jetson_slam_amd.synth import synth_stereo_pair
        self.torch, self.orb, self.lib = torch, orb, orb.load_library()
        self.km = orb.KeyframeMatcher(0)
        self.ex = orb.ORBExtractor(240, 320, 1.2, 3, 9, 14, 7, 20, None, 15, 15)
        self.ex.extract(synth_stereo_pair(7, 240, 320)[0])
        self.N = self.ex.n_keypoints(0)
        dev = self.dev = torch.device("cuda:0")
        self.cap_lo, self.cap_hi = orb.covisibility_build_caps()
        self.max_cand = orb.cull_keyframes_build_caps()[0]
        g = self.graph = orb.KeyframeGraph(2, 2, 2, device=dev)
        g.set_keyframe(0, [0], 10)
        g.set_keyframe(1, [0], 11)
        g.set_children(0, [1])
        g.set_parent(1, 0)
        g.set_neighbours(0, [1])
        g.set_neighbours(1, [0])
        t = self.table = orb.MapPointTable(2, device=dev)
        t.floats[2].fill_(2.0)                               # P = (0, 0, 2), Pn = (0, 0, 1), distances 0.1 .. 10
        t.floats[5].fill_(1.0)
        t.floats[6].fill_(10.0)
        t.floats[7].fill_(10.0)
        t.floats[8].fill_(0.1)
        cv = self.cov = orb.Covisibility(2, self.cap_lo, device=dev)
        self.views = orb.KeyframeViews(g, depth=True)
        self.kp = orb.KeyframeKeypoints(g, stereo=True)
        self.kp.x.fill_(160.0)
        self.kp.y.fill_(120.0)
        self.not_erase = torch.zeros(2, dtype=torch.uint8, device=dev)
        self.visible = torch.zeros(2, dtype=torch.int32, device=dev)
        self.cstate = orb.culling_state(g, t)
        self.fstate = orb.fuse_state(g, t)
        self.state = [getattr(g, k) for k in g.ARRAYS] + [t.floats, t.desc, t.bad] + [getattr(cv, k) for k in cv.ARRAYS]
        self.saved = [x.clone() for x in self.state]
        self.out = torch.zeros(WORDS, dtype=torch.int32, device=dev)
        self.host = np.zeros(WORDS, np.int32)
        self.i32 = torch.zeros(max(self.N, 16), dtype=torch.int32, device=dev)           # slot 0, row 0, candidate 0 ...
        self.one = torch.ones(16, dtype=torch.int32, device=dev)                          # ... and candidate / list row 1
        self.frame_row = torch.full((max(self.N, 16),), -1, dtype=torch.int32, device=dev)
        self.rec = np.zeros(1, orb.MAP_POINT_RECORD_DTYPE)
        self.rec["P"], self.rec["Pn"], self.rec["MaxDistance"] = (1, 2, 3), (0, 0, 1), 5
        self.rec_dev = torch.from_numpy(self.rec.view(np.uint8).copy()).to(dev)
        cam, bounds = (100.0, 100.0, 160.0, 120.0), (0.0, 320.0, 0.0, 240.0)
        lsf = float(np.log(np.float32(1.2)))
        eye = np.eye(3, dtype=np.float32)
        self.frustum = orb.make_frustum_params(eye, np.zeros(3), np.zeros(3), cam, (0, 320, 0, 240), 3, lsf)
        self.fuse = orb.make_fuse_params(cam, bounds, (1 / 320.0, 1 / 240.0), lsf, [1.0], cols=1, rows=1)
        self.kf01, self.kf_desc, self.kf_big = np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.array([0, BIG], np.int32)
        self.eye, self.f3, self.i0 = eye.reshape(-1).copy(), np.zeros(3, np.float32), np.zeros(4, np.int32)
        torch.cuda.synchronize()

    def reset(self):
        for x, s in zip(self.state, self.saved):
            x.copy_(s)

    def close(self):
        self.km.close()
        self.ex.close()


def ref(x):
    return None if x is None else C.byref(x)


class Entry:
    """one entry point or pair: the argument names behind the owner (`host`: those only the synchronous form has), the valid call's values,
    the outputs as (name, 32-bit words) - an output named in `host` lies in the host buffer, the others in the device buffer - the words the
    valid call reads from an output (`init`), and the statistics reader"""

    def __init__(self, ctx, name, names, host, base, outputs, owner="matcher", forms=(A, S), init=None, stats=None, extra=None):
        self.ctx, self.name, self.host, self.base, self.outputs, self.owner = ctx, name, host.split(), base, outputs, owner
        self.names = names.split()
        self.forms, self.init, self.stats_fn, self.extra = forms, init or {}, stats, extra
        self.handle = dict(matcher=ctx.km._m, extractor=ctx.ex._h, none=None)[owner]
        self.last_error = dict(matcher=ctx.lib.jsorb_keyframe_matcher_last_error, extractor=ctx.lib.jsorb_last_error, none=None)[owner]
        self.fn = {}
        if A in forms:
            self.fn[False] = getattr(ctx.lib, "jsorb_" + name + ("" if name == "covisibility_copy" or name.endswith("_async") else "_async"))
        if S in forms:
            self.fn[True] = getattr(ctx.lib, "jsorb_" + name)
        self.at, off = {}, {False: 0, True: 0}
        for k, n in outputs:
            h = k in self.host or owner == "none" and name == "covisibility_copy"
            self.at[k] = (h, off[h], n)
            off[h] += (n + 15) // 16 * 16                    # 64-byte steps: the descriptors' alignment
        assert max(off.values()) <= WORDS

    def args(self, sync, over):
        """the valid call's arguments with `over` on top: {"arg": value} or {"arg.field": value} (a copy of the struct with that field)"""
        ctx, v = self.ctx, dict(self.base)
        for k, (h, off, n) in self.at.items():
            v[k] = (ctx.host.ctypes.data if h else ctx.out.data_ptr()) + 4 * off
        for k, x in over.items():
            if "." in k:
                a, f = k.split(".")
                if v[a] is self.base.get(a):
                    v[a] = type(v[a]).from_buffer_copy(v[a])
                setattr(v[a], f, x)
            else:
                v[k] = x
        out = []
        for k in self.names + (self.host if sync else []):
            x = v[k]
            out.append(ref(x) if isinstance(x, C.Structure) else x.ctypes.data if isinstance(x, np.ndarray) else x)
        return out

    def call(self, sync, over, handle="own"):
        h = self.handle if handle == "own" else handle
        head = [] if self.owner == "none" else [h]
        rc = self.fn[sync](*head, *self.args(sync, over))
        return [rc, self.last_error(h).decode() if h is not None and rc != 0 else ""]

    def stats(self, handle="own"):
        """[rc, text], the statistics words (-7: not written)"""
        if self.stats_fn is None:
            return [[0, ""], []]
        h = self.handle if handle == "own" else handle
        rc, words = self.stats_fn(h)
        return [[rc, self.last_error(h).decode() if h is not None and rc != 0 else ""], words]

    def valid(self, sync, over=None):
        """the valid call on the state as it was at the start: [rc, text], every output as (name, words, the words that are not -7), the
        statistics"""
        ctx = self.ctx
        ctx.reset()
        ctx.out.fill_(-7)
        ctx.host[:] = -7
        for k, words in self.init.items():
            h, off, n = self.at[k]
            ctx.out[off:off + len(words)] = ctx.torch.tensor(words, dtype=ctx.torch.int32, device=ctx.dev)
        ctx.torch.cuda.synchronize()
        r = self.call(sync, over or {})
        ctx.km.sync()
        ctx.ex.sync()
        ctx.torch.cuda.synchronize()
        dev = ctx.out.cpu().numpy()
        outs = []
        for k, (h, off, n) in self.at.items():
            a = (ctx.host if h else dev)[off:off + n]
            outs.append([k, n, [[int(i), int(a[i])] for i in np.nonzero(a != -7)[0]]])
        res = dict(call=r, outputs=outs, stats=self.stats())
        if self.extra:
            res["state"] = self.extra()
        return res


def int_stats(fn, n):
    def read(h):
        v = [C.c_int(-7) for _ in range(n)]
        rc = fn(h, *[C.byref(x) for x in v])
        return rc, [x.value for x in v]
    return read


def array_stats(fn, n):
    def read(h):
        v = np.full(n, -7, np.int32)
        rc = fn(h, v.ctypes.data)
        return rc, [int(x) for x in v]
    return read


def entries(ctx):
    lib, N = ctx.lib, ctx.N
    g, t, cv = ctx.graph.struct(), ctx.table.struct(), ctx.cov.struct()
    vs, ks = ctx.views.struct(), ctx.kp.struct()
    i0, one, Cn, nb = ctx.i32.data_ptr(), ctx.one.data_ptr(), ctx.cap_lo, ctx.graph.neighbours.data_ptr()
    nw = (N + 3) // 4
    lm = Entry(ctx, "local_map_points",
               "image table prm n_keyframes kf_start kf_point_row frame_point_row capacity point_row u v invz predicted_level view_cos in_frustum mp_descriptors blocked_in counts_dev",
               "point_row_host counts_host",
               dict(image=0, table=t, prm=ctx.frustum, n_keyframes=1, kf_start=ctx.kf01, kf_point_row=i0, frame_point_row=ctx.frame_row.data_ptr(), capacity=1),
               [("point_row", 1), ("u", 1), ("v", 1), ("invz", 1), ("predicted_level", 1), ("view_cos", 1), ("in_frustum", 1), ("mp_descriptors", 8),
                ("blocked_in", nw), ("counts_dev", 8), ("point_row_host", 2), ("counts_host", 8)],
               owner="extractor", stats=int_stats(lib.jsorb_local_map_stats, 6))
    lk = Entry(ctx, "local_keyframes",
               "graph table frame_point_row n_frame kf_capacity entry_capacity local_kf_slot state_io local_kf_start local_point_row counts_dev",
               "local_kf_slot_host state_host counts_host",
               dict(graph=g, table=t, frame_point_row=i0, n_frame=1, kf_capacity=84, entry_capacity=2),
               [("local_kf_slot", 84), ("state_io", 2), ("local_kf_start", 85), ("local_point_row", 2), ("counts_dev", 8), ("local_kf_slot_host", 84),
                ("state_host", 2), ("counts_host", 8)],
               owner="extractor", init=dict(local_kf_slot=[0] * 84, state_io=[0, -1]), stats=int_stats(lib.jsorb_local_keyframes_stats, 8))

    def scratch():
        a, b = C.c_int(-7), C.c_int(-7)
        rc = lib.jsorb_update_connections_scratch(ctx.km._m, C.byref(a), C.byref(b))
        return [rc, a.value, b.value]

    uc = Entry(ctx, "update_connections", "graph table cov n_update update_slot neighbours parent_out conn_snapshot counts_dev", "parent_host counts_host",
               dict(graph=g, table=t, cov=cv, n_update=1, update_slot=i0, neighbours=nb, conn_snapshot=None),
               [("parent_out", 1), ("counts_dev", 8), ("parent_host", 2), ("counts_host", 8)], stats=int_stats(lib.jsorb_update_connections_stats, 7),
               extra=scratch)
    ck = Entry(ctx, "cull_keyframes",
               "graph table cov views state monocular first_slot n_cand cand_slot max_cull neighbours reparent_cap decision n_mps n_redundant culled_slot reparent_out counts_dev",
               "decision_host n_mps_host n_redundant_host culled_slot_host reparent_host counts_host",
               dict(graph=g, table=t, cov=cv, views=vs, state=ctx.cstate, monocular=0, first_slot=0, n_cand=1, cand_slot=one, max_cull=1, neighbours=nb, reparent_cap=1),
               [("decision", 1), ("n_mps", 1), ("n_redundant", 1), ("culled_slot", 1), ("reparent_out", 2), ("counts_dev", 10), ("decision_host", 1),
                ("n_mps_host", 1), ("n_redundant_host", 1), ("culled_slot_host", 2), ("reparent_host", 2), ("counts_host", 10)],
               stats=array_stats(lib.jsorb_cull_keyframes_stats, 10))
    fm = Entry(ctx, "fuse_map",
               "params replace_loop graph table kp state n_list list_row n_targets target_slot Rcw tcw Ow best_idx best_dist replace_point n_fused log_cap log_out counts_dev",
               "best_idx_host best_dist_host replace_point_host n_fused_host log_host counts_host",
               dict(params=ctx.fuse, replace_loop=0, graph=g, table=t, kp=ks, state=ctx.fstate, n_list=1, list_row=one, n_targets=1, target_slot=ctx.i0, Rcw=ctx.eye,
                    tcw=ctx.f3, Ow=ctx.f3, log_cap=1),
               [("best_idx", 1), ("best_dist", 1), ("replace_point", 1), ("n_fused", 1), ("log_out", 4), ("counts_dev", 10), ("best_idx_host", 1),
                ("best_dist_host", 1), ("replace_point_host", 1), ("n_fused_host", 1), ("log_host", 4), ("counts_host", 10)],
               stats=array_stats(lib.jsorb_fuse_map_stats, 10))
    ec = Entry(ctx, "erase_connections_async", "graph cov slot neighbours counts_dev", "", dict(graph=g, cov=cv, slot=0, neighbours=nb), [("counts_dev", 2)],
               forms=(A,))
    cm = Entry(ctx, "connected_mask_async", "cov slot mask", "", dict(cov=cv, slot=0), [("mask", 1)], forms=(A,))
    bc = Entry(ctx, "best_covisibles_async", "cov n slots N out out_len", "", dict(cov=cv, n=1, slots=i0, N=1), [("out", 1), ("out_len", 1)], forms=(A,))
    cc = Entry(ctx, "covisibility_copy", "cov slot lens conn_slot conn_weight ord_slot ord_weight", "", dict(cov=cv, slot=0),
               [("lens", 2), ("conn_slot", Cn), ("conn_weight", Cn), ("ord_slot", Cn), ("ord_weight", Cn)], owner="none", forms=(A,))
    fl = ctx.table.floats

    def table_row():
        return [int(x) for x in fl[:, 0].cpu().numpy().view(np.int32)] + [int(ctx.table.bad[0])]

    sc = Entry(ctx, "map_points_scatter_async",
               "hip_stream n_rows Px Py Pz Pnx Pny Pnz MaxDistance invariance_maxDistance invariance_minDistance bad n rows records", "",
               dict(dict(zip(ctx.orb.MAP_POINT_FLOATS, [fl[i].data_ptr() for i in range(9)])), hip_stream=None, n_rows=2, bad=ctx.table.bad.data_ptr(), n=1, rows=i0,
                    records=ctx.rec_dev.data_ptr()), [], owner="none", forms=(A,), extra=table_row)
    return dict(local_map_points=lm, local_keyframes=lk, update_connections=uc, cull_keyframes=ck, fuse_map=fm, erase_connections_async=ec,
                connected_mask_async=cm, best_covisibles_async=bc, covisibility_copy=cc, map_points_scatter_async=sc)


PAIRS = ["local_map_points", "local_keyframes", "update_connections", "cull_keyframes", "fuse_map"]


def covis_chain(ctx, form=B):
    """covis_check's lines, shared by four entry points"""
    return [("cov_null", {"cov": None}, form), ("cov_slots_neg", {"cov.max_keyframes": -1}, form), ("cov_slots", {"cov.max_keyframes": BIG}, form),
            ("conn_capacity", {"cov.conn_capacity": ctx.cap_lo - 1}, form), ("cov_array_null", {"cov.ord_weight": None}, form)]


def chains(ctx):
    """per entry point: the asynchronous form's checks in the order they fire, the synchronous form's own checks in front of them, further rows
    of the same lines, and pairs of consecutive checks given by hand.  A check: (name, the overrides that violate it, the forms that reach
    it); a pair names the row whose answer it must repeat.  edge: valid synchronous calls with one segment of the copy back empty."""
    odd = ctx.out.data_ptr() + 4 * 16 * 7 + 1                # inside the device buffer, not 16-byte aligned
    live = ctx.not_erase.data_ptr()
    snap = ctx.orb.JsorbConnSnapshot(None, ctx.out.data_ptr(), ctx.out.data_ptr())
    lm = dict(
        sync=[("host_null", {"counts_host": None}), ("capacity", {"capacity": -1})],
        chain=[("image", {"image": 5}, B), ("null", {"table": None}, B), ("negative", {"n_keyframes": -1}, B), ("table_null", {"table.Pz": None}, B),
               ("kf_null", {"kf_start": None}, B), ("kf_order", {"kf_start": ctx.kf_desc}, B), ("entries", {"kf_start": ctx.kf_big}, B),
               ("entry_null", {"kf_point_row": None}, B), ("out_null", {"u": None}, B), ("align", {"mp_descriptors": odd}, B)],
        more=[("image_neg", {"image": -1}, B), ("prm_null", {"prm": None}, B), ("counts_dev_null", {"counts_dev": None}, A), ("n_rows_neg", {"table.n_rows": -1}, B),
              ("capacity_neg", {"capacity": -1}, A), ("table_bad_null", {"table.bad": None}, B), ("kf_start_neg", {"kf_start": np.array([-1, 0], np.int32)}, B),
              ("point_row_null", {"point_row": None}, A), ("mp_descriptors_null", {"mp_descriptors": None}, B), ("align_table", {"table.desc": odd}, B),
              ("host_rows_null", {"point_row_host": None}, S)],
        pairs=[("n_rows_neg+table_null", {"table.n_rows": -1, "table.Pz": None}, "n_rows_neg", B)],
        edge=[("capacity_0", {"capacity": 0}), ("n_keyframes_0", {"n_keyframes": 0})])
    lk = dict(
        sync=[("host_null", {"counts_host": None})],
        chain=[("null", {"graph": None}, B), ("negative", {"n_frame": -1}, B), ("slots", {"graph.max_keyframes": BIG}, B), ("kf_capacity", {"kf_capacity": 83}, B),
               ("entries", {"entry_capacity": BIG}, B), ("graph_null", {"graph.state": None}, B), ("table_null", {"table.bad": None}, B),
               ("rows_null", {"local_point_row": None}, B)],
        more=[("table_arg_null", {"table": None}, B), ("slot_out_null", {"local_kf_slot": None}, B), ("state_io_null", {"state_io": None}, B),
              ("start_null", {"local_kf_start": None}, B), ("counts_dev_null", {"counts_dev": None}, B), ("slots_neg", {"graph.max_keyframes": -1}, B),
              ("pool_neg", {"graph.pool_entries": -1}, B), ("child_neg", {"graph.child_entries": -1}, B), ("n_rows_neg", {"table.n_rows": -1}, B),
              ("entry_capacity_neg", {"entry_capacity": -1}, B), ("child_pool_null", {"graph.child_pool": None}, B), ("point_pool_null", {"graph.point_pool": None}, B),
              ("host_slot_null", {"local_kf_slot_host": None}, S), ("host_state_null", {"state_host": None}, S)],
        pairs=[],
        edge=[("entry_capacity_0", {"entry_capacity": 0}), ("no_frame", {"frame_point_row": None})])
    uc = dict(
        sync=[("host_null", {"counts_host": None})],
        chain=[("null", {"graph": None}, B)] + covis_chain(ctx) +
              [("differ", {"graph.max_keyframes": 1}, B), ("negative", {"table.n_rows": -1}, B), ("n_update", {"n_update": 33}, B), ("update_null", {"update_slot": None}, B),
               ("graph_null", {"graph.order_key": None}, B), ("table_null", {"table.bad": None}, B), ("snapshot", {"conn_snapshot": snap}, B)],
        more=[("table_arg_null", {"table": None}, B), ("counts_dev_null", {"counts_dev": None}, B), ("conn_capacity_hi", {"cov.conn_capacity": ctx.cap_hi + 1}, B),
              ("first_connection_null", {"cov.first_connection": None}, B), ("pool_neg", {"graph.pool_entries": -1}, B), ("n_update_neg", {"n_update": -1}, B),
              ("point_pool_null", {"graph.point_pool": None}, B), ("host_parent_null", {"parent_host": None}, S)],
        pairs=[("cov_slots_neg+conn_capacity", {"cov.max_keyframes": -1, "cov.conn_capacity": 0}, "cov_slots_neg", B)],
        edge=[("n_update_0", {"n_update": 0}), ("no_parent_out", {"parent_out": None, "parent_host": None})])
    ck = dict(
        sync=[("host_null", {"counts_host": None})],
        chain=[("null", {"views": None}, B), ("negative", {"table.n_rows": -1}, B), ("slots", {"graph.max_keyframes": BIG}, B), ("differ", {"cov.max_keyframes": 1}, B),
               ("conn_capacity", {"cov.conn_capacity": ctx.cap_lo - 1}, B), ("cov_array_null", {"cov.ord_weight": None}, B), ("max_cull", {"max_cull": 17}, B),
               ("n_cand", {"n_cand": ctx.max_cand + 1}, B), ("cand_null", {"cand_slot": None}, B), ("culled_null", {"culled_slot": None}, B),
               ("reparent", {"reparent_cap": -1}, B), ("first_slot", {"first_slot": 2}, B), ("graph_null", {"graph.order_key": None}, B),
               ("registered_null", {"graph.registered": None}, B), ("table_null", {"table.bad": None}, B), ("views_differ", {"views.pool_entries": 1}, B),
               ("views_null", {"views.octave": None}, B), ("depth_null", {"views.depth": None}, B), ("state_differs", {"state.parent": None}, B),
               ("not_erase", {"state.not_erase": live}, B)],
        more=[("graph_arg_null", {"graph": None}, B), ("cov_null", {"cov": None}, B), ("state_null", {"state": None}, B), ("counts_dev_null", {"counts_dev": None}, B),
              ("slots_neg", {"graph.max_keyframes": -1}, B), ("pool_neg", {"graph.pool_entries": -1}, B), ("conn_capacity_hi", {"cov.conn_capacity": ctx.cap_hi + 1}, B),
              ("max_cull_0", {"max_cull": 0}, B), ("n_cand_neg", {"n_cand": -1}, B), ("decision_null", {"decision": None}, B), ("n_mps_null", {"n_mps": None}, B),
              ("reparent_big", {"reparent_cap": BIG}, B), ("reparent_null", {"reparent_out": None}, B), ("first_slot_neg", {"first_slot": -2}, B),
              ("th_depth_null", {"views.th_depth": None}, B), ("state_bad_differs", {"state.bad": None}, B), ("host_culled_null", {"culled_slot_host": None}, S),
              ("host_decision_null", {"decision_host": None}, S), ("host_reparent_null", {"reparent_host": None}, S)],
        pairs=[],
        edge=[("n_cand_0_reparent_0", {"n_cand": 0, "reparent_cap": 0}), ("first_connection_null", {"cov.first_connection": None}),
              ("monocular_without_depth", {"monocular": 1, "views.depth": None, "views.th_depth": None})])
    fm = dict(
        sync=[("sizes", {"n_targets": -1}), ("host_null", {"counts_host": None})],
        chain=[("null", {"kp": None}, B), ("n_levels", {"params.n_levels": 0}, B), ("th_low", {"params.th_low": 256}, B), ("grid", {"params.cols": 65, "params.rows": 64}, B),
               ("negative", {"table.n_rows": -1}, B), ("n_targets", {"n_targets": 257}, B), ("log_cap", {"log_cap": 1 << 27}, B), ("kp_differ", {"kp.pool_entries": 1}, B),
               ("pairs", {"n_targets": 256, "n_list": 1 << 23}, B), ("graph_null", {"graph.order_key": None}, B), ("registered_null", {"graph.registered": None}, B),
               ("kp_null", {"kp.octave": None}, B), ("table_null", {"table.Pnz": None}, B), ("align", {"kp.desc": odd}, B), ("state_differs", {"state.point_pool": None}, B),
               ("visible", {"state.visible": ctx.visible.data_ptr()}, B), ("list_null", {"list_row": None}, B), ("target_null", {"Rcw": None}, B),
               ("best_null", {"best_dist": None}, B), ("replace_null", {"params.check_reprojection": 0, "replace_point": None}, B), ("log_null", {"log_out": None}, B)],
        more=[("params_null", {"params": None}, B), ("state_null", {"state": None}, B), ("counts_dev_null", {"counts_dev": None}, B), ("n_levels_17", {"params.n_levels": 17}, B),
              ("th_low_neg", {"params.th_low": -1}, B), ("grid_zero", {"params.rows": 0}, B), ("slots_neg", {"graph.max_keyframes": -1}, B),
              ("n_list_neg", {"n_list": -1}, B), ("log_cap_neg", {"log_cap": -1}, B), ("n_targets_neg", {"n_targets": -1}, A),
              ("align_table", {"table.desc": odd}, B), ("state_desc_differs", {"state.desc": None}, B), ("found", {"state.found": ctx.visible.data_ptr()}, B),
              ("target_slot_null", {"target_slot": None}, B), ("n_fused_null", {"n_fused": None}, B), ("best_idx_null", {"best_idx": None}, B),
              ("host_fused_null", {"n_fused_host": None}, S), ("host_best_null", {"best_idx_host": None}, S), ("host_replace_null", {"replace_point_host": None}, S),
              ("host_log_null", {"log_host": None}, S)],
        pairs=[],
        edge=[("n_targets_0", {"n_targets": 0}), ("n_list_0", {"n_list": 0}), ("log_cap_0", {"log_cap": 0}), ("no_replace_point", {"replace_point": None})])
    ec = dict(sync=[], chain=[("null", {"graph": None}, A)] + covis_chain(ctx, A) +
              [("differ", {"graph.max_keyframes": 1}, A), ("slot", {"slot": 2}, A), ("graph_null", {"graph.order_key": None}, A)],
              more=[("counts_dev_null", {"counts_dev": None}, A), ("slot_neg", {"slot": -1}, A), ("first_connection_null", {"cov.first_connection": None}, A)],
              pairs=[], edge=[])
    cm = dict(sync=[], chain=covis_chain(ctx, A) + [("slot", {"slot": 2}, A), ("mask_null", {"mask": None}, A)], more=[("slot_neg", {"slot": -1}, A)], pairs=[], edge=[])
    bc = dict(sync=[], chain=covis_chain(ctx, A) + [("sizes", {"N": 0}, A), ("slots_null", {"slots": None}, A)],
              more=[("n_neg", {"n": -1}, A), ("n_x_N", {"n": 1 << 16, "N": 1 << 15}, A), ("out_null", {"out": None}, A)], pairs=[],
              edge=[("n_0", {"n": 0})])
    cc = dict(sync=[], chain=[("cov_null", {"cov": None}, A)],
              more=[("lens_null", {"lens": None}, A), ("slot_neg", {"slot": -1}, A), ("slot", {"slot": 2}, A), ("conn_capacity_0", {"cov.conn_capacity": 0}, A),
                    ("conn_len_null", {"cov.conn_len": None}, A), ("ord_weight_null", {"cov.ord_weight": None}, A)], pairs=[],
              edge=[("lens_only", {"conn_slot": None, "conn_weight": None, "ord_slot": None, "ord_weight": None})])
    sc = dict(sync=[], chain=[("n_neg", {"n": -1}, A), ("rows_null", {"rows": None}, A), ("float_null", {"Pnz": None}, A)],
              more=[("n_rows_neg", {"n_rows": -1}, A), ("records_null", {"records": None}, A), ("bad_null", {"bad": None}, A)], pairs=[],
              edge=[("n_0", {"n": 0, "rows": None, "records": None})])
    return dict(local_map_points=lm, local_keyframes=lk, update_connections=uc, cull_keyframes=ck, fuse_map=fm, erase_connections_async=ec,
                connected_mask_async=cm, best_covisibles_async=bc, covisibility_copy=cc, map_points_scatter_async=sc)


def rows_of(spec, forms):
    """(row name, synchronous form?, overrides, the row whose answer it must repeat or None) in the order they run"""
    out = []
    for sync in (False, True):
        form = S if sync else A
        if form not in forms:
            continue
        chain = ([(n, o) for n, o in spec["sync"]] if sync else []) + [(n, o) for n, o, f in spec["chain"] if f in (B, form)]
        for n, o in chain:
            out.append(("%s/%s" % (form, n), sync, o, None))
        for (n1, o1), (n2, o2) in zip(chain, chain[1:]):
            if set(o1) & set(o2) or any(k.split(".")[0] in o2 for k in o1) or any(k.split(".")[0] in o1 for k in o2):
                continue                                     # the two violations need the same argument (or one replaces the other's struct)
            out.append(("%s/%s+%s" % (form, n1, n2), sync, dict(o1, **o2), "%s/%s" % (form, n1)))
        for n, o, f in spec["more"]:
            if f in (B, form):
                out.append(("%s/%s" % (form, n), sync, o, None))
        for n, o, same, f in spec["pairs"]:
            if f in (B, form):
                out.append(("%s/%s" % (form, n), sync, o, "%s/%s" % (form, same)))
    return out


def run(ctx=None, strict=True):
    """every row's answer and the valid call after it: {entry point: {row: {"refusal": [rc, text], "same_as": row or None, "form": "async" /
    "sync", "after": valid()}}}; the edge calls are rows whose "refusal" is the accepted call's [0, ""] and whose "after" is its own result"""
    own = ctx is None
    ctx = ctx or Context()
    try:
        result, accepted = {}, []
        E, CH = entries(ctx), chains(ctx)
        before = {name: e.stats()[0] for name, e in E.items() if e.stats_fn}            # before any call on the two owners
        before["update_connections_scratch"] = [ctx.lib.jsorb_update_connections_scratch(ctx.km._m, None, None),
                                                ctx.lib.jsorb_keyframe_matcher_last_error(ctx.km._m).decode()]
        for name, e in E.items():
            rec = result[name] = {}
            first = A if A in e.forms else S
            if e.stats_fn:
                rec["stats/before"] = dict(refusal=before[name], same_as=None, form=first, after=e.valid(first == S))
                rec["stats/null_owner"] = dict(refusal=e.stats(handle=None)[0], same_as=None, form=e.forms[-1], after=e.valid(e.forms[-1] == S))
            if name == "update_connections":
                rec["scratch/before"] = dict(refusal=before["update_connections_scratch"], same_as=None, form=A, after=e.valid(False))
                rec["scratch/null_owner"] = dict(refusal=[ctx.lib.jsorb_update_connections_scratch(None, None, None), ""], same_as=None, form=A, after=e.valid(False))
            if name in ("cull_keyframes", "fuse_map"):
                fn = getattr(ctx.lib, "jsorb_%s_stats" % name)
                rec["stats/counts_null"] = dict(refusal=[fn(e.handle, None), e.last_error(e.handle).decode()], same_as=None, form=A, after=e.valid(False))
            for form in e.forms:
                if e.owner != "none":
                    rec["%s/null_owner" % form] = dict(refusal=e.call(form == S, {}, handle=None), same_as=None, form=form, after=e.valid(form == S))
            for row, sync, over, same in rows_of(CH[name], e.forms):
                r = e.call(sync, over)
                if r[0] == 0:
                    accepted.append("%s %s" % (name, row))
                rec[row] = dict(refusal=r, same_as=same, form=S if sync else A, after=e.valid(sync))
            for row, over in CH[name]["edge"]:
                form = e.forms[-1]
                got = e.valid(form == S, over)
                rec["edge/" + row] = dict(refusal=got["call"], same_as=None, form=form, after=got)
        if accepted and strict:
            raise AssertionError("not refused: " + ", ".join(accepted))
        if accepted:
            print("NOT REFUSED: " + ", ".join(accepted))
        return result
    finally:
        if own:
            ctx.close()


def pack(result):
    """the recording's form: an entry point's valid result once per form under "valid"; a row carries an "after" of its own only where it differs"""
    out = {}
    for name, rows in result.items():
        valid = {form: next((r["after"] for k, r in rows.items() if r["form"] == form and not k.startswith("edge/")), None) for form in (A, S)}
        packed = {}
        for row, r in rows.items():
            q = dict(refusal=r["refusal"], same_as=r["same_as"], form=r["form"])
            if r["after"] != valid[r["form"]]:
                q["after"] = r["after"]
            packed[row] = q
        out[name] = dict(valid=valid, rows=packed)
    return out


if __name__ == "__main__":
    # map_refusal_cases.py [file]: writes the recording (a GPU; JSORB_LIBRARY selects the build that answers)
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (behind PYTHONPATH: another orb.py there wins)
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = pack(json.loads(json.dumps(run(strict=False))))
    write(rec, path)
    print("%d rows" % sum(len(v["rows"]) for v in rec.values()))
