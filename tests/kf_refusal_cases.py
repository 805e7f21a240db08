"""The refusals of the five keyframe-set entry-point pairs and their `_stats` readers (jsorb_search_by_bow, jsorb_search_for_triangulation,
jsorb_fuse, jsorb_search_by_bow_kf, jsorb_search_by_sim3; include/jsorb.h), as calls on the C ABI: one row per refusing line with the
(rc, text) it answers, rows that violate two consecutive checks at once (the earlier one answers), and after every refused call the entry
point's valid call at n1 = 1 against one keyframe of one keypoint.  tests/test_gpu_kf_refusals.py holds the loaded library to the recording in
tests/golden/kf_matcher_refusals.json; running this module writes that file with whichever library JSORB_LIBRARY selects and whichever orb.py
is on the path (recorded once, with a build of the commit before the entry points' frames were shared).

Every pointer a row passes is NULL or a live buffer of the valid call, so a row that is (wrongly) not refused still runs on valid memory; the
sizes that would not are refused by a range check of their own."""
import ctypes as C
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kf_matcher_refusals.json")
BIG = 1 << 18


class Context:
    """a matcher, one extracted 320x240 frame and the buffers of every entry point's valid call"""

    def __init__(self):
        import torch
        from jetson_slam_amd import orb
        from jetson_slam_amd.synth import synth_stereo_pair
        self.orb, self.lib = orb, orb.load_library()
        self.km = orb.KeyframeMatcher(0)
        self.ex = orb.ORBExtractor(240, 320, 1.2, 3, 9, 14, 7, 20, None, 15, 15)
        self.ex.extract(synth_stereo_pair(7, 240, 320)[0])
        self.N = self.ex.n_keypoints(0)
        dev = torch.device("cuda:0")
        f = lambda v: torch.full((16,), v, dtype=torch.float32, device=dev)
        self.t = dict(zero=f(0.0), one=f(1.0), ten=f(10.0), cx=f(160.0), cy=f(120.0), i0=torch.zeros(max(self.N, 16), dtype=torch.int32, device=dev),
                      u1=torch.ones(16, dtype=torch.uint8, device=dev), desc=torch.zeros(64, dtype=torch.uint8, device=dev),
                      out=torch.zeros(4 * max(self.N, 16) + 64, dtype=torch.int32, device=dev))
        self.p = {k: v.data_ptr() for k, v in self.t.items()}
        assert self.p["desc"] % 16 == 0
        self.kf01 = np.array([0, 1], np.int32)
        self.kf_desc = np.array([1, 0], np.int32)            # not ascending
        self.kf_long = np.array([0, BIG], np.int32)          # a keyframe of 2^18 keypoints
        self.kf012 = np.array([0, 1, 2], np.int32)
        self.F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)      # a translation along x: the epipolar line of (x, y) is the row y
        self.f3 = np.zeros(3, np.float32)
        self.eye = np.eye(3, dtype=np.float32).reshape(-1)
        cam, bounds, grid = (100.0, 100.0, 160.0, 120.0), (0.0, 320.0, 0.0, 240.0), (64 / 320.0, 48 / 240.0)
        lsf = float(np.log(np.float32(1.2)))
        self.tri = orb.make_triangulation_params([1.0], th_low=50, check_orientation=True)
        self.fuse = orb.make_fuse_params(cam, bounds, grid, lsf, [1.0])
        self.bow = orb.make_bow_params()
        self.sim3 = orb.make_sim3_params(cam, bounds, grid, lsf, [1.0])
        self.host = np.zeros(4 * max(self.N, 16) + 64, np.int32)
        self.hp = self.host.ctypes.data

    def variant(self, params, **fields):
        q = type(params).from_buffer_copy(params)
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    def side(self, **fields):
        p = self.p
        s = self.orb.JsorbSim3Side(1)
        for k, v in dict(x=p["cx"], y=p["cy"], octave=p["i0"], kp_desc=p["desc"], Px=p["zero"], Py=p["zero"], Pz=p["one"], max_distance=p["ten"],
                         min_dist_inv=p["zero"], max_dist_inv=p["ten"], mp_desc=p["desc"], search=p["u1"]).items():
            setattr(s, k, v)
        s.Rw = (C.c_float * 9)(*self.eye.tolist())
        s.sR = (C.c_float * 9)(*self.eye.tolist())
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    def close(self):
        self.km.close()
        self.ex.close()


def ref(x):
    return None if x is None else C.byref(x)


class Entry:
    """one entry-point pair: the argument names behind the handle, the valid call's values, where the outputs go and how they are read"""

    def __init__(self, ctx, name, names, base, outputs, n_stats, on_extractor=False):
        self.ctx, self.name, self.names, self.base, self.outputs, self.n_stats = ctx, name, names.split(), base, outputs, n_stats
        self.handle = ctx.ex._h if on_extractor else ctx.km._m
        self.last_error = ctx.lib.jsorb_last_error if on_extractor else ctx.lib.jsorb_keyframe_matcher_last_error
        stats = dict(search_by_bow="jsorb_search_by_bow_stats", search_for_triangulation="jsorb_search_for_triangulation_stats", fuse="jsorb_fuse_stats",
                     search_by_bow_kf="jsorb_search_by_bow_kf_stats", search_by_sim3="jsorb_search_by_sim3_stats")[name]
        self.fn = {False: getattr(ctx.lib, "jsorb_%s_async" % name), True: getattr(ctx.lib, "jsorb_" + name)}
        self.stats_fn = getattr(ctx.lib, stats)

    def args(self, sync, over):
        """the valid call's arguments with `over` on top; the outputs are device words (asynchronous form) or host words (synchronous form)"""
        v = dict(self.base)
        off = 0
        for k, n in self.outputs:
            v[k] = (self.ctx.hp if sync else self.ctx.p["out"]) + 4 * off
            off += n
        v.update(over)
        out = []
        for k in self.names:
            x = v[k]
            out.append(ref(x) if isinstance(x, C.Structure) else x.ctypes.data if isinstance(x, np.ndarray) else x)
        return out

    def call(self, sync, over, handle="own"):
        h = self.handle if handle == "own" else handle
        fn = self.fn[sync]
        args = [C.cast(x, t) if isinstance(x, int) and t is C.POINTER(C.c_int) else x for x, t in zip(self.args(sync, over), fn.argtypes[1:])]
        rc = fn(h, *args)
        return [rc, self.last_error(h).decode() if h is not None and rc != 0 else ""]

    def stats(self, handle="own"):
        h = self.handle if handle == "own" else handle
        v = [C.c_int(-7) for _ in range(self.n_stats)]
        bins = (C.c_int * 3)(-7, -7, -7)
        tail = [bins] if self.name not in ("fuse", "search_by_sim3") else []
        rc = self.stats_fn(h, *[C.byref(x) for x in v], *tail)
        return [rc, self.last_error(h).decode() if h is not None and rc != 0 else ""], [x.value for x in v] + (list(bins) if tail else [])

    def valid(self, sync):
        """the valid call: [rc, text], every output as (length, the entries that are not -1), the statistics"""
        import torch
        ctx = self.ctx
        ctx.t["out"].fill_(-7)
        ctx.host[:] = -7
        torch.cuda.synchronize()
        r = self.call(sync, {})
        if not sync:
            ctx.km.sync()
            torch.cuda.synchronize()
        words = ctx.host if sync else ctx.t["out"].cpu().numpy()
        outs, off = [], 0
        for k, n in self.outputs:
            a = words[off:off + n]
            outs.append([k, n, [[int(i), int(a[i])] for i in np.nonzero(a != -1)[0]]])
            off += n
        return dict(call=r, outputs=outs, stats=self.stats())


def entries(ctx):
    p, N = ctx.p, ctx.N
    kf1 = dict(n1=1, node1=p["i0"], free1=p["u1"], stereo1=p["u1"], x1=p["cx"], y1=p["cy"], angle1=p["zero"], desc1=p["desc"])
    tri = Entry(ctx, "search_for_triangulation",
                "params n1 node1 free1 stereo1 x1 y1 angle1 desc1 n_keyframes kf_start node2 free2 stereo2 x2 y2 octave2 angle2 desc2 F12 epipole match12 n_matches",
                dict(kf1, params=ctx.tri, n_keyframes=1, kf_start=ctx.kf01, node2=p["i0"], free2=p["u1"], stereo2=p["u1"], x2=p["cx"], y2=p["cy"],
                     octave2=p["i0"], angle2=p["zero"], desc2=p["desc"], F12=ctx.F12, epipole=ctx.f3), [("n_matches", 1), ("match12", 1)], 4)
    fuse = Entry(ctx, "fuse",
                 "params n_points Px Py Pz Nx Ny Nz max_distance min_dist_inv max_dist_inv desc n_keyframes kf_start x y octave uright kf_desc Rcw tcw Ow skip best_idx best_dist n_matched",
                 dict(params=ctx.fuse, n_points=1, Px=p["zero"], Py=p["zero"], Pz=p["one"], Nx=p["zero"], Ny=p["zero"], Nz=p["one"], max_distance=p["ten"],
                      min_dist_inv=p["zero"], max_dist_inv=p["ten"], desc=p["desc"], n_keyframes=1, kf_start=ctx.kf01, x=p["cx"], y=p["cy"], octave=p["i0"],
                      uright=None, kf_desc=p["desc"], Rcw=ctx.eye, tcw=ctx.f3, Ow=ctx.f3, skip=None), [("n_matched", 1), ("best_idx", 1), ("best_dist", 1)], 4)
    bowkf = Entry(ctx, "search_by_bow_kf", "params n1 node1 valid1 angle1 desc1 n_keyframes kf_start node2 valid2 angle2 desc2 match12 n_matches",
                  dict(params=ctx.bow, n1=1, node1=p["i0"], valid1=p["u1"], angle1=p["zero"], desc1=p["desc"], n_keyframes=1, kf_start=ctx.kf01,
                       node2=p["i0"], valid2=p["u1"], angle2=p["zero"], desc2=p["desc"]), [("n_matches", 1), ("match12", 1)], 3)
    s1, s2 = ctx.side(), ctx.side()
    sim3 = Entry(ctx, "search_by_sim3", "params side1 side2 match1 match2 match12 n_found", dict(params=ctx.sim3, side1=s1, side2=s2),
                 [("n_found", 1), ("match1", 1), ("match2", 1), ("match12", 1)], 5)
    # the frame against one keyframe that holds the frame's own first keypoint: every frame keypoint in node 0
    bow = Entry(ctx, "search_by_bow", "image params f_node n_keyframes kf_start kf_node kf_valid kf_angle kf_descriptors match_kf n_matches",
                dict(image=0, params=ctx.bow, f_node=p["i0"], n_keyframes=1, kf_start=ctx.kf01, kf_node=p["i0"], kf_valid=p["u1"], kf_angle=p["zero"],
                     kf_descriptors=ctx.lib.jsorb_descriptors_device(ctx.ex._h, 0)), [("n_matches", 1), ("match_kf", N)], 3, on_extractor=True)
    return dict(search_for_triangulation=tri, fuse=fuse, search_by_bow_kf=bowkf, search_by_sim3=sim3, search_by_bow=bow)


def chains(ctx):
    """per entry point: the asynchronous form's checks in the order they fire, the synchronous form's own checks in front of them, further
    rows of the same lines, and the pairs of consecutive checks that only ONE argument (or one parameter struct) can violate together.  A check:
    (name, the overrides that violate it, the forms it can be reached in); a pair names the row whose answer it must repeat."""
    p, odd = ctx.p, ctx.p["desc"] + 1
    A, S, B = "async", "sync", "both"
    tri = dict(
        sync=[("n_keyframes", dict(n_keyframes=257)), ("n1", dict(n1=BIG)), ("host_null", dict(n_matches=None))],
        chain=[("params_null", dict(params=None), B), ("n_levels", dict(params=ctx.variant(ctx.tri, n_levels=0)), B), ("n_keyframes", dict(n_keyframes=257), A),
               ("n1", dict(n1=BIG), A), ("kf_null", dict(kf_start=None), B), ("kf_order", dict(kf_start=ctx.kf_desc), B), ("kf1_null", dict(x1=None), B),
               ("kf2_null", dict(octave2=None), B), ("align", dict(desc1=odd), B), ("match_null", dict(match12=None), A)],
        more=[("n_levels_17", dict(params=ctx.variant(ctx.tri, n_levels=17)), B), ("n_keyframes_neg", dict(n_keyframes=-1), B), ("n1_neg", dict(n1=-1), B),
              ("F12_null", dict(F12=None), B), ("epipole_null", dict(epipole=None), B), ("n_matches_null", dict(n_matches=None), A),
              ("kf_long_is_invalid", dict(kf_start=ctx.kf_long), B), ("align2", dict(desc2=odd), B), ("host_match_null", dict(match12=None), S)],
        pairs=[("kf_null+kf_order", dict(n_matches=None, kf_start=ctx.kf_desc), "kf_null", A)])
    fuse = dict(
        sync=[("n_keyframes", dict(n_keyframes=257)), ("n_points", dict(n_points=-1)), ("host_null", dict(n_matched=None)),
              ("rows", dict(n_points=2 ** 31 - 1, n_keyframes=2, kf_start=ctx.kf012))],
        chain=[("params_null", dict(params=None), B), ("n_levels", dict(params=ctx.variant(ctx.fuse, n_levels=0)), B),
               ("th_low", dict(params=ctx.variant(ctx.fuse, th_low=256)), B), ("grid", dict(params=ctx.variant(ctx.fuse, cols=65, rows=64)), B),
               ("n_keyframes", dict(n_keyframes=257), A), ("n_points", dict(n_points=-1), A), ("kf_null", dict(kf_start=None), B),
               ("kf_order", dict(kf_start=ctx.kf_desc), B), ("total", dict(n_keyframes=2, kf_start=np.array([0, BIG // 2, BIG], np.int32)), B),
               ("rows", dict(n_points=2 ** 31 - 1, n_keyframes=2, kf_start=ctx.kf012), A), ("point_null", dict(Nz=None), B), ("kf_array_null", dict(octave=None), B),
               ("align", dict(desc=odd), B), ("best_null", dict(best_dist=None), A)],
        more=[("n_levels_17", dict(params=ctx.variant(ctx.fuse, n_levels=17)), B), ("th_low_neg", dict(params=ctx.variant(ctx.fuse, th_low=-1)), B),
              ("grid_zero", dict(params=ctx.variant(ctx.fuse, cols=0)), B), ("n_keyframes_neg", dict(n_keyframes=-1), B), ("Rcw_null", dict(Rcw=None), B),
              ("tcw_null", dict(tcw=None), B), ("Ow_null", dict(Ow=None), B), ("n_matched_null", dict(n_matched=None), A),
              ("kf_long_is_invalid", dict(kf_start=ctx.kf_long), B), ("align2", dict(kf_desc=odd), B), ("best_idx_null", dict(best_idx=None), A),
              ("host_best_null", dict(best_idx=None), S)],
        pairs=[("n_levels+th_low", dict(params=ctx.variant(ctx.fuse, n_levels=0, th_low=256)), "n_levels", B),
               ("th_low+grid", dict(params=ctx.variant(ctx.fuse, th_low=256, cols=65, rows=64)), "th_low", B),
               ("kf_null+kf_order", dict(n_matched=None, kf_start=ctx.kf_desc), "kf_null", A),
               ("total+rows", dict(n_points=2 ** 31 - 1, n_keyframes=2, kf_start=np.array([0, BIG // 2, BIG], np.int32)), "total", A)])
    bowkf = dict(
        sync=[("n_keyframes", dict(n_keyframes=257)), ("n1", dict(n1=BIG)), ("host_null", dict(n_matches=None))],
        chain=[("params_null", dict(params=None), B), ("n_keyframes", dict(n_keyframes=257), A), ("n1", dict(n1=BIG), A), ("kf_null", dict(kf_start=None), B),
               ("kf_order", dict(kf_start=ctx.kf_desc), B), ("kf1_null", dict(angle1=None), B), ("cand_null", dict(valid2=None), B), ("align", dict(desc1=odd), B),
               ("match_null", dict(match12=None), A)],
        more=[("n_keyframes_neg", dict(n_keyframes=-1), B), ("n1_neg", dict(n1=-1), B), ("n_matches_null", dict(n_matches=None), A),
              ("kf_long_is_invalid", dict(kf_start=ctx.kf_long), B), ("align2", dict(desc2=odd), B), ("host_match_null", dict(match12=None), S)],
        pairs=[("kf_null+kf_order", dict(n_matches=None, kf_start=ctx.kf_desc), "kf_null", A)])
    bow = dict(
        sync=[("image", dict(image=5)), ("n_keyframes", dict(n_keyframes=257)), ("host_null", dict(n_matches=None))],
        chain=[("image", dict(image=5), A), ("params_null", dict(params=None), B), ("n_keyframes", dict(n_keyframes=257), A), ("kf_null", dict(kf_start=None), B),
               ("kf_order", dict(kf_start=ctx.kf_desc), B), ("kf_array_null", dict(kf_angle=None), B), ("align", dict(kf_descriptors=odd), B),
               ("match_null", dict(match_kf=None), A), ("f_node_null", dict(f_node=None), B)],
        more=[("image_neg", dict(image=-1), B), ("n_keyframes_neg", dict(n_keyframes=-1), B), ("n_matches_null", dict(n_matches=None), A),
              ("kf_long_is_unsupported", dict(kf_start=ctx.kf_long), B), ("host_match_null", dict(match_kf=None), S),
              ("image_before_n_keyframes", dict(image=5, n_keyframes=257), S)],
        pairs=[("kf_null+kf_order", dict(n_matches=None, kf_start=ctx.kf_desc), "kf_null", A)])
    sim3 = dict(
        sync=[],
        chain=[("params_null", dict(params=None), B), ("n_levels", dict(params=ctx.variant(ctx.sim3, n_levels=0)), B),
               ("th_high", dict(params=ctx.variant(ctx.sim3, th_high=256)), B), ("grid", dict(params=ctx.variant(ctx.sim3, cols=65, rows=64)), B),
               ("n_range", dict(side1=ctx.side(n=BIG)), B), ("side_null", dict(side1=ctx.side(Pz=None)), B), ("align", dict(side2=ctx.side(mp_desc=odd)), B),
               ("out_null", dict(n_found=None), B)],
        more=[("side1_null", dict(side1=None), B), ("side2_null", dict(side2=None), B), ("n_levels_17", dict(params=ctx.variant(ctx.sim3, n_levels=17)), B),
              ("th_high_neg", dict(params=ctx.variant(ctx.sim3, th_high=-1)), B), ("grid_zero", dict(params=ctx.variant(ctx.sim3, rows=0)), B),
              ("n_neg", dict(side2=ctx.side(n=-1)), B), ("side2_array_null", dict(side2=ctx.side(search=None)), B),
              ("align_kp", dict(side1=ctx.side(kp_desc=odd)), B), ("side1_null_before_align2", dict(side1=ctx.side(x=None), side2=ctx.side(kp_desc=odd)), B),
              ("match1_null", dict(match1=None), A), ("match2_null", dict(match2=None), A), ("match12_null", dict(match12=None), B)],
        pairs=[("n_levels+th_high", dict(params=ctx.variant(ctx.sim3, n_levels=0, th_high=256)), "n_levels", B),
               ("th_high+grid", dict(params=ctx.variant(ctx.sim3, th_high=256, cols=65, rows=64)), "th_high", B),
               ("n_range+side_null", dict(side1=ctx.side(n=BIG, Pz=None)), "n_range", B),
               ("side_null+align_of_one_side", dict(side1=ctx.side(Pz=None, kp_desc=odd)), "side_null", B)])
    return dict(search_for_triangulation=tri, fuse=fuse, search_by_bow_kf=bowkf, search_by_sim3=sim3, search_by_bow=bow)


def rows_of(spec):
    """(row name, synchronous form?, overrides, the row whose answer it must repeat or None) in the order they run"""
    out = []
    for sync in (False, True):
        form = "sync" if sync else "async"
        chain = ([(n, o) for n, o in spec["sync"]] if sync else []) + [(n, o) for n, o, f in spec["chain"] if f in ("both", form)]
        for n, o in chain:
            out.append(("%s/%s" % (form, n), sync, o, None))
        for (n1, o1), (n2, o2) in zip(chain, chain[1:]):
            if set(o1) & set(o2):
                continue                                     # the two violations need the same argument
            out.append(("%s/%s+%s" % (form, n1, n2), sync, dict(o1, **o2), "%s/%s" % (form, n1)))
        for n, o, f in spec["more"]:
            if f in ("both", form):
                out.append(("%s/%s" % (form, n), sync, o, None))
        for n, o, same, f in spec["pairs"]:
            if f in ("both", form) and "%s/%s" % (form, n) not in [r[0] for r in out]:
                out.append(("%s/%s" % (form, n), sync, o, "%s/%s" % (form, same)))
    return out


def run(ctx=None):
    """every row's answer and the valid call after it: {entry point: {row: {"refusal": [rc, text], "same_as": row or None, "form": "async" /
    "sync", "after": valid()}}}"""
    own = ctx is None
    ctx = ctx or Context()
    try:
        result = {}
        E, CH = entries(ctx), chains(ctx)
        for name, e in E.items():
            rec = result[name] = {}
            r, _ = e.stats()                                 # before the entry point's first call on this owner
            rec["stats/before"] = dict(refusal=r, same_as=None, form="async", after=e.valid(False))
            r, _ = e.stats(handle=None)
            rec["stats/null_owner"] = dict(refusal=r, same_as=None, form="sync", after=e.valid(True))
            for sync in (False, True):
                form = "sync" if sync else "async"
                rec["%s/null_owner" % form] = dict(refusal=e.call(sync, {}, handle=None), same_as=None, form=form, after=e.valid(sync))
            for row, sync, over, same in rows_of(CH[name]):
                r = e.call(sync, over)
                if r[0] == 0:
                    raise AssertionError("%s %s was not refused" % (name, row))
                rec[row] = dict(refusal=r, same_as=same, form="sync" if sync else "async", after=e.valid(sync))
        return result
    finally:
        if own:
            ctx.close()


# ---- the recording's form: an entry point's valid result once per form under "valid"; a row carries an "after" of its own only where it differs ----
def pack(result):
    out = {}
    for name, rows in result.items():
        valid = {form: next(r["after"] for r in rows.values() if r["form"] == form) for form in ("async", "sync")}
        packed = {}
        for row, r in rows.items():
            q = dict(refusal=r["refusal"], same_as=r["same_as"], form=r["form"])
            if r["after"] != valid[r["form"]]:
                q["after"] = r["after"]
            packed[row] = q
        out[name] = dict(valid=valid, rows=packed)
    return out


def unpack(recording):
    return {name: {row: dict(r, after=r.get("after", e["valid"][r["form"]])) for row, r in e["rows"].items()} for name, e in recording.items() if name != "bindings"}


def write(recording, path):
    """one line per row"""
    lines = []
    for name in sorted(recording):
        e = recording[name]
        if name == "bindings":
            body = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(e[k])) for k in sorted(e))
            lines.append("%s: {\n%s\n }" % (json.dumps(name), body))
        else:
            body = ",\n".join("   %s: %s" % (json.dumps(k), json.dumps(e["rows"][k], sort_keys=True)) for k in sorted(e["rows"]))
            lines.append('%s: {\n  "valid": %s,\n  "rows": {\n%s\n  }\n }' % (json.dumps(name), json.dumps(e["valid"], sort_keys=True), body))
    with open(path, "w") as f:
        f.write("{\n " + ",\n ".join(lines) + "\n}\n")


# ---- the JsorbError texts of KeyframeMatcher's four argument builders (jetson_slam_amd/orb.py): no GPU, the tensors are stand-ins ----
class FakeTensor:
    """what the builders read of a device tensor: data_ptr, is_cuda, dtype, shape, is_contiguous (and numel, device)"""
    device = None

    def __init__(self, dtype, shape, ptr=4096, is_cuda=True, contiguous=True):
        self.dtype, self.shape, self.ptr, self.is_cuda, self.contiguous = dtype, tuple(shape), ptr, is_cuda, contiguous

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return self.contiguous

    def numel(self):
        return int(np.prod(self.shape))


def binding_rows(orb):
    """{row: "JsorbError: text" / the name of another exception / "ok"}: per builder and side one row per message"""
    import torch
    K = orb.KeyframeMatcher
    m = K.__new__(K)                                          # the builders read class attributes only: no matcher is created
    i32, u8, f32 = torch.int32, torch.uint8, torch.float32

    def side(keys, n, dtypes):
        return {k: FakeTensor(dtypes.get(k, f32), (n, 32) if k.endswith("desc") else (n,)) for k in keys}

    tri_dt = dict(node=i32, octave=i32, free=u8, stereo=torch.bool, desc=u8)
    fuse_dt = dict(octave=i32, desc=u8)
    bow_dt = dict(node=i32, valid=u8, desc=u8)
    sim3_dt = dict(octave=i32, kp_desc=u8, mp_desc=u8, search=u8)
    pose = dict(Rw=np.zeros(9), tw=np.zeros(3), sR=np.zeros(9), t=np.zeros(3))
    lsf = 0.18
    params = dict(tri=orb.make_triangulation_params([1.0]), fuse=orb.make_fuse_params((1, 1, 0, 0), (0, 1, 0, 1), (1, 1), lsf, [1.0]), bow=orb.make_bow_params(),
                  sim3=orb.make_sim3_params((1, 1, 0, 0), (0, 1, 0, 1), (1, 1), lsf, [1.0]))
    ks = np.array([0, 2, 5], np.int32)                        # two keyframes, five keypoints

    def tri(kf1=None, kf2=None, kf_start=ks, F12=np.zeros(18), epipole=np.zeros(4), p=params["tri"]):
        return K._args(m, kf1 or side(K.KF1_KEYS, 3, tri_dt), kf_start, kf2 or side(K.KF2_KEYS, 5, tri_dt), F12, epipole, p)

    def fuse(points=None, kfs=None, kf_start=ks, Rcw=np.zeros(18), tcw=np.zeros(6), Ow=np.zeros(6), p=params["fuse"], skip=None):
        return K._fuse_args(m, points or side(K.POINT_KEYS, 3, fuse_dt), kf_start, kfs or side(K.FUSE_KF_KEYS, 5, fuse_dt), Rcw, tcw, Ow, p, skip)

    def bow(kf1=None, cands=None, kf_start=ks, p=params["bow"]):
        return K._bow_kf_args(m, kf1 or side(K.BOW_KF_KEYS, 3, bow_dt), kf_start, cands or side(K.BOW_KF_KEYS, 5, bow_dt), p)

    def sim3(s1=None, s2=None, p=params["sim3"]):
        return K._sim3_args(m, s1 or dict(side(K.SIM3_KEYS, 3, sim3_dt), **pose), s2 or dict(side(K.SIM3_KEYS, 5, sim3_dt), **pose), p)

    def broken(keys, n, dtypes, key, **change):
        """a good side with one tensor replaced: by `value`, or by a stand-in with the changed properties"""
        d = side(keys, n, dtypes)
        if "value" in change:
            d[key] = change["value"]
        else:
            t = d[key]
            d[key] = FakeTensor(change.get("dtype", t.dtype), change.get("shape", t.shape), change.get("ptr", t.ptr), change.get("is_cuda", True),
                                change.get("contiguous", True))
        return d

    faults = [("not_a_tensor", dict(value=np.zeros(3))), ("not_on_the_device", dict(is_cuda=False)), ("dtype", dict(dtype=torch.float64)),
              ("shape", dict(shape=(7,))), ("not_contiguous", dict(contiguous=False))]
    rows = {}

    def add(name, f):
        try:
            f()
            rows[name] = "ok"
        except orb.JsorbError as e:
            rows[name] = "JsorbError: %s" % e
        except Exception as e:                                # (recorded as it is: what the builder does with such an input)
            rows[name] = type(e).__name__

    sides = [("tri", tri, "kf1", K.KF1_KEYS, 3, tri_dt, "x"), ("tri", tri, "kf2", K.KF2_KEYS, 5, tri_dt, "octave"),
             ("fuse", fuse, "points", K.POINT_KEYS, 3, fuse_dt, "Nz"), ("fuse", fuse, "kfs", K.FUSE_KF_KEYS, 5, fuse_dt, "octave"),
             ("bow_kf", bow, "kf1", K.BOW_KF_KEYS, 3, bow_dt, "valid"), ("bow_kf", bow, "cands", K.BOW_KF_KEYS, 5, bow_dt, "angle"),
             ("sim3", sim3, "s1", K.SIM3_KEYS, 3, sim3_dt, "search"), ("sim3", sim3, "s2", K.SIM3_KEYS, 5, sim3_dt, "Pz")]
    for what, call, arg, keys, n, dt, key in sides:
        extra = pose if what == "sim3" else {}
        for fault, change in faults:
            add("%s/%s/%s" % (what, arg, fault), lambda: call(**{arg: dict(broken(keys, n, dt, key, **change), **extra)}))
        for dk in [k for k in keys if k.endswith("desc")]:
            add("%s/%s/misaligned_%s" % (what, arg, dk), lambda: call(**{arg: dict(broken(keys, n, dt, dk, ptr=4104), **extra)}))
            add("%s/%s/shape_%s" % (what, arg, dk), lambda: call(**{arg: dict(broken(keys, n, dt, dk, shape=(n, 31)), **extra)}))
    for what, call in (("tri", tri), ("fuse", fuse), ("bow_kf", bow)):
        add(what + "/ok", call)
        add(what + "/kf_start_2d", lambda: call(kf_start=np.zeros((2, 2), np.int32)))
        add(what + "/kf_start_empty", lambda: call(kf_start=np.zeros(0, np.int32)))
        add(what + "/params_class", lambda: call(p=object()))
        add(what + "/params_of_another_matcher", lambda: call(p=params["sim3"]))
    add("sim3/ok", sim3)
    add("sim3/params_class", lambda: sim3(p=object()))
    add("sim3/params_of_another_matcher", lambda: sim3(p=params["bow"]))
    add("sim3/params_before_self", lambda: K._sim3_args(None, {}, {}, object()))
    add("tri/F12_count", lambda: tri(F12=np.zeros(17)))
    add("tri/epipole_count", lambda: tri(epipole=np.zeros(5)))
    add("fuse/Rcw_count", lambda: fuse(Rcw=np.zeros(9)))
    add("fuse/tcw_count", lambda: fuse(tcw=np.zeros(3)))
    add("fuse/Ow_count", lambda: fuse(Ow=np.zeros(7)))
    add("fuse/uright_none", lambda: fuse(kfs=broken(K.FUSE_KF_KEYS, 5, fuse_dt, "uright", value=None)))
    add("fuse/octave_missing", lambda: fuse(kfs={k: v for k, v in side(K.FUSE_KF_KEYS, 5, fuse_dt).items() if k != "octave"}))
    add("fuse/skip_ok", lambda: fuse(skip=FakeTensor(u8, (2, 3))))
    for fault, change in (("not_on_the_device", dict(is_cuda=False)), ("dtype", dict(dtype=f32)), ("count", dict(shape=(7,))), ("not_contiguous", dict(contiguous=False))):
        add("fuse/skip_" + fault, lambda: fuse(skip=FakeTensor(change.get("dtype", torch.bool), change.get("shape", (2, 3)), 4096, change.get("is_cuda", True),
                                                               change.get("contiguous", True))))
    for k, size in K.SIM3_POSE:
        for arg in ("s1", "s2"):
            add("sim3/%s/pose_%s" % (arg, k), lambda: sim3(**{arg: dict(side(K.SIM3_KEYS, 3, sim3_dt), **dict(pose, **{k: np.zeros(size + 1)}))}))
    return rows


if __name__ == "__main__":
    # kf_refusal_cases.py [--bindings-only] [file]: --bindings-only rewrites the "bindings" rows of an existing recording (no GPU)
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (behind PYTHONPATH: another orb.py there wins)
    argv = [a for a in sys.argv[1:] if a != "--bindings-only"]
    path = argv[0] if argv else GOLDEN
    if "--bindings-only" in sys.argv:
        with open(path) as f:
            rec = json.load(f)
    else:
        rec = pack(run())
    from jetson_slam_amd import orb
    rec["bindings"] = binding_rows(orb)
    write(rec, path)
    print("%d rows" % sum(len(v.get("rows", v)) for v in rec.values()))
