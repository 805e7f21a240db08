"""Binding of oracle/_ref/libref_matcher.so - the reference's own src/ORBmatcher.cpp behind the drivers of oracle/ref_matcher/harness.cpp - and the
case <-> npz plumbing of tests/golden/ref_matcher_*.npz.  TEST INFRASTRUCTURE ONLY.  The library exists only where the reference tree was present at
build time (oracle/Makefile, target ref_matcher); everything else here works without it.

A case is a dict of dicts of arrays and scalars in the vocabulary of the host tests (tests/test_search_local_host.py and its siblings): the sides
(F, P, KF, ...) and prm.  run(name, case) calls the driver of that entry point and returns a dict of outputs."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
c_f, c_i, c_p = ctypes.c_float, ctypes.c_int32, ctypes.c_void_p


def lib_path(fused=False):
    return os.path.join(HERE, "_ref", "libref_matcher_fused.so" if fused else "libref_matcher.so")


def available(fused=False):
    return os.path.exists(lib_path(fused))


_libs = {}


def lib(fused=False):
    if fused not in _libs:
        l = ctypes.CDLL(lib_path(fused))
        assert l.rm_abi_version() == 2
        l.rm_fuse.restype = l.rm_fuse_sim3.restype = l.rm_log_sizes.restype = l.rm_log_copy.restype = None
        _libs[fused] = l
    return _libs[fused]


class View(ctypes.Structure):
    """rm_view of harness.cpp"""
    _fields_ = [("n", c_i), ("kx", c_p), ("ky", c_p), ("octave", c_p), ("angle", c_p), ("desc", c_p), ("u_right", c_p), ("cols", c_i), ("rows", c_i),
                ("cell_start", c_p), ("cell_items", c_p), ("min_x", c_f), ("max_x", c_f), ("min_y", c_f), ("max_y", c_f), ("inv_w", c_f), ("inv_h", c_f),
                ("n_levels", c_i), ("scale", c_p), ("sigma2", c_p), ("inv_sigma2", c_p), ("log_scale", c_f), ("fx", c_f), ("fy", c_f), ("cx", c_f),
                ("cy", c_f), ("mbf", c_f), ("mb", c_f), ("Rcw", c_p), ("tcw", c_p), ("Ow", c_p), ("node", c_p)]


class _Keep:
    """arrays handed to a driver, kept alive for the call"""

    def __init__(self):
        self.held = []

    def arr(self, a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype)
        if a.size == 0:
            a = np.zeros(1, dtype)
        self.held.append(a)
        return a.ctypes.data


def view(keep, side, n, x="kx", y="ky", **scalars):
    """an rm_view from one side's dict: whatever of kx / ky (or x / y), octave, angle, desc, u_right, the grid CSR, scale tables, pose and node it holds"""
    v = View()
    v.n = int(n)
    g = side.get
    v.kx, v.ky = keep.arr(g(x), np.float32), keep.arr(g(y), np.float32)
    v.octave, v.angle = keep.arr(g("octave"), np.int32), keep.arr(g("angle"), np.float32)
    v.desc, v.u_right = keep.arr(g("desc"), np.uint8), keep.arr(g("u_right"), np.float32)
    if g("start") is not None:
        v.cols, v.rows = int(side["cols"]), int(side["rows"])
        v.cell_start, v.cell_items = keep.arr(side["start"], np.int32), keep.arr(side["items"], np.int32)
        v.min_x, v.min_y, v.inv_w, v.inv_h = (float(side[k]) for k in ("min_x", "min_y", "inv_w", "inv_h"))
    if g("scale") is not None:
        v.n_levels, v.scale = len(side["scale"]), keep.arr(side["scale"], np.float32)
    v.sigma2, v.inv_sigma2 = keep.arr(g("sigma2"), np.float32), keep.arr(g("inv_sigma2"), np.float32)
    v.node = keep.arr(g("node"), np.int32)
    for k in ("Rcw", "tcw", "Ow"):
        setattr(v, k, keep.arr(g(k), np.float32))
    for k, val in scalars.items():
        setattr(v, k, val)
    return v


# ---- one wrapper per driver: case dict -> outputs dict ----
def _local(l, c):
    F, P, prm = c["F"], c["P"], c["prm"]
    k = _Keep()
    N, n = len(F["kx"]), len(P["u"])
    v = view(k, F, N, mbf=float(F["mbf"]))
    out = np.full(max(N, 1), -1, np.int32)
    cnt = l.rm_search_local(ctypes.byref(v), n, *(c_p(k.arr(P[a], t)) for a, t in (("u", np.float32), ("v", np.float32), ("invz", np.float32), (
        "level", np.int32), ("view_cos", np.float32), ("in_frustum", np.uint8), ("desc", np.uint8))), c_p(k.arr(F["blocked"], np.uint8)),
        c_f(prm["th"]), c_f(prm["nn_ratio"]), c_p(out.ctypes.data))
    return dict(kp_match=out[:N].copy(), nmatches=np.int32(cnt))


def _last(l, c):
    F, P, prm = c["F"], c["P"], c["prm"]
    k = _Keep()
    N, n = len(F["kx"]), len(P["Px"])
    v = view(k, F, N, mbf=float(F["mbf"]), Rcw=k.arr(prm["Rcw"], np.float32), tcw=k.arr(prm["tcw"], np.float32),
             **{a: float(prm[a]) for a in ("fx", "fy", "cx", "cy", "max_x", "max_y")})
    out = np.full(max(N, 1), -1, np.int32)
    cnt = l.rm_search_last_frame(ctypes.byref(v), n, *(c_p(k.arr(P[a], t)) for a, t in (("Px", np.float32), ("Py", np.float32), ("Pz", np.float32), (
        "octave", np.int32), ("angle", np.float32), ("desc", np.uint8))), int(prm["direction"]), c_f(prm["th"]), int(prm["check_orientation"]),
        c_p(out.ctypes.data))
    return dict(kp_match=out[:N].copy(), nmatches=np.int32(cnt))


def _init(l, c):
    F1, F2, prm = c["F1"], c["F2"], c["prm"]
    k = _Keep()
    n1, N = len(F1["octave"]), len(F2["kx"])
    v = view(k, F2, N)
    prev = np.ascontiguousarray(c["prev"], np.float32).reshape(2, n1).copy()
    buf = prev if n1 else np.zeros((2, 1), np.float32)
    out = np.full(max(n1, 1), -1, np.int32)
    window = int(prm["window"])
    assert window == prm["window"]                   # windowSize is an int in the reference
    cnt = l.rm_search_for_initialization(n1, c_p(k.arr(F1["octave"], np.int32)), c_p(k.arr(F1["angle"], np.float32)), c_p(k.arr(F1["desc"], np.uint8)),
                                         ctypes.byref(v), c_p(buf.ctypes.data), window, c_f(prm["nn_ratio"]), int(prm["check_orientation"]),
                                         c_p(out.ctypes.data))
    return dict(matches12=out[:n1].copy(), nmatches=np.int32(cnt), prev=prev)


def _bow(l, c):
    KF, F, prm = c["KF"], c["F"], c["prm"]
    k = _Keep()
    nk, N = len(KF["node"]), len(F["node"])
    vk, vf = view(k, KF, nk), view(k, F, N)
    out = np.full(max(N, 1), -1, np.int32)
    cnt = l.rm_search_by_bow(ctypes.byref(vk), c_p(k.arr(KF["valid"], np.uint8)), ctypes.byref(vf), c_f(prm["nn_ratio"]), int(prm["check_orientation"]),
                             c_p(out.ctypes.data))
    return dict(match_kf=out[:N].copy(), nmatches=np.int32(cnt))


def _bow_kf(l, c):
    K1, K2, prm = c["KF1"], c["KF2"], c["prm"]
    k = _Keep()
    n1, n2 = len(K1["node"]), len(K2["node"])
    v1, v2 = view(k, K1, n1), view(k, K2, n2)
    out = np.full(max(n1, 1), -1, np.int32)
    cnt = l.rm_search_by_bow_kf(ctypes.byref(v1), c_p(k.arr(K1["valid"], np.uint8)), ctypes.byref(v2), c_p(k.arr(K2["valid"], np.uint8)),
                                c_f(prm["nn_ratio"]), int(prm["check_orientation"]), c_p(out.ctypes.data))
    return dict(matches12=out[:n1].copy(), nmatches=np.int32(cnt))


def _tri(l, c):
    K1, K2, geom, prm = c["KF1"], c["KF2"], c["geom"], c["prm"]
    k = _Keep()
    n1, n2 = len(K1["node"]), len(K2["node"])
    s2 = np.asarray(prm["level_sigma2"], np.float32)
    sides = []
    for K, n in ((K1, n1), (K2, n2)):
        K = dict(K, u_right=np.where(np.asarray(K["stereo"]) != 0, 1.0, -1.0).astype(np.float32), scale=prm["scale_factor"], sigma2=s2)
        sides.append(view(k, K, n, x="x", y="y"))
    pairs = np.full((max(n1, 1), 2), -1, np.int32)
    n_pairs = c_i()
    cnt = l.rm_search_for_triangulation(ctypes.byref(sides[0]), c_p(k.arr(K1["free"], np.uint8)), ctypes.byref(sides[1]), c_p(k.arr(K2["free"], np.uint8)),
                                        c_p(k.arr(geom["F12"], np.float32)), c_f(geom["ex"]), c_f(geom["ey"]), int(prm["only_stereo"]),
                                        int(prm["check_orientation"]), c_p(pairs.ctypes.data), ctypes.byref(n_pairs))
    return dict(pairs=pairs[:n_pairs.value].copy(), nmatches=np.int32(cnt))


def logs(l):
    """the event log [E, 4], the descriptors of its descriptor events [D, 32] and the probe log [P, 5] of the last logging driver"""
    sizes = (c_i * 3)()
    l.rm_log_sizes(sizes)
    ev, de, pr = np.zeros((sizes[0], 4), np.int32), np.zeros((sizes[1], 32), np.uint8), np.zeros((sizes[2], 5), np.float32)
    l.rm_log_copy(c_p(ev.ctypes.data if ev.size else None), c_p(de.ctypes.data if de.size else None), c_p(pr.ctypes.data if pr.size else None))
    return ev, de, pr


def _map_args(k, c):
    """the live map of a fuse case as build_map of harness.cpp takes it; returns (arguments, keyframe sizes, number of points)"""
    KF, P, prm = c["KF"], c["P"], c["prm"]
    views = (View * len(KF))()
    for i, K in enumerate(KF):
        side = dict(K, u_right=K["uright"], scale=prm["scale"], inv_sigma2=prm["inv_sigma2"], start=K["_start"], items=K["_items"],
                    **{a: prm[a] for a in ("cols", "rows", "min_x", "min_y", "inv_w", "inv_h")})      # (_start, _items: the grid's CSR, built by the caller)
        views[i] = view(k, side, len(K["x"]), x="x", y="y", max_x=float(prm["max_x"]), max_y=float(prm["max_y"]), log_scale=float(prm["log_sf"]),
                        fx=float(prm["fx"]), fy=float(prm["fy"]), cx=float(prm["cx"]), cy=float(prm["cy"]), mbf=float(prm["bf"]))
    sizes = [len(K["x"]) for K in KF]
    mps = np.concatenate([np.asarray(K["mps"], np.int32) for K in KF] + [np.zeros(0, np.int32)])
    n = len(P["Px"])
    pos = np.stack([P["Px"], P["Py"], P["Pz"]], 1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    nrm = np.stack([P["Nx"], P["Ny"], P["Nz"]], 1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    obs = np.asarray(c["obs"], np.int32).reshape(-1, 3)
    args = [len(KF), views, c_p(k.arr(mps, np.int32)), n, c_p(k.arr(pos, np.float32)), c_p(k.arr(nrm, np.float32)), c_p(k.arr(P["maxd"], np.float32)),
            c_p(k.arr(P["mind"], np.float32)), c_p(k.arr(P["desc"], np.uint8)), c_p(k.arr(P["bad"], np.uint8)), len(obs), c_p(k.arr(obs, np.int32)),
            len(c["targets"]), c_p(k.arr(c["targets"], np.int32))]
    return args, sizes, n


def _map_outs(l, sizes, n):
    mps_out, state, desc = np.full(max(sum(sizes), 1), -1, np.int32), np.zeros((max(n, 1), 3), np.int32), np.zeros((max(n, 1), 32), np.uint8)
    return (mps_out, state, desc), lambda: dict(kf_mps=mps_out[:sum(sizes)].copy(), pt_bad=state[:n, 0].astype(np.uint8), pt_replaced=state[:n, 1].copy(),
                                                pt_nobs=state[:n, 2].copy(), pt_desc=desc[:n].copy(), **dict(zip(("events", "ev_desc", "probe"), logs(l))))


def _fuse(l, c):
    k = _Keep()
    args, sizes, n = _map_args(k, c)
    lst = np.asarray(c["list"], np.int32)
    nf = np.zeros(max(len(c["targets"]), 1), np.int32)
    (mps_out, state, desc), outs = _map_outs(l, sizes, n)
    l.rm_fuse(*args, len(lst), c_p(k.arr(lst, np.int32)), c_f(c["prm"]["th"]), c_p(nf.ctypes.data), c_p(mps_out.ctypes.data), c_p(state.ctypes.data),
              c_p(desc.ctypes.data))
    return dict(outs(), nfused=nf[:len(c["targets"])].copy(), nmatches=np.int32(nf[:len(c["targets"])].sum()))


def _fuse_sim3(l, c):
    k = _Keep()
    args, sizes, n = _map_args(k, c)
    lst = np.asarray(c["list"], np.int32)
    nt = len(c["targets"])
    nf, rep = np.zeros(max(nt, 1), np.int32), np.full((max(nt, 1), max(len(lst), 1)), -1, np.int32)
    (mps_out, state, desc), outs = _map_outs(l, sizes, n)
    l.rm_fuse_sim3(*args, c_p(k.arr(c["Scw"], np.float32)), int(c["replace_loop"]), len(lst), c_p(k.arr(lst, np.int32)), c_f(c["prm"]["th"]),
                   c_p(nf.ctypes.data), c_p(rep.ctypes.data), c_p(mps_out.ctypes.data), c_p(state.ctypes.data), c_p(desc.ctypes.data))
    return dict(outs(), nfused=nf[:nt].copy(), nmatches=np.int32(nf[:nt].sum()), replace=rep[:nt, :len(lst)].copy())


def _sim3(l, c):
    k = _Keep()
    prm, P = c["prm"], c["P"]
    views = (View * 2)()
    for i, K in enumerate(c["KF"]):
        side = dict(K, scale=prm["scale"], start=K["_start"], items=K["_items"], **{a: prm[a] for a in ("cols", "rows", "min_x", "min_y", "inv_w", "inv_h")})
        views[i] = view(k, side, len(K["x"]), x="x", y="y", max_x=float(prm["max_x"]), max_y=float(prm["max_y"]), log_scale=float(prm["log_sf"]),
                        fx=float(prm["fx"]), fy=float(prm["fy"]), cx=float(prm["cx"]), cy=float(prm["cy"]))
    n, n1 = len(P["Px"]), len(c["KF"][0]["x"])
    pos = np.stack([P["Px"], P["Py"], P["Pz"]], 1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    obs = np.asarray(c["obs"], np.int32).reshape(-1, 3)
    m12 = np.full(max(n1, 1), -1, np.int32)
    m12[:n1] = c["matches12"]
    cnt = l.rm_search_by_sim3(views, c_p(k.arr(c["KF"][0]["mps"], np.int32)), c_p(k.arr(c["KF"][1]["mps"], np.int32)), n, c_p(k.arr(pos, np.float32)),
                              c_p(k.arr(P["maxd"], np.float32)), c_p(k.arr(P["mind"], np.float32)), c_p(k.arr(P["desc"], np.uint8)),
                              c_p(k.arr(P["bad"], np.uint8)), len(obs), c_p(k.arr(obs, np.int32)), c_f(c["s12"]), c_p(k.arr(c["R12"], np.float32)),
                              c_p(k.arr(c["t12"], np.float32)), c_f(prm["th"]), c_p(m12.ctypes.data))
    return dict(matches12=m12[:n1].copy(), nmatches=np.int32(cnt), probe=logs(l)[2])


def _kf(l, c):
    F, P, prm = c["F"], c["P"], c["prm"]
    k = _Keep()
    N, n = len(F["kx"]), len(P["Px"])
    v = view(k, F, N, Rcw=k.arr(prm["Rcw"], np.float32), tcw=k.arr(prm["tcw"], np.float32), log_scale=float(prm["log_sf"]),
             **{a: float(prm[a]) for a in ("fx", "fy", "cx", "cy", "max_x", "max_y")})
    pos = np.stack([P["Px"], P["Py"], P["Pz"]], 1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    out = np.full(max(N, 1), -1, np.int32)
    cnt = l.rm_search_kf(ctypes.byref(v), c_p(k.arr(F["blocked"], np.uint8)), n, c_p(k.arr(P["state"], np.uint8)), c_p(k.arr(pos, np.float32)),
                         c_p(k.arr(P["maxd"], np.float32)), c_p(k.arr(P["mind"], np.float32)), c_p(k.arr(P["desc"], np.uint8)),
                         c_p(k.arr(P["angle"], np.float32)), c_f(prm["th"]), int(prm["orb_dist"]), int(prm["check_orientation"]), c_p(out.ctypes.data))
    return dict(kp_match=out[:N].copy(), nmatches=np.int32(cnt), probe=logs(l)[2])


DRIVERS = {"search_kf": _kf, "fuse": _fuse, "fuse_sim3": _fuse_sim3, "search_by_sim3": _sim3, "search_local": _local, "search_last_frame": _last, "search_init": _init, "search_by_bow": _bow, "search_by_bow_kf": _bow_kf,
           "search_for_triangulation": _tri}


def run(name, case, fused=False):
    return DRIVERS[name](lib(fused), case)


# ---- cases <-> flat npz entries ----
def flatten(prefix, obj, out):
    """dict of dicts / arrays / scalars / None -> out["a/b/c"]; a side's `grid` (lists of lists) is left out: unflatten rebuilds it from the CSR"""
    if isinstance(obj, dict):
        for k, v in obj.items():
            if k == "grid" or k.startswith("_"):
                continue
            flatten(prefix + "/" + k if prefix else k, v, out)
    elif obj is None:
        out[prefix + "@none"] = np.zeros(0, np.uint8)
    elif isinstance(obj, (list, tuple)) and len(obj) and isinstance(obj[0], dict):
        out[prefix + "@len"] = np.int64(len(obj))
        for i, v in enumerate(obj):
            flatten("%s/%d" % (prefix, i), v, out)
    else:
        out[prefix] = np.asarray(obj)


def unflatten(flat):
    root = {}
    for key in sorted(flat):
        parts = key.split("/")
        d = root
        for p in parts[:-1]:
            d = d.setdefault(p, {})
        leaf = parts[-1]
        if leaf.endswith("@none"):
            d[leaf[:-5]] = None
        elif leaf.endswith("@len"):
            d.setdefault(leaf[:-4], {})["@len"] = int(flat[key])
        else:
            a = flat[key]
            d[leaf] = a[()] if a.ndim == 0 else a
    return _finish(root)


def _finish(d):
    if not isinstance(d, dict):
        return d
    if "@len" in d:
        return [_finish(d[str(i)]) for i in range(d["@len"])]
    d = {k: _finish(v) for k, v in d.items()}
    if "start" in d and "items" in d and "cols" in d and "rows" in d:
        s, it, rows = d["start"], d["items"], int(d["rows"])
        d["grid"] = [[[int(k) for k in it[s[i * rows + j]:s[i * rows + j + 1]]] for j in range(rows)] for i in range(int(d["cols"]))]
    return d


def golden_path(name):
    return os.path.join(os.path.dirname(HERE), "tests", "golden", "ref_matcher_%s.npz" % name)


def load_golden(name):
    """{case name: dict(inputs..., out=..., counters=...)} in the file's order.  The file holds three arrays: the case names, one byte blob and an
    index of tab-separated "key dtype shape offset" lines into it (thousands of small arrays as npz members would cost more in zip headers than in data)."""
    with np.load(golden_path(name)) as z:
        order, index, blob = [str(s) for s in z["cases"]], [str(s) for s in z["index"]], z["blob"]
    flat = {}
    for line in index:
        key, dtype, shape, offset = line.split("\t")
        shape = tuple(int(v) for v in shape.split(",") if v)
        dt = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        flat[key] = np.frombuffer(blob[int(offset):int(offset) + n].tobytes(), dt).reshape(shape).copy()
    tree = unflatten(flat)
    return {k: tree[k] for k in order}


def save_golden(name, cases):
    flat = {}
    for k, c in cases.items():
        assert "/" not in k and "\t" not in k
        flatten(k, c, flat)
    index, chunks, offset, seen = [], [], 0, {}
    for key in sorted(flat):
        a = np.asarray(flat[key])
        a = a if a.ndim == 0 else np.ascontiguousarray(a)
        assert a.dtype.kind in "iufb", (key, a.dtype)
        raw = a.tobytes()
        if len(raw) >= 64 and raw in seen:         # the cases of a block share their frame: one copy in the blob
            index.append("%s\t%s\t%s\t%d" % (key, a.dtype.str, ",".join(str(v) for v in a.shape), seen[raw]))
            continue
        seen[raw] = offset
        index.append("%s\t%s\t%s\t%d" % (key, a.dtype.str, ",".join(str(v) for v in a.shape), offset))
        chunks.append(raw)
        offset += len(raw)
    members = {"cases": np.array(list(cases)), "index": np.array(index), "blob": np.frombuffer(b"".join(chunks), np.uint8)}
    # a fixed member order and no timestamps: regenerating gives the same bytes
    import io
    import zipfile
    path = golden_path(name)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in ("cases", "index", "blob"):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, members[key], allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    return path
