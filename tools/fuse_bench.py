"""GPU time of jsorb_fuse_async (k_fuse_grids + k_fuse_match) on a jsorb_keyframe_matcher for the two shapes of LocalMapping::SearchInNeighbors
(LocalMapping.cpp:460-540): the current keyframe's map points into every target keyframe (60 keyframes x about 1000 points) and every map point of
the targets into the current keyframe (1 keyframe x about 30000 points).  The keyframe is the left view of a synthetic pair at C2 (752x480, 8
levels, tile 30), every second keypoint with a stereo measurement; the map points are its keypoints back-projected at depth 4 (for the second shape
30 copies of them, each jittered by a fraction of a pixel); the target keyframes are the same keyframe at poses a few millimetres apart, so that
most points find their keypoint.  Per case: median over --reps of the hipEvent span of the whole call on the matcher's stream, and the same with 16
points only - one workgroup of k_fuse_match per keyframe, so what remains is k_fuse_grids and the launches.  The time these medians stand against
is the sequential loop of examples/search_in_neighbors.cpp on the host, which the tool builds and runs at C1 (--no-example skips it).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C1 = dict(h=240, w=320, L=3, tile=15)
C2 = dict(h=480, w=752, L=8, tile=30)
FX, BF = 435.2, 47.906


def host_loop_us():
    """host_sequential_us of examples/search_in_neighbors.cpp at C1: one current keyframe against three targets, both directions"""
    from jetson_slam_amd import build as jb
    from jetson_slam_amd.synth import synth_stereo_pair
    with tempfile.TemporaryDirectory() as tmp:
        exe = jb.build_example("search_in_neighbors", os.path.join(tmp, "search_in_neighbors"), ["-O2"])
        left, right = synth_stereo_pair(31, C1["h"], C1["w"])
        paths = []
        for i, img in enumerate((left, right, left, synth_stereo_pair(32, C1["h"], C1["w"])[1])):
            paths.append(os.path.join(tmp, "kf%d.raw" % i))
            img.tofile(paths[-1])
        out = subprocess.run([exe, str(C1["h"]), str(C1["w"]), str(C1["L"]), str(C1["tile"]), "20", "1"] + paths + [os.path.join(tmp, "out.bin")],
                             capture_output=True, text=True, timeout=300)
        m = re.search(r"keyframes=([\d,]+) points=(\d+),(\d+) fused=(-?\d+),(-?\d+) host_sequential_us=([\d.]+)", out.stdout)
        if out.returncode != 0 or not m:
            return {"error": (out.stderr or out.stdout)[-300:]}
        return {"keyframes": m.group(1), "points": [int(m.group(2)), int(m.group(3))], "fused": [int(m.group(4)), int(m.group(5))],
                "host_sequential_us": float(m.group(6))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-example", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    from jetson_slam_amd.synth import synth_stereo_pair
    lib = orb.load_library()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    m = orb.KeyframeMatcher()
    m.set_stream(stream.cuda_stream)
    c = C2
    left, _ = synth_stereo_pair(31, c["h"], c["w"])
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, 20, None, c["tile"], c["tile"])
    g.extract(left)
    kp = g.keypoints()
    N = len(kp) // 6
    x, y, octave = kp[:N].astype(np.float32), kp[N:2 * N].astype(np.float32), kp[4 * N:5 * N].astype(np.int32)
    desc = np.asarray(g.descriptors(), np.uint8).reshape(N, 32).copy()
    scale = np.ones(c["L"], np.float32)
    for l in range(1, c["L"]):
        scale[l] = np.float32(scale[l - 1] * np.float32(1.2))
    cx, cy, z = c["w"] / 2, c["h"] / 2, 4.0
    uright = np.where(np.arange(N) % 2 == 1, x - BF / z, -1).astype(np.float32)
    prm = orb.make_fuse_params((FX, FX, cx, cy), (0, c["w"], 0, c["h"]), (64 / c["w"], 48 / c["h"]), float(np.log(np.float32(1.2))), scale, bf=BF)

    def points(idx, jitter, rng):
        """the map points of keypoints idx: back-projected at depth z from the identity pose, `jitter` pixels off"""
        px, py = x[idx] + rng.normal(0, jitter, len(idx)), y[idx] + rng.normal(0, jitter, len(idx))
        P = np.stack([(px - cx) * z / FX, (py - cy) * z / FX, np.full(len(idx), z)])
        dist = np.sqrt((P * P).sum(0))
        maxd = (dist * scale[octave[idx]]).astype(np.float32)
        f = [P[0], P[1], P[2], P[0] / dist, P[1] / dist, P[2] / dist, maxd, np.float32(0.8) * maxd / scale[-1], np.float32(1.2) * maxd]
        d = {k: dev(np.asarray(v, np.float32)) for k, v in zip(orb.KeyframeMatcher.POINT_KEYS[:9], f)}
        d["desc"] = dev(desc[idx])
        return d

    result = {"tool": "fuse_bench", "reps": args.reps, "lanes_per_pair": 16, "frame": "C2", "keyframe_keypoints": N, "cases": []}
    rng = np.random.default_rng(7)
    shapes = (("neighbours", 60, np.arange(min(N, 1000)), 0.0), ("current", 1, np.tile(np.arange(N), -(-30000 // N))[:30000], 0.3))
    for name, n_kf, idx, jitter in shapes:
        P = points(idx, jitter, rng)
        n = len(idx)
        K = dict(x=dev(np.tile(x, n_kf)), y=dev(np.tile(y, n_kf)), octave=dev(np.tile(octave, n_kf)), uright=dev(np.tile(uright, n_kf)),
                 desc=dev(np.tile(desc, (n_kf, 1))))
        ks = (np.arange(n_kf + 1) * N).astype(np.int32)
        R = np.tile(np.eye(3, dtype=np.float32).ravel(), n_kf)
        t = (rng.normal(0, 0.002, (n_kf, 3))).astype(np.float32)
        O = (-t).astype(np.float32)
        bi = torch.empty(n_kf * n, dtype=torch.int32, device="cuda")
        bd = torch.empty(n_kf * n, dtype=torch.int32, device="cuda")
        cnt = torch.empty(n_kf, dtype=torch.int32, device="cuda")
        pp, pk = [P[k].data_ptr() for k in orb.KeyframeMatcher.POINT_KEYS], [K[k].data_ptr() for k in orb.KeyframeMatcher.FUSE_KF_KEYS]
        call = lambda n_: lib.jsorb_fuse_async(m.handle, C.byref(prm), n_, *pp, n_kf, ks.ctypes.data, *pk, R.ctypes.data, t.ctypes.data, O.ctypes.data,
                                               None, bi.data_ptr(), bd.data_ptr(), cnt.data_ptr())
        row = {"shape": name, "keyframes": n_kf, "points": n}
        for label, n_ in (("", n), ("_16_points", min(16, n))):
            torch.cuda.synchronize()
            for _ in range(10):
                assert call(n_) == 0
            spans = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                assert call(n_) == 0
                b.record(stream)
                b.synchronize()
                spans.append(a.elapsed_time(b) * 1e3)
            if not label:
                windows, walked, dists, largest = m.fuse_stats()
                row.update(matched=int(cnt.sum().item()), windows=windows, walked=walked, distances=dists, largest_window=largest)
            row.update({"median_us" + label: round(float(np.median(spans)), 2), "p10_us" + label: round(float(np.percentile(spans, 10)), 2),
                        "p90_us" + label: round(float(np.percentile(spans, 90)), 2)})
        result["cases"].append(row)
    m.close()
    if not args.no_example:
        result["host_loop_c1"] = host_loop_us()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
