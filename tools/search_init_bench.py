"""GPU time of jsorb_search_for_initialization_async (k_assign_grid + k_init_candidates + k_init_resolve) at the C1 (320x240, 3 levels, tile 15)
and C2 (752x480, 8 levels, tile 30) geometries: F1 = the level-0 keypoints of the left view of a synthetic pair (n1 = all of them,
prev_matched = their positions), F2 = the right view, window 50, ORBmatcher(0.9, true).  A second case per geometry passes ALL keypoints of the
left view as F1 (what a kept initial frame does: the octave > 0 entries are skipped on the device).  Per case: median over --reps of the
hipEvent span of the whole call on the handle's stream (prev_matched restored by a device copy outside the span), matches, fixed-point rounds,
candidates, displaced claims.  For scale the motion-model matcher (jsorb_search_last_frame_async, 1500 points, th 7, one pass: DESIGN section 12)
is timed the same way in the same run on the C2 frame.  The new kernels have no ids of their own for jsorb_kernel_time: run under
`rocprofv3 --kernel-trace --stats -- python tools/search_init_bench.py` for per-kernel times.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C1": dict(h=240, w=320, L=3, tile=15), "C2": dict(h=480, w=752, L=8, tile=30)}


def spans_us(torch, stream, call, reps, before=None):
    for _ in range(10):
        if before:
            before()
        assert call() == 0
    out = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        assert call() == 0
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    from jetson_slam_amd.synth import synth_stereo_pair
    lib = orb.load_library()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()            # a stream of its own: the events below bracket the handle's work
    torch.cuda.set_stream(stream)
    for name, c in CONFIGS.items():
        h, w = c["h"], c["w"]
        left, right = synth_stereo_pair(31, h, w)
        g = orb.ORBExtractor(h, w, 1.2, c["L"], 9, 14, 7, 20, None, c["tile"], c["tile"])
        g.set_stream(stream.cuda_stream)
        kp, desc = g.extract(left)
        n_all = len(kp) // 6
        kp, desc = kp.copy(), desc.copy()
        g.extract(right)
        N = g.n_keypoints(0)
        prm = orb.make_init_params((0.0, 0.0, np.float32(64) / np.float32(w), np.float32(48) / np.float32(h)))
        octave = kp[4 * n_all:5 * n_all]
        angle = kp[3 * n_all:4 * n_all].astype(np.int32).view(np.float32)
        xy = np.stack([kp[:n_all], kp[n_all:2 * n_all]]).astype(np.float32)
        for kind, sel in (("level0", np.nonzero(octave == 0)[0]), ("all_levels", np.arange(n_all))):
            n1 = len(sel)
            tens = [dev(octave[sel].astype(np.int32)), dev(angle[sel]), dev(desc[sel])]
            prev0, prev = dev(xy[:, sel]), dev(xy[:, sel])
            m12 = torch.empty(max(n1, 1), dtype=torch.int32, device="cuda")
            m21 = torch.empty(max(N, 1), dtype=torch.int32, device="cuda")
            cnt = torch.empty(1, dtype=torch.int32, device="cuda")
            call = lambda: lib.jsorb_search_for_initialization_async(g.handle, 0, C.byref(prm), n1, *[t.data_ptr() for t in tens], prev.data_ptr(),
                                                                     m12.data_ptr(), m21.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            spans = spans_us(torch, stream, call, args.reps, before=lambda: prev.copy_(prev0))
            rounds, n_cand, n_over, n_disp, ind = g.search_for_initialization_stats()
            print(json.dumps({"frame": name, "case": kind, "n1": n1, "level0_points": int((octave[sel] == 0).sum()), "keypoints_F2": N,
                              "window": 50, "median_us": round(float(np.median(spans)), 2), "p10_us": round(float(np.percentile(spans, 10)), 2),
                              "p90_us": round(float(np.percentile(spans, 90)), 2), "matches": int(cnt.item()), "rounds": rounds,
                              "candidates": n_cand, "overflowed_points": n_over, "displaced": n_disp, "kept_bins": ind}), flush=True)
        if name != "C2":
            continue
        # for scale: the motion-model matcher on the same frame, 1500 points, th 7, one pass (monocular: no uRight)
        rng = np.random.default_rng(1507)
        kp2 = g.keypoints(0)
        x, y = kp2[:N].astype(np.float32), kp2[N:2 * N].astype(np.float32)
        fx, cx, cy = 435.2, np.float32(w / 2), np.float32(h / 2)
        n = 1500
        src = rng.integers(0, N, n)
        z = rng.uniform(1.0, 15.0, n)
        t = np.array([0.002, -0.001, 0.003], np.float32)
        Pc = np.stack([(x[src] + rng.normal(0, 1, n) - cx) * z / fx, (y[src] + rng.normal(0, 1, n) - cy) * z / fx, z])
        P = (Pc - t.astype(np.float64)[:, None]).astype(np.float32)
        d = g.descriptors(0)[src].copy()
        lvl = np.clip(kp2[4 * N:5 * N][src] + rng.integers(-1, 2, n), 0, c["L"] - 1).astype(np.int32)
        ang = np.mod(kp2[3 * N:4 * N].astype(np.int32).view(np.float32)[src] + 12.0, 360).astype(np.float32)
        tens = [dev(a) for a in (P[0], P[1], P[2], lvl, ang, d)]
        mk, md = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        km = torch.empty(N, dtype=torch.int32, device="cuda")
        cnt = torch.empty(1, dtype=torch.int32, device="cuda")
        lp = orb.make_last_frame_params(np.eye(3, dtype=np.float32), t, (fx, fx, cx, cy), (0, w, 0, h),
                                        (np.float32(64) / np.float32(w), np.float32(48) / np.float32(h)), th=7, direction=0, retry_below=0)
        call = lambda: lib.jsorb_search_last_frame_async(g.handle, 0, C.byref(lp), n, *[a.data_ptr() for a in tens], None, mk.data_ptr(),
                                                         md.data_ptr(), km.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        spans = spans_us(torch, stream, call, args.reps)
        print(json.dumps({"frame": name, "case": "motion_model_matcher_for_scale", "points": n, "th": 7, "median_us": round(float(np.median(spans)), 2),
                          "p10_us": round(float(np.percentile(spans, 10)), 2), "p90_us": round(float(np.percentile(spans, 90)), 2),
                          "matches": int(cnt.item())}), flush=True)


if __name__ == "__main__":
    main()
