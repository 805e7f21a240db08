"""GPU time of jsorb_search_local_points_async (k_assign_grid + k_local_candidates + k_local_resolve) on one C2 stereo frame (752x480, 8 levels,
tile 30): 2 k / 5 k / 10 k local map points projected next to keypoints, th 1 / 3 / 5, and a conflict-heavy case (every point with the same
descriptor in a few spots).  Per case: median over --reps of the hipEvent span of the whole call on the handle's stream, the per-kernel hipEvent
times (jsorb_enable_kernel_timing, a separate pass: it serialises launches) and the resolver's rounds / candidates / overflowing points.
Run under `rocprofv3 --kernel-trace --stats -- python tools/search_local_bench.py` for the kernel-trace times.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    from jetson_slam_amd.synth import synth_stereo_pair
    h, w, L, tile, bf, fx = 480, 752, 8, 30, 47.906, 435.2
    left, right = synth_stereo_pair(31, h, w)
    gl = orb.ORBExtractor(h, w, 1.2, L, 9, 14, 7, 20, None, tile, tile)
    gr = orb.ORBExtractor(h, w, 1.2, L, 9, 14, 7, 20, None, tile, tile)
    kp, desc = gl.extract(left)
    gr.extract(right)
    u_right, _, _ = orb.compute_stereo_matches(gl, gr, bf / fx, bf)
    N = len(kp) // 6
    lib = orb.load_library()
    stream = torch.cuda.Stream()            # a stream of its own: the events below bracket the handle's work (the null stream would not be adopted)
    torch.cuda.set_stream(stream)
    gl.set_stream(stream.cuda_stream)
    x, y, octave = kp[:N].astype(np.float32), kp[N:2 * N].astype(np.float32), kp[4 * N:5 * N]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ur = dev(u_right)
    prm_of = lambda th: orb.JsorbSearchParams(th, 0.8, 100, bf, 0.0, 0.0, np.float32(64) / np.float32(w), np.float32(48) / np.float32(h), 64, 48)
    print(json.dumps({"frame": "C2 752x480 L8 tile30", "keypoints": N}), flush=True)
    for n, th, kind in [(2000, 1.0, "near"), (5000, 1.0, "near"), (10000, 1.0, "near"), (5000, 3.0, "near"), (5000, 5.0, "near"), (5000, 1.0, "conflict")]:
        rng = np.random.default_rng(n + int(th))
        if kind == "near":
            src = rng.integers(0, N, n)
            d = desc[src].copy()
            flip = rng.random(d.shape) < 0.06
            d[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
        else:                                    # 5 spots, every point of a spot with the same descriptor: long claim chains
            src = rng.integers(0, N, 5)[rng.integers(0, 5, n)]
            d = desc[src].copy()
        u = (x[src] + rng.normal(0, 2, n)).astype(np.float32)
        v = (y[src] + rng.normal(0, 2, n)).astype(np.float32)
        lvl = np.clip(octave[src] + rng.integers(0, 2, n), 0, L - 1).astype(np.int32)
        invz = np.where(u_right[src] > 0, (u - u_right[src]) / np.float32(bf), 0.1).astype(np.float32)
        vc = rng.choice(np.array([0.9, 1.0], np.float32), n)
        ins = np.ones(n, np.uint8)
        t = [dev(a) for a in (u, v, invz, lvl, vc, ins, d)]
        mk, md = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        km = torch.empty(N, dtype=torch.int32, device="cuda")
        cnt = torch.empty(1, dtype=torch.int32, device="cuda")
        prm = prm_of(th)
        call = lambda: lib.jsorb_search_local_points_async(gl.handle, 0, C.byref(prm), n, *[a.data_ptr() for a in t], ur.data_ptr(), None,
                                                          mk.data_ptr(), md.data_ptr(), km.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        for _ in range(10):
            assert call() == 0
        spans = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            assert call() == 0
            b.record(stream)
            b.synchronize()
            spans.append(a.elapsed_time(b) * 1e3)
        gl.enable_kernel_timing(True)
        per = {k: [] for k in ("k_assign_grid", "k_local_candidates", "k_local_resolve")}
        for _ in range(min(args.reps, 50)):
            gl.reset_kernel_timing()
            assert call() == 0
            for k, (ms, _) in gl.search_local_kernel_times().items():
                per[k].append(ms * 1e3)
        gl.enable_kernel_timing(False)
        rounds, n_cand, n_over = gl.search_local_stats()
        print(json.dumps({"points": n, "th": th, "case": kind, "median_us": round(float(np.median(spans)), 2),
                          "p10_us": round(float(np.percentile(spans, 10)), 2), "p90_us": round(float(np.percentile(spans, 90)), 2),
                          "kernel_median_us": {k: round(float(np.median(vs)), 2) for k, vs in per.items()},
                          "matches": int(cnt.item()), "rounds": rounds, "candidates": n_cand, "overflow_points": n_over}), flush=True)


if __name__ == "__main__":
    main()
