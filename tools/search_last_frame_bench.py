"""GPU time of jsorb_search_last_frame_async (k_assign_grid + k_last_match + k_last_resolve per pass) on one C2 stereo frame (752x480, 8 levels,
tile 30): 500 / 1500 / 3000 last-frame points back-projected from keypoints through a slightly perturbed pose, one pass at th 7 (retry_below 20, and 0: the second pass not even enqueued), a forced retry
(retry_below above any count: the second pass runs at th 14 and its results stand), and monocular at th 15.  Per case: median over
--reps of the hipEvent span of the whole call on the handle's stream, the per-kernel hipEvent times (jsorb_enable_kernel_timing, a separate pass:
it serialises launches), passes and candidates.  Run under `rocprofv3 --kernel-trace --stats -- python tools/search_last_frame_bench.py` for the
kernel-trace times.  Prints one JSON line per case."""
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
    angle = kp[3 * N:4 * N].astype(np.int32).view(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ur = dev(u_right)
    cx, cy = np.float32(w / 2), np.float32(h / 2)
    R, t = np.eye(3, dtype=np.float32), np.array([0.002, -0.001, 0.003], np.float32)
    print(json.dumps({"frame": "C2 752x480 L8 tile30", "keypoints": N}), flush=True)
    for n, th, kind in [(500, 7, "stereo"), (1500, 7, "stereo"), (3000, 7, "stereo"), (1500, 7, "retry_off"), (1500, 7, "forced_retry"),
                          (1500, 15, "mono")]:
        rng = np.random.default_rng(n + th)
        src = rng.integers(0, N, n)
        z = rng.uniform(1.0, 15.0, n)
        Pc = np.stack([(x[src] + rng.normal(0, 1, n) - cx) * z / fx, (y[src] + rng.normal(0, 1, n) - cy) * z / fx, z])
        P = (Pc - t.astype(np.float64)[:, None]).astype(np.float32)
        d = desc[src].copy()
        flip = rng.random(d.shape) < 0.03
        d[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
        lvl = np.clip(octave[src] + rng.integers(-1, 2, n), 0, L - 1).astype(np.int32)
        ang = np.mod(angle[src] + np.where(rng.random(n) < 0.3, rng.uniform(0, 360, n), 12.0), 360).astype(np.float32)
        tens = [dev(a) for a in (P[0], P[1], P[2], lvl, ang, d)]
        mk, md = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        km = torch.empty(N, dtype=torch.int32, device="cuda")
        cnt = torch.empty(1, dtype=torch.int32, device="cuda")
        prm = orb.make_last_frame_params(R, t, (fx, fx, cx, cy), (0, w, 0, h), (np.float32(64) / np.float32(w), np.float32(48) / np.float32(h)),
                                         th=th, direction=0, mbf=bf, retry_below={"forced_retry": 10 ** 6, "retry_off": 0}.get(kind, 20))
        u_arg = None if kind == "mono" else ur.data_ptr()
        call = lambda: lib.jsorb_search_last_frame_async(gl.handle, 0, C.byref(prm), n, *[a.data_ptr() for a in tens], u_arg, mk.data_ptr(),
                                                         md.data_ptr(), km.data_ptr(), cnt.data_ptr())
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
        per = {k: [] for k in ("k_assign_grid", "k_last_match", "k_last_resolve")}
        for _ in range(min(args.reps, 50)):
            gl.reset_kernel_timing()
            assert call() == 0
            for k, (ms, _) in gl.search_last_frame_kernel_times().items():
                per[k].append(ms * 1e3)
        gl.enable_kernel_timing(False)
        passes, n_cand, ind = gl.search_last_frame_stats()
        print(json.dumps({"points": n, "th": th, "case": kind, "median_us": round(float(np.median(spans)), 2),
                          "p10_us": round(float(np.percentile(spans, 10)), 2), "p90_us": round(float(np.percentile(spans, 90)), 2),
                          "kernel_median_us (both passes)": {k: round(float(np.median(vs)), 2) for k, vs in per.items()},
                          "matches": int(cnt.item()), "passes": passes, "candidates": n_cand, "kept_bins": ind}), flush=True)


if __name__ == "__main__":
    main()
