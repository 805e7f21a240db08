"""GPU time of jsorb_search_by_projection_kf_async (k_assign_grid + k_kf_candidates + k_kf_resolve) on one C1 (320x240, 3 levels, tile 15) and one C2
(752x480, 8 levels, tile 30) frame: 500 / 1500 keyframe points back-projected from keypoints through a slightly perturbed pose, with distance
ranges that predict the keypoint's octave +-1, at th 10 / ORBdist 100 and at th 3 / ORBdist 64 (Tracking.cpp:2065, :2079).  Per case: median over
--reps of the hipEvent span of the whole call on the handle's stream (grid included), the per-kernel hipEvent times (jsorb_enable_kernel_timing, a
separate pass: it serialises launches), rounds, candidates and overflowed points.  For scale, jsorb_search_local_points_async on the same frame
and point count (th 1, monocular, the projections and levels of the same points) is timed the same way in the same run.  No time is a pass
criterion.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C1": dict(h=240, w=320, L=3, tile=15), "C2": dict(h=480, w=752, L=8, tile=30)}


def spans_us(torch, stream, call, reps):
    for _ in range(10):
        assert call() == 0
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        assert call() == 0
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(float(np.median(out)), 2), "p10_us": round(float(np.percentile(out, 10)), 2), "p90_us": round(float(np.percentile(out, 90)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    from jetson_slam_amd.synth import synth_stereo_pair
    lib = orb.load_library()
    fx = 435.2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for name, c in CONFIGS.items():
        h, w, L, tile = c["h"], c["w"], c["L"], c["tile"]
        g = orb.ORBExtractor(h, w, 1.2, L, 9, 14, 7, 20, None, tile, tile)
        kp, desc = g.extract(synth_stereo_pair(31, h, w)[0])
        N = len(kp) // 6
        stream = torch.cuda.Stream()            # a stream of its own: the events bracket the handle's work (the null stream would not be adopted)
        torch.cuda.set_stream(stream)
        g.set_stream(stream.cuda_stream)
        x, y, octave = kp[:N].astype(np.float32), kp[N:2 * N].astype(np.float32), kp[4 * N:5 * N]
        angle = kp[3 * N:4 * N].astype(np.int32).view(np.float32)
        scale = g.get_scale_factors()
        cx, cy = np.float32(w / 2), np.float32(h / 2)
        R, t = np.eye(3, dtype=np.float32), np.array([0.002, -0.001, 0.003], np.float32)
        grid = (np.float32(64) / np.float32(w), np.float32(48) / np.float32(h))
        print(json.dumps({"frame": "%s %dx%d L%d tile%d" % (name, w, h, L, tile), "keypoints": N}), flush=True)
        for n, th, orb_dist in [(500, 10, 100), (1500, 10, 100), (500, 3, 64), (1500, 3, 64)]:
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
            prm = orb.make_kf_projection_params(R, t, (fx, fx, cx, cy), (0, w, 0, h), grid, float(np.log(np.float32(1.2))), th=th, orb_dist=orb_dist)
            dist = np.sqrt(((P.astype(np.float64) - np.array(list(prm.Ow))[:, None]) ** 2).sum(0))
            maxd = (dist * 1.2 ** (lvl - 0.5)).astype(np.float32)                      # PredictScale gives lvl
            tens = [dev(a) for a in (P[0], P[1], P[2], maxd, maxd * np.float32(1.2), np.float32(0.8) * maxd / scale[-1], ang, d)]
            mk, md = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
            km = torch.empty(N, dtype=torch.int32, device="cuda")
            cnt = torch.empty(1, dtype=torch.int32, device="cuda")
            call = lambda: lib.jsorb_search_by_projection_kf_async(g.handle, 0, C.byref(prm), n, *[a.data_ptr() for a in tens], None, mk.data_ptr(),
                                                                   md.data_ptr(), km.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            res = spans_us(torch, stream, call, args.reps)
            g.enable_kernel_timing(True)
            per = {k: [] for k in ("k_assign_grid", "k_kf_candidates", "k_kf_resolve")}
            for _ in range(min(args.reps, 50)):
                g.reset_kernel_timing()
                assert call() == 0
                for k, (ms, _) in g.search_by_projection_kf_kernel_times().items():
                    per[k].append(ms * 1e3)
            g.enable_kernel_timing(False)
            rounds, n_cand, n_over, ind = g.search_by_projection_kf_stats()
            # for scale: the local-map matcher over the same points (their projections and levels), th 1, monocular
            u = (fx * P[0] / P[2] + cx).astype(np.float32)
            v = (fx * P[1] / P[2] + cy).astype(np.float32)
            lt = [dev(a) for a in (u, v, (1 / P[2]).astype(np.float32), lvl, np.ones(n, np.float32), np.ones(n, np.uint8), d)]
            sp = orb.JsorbSearchParams(1.0, 0.8, 100, 0.0, 0.0, 0.0, float(grid[0]), float(grid[1]), 64, 48)
            local = lambda: lib.jsorb_search_local_points_async(g.handle, 0, C.byref(sp), n, *[a.data_ptr() for a in lt], None, None, mk.data_ptr(),
                                                                md.data_ptr(), km.data_ptr(), cnt.data_ptr())
            assert call() == 0
            torch.cuda.synchronize()
            matches = int(cnt.item())
            loc = spans_us(torch, stream, local, args.reps)
            print(json.dumps(dict({"frame": name, "points": n, "th": th, "orb_dist": orb_dist}, **res,
                                  **{"kernel_median_us": {k: round(float(np.median(vs)), 2) for k, vs in per.items()}, "matches": matches, "rounds": rounds,
                                     "candidates": n_cand, "overflowed_points": n_over, "kept_bins": ind,
                                     "search_local_points_median_us": loc["median_us"]})), flush=True)
        g.set_stream(None)
        g.close()


if __name__ == "__main__":
    main()
