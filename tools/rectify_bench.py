"""Cost of rectifying raw images on the device (k_rectify) at C2 (752 x 480, 8 levels, tile 30): one JSON line.

The step is bench.py's: 128 device-resident stereo pairs per step, left and right batches + the batched stereo match, four input sets of
synthetic pairs rotated through the steps (the same seeds bench.py uses).  Measured in ONE process, blocks of steps alternating between a
handle pair without maps and one with EuRoC-like maps (left and right differ), so that both see the same box:
  pairs_per_s_plain / pairs_per_s_rectified   medians over the blocks, and their ratio
  k_rectify_ms_per_step                        per-kernel hipEvent timing on a one-lane handle pair (serialised launches, both images of 128 pairs)
  frame_latency_us_plain / _rectified          median of the synchronous single-frame call shape (extract L, extract R, match) from Python
  parity                                       the last rectified step's outputs (every pair of the set) against the CPU oracle run on the
                                               numpy-rectified images (tests/test_gpu_rectify.py restates the same arithmetic)
Usage: python tools/rectify_bench.py [--steps 20 --warmup 5 --blocks 5 --frames 300]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def remap_ref(src, mapx, mapy):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) in OpenCV's fixed-point form (include/jsorb.h, k_rectify.hip)"""
    H, W = src.shape
    with np.errstate(invalid="ignore", over="ignore"):
        fxy = [np.asarray(m, np.float32) * np.float32(32) for m in (mapx, mapy)]
    XY = []
    for f in fxy:
        ok = np.isfinite(f) & (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
        XY.append(np.where(ok, np.rint(np.where(ok, f, 0)).astype(np.float64), -2147483648.0).astype(np.int64))
    X, Y = XY
    ix, iy, fx, fy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767), X & 31, Y & 31
    acc = np.zeros(src.shape, np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            sx, sy = ix + dx, iy + dy
            inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            acc += np.where(inside, src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(np.int64) * wx * wy, 0)
    return ((acc + 512) >> 10).astype(np.uint8)


def euroc_like_maps(h, w, right):
    """made-up EuRoC-like calibration (barrel distortion k1 ~ -0.28, a small rectifying rotation); left and right differ"""
    from jetson_slam_amd.rectify import undistort_rectify_map
    if right:
        K, D, ang = [[457.6, 0, 379.9], [0, 456.1, 255.2], [0, 0, 1]], [-0.284, 0.0745, -1.0e-4, -3.5e-5], [0.3, -0.5, 0.3]
    else:
        K, D, ang = [[458.7, 0, 367.4], [0, 457.3, 248.6], [0, 0, 1]], [-0.283, 0.0741, 1.9e-4, 1.7e-5], [0.4, -0.7, 0.25]
    c, s = np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
    R = (np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]) @ np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
         @ np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]]))
    P = np.array([[435.2, 0, 367.2, 0], [0, 435.2, 252.1, 0], [0, 0, 1, 0]])
    return undistort_rectify_map(np.array(K, float), D, R, P, w, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per arm (alternating plain / rectified)")
    ap.add_argument("--frames", type=int, default=300, help="single frames per arm for the latency medians")
    ap.add_argument("--pairs", type=int, default=128)
    args = ap.parse_args()

    from multiprocessing import Pool
    from jetson_slam_amd.synth import synth_stereo_pair

    H, W, L, tile, th, fx, bf = 480, 752, 8, 30, 20, 435.2, 47.906
    P, n_sets = args.pairs, 4
    mb = bf / fx
    seeds = [1 + si * P + i for si in range(n_sets) for i in range(P)]          # bench.py's input sets (seed_base 1, one rank)
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool:                # (before anything touches the GPU)
        pairs = pool.starmap(synth_stereo_pair, [(s, H, W) for s in seeds])
    import torch
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    from jetson_slam_amd import orb
    sets_u = [(np.stack([p[0] for p in pairs[si * P:(si + 1) * P]]), np.stack([p[1] for p in pairs[si * P:(si + 1) * P]])) for si in range(n_sets)]
    sets_d = [(torch.from_numpy(l).to(dev), torch.from_numpy(r).to(dev)) for l, r in sets_u]
    ml, mr = euroc_like_maps(H, W, False), euroc_like_maps(H, W, True)

    mk = lambda b=P: orb.ORBExtractor(H, W, 1.2, L, 9, 14, 7, th, None, tile, tile, max_batch=b)
    plain, rect = (mk(), mk()), (mk(), mk())
    rect[0].set_rectify_maps(*ml)
    rect[1].set_rectify_maps(*mr)
    cur = [0]

    def step(hp, si=None):
        si = cur[0] if si is None else si
        cur[0] = (si + 1) % n_sets
        ld, rd = sets_d[si]
        hp[0].extract_batch_device_async(ld.data_ptr(), H * W, W, P, keep=ld)
        hp[1].extract_batch_device_async(rd.data_ptr(), H * W, W, P, keep=rd)
        orb.stereo_match_batch_async(hp[0], hp[1], mb, bf)

    def fence(hp):
        hp[0].sync(); hp[1].sync()
        torch.cuda.synchronize(dev)

    def block(hp):
        fence(hp)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(hp)
        fence(hp)
        return time.perf_counter() - t0

    for hp in (plain, rect):
        for _ in range(args.warmup):
            step(hp)
        fence(hp)
    t_plain, t_rect = [], []
    for _ in range(args.blocks):
        t_plain.append(block(plain))
        t_rect.append(block(rect))
    pps_plain = args.steps * P / float(np.median(t_plain))
    pps_rect = args.steps * P / float(np.median(t_rect))

    # parity: one more rectified step on set 0, every pair against the oracle on numpy-rectified images
    step(rect, 0)
    fence(rect)
    from oracle import pyoracle as po
    po.build()
    okw = dict(height=H, width=W, n_levels=L, tile_h=tile, tile_w=tile, th_fast_max=th)
    n_bad = 0
    for i in range(P):
        rl, rr = remap_ref(sets_u[0][0][i], *ml), remap_ref(sets_u[0][1][i], *mr)
        ol, orr_ = po.OracleExtractor(**okw), po.OracleExtractor(**okw)
        ol.extract(rl); orr_.extract(rr)
        ou, od, ost = po.stereo_match(ol, orr_, mb, bf)
        u, d, st = orb.stereo_result(rect[0], i)
        ok = (np.array_equal(rect[0].level_image(0, i), rl) and np.array_equal(rect[1].level_image(0, i), rr)
              and np.array_equal(rect[0].keypoints(i), ol.keypoints()) and np.array_equal(rect[0].descriptors(i), ol.descriptors())
              and np.array_equal(rect[1].keypoints(i), orr_.keypoints()) and np.array_equal(rect[1].descriptors(i), orr_.descriptors())
              and np.array_equal(u.view(np.uint32), ou.view(np.uint32)) and np.array_equal(d.view(np.uint32), od.view(np.uint32))
              and st["n_final"] == ost["n_final"])
        n_bad += 0 if ok else 1

    # k_rectify time per step: per-kernel timing (one lane, serialised) on a separate rectified pair
    tl, tr = mk(), mk()
    tl.set_rectify_maps(*ml); tr.set_rectify_maps(*mr)
    step((tl, tr)); fence((tl, tr))
    for h in (tl, tr):
        h.enable_kernel_timing(True); h.reset_kernel_timing()
    n_prof = 5
    for _ in range(n_prof):
        step((tl, tr))
    fence((tl, tr))
    rect_ms = (tl.rectify_kernel_time()[0] + tr.rectify_kernel_time()[0]) / n_prof
    stage_ms = sum(v[0] for h in (tl, tr) for v in h.kernel_times().values()) / n_prof

    # single-frame latency (extract L, extract R, match), medians
    lat = {}
    l0, r0 = sets_u[0][0][0], sets_u[0][1][0]
    for name, maps in (("plain", None), ("rectified", (ml, mr))):
        a, b = mk(1), mk(1)
        if maps:
            a.set_rectify_maps(*maps[0]); b.set_rectify_maps(*maps[1])
        ts = []
        for k in range(args.frames + 20):
            t0 = time.perf_counter()
            a.extract(l0); b.extract(r0)
            orb.compute_stereo_matches(a, b, mb, bf)
            if k >= 20:
                ts.append(time.perf_counter() - t0)
        lat[name] = float(np.median(ts)) * 1e6

    print(json.dumps({
        "config": "c2", "pairs_per_step": P, "steps": args.steps, "blocks": args.blocks,
        "pairs_per_s_plain": round(pps_plain, 1), "pairs_per_s_rectified": round(pps_rect, 1),
        "rectified_step_over_plain": round(pps_plain / pps_rect, 4),
        "ms_per_step_plain": round(1e3 * P / pps_plain, 4), "ms_per_step_rectified": round(1e3 * P / pps_rect, 4),
        "k_rectify_ms_per_step": round(rect_ms, 4), "pipeline_kernels_ms_per_step_serialised": round(stage_ms, 4),
        "frame_latency_us_plain": round(lat["plain"], 1), "frame_latency_us_rectified": round(lat["rectified"], 1),
        "parity": n_bad == 0, "parity_pairs": P, "parity_mismatches": n_bad,
        "latency_note": "median wall time of extract(L) + extract(R) + compute_stereo_matches from Python, one thread",
    }))


if __name__ == "__main__":
    main()
