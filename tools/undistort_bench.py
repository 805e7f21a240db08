"""Cost of the mono / RGB-D Frame steps on the device (k_undistort, k_rgbd): one JSON line.

  images_per_s_plain / _camera     C2 geometry (752 x 480, 8 levels, tile 30), 128 device-resident images per step (bench.py's left images),
                                   blocks of steps alternating between a handle without a camera and one with the EuRoC mono camera; medians and
                                   their ratio
  k_undistort_ms_per_step          per-kernel hipEvent timing on a one-lane handle (serialised launches) of the same 128-image step; k_rgbd_ms_per_step
                                   likewise for the batched depth sample of those images (u16 depth in device memory)
  frame_us_plain / _camera         median of the synchronous mono frame (jsorb_extract + jsorb_unpack_frame_un: mvKeys, mvKeysUn, descriptors) at C2
  rgbd_us / rgbd_frame_us          640 x 480 TUM1 camera, u16 depth: median of jsorb_rgbd_depth alone, and of the whole RGB-D frame (extract, unpack,
                                   depth sample)
Usage: python tools/undistort_bench.py [--steps 20 --warmup 5 --blocks 5 --frames 300]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

EUROC = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]], np.float32), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
TUM1 = np.array([[517.306408, 0, 318.643040], [0, 516.469215, 255.313989], [0, 0, 1]], np.float32), (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--images", type=int, default=128)
    args = ap.parse_args()

    from multiprocessing import Pool
    from jetson_slam_amd.synth import synth_stereo_pair

    H, W, L, tile, th = 480, 752, 8, 30, 20
    B = args.images
    with Pool(min(16, len(os.sched_getaffinity(0)))) as pool:                # (before anything touches the GPU)
        pairs = pool.starmap(synth_stereo_pair, [(1 + i, H, W) for i in range(B)] + [(9001, 480, 640)])
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    imgs = np.stack([p[0] for p in pairs[:B]])
    dev = torch.from_numpy(imgs).cuda()
    rng = np.random.default_rng(3)
    depth = rng.integers(0, 40000, (B, H, W)).astype(np.uint16)
    ddev = torch.from_numpy(depth.view(np.int16)).cuda()
    torch.cuda.synchronize()

    def mk(max_batch, camera):
        g = orb.ORBExtractor(H, W, 1.2, L, 9, 14, 7, th, None, tile, tile, max_batch=max_batch)
        if camera:
            g.set_camera(*EUROC)
        return g

    def step(g):
        g.extract_batch_device_async(dev.data_ptr(), H * W, W, B, keep=dev)
        g.sync()

    arms = {"plain": mk(B, False), "camera": mk(B, True)}
    for g in arms.values():
        for _ in range(args.warmup):
            step(g)
    rates = {k: [] for k in arms}
    for _ in range(args.blocks):
        for k, g in arms.items():
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(g)
            rates[k].append(B * args.steps / (time.perf_counter() - t0))
    out = {"geometry": "C2 752x480 L8 tile30", "images_per_step": B}
    for k in arms:
        out["images_per_s_" + k] = round(float(np.median(rates[k])), 1)
    out["camera_over_plain"] = round(out["images_per_s_camera"] / out["images_per_s_plain"], 4)

    # per-kernel times: a one-lane handle (timing serialises the launches)
    t = mk(B, True)
    t.enable_kernel_timing(True)
    step(t)
    t.rgbd_depth(ddev, 40.0, 1.0 / 5000)
    t.sync()
    t.reset_kernel_timing()
    for _ in range(args.steps):
        step(t)
        t.rgbd_depth(ddev, 40.0, 1.0 / 5000)
        t.sync()
    out["k_undistort_ms_per_step"] = round(t.undistort_kernel_time()[0] / args.steps, 4)
    out["k_rgbd_ms_per_step"] = round(t.rgbd_kernel_time()[0] / args.steps, 4)
    out["k_describe_ms_per_step"] = round(t.kernel_times()["k_describe"][0] / args.steps, 4)

    # synchronous frames through the C ABI (ctypes, preallocated outputs)
    lib = orb.load_library()

    def frame_us(g, img, depth_img=None):
        n = C.c_int()
        cap = g.T
        keys, keys_un = np.zeros(cap, orb.KEYPOINT_DTYPE), np.zeros(cap, orb.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        u, d = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        ts, tr = [], []
        for it in range(args.frames + 20):
            t0 = time.perf_counter()
            g._chk(lib.jsorb_extract(g.handle, img.ctypes.data, img.strides[0], C.byref(n)))
            g._chk(lib.jsorb_unpack_frame_un(g.handle, 0, keys.ctypes.data, keys_un.ctypes.data, desc.ctypes.data))
            t1 = time.perf_counter()
            if depth_img is not None:
                g._chk(lib.jsorb_rgbd_depth(g.handle, depth_img.ctypes.data, orb.DEPTH_U16, depth_img.strides[0], C.c_float(1.0 / 5000), C.c_float(40.0),
                                            u.ctypes.data, d.ctypes.data))
            t2 = time.perf_counter()
            if it >= 20:
                ts.append((t2 - t0) * 1e6)
                tr.append((t2 - t1) * 1e6)
        return float(np.median(ts)), float(np.median(tr))

    f_plain, f_cam = mk(1, False), mk(1, True)
    out["frame_us_plain"] = round(frame_us(f_plain, imgs[0])[0], 1)
    out["frame_us_camera"] = round(frame_us(f_cam, imgs[0])[0], 1)
    out["frame_us_plain_again"] = round(frame_us(f_plain, imgs[0])[0], 1)
    g = orb.ORBExtractor(480, 640, 1.2, 8, 9, 14, 7, 20, None, 30, 30)
    g.set_camera(*TUM1)
    d640 = np.ascontiguousarray(depth[0, :, :640])
    full, dep = frame_us(g, np.ascontiguousarray(pairs[B][0]), d640)
    out["rgbd_frame_us"] = round(full, 1)
    out["rgbd_us"] = round(dep, 1)
    out["rgbd_n_keypoints"] = g.n_keypoints(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
