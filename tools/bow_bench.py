"""GPU time of jsorb_bow_transform_async (k_bow_transform) and jsorb_search_by_bow_async (k_bow_group + k_bow_match + k_bow_resolve) at the C1
(320x240, 3 levels, tile 15) and C2 (752x480, 8 levels, tile 30) geometries.  The vocabulary is vocabulary.random_tree(k = 10, L = 6): 1 111 111
nodes, the ORB vocabulary's shape with random descriptors (the vocabulary file itself is not needed), levels_up 4.  The keyframe is the left view
of a synthetic pair, the frame the right view; the matcher is timed with 1 keyframe (TrackReferenceKeyFrame) and with 8 copies of it
(Relocalization's candidates).  Per case: median over --reps of the hipEvent span of the whole call on the handle's stream.
The round trip the feature replaces is timed in the same run as the HOST BASELINE: jsorb_copy_descriptors (one blocking copy back, host clock)
plus a single-threaded numpy walk of the same tree over the same descriptors (per level one gather of the current nodes' children and a byte-table
popcount, host clock).  That walk is this project's own stand-in: it is NOT DBoW2, which is not installed here; DBoW2's transform does the same
~60 Hamming distances per keypoint in C++.  For scale the motion-model matcher (jsorb_search_last_frame_async, 1500 points, th 7, one pass: DESIGN
section 12) is timed the same way in the same run on the C2 frame.  Prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C1": dict(h=240, w=320, L=3, tile=15), "C2": dict(h=480, w=752, L=8, tile=30)}
POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int32)


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
    return out


def stats(spans):
    return {"median_us": round(float(np.median(spans)), 2), "p10_us": round(float(np.percentile(spans, 10)), 2), "p90_us": round(float(np.percentile(spans, 90)), 2)}


def numpy_walk(tree, desc, levels_up):
    """the host baseline's tree walk for a UNIFORM tree (every inner node k children, ids breadth-first): all descriptors one level at a time"""
    cs, ch, D, k = tree["child_start"], tree["children"], tree["descriptors"], tree["k"]
    cur = np.zeros(len(desc), np.int64)
    node = np.zeros(len(desc), np.int64)
    for level in range(1, tree["depth_L"] + 1):
        kids = ch[cs[cur][:, None] + np.arange(k)[None, :]]                          # n x k child ids
        d = POP8[D[kids] ^ desc[:, None, :]].sum(axis=2)                             # n x k Hamming distances
        cur = kids[np.arange(len(desc)), np.argmin(d, axis=1)].astype(np.int64)       # argmin: the first minimum, as the strict <
        if level == tree["depth_L"] - levels_up:
            node = cur.copy()
    return tree["word_id"][cur], np.where(tree["weight"][cur] > 0, node, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=6)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb, vocabulary
    from jetson_slam_amd.synth import synth_stereo_pair
    lib = orb.load_library()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()            # a stream of its own: the events below bracket the handle's work
    torch.cuda.set_stream(stream)
    levels_up = min(4, args.L)
    tree = vocabulary.random_tree(0, args.k, args.L)
    voc = orb.Vocabulary(tree, levels_up=levels_up)
    print(json.dumps({"vocabulary": voc.info(), "kind": "random_tree"}), flush=True)
    for name, c in CONFIGS.items():
        h, w = c["h"], c["w"]
        left, right = synth_stereo_pair(31, h, w)
        g = orb.ORBExtractor(h, w, 1.2, c["L"], 9, 14, 7, 20, None, c["tile"], c["tile"])
        g.set_stream(stream.cuda_stream)
        kp, desc = g.extract(left)
        n_kf = len(kp) // 6
        kp, desc = kp.copy(), desc.copy()
        g.bow_transform(voc)
        kf_node = g.bow()[1].copy()
        g.extract(right)
        N = g.n_keypoints(0)
        # the transform
        call = lambda: lib.jsorb_bow_transform_async(g.handle, 0, voc.handle)
        torch.cuda.synchronize()
        spans = spans_us(torch, stream, call, args.reps)
        word, node = g.bow()
        print(json.dumps(dict({"frame": name, "case": "bow_transform", "keypoints": N, "distinct_nodes": int(len(set(node.tolist()))),
                               "shallow": g.bow_transform_stats()}, **stats(spans))), flush=True)
        # the host baseline: the copy back, then the walk
        buf = np.zeros((N, 32), np.uint8)
        t_copy, t_walk = [], []
        for _ in range(max(args.reps // 10, 5)):
            t0 = time.perf_counter()
            assert lib.jsorb_copy_descriptors(g.handle, 0, buf.ctypes.data) == 0
            t1 = time.perf_counter()
            hw, hn = numpy_walk(tree, buf, levels_up)
            t2 = time.perf_counter()
            t_copy.append((t1 - t0) * 1e6)
            t_walk.append((t2 - t1) * 1e6)
        assert np.array_equal(hw, word) and np.array_equal(hn, node), "the host walk and the device disagree"
        print(json.dumps({"frame": name, "case": "host_baseline", "kind": "jsorb_copy_descriptors + single-threaded numpy tree walk (not DBoW2)",
                          "keypoints": N, "copy_back_median_us": round(float(np.median(t_copy)), 2), "walk_median_us": round(float(np.median(t_walk)), 2)}), flush=True)
        # the matcher: 1 keyframe and 8
        angle = kp[3 * n_kf:4 * n_kf].astype(np.int32).view(np.float32)
        prm = orb.make_bow_params(0.7)
        for n_keyframes in (1, 8):
            ks = (np.arange(n_keyframes + 1) * n_kf).astype(np.int32)
            tens = [dev(np.tile(kf_node.astype(np.int32), n_keyframes)), dev(np.ones(n_kf * n_keyframes, np.uint8)), dev(np.tile(angle, n_keyframes)),
                    dev(np.tile(desc, (n_keyframes, 1)))]
            mk = torch.empty(n_keyframes * max(N, 1), dtype=torch.int32, device="cuda")
            cnt = torch.empty(n_keyframes, dtype=torch.int32, device="cuda")
            call = lambda: lib.jsorb_search_by_bow_async(g.handle, 0, C.byref(prm), None, n_keyframes, ks.ctypes.data, *[t.data_ptr() for t in tens],
                                                         mk.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            spans = spans_us(torch, stream, call, args.reps)
            pairs, dists, largest, ind = g.search_by_bow_stats()
            print(json.dumps(dict({"frame": name, "case": "search_by_bow", "keyframes": n_keyframes, "keyframe_keypoints": n_kf, "keypoints": N,
                                   "matches": cnt.cpu().tolist()[:2], "node_pairs": pairs, "distances": dists, "largest_node": largest, "kept_bins": ind},
                                  **stats(spans))), flush=True)
        g.enable_kernel_timing(True)
        for _ in range(20):
            assert lib.jsorb_bow_transform_async(g.handle, 0, voc.handle) == 0 and call() == 0
        kt = g.bow_kernel_times()
        g.enable_kernel_timing(False)
        print(json.dumps({"frame": name, "case": "per_kernel_mean_us_8_keyframes", **{k: round(v[0] * 1e3 / max(v[1], 1), 2) for k, v in kt.items()}}), flush=True)
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
        print(json.dumps(dict({"frame": name, "case": "motion_model_matcher_for_scale", "points": n, "th": 7, "matches": int(cnt.item())}, **stats(spans))), flush=True)


if __name__ == "__main__":
    main()
