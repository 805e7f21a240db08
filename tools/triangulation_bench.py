"""GPU time of jsorb_search_for_triangulation_async (k_bow_group + k_tri_match + k_tri_resolve) on a jsorb_keyframe_matcher: one call for 1, 10 and
20 neighbours (LocalMapping::CreateNewMapPoints: 10 with a stereo or RGB-D sensor, 20 with a monocular one) at the C1 (320x240, 3 levels, tile 15)
and C2 (752x480, 8 levels, tile 30) keypoint counts.  The keyframe is the left view of a synthetic pair, every neighbour the right view (rectified:
x1^T F12 x2 = y2 - y1, the epipole far outside); the FeatureVector nodes come from a vocabulary sampled from the keyframe's descriptors (k = 10,
L = 3, levels_up 1: about 100 nodes); every fifth keypoint has a map point, every second one a stereo measurement; ORBmatcher matcher(0.6, false):
no orientation check.  Per case: median over --reps of the hipEvent span of the whole call on the matcher's stream.  The time these medians stand
against is the sequential loop of examples/create_new_map_points.cpp on the host (its host_sequential_us, three neighbours at C1).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C1": dict(h=240, w=320, L=3, tile=15), "C2": dict(h=480, w=752, L=8, tile=30)}


def side_of(g, n_levels):
    kp, desc = g.keypoints(), g.descriptors()
    n = len(kp) // 6
    return dict(x=kp[:n].astype(np.float32), y=kp[n:2 * n].astype(np.float32), angle=kp[3 * n:4 * n].astype(np.int32).view(np.float32).copy(),
                octave=kp[4 * n:5 * n].astype(np.int32), desc=np.asarray(desc, np.uint8).reshape(n, 32).copy(),
                free=(np.arange(n) % 5 != 4).astype(np.uint8), stereo=(np.arange(n) % 2).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb, vocabulary
    from jetson_slam_amd.synth import synth_stereo_pair
    lib = orb.load_library()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    m = orb.KeyframeMatcher()
    m.set_stream(stream.cuda_stream)
    result = {"tool": "triangulation_bench", "reps": args.reps, "lanes_per_keypoint": 16, "cases": []}
    for name, c in CONFIGS.items():
        left, right = synth_stereo_pair(31, c["h"], c["w"])
        g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, 20, None, c["tile"], c["tile"])
        g.extract(left)
        K1 = side_of(g, c["L"])
        rng = np.random.default_rng(7)
        tree = vocabulary.sampled_tree(7, K1["desc"][rng.choice(len(K1["desc"]), len(K1["desc"]) // 2, replace=False)], 10, 3)
        voc = orb.Vocabulary(tree, levels_up=1)
        g.extract(right)
        K2 = side_of(g, c["L"])
        for s in (K1, K2):
            s["node"] = orb.bow_transform_descriptors(voc, dev(s["desc"]))[1].cpu().numpy().astype(np.int32)
        scale = np.ones(c["L"], np.float32)
        for l in range(1, c["L"]):
            scale[l] = np.float32(scale[l - 1] * np.float32(1.2))
        prm = orb.make_triangulation_params(scale, check_orientation=False)
        d1 = {k: dev(K1[k]) for k in orb.KeyframeMatcher.KF1_KEYS}
        n1, n2 = len(K1["node"]), len(K2["node"])
        for n_kf in (1, 10, 20):
            d2 = {k: dev(np.concatenate([K2[k]] * n_kf)) for k in orb.KeyframeMatcher.KF2_KEYS}
            ks = (np.arange(n_kf + 1) * n2).astype(np.int32)
            F = np.tile(np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32), n_kf)
            E = np.tile(np.array([1e9, c["h"] / 2], np.float32), n_kf)
            mk = torch.empty(n_kf * max(n1, 1), dtype=torch.int32, device="cuda")
            cnt = torch.empty(n_kf, dtype=torch.int32, device="cuda")
            call = lambda: lib.jsorb_search_for_triangulation_async(m.handle, C.byref(prm), n1, *[d1[k].data_ptr() for k in orb.KeyframeMatcher.KF1_KEYS], n_kf,
                                                                    ks.ctypes.data, *[d2[k].data_ptr() for k in orb.KeyframeMatcher.KF2_KEYS],
                                                                    F.ctypes.data, E.ctypes.data, mk.data_ptr(), cnt.data_ptr())
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
            pairs, dists, lines, largest, _ = m.stats()
            result["cases"].append({"frame": name, "neighbours": n_kf, "kf1_keypoints": n1, "kf2_keypoints": n2, "matches_first": int(cnt[0].item()),
                                    "node_pairs": pairs, "distances": dists, "line_tests": lines, "largest_node": largest,
                                    "median_us": round(float(np.median(spans)), 2), "p10_us": round(float(np.percentile(spans, 10)), 2),
                                    "p90_us": round(float(np.percentile(spans, 90)), 2)})
        voc.close()
    m.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
