"""GPU time of the three matchers of LoopClosing::ComputeSim3 on a jsorb_keyframe_matcher: jsorb_search_by_bow_kf_async (k_bow_group +
k_loop_bow_match + k_tri_resolve) for the current keyframe against 1, 3 and 10 loop candidates in one call, jsorb_search_by_sim3_async
(k_fuse_grids x 2 + k_sim3_match + k_sim3_agree) for one keyframe pair, and jsorb_search_by_projection_sim3_async (k_fuse_grids + k_scw_candidates +
k_scw_resolve) for 2 000 and 8 000 loop points against the current keyframe, beside the sequential loop of examples/compute_sim3.cpp on the same
inputs (-O2, one thread, this machine).  The current keyframe is the left view of a synthetic pair at C2 (752x480,
8 levels, tile 30), the candidates are the right and left views in turn; the vocabulary is sampled from the left view's descriptors (10 children, 3
levels, nodes one level above the words), nine keypoints in ten carry a map point.  For the Sim3 call the map points are the keypoints back-projected
at depth 4, the right camera a baseline beside the left one and the similarity between them that baseline, slightly off.  The loop points are
the keypoints of both views back-projected the same way, drawn with replacement, a fifth of them with a descriptor beyond TH_LOW; a quarter of the
current keyframe's keypoints hold a point before the call.  Per case: median over --reps
of the hipEvent span of the whole call on the matcher's stream.  Nobody has measured these calls before: there is no time to stand against.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C2 = dict(h=480, w=752, L=8, tile=30)
FX, BF = 435.2, 47.906


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    from jetson_slam_amd import vocabulary as V
    from jetson_slam_amd.synth import synth_stereo_pair
    lib = orb.load_library()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    m = orb.KeyframeMatcher()
    m.set_stream(stream.cuda_stream)
    c = C2
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, 20, None, c["tile"], c["tile"])
    rng = np.random.default_rng(7)
    frames = []
    for img in synth_stereo_pair(31, c["h"], c["w"]):
        g.extract(img)
        kp = g.keypoints()
        N = len(kp) // 6
        frames.append(dict(x=kp[:N].astype(np.float32), y=kp[N:2 * N].astype(np.float32), angle=kp[3 * N:4 * N].astype(np.int32).view(np.float32).copy(),
                           octave=kp[4 * N:5 * N].astype(np.int32), desc=np.asarray(g.descriptors(), np.uint8).reshape(N, 32).copy(),
                           valid=(rng.random(N) < 0.9).astype(np.uint8)))
    left, right = frames
    sample = left["desc"][rng.choice(len(left["desc"]), len(left["desc"]) // 2, replace=False)]
    voc = orb.Vocabulary(V.sampled_tree(7, sample, 10, 3), levels_up=1)
    for f in frames:
        f["node"] = orb.bow_transform_descriptors(voc, dev(f["desc"]))[1].cpu().numpy()

    def spans(call):
        torch.cuda.synchronize()
        for _ in range(10):
            assert call() == 0
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            assert call() == 0
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return {"median_us": round(float(np.median(out)), 2), "p10_us": round(float(np.percentile(out, 10)), 2), "p90_us": round(float(np.percentile(out, 90)), 2)}

    result = {"tool": "loop_bench", "reps": args.reps, "frame": "C2", "keypoints": [len(left["x"]), len(right["x"])], "node_regs": orb.loop_build_caps(),
              "bow": [], "sim3": None, "scw": []}
    keys = orb.KeyframeMatcher.BOW_KF_KEYS
    n1 = len(left["x"])
    d1 = {k: dev(left[k]) for k in keys}
    prm = orb.make_bow_params(nn_ratio=0.75)
    for n_kf in (1, 3, 10):
        cands = [right if i % 2 == 0 else left for i in range(n_kf)]
        d2 = {k: dev(np.concatenate([f[k] for f in cands])) for k in keys}
        ks = np.cumsum([0] + [len(f["x"]) for f in cands]).astype(np.int32)
        mk = torch.empty(n_kf * n1, dtype=torch.int32, device="cuda")
        cnt = torch.empty(n_kf, dtype=torch.int32, device="cuda")
        p1, p2 = [d1[k].data_ptr() for k in keys], [d2[k].data_ptr() for k in keys]
        row = {"candidates": n_kf, "candidate_keypoints": int(ks[-1])}
        row.update(spans(lambda: lib.jsorb_search_by_bow_kf_async(m.handle, C.byref(prm), n1, *p1, n_kf, ks.ctypes.data, *p2, mk.data_ptr(), cnt.data_ptr())))
        pairs, dists, largest, _ = m.search_by_bow_kf_stats()
        row.update(matches=[int(v) for v in cnt.cpu()], node_pairs=pairs, distances=dists, largest_node=largest)
        result["bow"].append(row)
    # one pair: left as keyframe 1, right as keyframe 2
    scale = np.ones(c["L"], np.float32)
    for l in range(1, c["L"]):
        scale[l] = np.float32(scale[l - 1] * np.float32(1.2))
    cx, cy, z, base = c["w"] / 2, c["h"] / 2, 4.0, BF / FX
    sp = orb.make_sim3_params((FX, FX, cx, cy), (0, c["w"], 0, c["h"]), (64 / c["w"], 48 / c["h"]), float(np.log(np.float32(1.2))), scale)
    eye = np.eye(3, dtype=np.float32).ravel()
    sides = []
    for f, tw, s_other, t_other in ((left, [0, 0, 0], 1 / 1.02, [-base / 1.02 + 0.002, 0.001, 0]), (right, [-base, 0, 0], 1.02, [base - 0.002, -0.001, 0])):
        Pc = np.stack([(f["x"] - cx) * z / FX, (f["y"] - cy) * z / FX, np.full(len(f["x"]), z)])
        dist = np.sqrt((Pc * Pc).sum(0))
        maxd = (dist * scale[f["octave"]]).astype(np.float32)
        Pw = Pc - np.asarray(tw, np.float64)[:, None]
        d = dict(x=dev(f["x"]), y=dev(f["y"]), octave=dev(f["octave"]), kp_desc=dev(f["desc"]), mp_desc=dev(f["desc"]), search=dev(f["valid"]),
                 Px=dev(Pw[0].astype(np.float32)), Py=dev(Pw[1].astype(np.float32)), Pz=dev(Pw[2].astype(np.float32)), max_distance=dev(maxd),
                 min_dist_inv=dev(np.float32(0.8) * maxd / scale[-1]), max_dist_inv=dev(np.float32(1.2) * maxd),
                 Rw=eye, tw=np.asarray(tw, np.float32), sR=np.float32(s_other) * eye, t=np.asarray(t_other, np.float32))
        sides.append(d)
    s1, s2, a = m._sim3_args(sides[0], sides[1], sp)
    out = [torch.empty(max(s1.n, s2.n), dtype=torch.int32, device="cuda") for _ in range(4)]
    row = {"keypoints": [s1.n, s2.n]}
    row.update(spans(lambda: lib.jsorb_search_by_sim3_async(m.handle, *a, *[o.data_ptr() for o in out])))
    windows, walked, dists, largest, agree = m.search_by_sim3_stats()
    row.update(windows=windows, walked=walked, distances=dists, largest_window=largest, found=agree)
    result["sim3"] = row
    # the acceptance test: the loop points against the left view, Scw = the identity scaled by 1.02 (the points' world frame is the left camera's)
    import subprocess
    import tempfile
    from jetson_slam_amd import build as jb
    tmp = tempfile.mkdtemp()
    exe = jb.build_example("compute_sim3", os.path.join(tmp, "compute_sim3"), ["-O2"])
    S = np.eye(4, dtype=np.float32)
    S[:3, :3] *= np.float32(1.02)
    S[:3, 3] = np.float32(1.02) * np.array([0.002, -0.001, 0.0], np.float32)
    cp = orb.scw_params((FX, FX, cx, cy), (0, c["w"], 0, c["h"]), (64 / c["w"], 48 / c["h"]), float(np.log(np.float32(1.2))), scale, *orb.scw_from_pose(S))
    N = len(left["x"])
    blocked = (rng.random(N) < 0.25).astype(np.uint8)
    kf = dict(x=dev(left["x"]), y=dev(left["y"]), octave=dev(left["octave"]), desc=dev(left["desc"]), blocked=dev(blocked))
    pool = []
    for f, tw in ((left, [0, 0, 0]), (right, [-base, 0, 0])):
        Pc = np.stack([(f["x"] - cx) * z / FX, (f["y"] - cy) * z / FX, np.full(len(f["x"]), z)])
        Pw = Pc - np.asarray(tw, np.float64)[:, None]
        o = Pw - (-np.asarray(tw, np.float64))[:, None]
        dist = np.sqrt((o * o).sum(0))
        maxd = (dist * scale[f["octave"]]).astype(np.float32)
        pool.append(dict(pos=Pw.T.astype(np.float32), normal=(o / dist).T.astype(np.float32), maxd=maxd, mindi=(np.float32(0.8) * maxd / scale[-1]).astype(np.float32),
                         maxdi=(np.float32(1.2) * maxd).astype(np.float32), desc=f["desc"]))
    pool = {k: np.concatenate([q[k] for q in pool]) for k in pool[0]}
    for n in (2000, 8000):
        pick = rng.integers(0, len(pool["maxd"]), n)
        P = {k: np.ascontiguousarray(v[pick]) for k, v in pool.items()}
        far = rng.random(n) < 0.2
        P["desc"][far] ^= rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)
        pts = dict(Px=dev(P["pos"][:, 0]), Py=dev(P["pos"][:, 1]), Pz=dev(P["pos"][:, 2]), Nx=dev(P["normal"][:, 0]), Ny=dev(P["normal"][:, 1]),
                   Nz=dev(P["normal"][:, 2]), max_distance=dev(P["maxd"]), min_dist_inv=dev(P["mindi"]), max_dist_inv=dev(P["maxdi"]), desc=dev(P["desc"]))
        _, _, _, a = m._scw_args(pts, kf, cp)
        out = [torch.empty(max(n, N), dtype=torch.int32, device="cuda") for _ in range(4)]
        row = {"loop_points": n, "keypoints": N, "blocked": int(blocked.sum()), "caps": list(orb.scw_build_caps())}
        row.update(spans(lambda: lib.jsorb_search_by_projection_sim3_async(m.handle, *m._c_args(a), *[o.data_ptr() for o in out])))
        rounds, kept, over, windows, dists, largest = m.search_by_projection_sim3_stats()
        row.update(matches=int(out[3].cpu()[0]), rounds=rounds, keys_kept=kept, over_cap=over, windows=windows, distances=dists, largest_window=largest)
        path = os.path.join(tmp, "scw_%d.bin" % n)
        with open(path, "wb") as fh:
            fh.write(np.array([N, n], np.int32).tobytes() + bytes(cp))
            for v in (left["x"], left["y"], left["octave"], left["desc"], blocked):
                fh.write(np.ascontiguousarray(v).tobytes())
            fh.write(np.concatenate([P["pos"], P["normal"], P["maxd"][:, None], P["mindi"][:, None], P["maxdi"][:, None]], 1).astype(np.float32).tobytes())
            fh.write(P["desc"].tobytes())
        host = subprocess.run([exe, "--scw-host-loop", path, "21"], capture_output=True, text=True, check=True).stdout.split()
        hv = dict(kv.split("=") for kv in host[1:])
        assert int(hv["nmatches"]) == row["matches"], (hv, row["matches"])      # the same loop on the same inputs
        row["host_loop_median_us"] = float(hv["median_us"])
        result["scw"].append(row)
    m.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
