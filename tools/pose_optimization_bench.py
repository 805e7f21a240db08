"""Optimizer::PoseOptimization on the device for 200 / 500 / 1 500 edges and for 1 and 8 problems (the relocalisation candidates), beside the path
it replaces:
  new    ORBExtractor.pose_optimization on a C2-sized frame: the median hipEvent span of the enqueued call over --reps (two events around it on the
         handle's stream), and the host clock around the synchronous form
  today  the replaced path as examples/pose_optimization.cpp runs it, built here with -O2 (`bench EDGES KEYPOINTS`): match_kp copied back, applied
         on the host, the plain C++ double loop of the same algorithm, frame_point_row uploaded again - ONE problem; its world is the example's own
         synthetic frame, not the seeded world of the `new` side.  g2o's own figure cannot be taken here: Thirdparty/g2o needs Eigen.
Before timing, the device's counts and flags must equal tests/pose_optimization_cases.py's transcription.  Prints one JSON line per size."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--edges", type=int, nargs="*", default=[200, 500, 1500])
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 8])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import pose_optimization_cases as pc
    from jetson_slam_amd import build as jb, orb
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q = lambda t: dict(median=round(float(np.median(t)), 1), p10=round(float(np.percentile(t, 10)), 1), p90=round(float(np.percentile(t, 90)), 1))
    F = pc.frame("main")
    c = F["c"]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])
    s = torch.cuda.Stream()
    g.set_stream(s.cuda_stream)
    g.extract(F["image"])
    with tempfile.TemporaryDirectory() as tmp:
        exe = jb.build_example("pose_optimization", os.path.join(tmp, "example"), ["-O2"])
        for n_edges in args.edges:
            W = pc.make_world(500 + n_edges, n_edges, stereo=0.5, gross=0.1, n_rows=max(pc.N_ROWS, n_edges))
            ref = pc.reference(W)
            table = orb.MapPointTable(W["n_rows"])
            table.floats[0:3, :W["n_rows"]].copy_(dev(np.ascontiguousarray(W["P"].T)))
            p = W["prm"]
            prm = orb.make_pose_params((p["fx"], p["fy"], p["cx"], p["cy"]), p["bf"], p["inv_level_sigma2"])
            ur = dev(W["u_right"])
            line = dict(edges=n_edges, keypoints=W["N"], inliers=int(ref["counts"][2]))
            for n_problems in args.problems:
                rows = dev(np.repeat(W["rows"][None], n_problems, 0))
                Tcw = dev(np.repeat(W["Tcw"][None], n_problems, 0))
                out = g.pose_optimization(table, prm, rows, Tcw, ur)
                for k in range(n_problems):
                    assert out["counts"][k].cpu().numpy().tolist() == ref["counts"].tolist() and np.array_equal(out["outlier"][k].cpu().numpy(), ref["outlier"])
                span, sync = [], []
                for rep in range(args.reps + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    with torch.cuda.stream(s):
                        e0.record(s)
                        g.pose_optimization(table, prm, rows, Tcw, ur, out=out, wait=False)
                        e1.record(s)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    g.pose_optimization(table, prm, rows, W["Tcw"][None].repeat(n_problems, 0), ur, sync=True, point_rows=False)
                    dt = (time.perf_counter() - t0) * 1e6
                    if rep >= 2:
                        span.append(e0.elapsed_time(e1) * 1e3)
                        sync.append(dt)
                line["new_span_us_%d" % n_problems], line["new_sync_us_%d" % n_problems] = q(span), q(sync)
                line.setdefault("stats_of_%d" % n_problems, g.pose_optimization_stats())
            r = subprocess.run([exe, "bench", str(n_edges), str(W["N"])], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            line["today_us_1"] = float(re.search(r"host_us=([0-9.]+)", r.stdout).group(1))
            line["example"] = r.stdout.strip()
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
