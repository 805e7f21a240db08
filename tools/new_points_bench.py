"""LocalMapping::CreateNewMapPoints for a C2-sized keyframe (--keypoints per keyframe) against 10 and 20 neighbours, two ways:
  new    KeyframeMatcher.create_new_map_points on the device state: the median hipEvent span of the enqueued call over --reps, the map reloaded
         in front of every repetition (outside the span), and the host clock around the synchronous form
  today  the path it replaces, as examples/triangulate_new_map_points.cpp runs it, built here at the same size with -O2: one
         jsorb_search_for_triangulation for all neighbours with its copy back, then the loop body on the host.  The example's clock does NOT include
         jsorb_map_points_scatter_async, the descriptor upload and the writes into point_pool / registered that follow on that path: it is a lower
         bound of today's cost.  Its map is the example's own (identity rotations), not the seeded world of the `new` side.
Before timing, the device must leave the map tests/new_points_cases.py's sequential loop leaves (checked with --check; the loop is Python and takes
minutes at this size).  Prints one JSON line per neighbour count."""
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--keypoints", type=int, default=2500)
    ap.add_argument("--neighbours", type=int, nargs="*", default=[10, 20])
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import new_points_cases as nc
    from jetson_slam_amd import build as jb, orb
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    q = lambda t: dict(median=round(float(np.median(t)), 1), p10=round(float(np.percentile(t, 10)), 1), p90=round(float(np.percentile(t, 90)), 1))
    for n_nb in args.neighbours:
        W = nc.scene(101 + n_nb, n1=args.keypoints, n_nb=n_nb, n_kp2=args.keypoints, n_nodes=250, name="bench%d" % n_nb)
        graph, table = orb.KeyframeGraph(W["S"], W["pool"], 1), orb.MapPointTable(W["n_rows"])
        kp, extra = orb.KeyframeKeypoints(graph), orb.NewPointKeypoints(graph)
        kp.load(**{k: W[k] for k in kp.ARRAYS})
        extra.load(**{k: W[k] for k in extra.ARRAYS})
        side = {k: dev(W[k]) for k in ("ref_slot", "replaced", "visible", "found", "first_kf_id")}
        state = orb.new_point_state(graph, table, **side)
        params = orb.make_triangulation_params(W["prm"]["scale_factor"], W["prm"]["level_sigma2"], check_orientation=False)
        poses = np.zeros(len(W["poses"]), orb.KEYFRAME_POSE_DTYPE)
        for i, p in enumerate(W["poses"]):
            for k in orb.KEYFRAME_POSE_DTYPE.names:
                poses[i][k] = p[k]
        new_row = dev(W["new_row"])
        a = (params, graph, table, kp, extra, state, W["current_slot"], W["n1"], W["run_capacity"], W["neighbours"], poses, W["F12"], W["epipole"],
             float(W["ratio_factor"]), W["current_kf_id"], new_row)

        def load():
            graph.load(**{k: W[k] for k in ("state", "order_key", "point_off", "point_len", "point_pool", "registered")})
            table.floats[:, :W["n_rows"]].copy_(dev(W["floats"]))
            table.bad[:W["n_rows"]].copy_(dev(W["bad"]))
            table.desc[:W["n_rows"]].copy_(dev(W["tdesc"]))
            torch.cuda.synchronize()

        m = orb.KeyframeMatcher()
        s = torch.cuda.Stream()
        m.set_stream(s.cuda_stream)
        load()
        out = m.create_new_map_points(*a, log_cap=len(W["new_row"]))
        torch.cuda.synchronize()
        counts = dict(zip(orb.NEW_POINTS_COUNTS, out["counts"].cpu().numpy().tolist()))
        if args.check:
            want = nc.restate(W)
            assert np.array_equal(want["verdict"], out["verdict"].cpu().numpy()) and np.array_equal(want["point_pool"], graph.point_pool[:W["pool"]].cpu().numpy())
            assert np.array_equal(want["floats"].view(np.uint32), table.floats[:, :W["n_rows"]].cpu().numpy().view(np.uint32))
        span, sync = [], []
        for rep in range(args.reps + 2):
            load()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                m.create_new_map_points(*a, log_cap=len(W["new_row"]), out=out, wait=False)
                e1.record(s)
            torch.cuda.synchronize()
            load()
            t0 = time.perf_counter()
            m.create_new_map_points(*a, log_cap=len(W["new_row"]), out=out, sync=True)
            dt = (time.perf_counter() - t0) * 1e6
            if rep >= 2:
                span.append(e0.elapsed_time(e1) * 1e3)
                sync.append(dt)
        with tempfile.TemporaryDirectory() as tmp:
            exe = jb.build_example("triangulate_new_map_points", os.path.join(tmp, "example"), ["-O2", "-DN_KP=%d" % args.keypoints, "-DN_NB=%d" % n_nb])
            today = []
            for rep in range(min(args.reps, 5) + 1):
                r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
                assert r.returncode == 0, r.stdout + r.stderr
                if rep:
                    today.append(float(re.search(r"host_path_us=(\d+)", r.stdout).group(1)))
            example = r.stdout.strip()
        print(json.dumps(dict(neighbours=n_nb, keypoints_per_keyframe=args.keypoints, pairs=n_nb * args.keypoints, new_span_us=q(span), new_sync_us=q(sync),
                              today_without_uploads_us=q(today), counts=counts, example=example)), flush=True)


if __name__ == "__main__":
    main()
