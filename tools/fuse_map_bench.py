"""Direction A of LocalMapping::SearchInNeighbors - the current keyframe's map points into 20 target keyframes of a C2-sized frame's keypoint count,
about 1 000 list points - two ways over the same map, alternating in one run, each side ending in a synchronisation, the host clock around each:
  new    KeyframeMatcher.fuse_map: the search, the head test, the tail, Replace and the descriptors in one call on the device state
  today  the caller's loop of include/jsorb.h (jsorb_fuse_async): one batched jsorb_fuse over all targets, tests/fuse_replay.py's host replay of the
         head test and the tail (mode "research": after every replayed keyframe the points whose descriptor changed are searched again by one more
         jsorb_fuse call), then the upload of the slots, registered bytes, bad bytes and descriptors to the device map.  The replay here is the
         Python one, with MapPoint::ComputeDistinctiveDescriptors on the host: `today_calls_us` is the part of it spent inside the jsorb_fuse calls
         and the uploads, which a C++ binding pays as well; the rest is the interpreter's.
Before timing, both sides must leave the same map (slots, bad flags, the descriptors of the living rows, the events).  The map is a random block of
the generator behind tests/golden/ref_matcher_fuse.npz (tests/ref_matcher_cases.py).  Prints one JSON line: medians with p10 and p90 over --reps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--keypoints", type=int, default=2000)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import fuse_apply_cases as fa
    import fuse_replay
    import ref_matcher_cases as cases
    from jetson_slam_amd import orb
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(29)
    c = cases.named(cases.with_grids(cases.Fuse.random_block(rng, n_targets=args.targets, n=args.points, N=args.keypoints, n_world=3 * args.keypoints)), "fuse", "bench")
    W = fa.to_world(c)
    prm = cases.fuse_prm(c)
    params = orb.make_fuse_params((prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]), (prm["inv_w"], prm["inv_h"]),
                                  float(prm["log_sf"]), prm["scale"], prm["inv_sigma2"], th=float(prm["th"]), th_low=prm["th_low"], check_reprojection=prm["check"],
                                  bf=float(prm["bf"]), cols=prm["cols"], rows=prm["rows"])
    m = orb.KeyframeMatcher()
    graph, table = orb.KeyframeGraph(W["S"], W["pool"], 1), orb.MapPointTable(W["n_rows"])
    kp = orb.KeyframeKeypoints(graph)
    kp.load(**{k: W[k] for k in kp.ARRAYS})
    table.floats[:, :W["n_rows"]].copy_(dev(W["floats"]))
    replaced = torch.empty(W["n_rows"], dtype=torch.int32, device="cuda")
    state = orb.fuse_state(graph, table, replaced)

    def load():
        graph.load(**{k: W[k] for k in ("state", "order_key", "point_off", "point_len", "point_pool", "registered")})
        table.bad[:W["n_rows"]].copy_(dev(W["bad"]))
        table.desc[:W["n_rows"]].copy_(dev(W["tdesc"]))
        replaced.fill_(-1)
        torch.cuda.synchronize()
    lst = dev(W["list"])

    def new():
        out = m.fuse_map(params, graph, table, kp, state, lst, W["targets"], W["Rcw"], W["tcw"], W["Ow"], log_cap=W["log_cap"], wait=True)
        return out

    # today's path: the targets' keypoints as jsorb_fuse takes them (uploaded once, outside the clock: they do not change)
    targets = [int(k) for k in c["targets"]]
    kf_start = np.concatenate([[0], np.cumsum([len(c["KF"][k]["x"]) for k in targets])]).astype(np.int32)
    cat = lambda key, dt: dev(np.concatenate([np.asarray(c["KF"][k][key], dt).reshape(len(c["KF"][k]["x"]), -1) for k in targets]).squeeze())
    kfs = dict(x=cat("x", np.float32), y=cat("y", np.float32), octave=cat("octave", np.int32), uright=cat("uright", np.float32), desc=cat("desc", np.uint8))
    pmap = dict(Px="Px", Py="Py", Pz="Pz", Nx="Nx", Ny="Ny", Nz="Nz", max_distance="maxd", min_dist_inv="mindi", max_dist_inv="maxdi")
    in_calls = [0.0]

    def search(ts, idxs, desc, skip):
        t0 = time.perf_counter()
        P = cases.list_points(c, idxs, desc)
        pts = {k: dev(np.asarray(P[v], np.float32)) for k, v in pmap.items()}
        pts["desc"] = dev(P["desc"])
        rows = np.full((len(targets), len(idxs)), 1, np.uint8)           # the call's keyframes are all targets; only `ts` are searched
        rows[ts] = skip
        bi, bd, _ = m.fuse_host(pts, kf_start, kfs, W["Rcw"], W["tcw"], W["Ow"], params, skip=dev(rows))
        in_calls[0] += time.perf_counter() - t0
        return bi[ts].astype(np.int64), bd[ts].astype(np.int64)

    def today():
        in_calls[0] = 0.0
        out = fuse_replay.replay(c, search, "research")[0]
        t0 = time.perf_counter()
        held = out["kf_mps"]
        graph.load(point_pool=held, registered=((held >= 0) & (out["pt_bad"][np.maximum(held, 0)] == 0)).astype(np.uint8))
        table.bad[:W["n_rows"]].copy_(dev(out["pt_bad"]))
        table.desc[:W["n_rows"]].copy_(dev(out["pt_desc"]))
        torch.cuda.synchronize()
        in_calls[0] += time.perf_counter() - t0
        return out

    # both sides leave the same map
    load()
    got = new()
    torch.cuda.synchronize()
    pool, bad, desc = graph.point_pool[:W["pool"]].cpu().numpy(), table.bad[:W["n_rows"]].cpu().numpy(), table.desc[:W["n_rows"]].cpu().numpy()
    counts = dict(zip(orb.FUSE_MAP_COUNTS, got["counts"].cpu().numpy().tolist()))
    log = got["log"].cpu().numpy()
    load()
    ref = today()
    ev = ref["events"][np.isin(ref["events"][:, 0], (2, 3))]
    live = bad == 0
    assert np.array_equal(pool, ref["kf_mps"]) and np.array_equal(bad, ref["pt_bad"]) and np.array_equal(desc[live], ref["pt_desc"][live])
    assert np.array_equal(fa.events_as_reference(W, log[:counts["n_log"]]), ev) and counts["n_replace"] > 0 and counts["n_add"] > 0
    t_new, t_today, t_calls = [], [], []
    for rep in range(args.reps + 2):
        for side in (("new", "today") if rep % 2 == 0 else ("today", "new")):
            load()
            t0 = time.perf_counter()
            (new if side == "new" else today)()
            dt = (time.perf_counter() - t0) * 1e6
            if rep >= 2:
                (t_new if side == "new" else t_today).append(dt)
                if side == "today":
                    t_calls.append(in_calls[0] * 1e6)
    q = lambda t: dict(median=round(float(np.median(t)), 1), p10=round(float(np.percentile(t, 10)), 1), p90=round(float(np.percentile(t, 90)), 1))
    print(json.dumps(dict(targets=len(targets), list_points=int(len(W["list"])), keypoints_per_keyframe=args.keypoints, pool_entries=W["pool"], rows=W["n_rows"],
                          new_us=q(t_new), today_us=q(t_today), today_calls_us=q(t_calls), counts=counts)), flush=True)


if __name__ == "__main__":
    main()
