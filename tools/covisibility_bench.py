"""KeyFrame::UpdateConnections for 1 and for 32 keyframes in a row over maps of 100 / 1 000 / 5 000 keyframes of 1 000 entries each, two ways in the
same run, alternating:
  device  jsorb_update_connections_async through the Python binding on the matcher's stream (the slots are on the device already, the
          neighbours table is the graph's), one synchronisation
  host    the loop it replaces over an observation index in numpy: per keyframe the rows of its run that are not bad, the observations of
          those rows counted with np.unique, the threshold or the first maximum, AddConnection on each target against a dict per keyframe
          with the early return, the re-sort by np.lexsort where a map changed - not the reference's std::map copies under a mutex per map
          point: this side is flattered.  It uploads nothing: a binding that keeps the graph on the host still owes the device the neighbour
          rows that changed.
The map: keyframe k sees ~750 of the rows 200 k .. 200 k + 1 000 (a row is in about five keyframes, a keyframe shares rows with about eight
others), order keys are a random permutation.  Every keyframe has been updated once before the clock starts (on the device; the host loop starts
from a copy of that state), so the timed calls find every weight unchanged, as a LocalMapping that revisits a neighbourhood mostly does.
The device pass reads the whole pool - every slot's run - whatever n_update is, while the host loop grows with the neighbourhood only: expect the
host loop to win at n_update = 1 on the larger maps.  Both sides are checked against each other before they are timed.  Prints one JSON line per
case: the median, p10 and p90 over --reps of the host clock around each side.
Run under `rocprofv3 --kernel-trace --stats -- python tools/covisibility_bench.py --reps 20` for the per-kernel times (k_cv_marks, k_cv_counts,
k_cv_select, k_cv_apply, k_cv_reset)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TH = 15


def host_update(A, pool, bad, obs_start, obs_kf, key, conn, ordered):
    """UpdateConnections (KeyFrame.cpp:293-383) of keyframe A from array operations; conn[k]: dict slot -> weight, ordered[k]: (slots, weights)"""
    rows = pool[A]
    rows = rows[rows >= 0]
    rows = rows[bad[rows] == 0]
    lens = obs_start[rows + 1] - obs_start[rows]
    idx = np.repeat(obs_start[rows], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    others, cnt = np.unique(obs_kf[idx], return_counts=True)
    keep = others != A
    others, cnt = others[keep], cnt[keep]
    if len(others) == 0:
        return
    order = np.argsort(key[others], kind="stable")
    others, cnt = others[order], cnt[order]
    sel = cnt >= TH
    if not sel.any():
        sel = np.zeros(len(cnt), bool)
        sel[np.argmax(cnt)] = True
    for B, w in zip(others[sel].tolist(), cnt[sel].tolist()):
        m = conn[B]
        if m.get(A) == w:
            continue
        m[A] = w
        s, ws = np.fromiter(m.keys(), np.int64, len(m)), np.fromiter(m.values(), np.int64, len(m))
        o = np.lexsort((key[s], ws))[::-1]
        ordered[B] = (s[o], ws[o])
    conn[A] = dict(zip(others.tolist(), cnt.tolist()))
    o = np.lexsort((key[others[sel]], cnt[sel]))[::-1]
    ordered[A] = (others[sel][o], cnt[sel][o])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--maps", type=int, nargs="*", default=[100, 1000, 5000])
    ap.add_argument("--capacity", type=int, default=64)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    m = orb.KeyframeMatcher()
    C = args.capacity
    print(json.dumps({"entries_per_keyframe": 1000, "conn_capacity": C, "reps": args.reps}), flush=True)
    for S in args.maps:
        rng = np.random.default_rng(S)
        n_rows = 200 * S + 800
        bad = (rng.random(n_rows) < 0.03).astype(np.uint8)
        table = orb.MapPointTable(n_rows)
        table.bad.copy_(dev(bad))
        pool = (200 * np.arange(S)[:, None] + np.argsort(rng.random((S, 1000)), axis=1)).astype(np.int32)
        pool[rng.random((S, 1000)) < 0.25] = -1
        key = (0x7F0000000000 + 4096 * rng.permutation(S)).astype(np.int64)
        ks = np.arange(S)
        graph = orb.KeyframeGraph(S, pool.size, 1)
        graph.load(state=np.ones(S, np.uint8), order_key=key, point_off=(1000 * ks).astype(np.int32), point_len=np.full(S, 1000, np.int32), point_pool=pool.ravel())
        flat = pool.ravel()
        e_ok = np.nonzero(flat >= 0)[0]
        by_row = np.argsort(flat[e_ok], kind="stable")
        obs_kf = (e_ok[by_row] // 1000).astype(np.int64)
        obs_start = np.concatenate([[0], np.cumsum(np.bincount(flat[e_ok], minlength=n_rows))]).astype(np.int64)
        cov = orb.Covisibility(S, C)
        cov.first_connection[1:] = 1
        for a in range(0, S, 32):                # every keyframe updated once, in slot order
            m.update_connections(graph, table, cov, list(range(a, min(a + 32, S))), neighbours=graph.neighbours)
        st = cov.arrays()
        assert st["conn_len"].max() < C, "raise --capacity"
        conn = [dict(zip(st["conn_slot"][k, :st["conn_len"][k]].tolist(), st["conn_weight"][k, :st["conn_len"][k]].tolist())) for k in range(S)]
        ordered = [(st["ord_slot"][k, :st["ord_len"][k]].astype(np.int64), st["ord_weight"][k, :st["ord_len"][k]].astype(np.int64)) for k in range(S)]
        for n_update in (1, 32):
            if n_update + 8 > S:
                continue
            a = int(rng.integers(4, S - n_update - 3))
            slots = list(range(a, a + n_update))
            slots_dev = dev(np.array(slots, np.int32))
            out = m.update_connections(graph, table, cov, slots_dev, neighbours=graph.neighbours)
            counts = out["counts"].cpu().numpy().tolist()

            def device_side():
                m.update_connections(graph, table, cov, slots_dev, neighbours=graph.neighbours, out=out, wait=False)
                m.sync()

            def host_side():
                for A in slots:
                    host_update(A, pool, bad, obs_start, obs_kf, key, conn, ordered)

            for _ in range(3):
                device_side()
                host_side()
            st = cov.arrays()
            for k in range(max(a - 8, 0), min(a + n_update + 8, S)):      # the neighbourhood: maps, lists and weights agree
                assert dict(zip(st["conn_slot"][k, :st["conn_len"][k]].tolist(), st["conn_weight"][k, :st["conn_len"][k]].tolist())) == conn[k], k
                assert st["ord_slot"][k, :st["ord_len"][k]].tolist() == ordered[k][0].tolist() and st["ord_weight"][k, :st["ord_len"][k]].tolist() == ordered[k][1].tolist(), k
            td_, th_ = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                device_side()
                t1 = time.perf_counter()
                host_side()
                t2 = time.perf_counter()
                td_.append((t1 - t0) * 1e6)
                th_.append((t2 - t1) * 1e6)
            q = lambda v: {"median_us": round(float(np.median(v)), 1), "p10_us": round(float(np.percentile(v, 10)), 1), "p90_us": round(float(np.percentile(v, 90)), 1)}
            print(json.dumps({"map_keyframes": S, "pool_entries": int(pool.size), "table_rows": n_rows, "n_update": n_update, "n_processed": counts[0],
                              "n_add_connection": counts[3], "largest_map": int(st["conn_len"].max()), "device_call": q(td_), "host_loop": q(th_)}), flush=True)


if __name__ == "__main__":
    main()
