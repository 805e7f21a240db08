"""LocalMapping::KeyFrameCulling on the device (jsorb_cull_keyframes_async through the Python binding, one synchronisation) over maps of 100 /
1 000 / 5 000 keyframes of 1 000 entries each, with max_cull 4 and 16.  The map: keyframe k sees ~750 of the rows 150 k .. 150 k + 1 000, a
fifth of the entries stereo, octaves 0 - 3 (nothing is redundant: the call only judges) or 0 - 1 (the first candidates are culled), so a row is
in about five keyframes and a keyframe shares rows with about twelve others; the covisibility state is what update_connections leaves.  The candidates are the ordered list of a keyframe in the middle of the map.  The call changes the map, so the arrays
it writes are restored from device copies before every repetition, outside the clock.  Only the device side is timed: no host loop stands next to
it.  Prints one JSON line per map: the median, p10 and p90 over --reps of the host clock around the call, and what the call decided.
Run under `rocprofv3 --kernel-trace --stats -- python tools/culling_bench.py --reps 20` for the per-kernel times (k_kc_count, k_kc_scan_blocks,
k_kc_scan_top, k_kc_scatter, k_kc_eval, k_kc_pick, k_cv_erase_dev, k_kc_apply)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--maps", type=int, nargs="*", default=[100, 1000, 5000])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    m = orb.KeyframeMatcher()
    for S, octaves, max_cull in [(S, o, c) for S in args.maps for o in (4, 2) for c in (4, 16)]:
        rng = np.random.default_rng(S)
        run, step = 1000, 150
        n_rows = step * S + run
        rows = (np.arange(S)[:, None] * step + np.arange(run)[None, :]).astype(np.int32)
        rows[rng.random(rows.shape) < 0.25] = -1
        graph, table, cov = orb.KeyframeGraph(S, S * run, 1), orb.MapPointTable(n_rows), orb.Covisibility(S, 64)
        graph.load(state=np.ones(S, np.uint8), order_key=(rng.permutation(S).astype(np.int64) * 64 + 4096), point_off=(np.arange(S) * run).astype(np.int32),
                   point_len=np.full(S, run, np.int32), point_pool=rows.ravel(), parent=np.maximum(np.arange(S) - 1, -1).astype(np.int32))
        views = orb.KeyframeViews(graph, depth=False)
        views.load(octave=rng.integers(0, octaves, S * run).astype(np.uint8), stereo=(rng.random(S * run) < 0.2).astype(np.uint8))
        cov.first_connection.fill_(0)
        for at in range(0, S, orb.UPDATE_CONNECTIONS_MAX):
            m.update_connections(graph, table, cov, list(range(at, min(at + orb.UPDATE_CONNECTIONS_MAX, S))), neighbours=graph.neighbours)
        state = orb.culling_state(graph, table)
        cand = m.best_covisibles(cov, [S // 2], cov.conn_capacity)[0].reshape(-1).contiguous()
        written = [graph.state, graph.registered, graph.point_pool, graph.parent, graph.neighbours, table.bad] + [getattr(cov, k) for k in cov.ARRAYS]
        saved = [t.clone() for t in written]
        times, out = [], None
        for rep in range(args.reps + 3):
            for t, s in zip(written, saved):
                t.copy_(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.cull_keyframes(graph, table, cov, views, state, cand, first_slot=0, monocular=True, max_cull=max_cull, neighbours=graph.neighbours, wait=True)
            times.append((time.perf_counter() - t0) * 1e6)
        t = np.array(times[3:])
        counts = dict(zip(orb.CULL_COUNTS, out["counts"].cpu().numpy().tolist()))
        print(json.dumps(dict(keyframes=S, octaves=octaves, max_cull=max_cull, pool_entries=S * run, rows=n_rows, candidates=int((cand >= 0).sum().item()), us_median=round(float(np.median(t)), 1),
                              us_p10=round(float(np.percentile(t, 10)), 1), us_p90=round(float(np.percentile(t, 90)), 1), counts=counts)), flush=True)


if __name__ == "__main__":
    main()
