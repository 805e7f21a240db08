"""One Tracking::TrackLocalMap step on a C2 frame (752x480, 8 levels, tile 30) over maps of 100 / 1 000 / 5 000 keyframes of 1 000 entries each,
with 20 and 80 local keyframes, three ways in the same run, alternating:
  keyframes  jsorb_local_keyframes_async alone, one synchronisation
  device     jsorb_local_keyframes_async + jsorb_local_map_points_async (one keyframe over local_point_row) + jsorb_search_local_points_async on the
             handle's stream, one synchronisation at the end.  Counted in: the upload of frame_point_row (N int32) from pinned host memory, the
             only per-frame input.
  host       the path it replaces: UpdateLocalKeyFrames in numpy over an observation index (the votes by np.unique over the tracked points'
             observation lists, the walk of at most 80 elements in Python - not the reference's std::map copies under mutexes: this side is
             flattered), the keyframes' rows concatenated on the host, the upload of that list, then the same two device calls with a host
             kf_start.
The map: keyframe k sees ~750 of the rows 200 k .. 200 k + 1 000 (a row is in about five keyframes), its neighbours are k -+ 1 .. 5, its parent
k - 1, its child k + 1; order keys are a random permutation.  About 400 keypoints of the frame are tracked, in a window of the map sized for the
wanted number of local keyframes.  Per case: the median, p10 and p90 over --reps of the host clock around each side, and the sizes.  All sides
produce the same list and the same matches; the tool checks that before it times.  Prints one JSON line per case.
Run under `rocprofv3 --kernel-trace --stats -- python tools/local_kf_bench.py --reps 20` for the per-kernel times (k_lk_marks, k_lk_votes,
k_lk_rank, k_lk_expand, k_lk_gather)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_walk(frame_rows, bad, obs_start, obs_kf, key, state, neighbours, child, parent):
    """UpdateLocalKeyFrames (Tracking.cpp:1844-1952) from array operations; child[k]: the one child of k or -1.  Returns (slots, ref_slot)."""
    fr = frame_rows[frame_rows >= 0]
    fr = fr[bad[fr] == 0]
    lens = obs_start[fr + 1] - obs_start[fr]
    idx = np.repeat(obs_start[fr], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    voters, votes = np.unique(obs_kf[idx], return_counts=True)
    if len(voters) == 0:
        return None, None
    good = state[voters] == 1
    voters, votes = voters[good], votes[good]
    order = np.argsort(key[voters], kind="stable")
    voters, votes = voters[order], votes[order]
    slots = voters.tolist()
    ref = int(voters[np.argmax(votes)]) if len(voters) else None
    member = np.zeros(len(state), bool)
    member[voters] = True
    for s in list(slots):
        if len(slots) > 80:
            break
        for cand in (neighbours[s], child[s:s + 1]):
            for c in cand:
                if c >= 0 and state[c] == 1 and not member[c]:
                    slots.append(int(c))
                    member[c] = True
                    break
        p = parent[s]
        if p >= 0 and state[p] != 0 and not member[p]:
            slots.append(int(p))
            break
    return slots, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--maps", type=int, nargs="*", default=[100, 1000, 5000])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    from jetson_slam_amd.synth import synth_stereo_pair
    h, w, L, tile, bf, fx = 480, 752, 8, 30, 47.906, 435.2
    f32 = np.float32
    left, right = synth_stereo_pair(31, h, w)
    gl = orb.ORBExtractor(h, w, 1.2, L, 9, 14, 7, 20, None, tile, tile)
    gr = orb.ORBExtractor(h, w, 1.2, L, 9, 14, 7, 20, None, tile, tile)
    kp, desc = gl.extract(left)
    gr.extract(right)
    u_right, depth, _ = orb.compute_stereo_matches(gl, gr, bf / fx, bf)
    N = len(kp) // 6
    lib = orb.load_library()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    gl.set_stream(stream.cuda_stream)
    x, y, octave = kp[:N].astype(f32), kp[N:2 * N].astype(f32), kp[4 * N:5 * N]
    scale = gl.get_scale_factors()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ur = dev(u_right)
    cam = (fx, fx, w / 2, h / 2)
    frustum = orb.make_frustum_params(np.eye(3, dtype=f32), np.zeros(3, f32), np.zeros(3, f32), cam, (0, w, 0, h), L, float(np.log(f32(1.2))), 0.5)
    sprm = orb.JsorbSearchParams(1.0, 0.8, 100, bf, 0.0, 0.0, f32(64) / f32(w), f32(48) / f32(h), 64, 48)
    print(json.dumps({"frame": "C2 752x480 L8 tile30", "keypoints": N, "reps": args.reps}), flush=True)
    for n_map in args.maps:
        rng = np.random.default_rng(n_map)
        n_rows = 200 * n_map + 800
        ok = np.nonzero(depth > 0)[0]
        src = rng.choice(ok, n_rows)
        z = depth[src].astype(f32)
        P = np.stack([(x[src] + rng.normal(0, 1, n_rows).astype(f32) - f32(cam[2])) * z / f32(fx), (y[src] - f32(cam[3])) * z / f32(fx), z]).astype(f32)
        vis = rng.random(n_rows) < 0.3
        P[0, ~vis] += f32(40.0) * z[~vis]
        dist = np.linalg.norm(P, axis=0).astype(f32)
        maxd = (dist * scale[octave[src]] * f32(0.999)).astype(f32)
        T = np.concatenate([P, (P / dist).astype(f32), np.stack([maxd, maxd * f32(1.2), maxd / scale[-1] * f32(0.8)])]).astype(f32)
        d = desc[src].copy()
        bad = (rng.random(n_rows) < 0.03).astype(np.uint8)
        table = orb.MapPointTable(n_rows)
        table.floats.copy_(dev(T))
        table.desc.copy_(dev(d))
        table.bad.copy_(dev(bad))
        # the keyframes: unique rows per keyframe, so the observation index is the transpose of the runs
        pool = (200 * np.arange(n_map)[:, None] + np.argsort(rng.random((n_map, 1000)), axis=1)).astype(np.int32)
        pool[rng.random((n_map, 1000)) < 0.25] = -1
        pool = pool.ravel()
        S = n_map
        ks = np.arange(S)
        nb = np.stack([ks + o for o in (-1, 1, -2, 2, -3, 3, -4, 4, -5, 5)], axis=1).astype(np.int32)
        nb[(nb < 0) | (nb >= S)] = -1
        child = np.where(ks + 1 < S, ks + 1, -1).astype(np.int32)
        parent = (ks - 1).astype(np.int32)
        key = (0x7F0000000000 + 4096 * rng.permutation(S)).astype(np.int64)
        state = np.ones(S, np.uint8)
        state[rng.random(S) < 0.02] = 2
        graph = orb.KeyframeGraph(S, len(pool), S)
        graph.load(state=state, order_key=key, point_off=(1000 * ks).astype(np.int32), point_len=np.full(S, 1000, np.int32), point_pool=pool, neighbours=nb,
                   child_off=ks.astype(np.int32), child_len=(child >= 0).astype(np.int32), child_pool=child, parent=parent)
        e_ok = np.nonzero(pool >= 0)[0]
        by_row = np.argsort(pool[e_ok], kind="stable")
        obs_kf = (e_ok[by_row] // 1000).astype(np.int32)
        obs_start = np.concatenate([[0], np.cumsum(np.bincount(pool[e_ok], minlength=n_rows))]).astype(np.int64)
        for n_local in (20, 80):
            if n_local + 10 > S:
                continue
            a = int(rng.integers(5, S - n_local - 4))
            span = n_local - 7                       # rows of 200 a .. 200 (a + span): span + 4 voters, and up to three more from the walk
            frame_rows = np.full(N, -1, np.int32)
            tracked = rng.choice(N, min(400, N), replace=False)
            frame_rows[tracked] = rng.integers(200 * a, 200 * (a + span), len(tracked))
            pin_f, dev_f = torch.from_numpy(frame_rows).pin_memory(), torch.empty(N, dtype=torch.int32, device="cuda")
            kf_capacity, entry_capacity, capacity = 84, 84 * 1000, 8192
            lk = gl.local_keyframes(graph, table, dev(frame_rows), kf_capacity, entry_capacity)
            lm = gl.local_map_points(table, frustum, [0, entry_capacity], lk["local_point_row"], dev(frame_rows), capacity)
            mk, md = (torch.empty(capacity, dtype=torch.int32, device="cuda") for _ in range(2))
            km, cnt = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")

            def search(o, km, cnt):
                assert lib.jsorb_search_local_points_async(gl.handle, 0, C.byref(sprm), capacity, *[o[k].data_ptr() for k in
                                                           ("u", "v", "invz", "predicted_level", "view_cos", "in_frustum", "mp_descriptors")], ur.data_ptr(),
                                                           o["blocked_in"].data_ptr(), mk.data_ptr(), md.data_ptr(), km.data_ptr(), cnt.data_ptr()) == 0

            def keyframes_only():
                dev_f.copy_(pin_f, non_blocking=True)
                gl.local_keyframes(graph, table, dev_f, kf_capacity, entry_capacity, out=lk, wait=False)
                stream.synchronize()

            def device_side():
                dev_f.copy_(pin_f, non_blocking=True)
                gl.local_keyframes(graph, table, dev_f, kf_capacity, entry_capacity, out=lk, wait=False)
                gl.local_map_points(table, frustum, [0, entry_capacity], lk["local_point_row"], dev_f, capacity, out=lm, wait=False)
                search(lm, km, cnt)
                stream.synchronize()

            hm = dict(km=torch.empty(N, dtype=torch.int32, device="cuda"), cnt=torch.empty(1, dtype=torch.int32, device="cuda"),
                      entries=torch.empty(entry_capacity, dtype=torch.int32, device="cuda"), out=None)

            def host_side():
                slots, ref = host_walk(frame_rows, bad, obs_start, obs_kf, key, state, nb, child, parent)
                runs = pool.reshape(S, 1000)[slots]
                kf_start = np.arange(0, 1000 * (len(slots) + 1), 1000, dtype=np.int32)
                hm["entries"][:runs.size].copy_(torch.from_numpy(runs.ravel()), non_blocking=True)
                dev_f.copy_(pin_f, non_blocking=True)
                hm["out"] = gl.local_map_points(table, frustum, kf_start, hm["entries"], dev_f, capacity, out=hm["out"], wait=False)
                search(hm["out"], hm["km"], hm["cnt"])
                stream.synchronize()
                hm["slots"], hm["ref"] = slots, ref

            for _ in range(5):
                keyframes_only()
                device_side()
                host_side()
            counts = lk["counts"].cpu().numpy().tolist()
            assert lk["local_kf_slot"].cpu().numpy()[:counts[2]].tolist() == hm["slots"] and counts[3] == hm["ref"] and counts[5:] == [0, 0, 0], (counts, hm["slots"])
            assert np.array_equal(km.cpu().numpy(), hm["km"].cpu().numpy()) and int(cnt.item()) == int(hm["cnt"].item()) > 0
            tk, td_, th_ = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                keyframes_only()
                t1 = time.perf_counter()
                device_side()
                t2 = time.perf_counter()
                host_side()
                t3 = time.perf_counter()
                tk.append((t1 - t0) * 1e6)
                td_.append((t2 - t1) * 1e6)
                th_.append((t3 - t2) * 1e6)
            q = lambda v: {"median_us": round(float(np.median(v)), 1), "p10_us": round(float(np.percentile(v, 10)), 1), "p90_us": round(float(np.percentile(v, 90)), 1)}
            print(json.dumps({"map_keyframes": S, "pool_entries": len(pool), "table_rows": n_rows, "tracked": int((frame_rows >= 0).sum()), "n_counter": counts[0],
                              "n_first": counts[1], "local_keyframes": counts[2], "entries": counts[4], "matches": int(cnt.item()),
                              "local_keyframes_call": q(tk), "device_step": q(td_), "host_step": q(th_)}), flush=True)


if __name__ == "__main__":
    main()
