"""One Tracking::TrackLocalMap step on a C2 stereo frame (752x480, 8 levels, tile 30) both ways, in the same run, alternating:
  device  jsorb_local_map_points_async + jsorb_search_local_points_async on the handle's stream, one synchronisation at the end.  Counted in: the
          upload of this frame's kf_point_row (E int32) and frame_point_row (N int32) from pinned host memory - the only per-frame inputs.
  host    the path it replaces: the dedupe, the seen / bad filters and the gathers in numpy (array operations, not the reference's pointer walk
          under mutexes - this side is flattered), twelve uploads, jsorb_is_in_frustum (which synchronises), jsorb_search_local_points_async, one
          synchronisation.
For 20 and 80 local keyframes of about 1 000 map points each, covisible (a map point is seen by about five of them).  Per case: the median, p10 and
p90 over --reps of the host clock around each side (every timed region ends in a synchronisation), the hipEvent span of the device side's two
calls, and the sizes.  Both sides produce the same matches; the tool checks that before it times.  Prints one JSON line per case.
Run under `rocprofv3 --kernel-trace --stats -- python tools/local_map_bench.py --reps 20` for the per-kernel times (k_lm_marks, k_lm_list,
k_lm_scan, k_lm_write)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
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
    logsf = float(np.log(f32(1.2)))
    Rcw, tcw, Ow = np.eye(3, dtype=f32), np.zeros(3, f32), np.zeros(3, f32)
    frustum = orb.make_frustum_params(Rcw, tcw, Ow, cam, (0, w, 0, h), L, logsf, 0.5)
    sprm = orb.JsorbSearchParams(1.0, 0.8, 100, bf, 0.0, 0.0, f32(64) / f32(w), f32(48) / f32(h), 64, 48)
    print(json.dumps({"frame": "C2 752x480 L8 tile30", "keypoints": N, "reps": args.reps}), flush=True)
    for n_kf in (20, 80):
        rng = np.random.default_rng(n_kf)
        n_rows = 200 * n_kf + 800                # keyframe k sees ~1 000 of the rows 200 k .. 200 k + 1 000: a row is in about five keyframes
        ok = np.nonzero(depth > 0)[0]
        src = rng.choice(ok, n_rows)
        z = depth[src].astype(f32)
        vis = rng.random(n_rows) < 0.3           # three tenths of the map project next to a keypoint of this frame, the rest lies outside the image
        P = np.stack([(x[src] + rng.normal(0, 1, n_rows).astype(f32) - f32(cam[2])) * z / f32(fx), (y[src] - f32(cam[3])) * z / f32(fx), z]).astype(f32)
        P[0, ~vis] += f32(40.0) * z[~vis]
        dist = np.linalg.norm(P, axis=0).astype(f32)
        maxd = (dist * scale[octave[src]] * f32(0.999)).astype(f32)
        T = np.concatenate([P, (P / dist).astype(f32), np.stack([maxd, maxd * f32(1.2), maxd / scale[-1] * f32(0.8)])]).astype(f32)
        d = desc[src].copy()
        flip = rng.random(d.shape) < 0.04
        d[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
        bad = (rng.random(n_rows) < 0.03).astype(np.uint8)
        kfs = []
        for k in range(n_kf):
            r = (200 * k + rng.integers(0, 1000, 1000)).astype(np.int32)
            r[rng.random(1000) < 0.25] = -1      # keypoints without a map point
            kfs.append(r)
        entries = np.concatenate(kfs)
        kf_start = np.arange(0, 1000 * (n_kf + 1), 1000, dtype=np.int32)
        E = len(entries)
        frame_rows = np.full(N, -1, np.int32)
        tracked = rng.random(N) < 0.3            # TrackReferenceKeyFrame / the motion model matched these already
        frame_rows[tracked] = rng.choice(entries[entries >= 0], int(tracked.sum()))
        table = orb.MapPointTable(n_rows)
        table.floats.copy_(dev(T))
        table.desc.copy_(dev(d))
        table.bad.copy_(dev(bad))
        # ---- device side ----
        pin_e, pin_f = torch.from_numpy(entries).pin_memory(), torch.from_numpy(frame_rows).pin_memory()
        dev_e, dev_f = torch.empty(E, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
        capacity = 8192
        out = gl.local_map_points(table, frustum, kf_start, dev(entries), dev(frame_rows), capacity)      # buffers and scratch at their size
        mk, md = (torch.empty(capacity, dtype=torch.int32, device="cuda") for _ in range(2))
        km, cnt = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")

        def device_side():
            dev_e.copy_(pin_e, non_blocking=True)
            dev_f.copy_(pin_f, non_blocking=True)
            gl.local_map_points(table, frustum, kf_start, dev_e, dev_f, capacity, out=out, wait=False)
            assert lib.jsorb_search_local_points_async(gl.handle, 0, C.byref(sprm), capacity, *[out[k].data_ptr() for k in
                                                       ("u", "v", "invz", "predicted_level", "view_cos", "in_frustum", "mp_descriptors")], ur.data_ptr(),
                                                       out["blocked_in"].data_ptr(), mk.data_ptr(), md.data_ptr(), km.data_ptr(), cnt.data_ptr()) == 0
            stream.synchronize()

        # ---- host side ----
        hm = {}

        def host_side():
            fr = frame_rows
            okf = (fr >= 0) & (fr < n_rows)
            okf[okf] = bad[fr[okf]] == 0
            seen = np.zeros(n_rows, bool)
            seen[fr[okf]] = True
            e = entries
            cand = np.nonzero((e >= 0) & (e < n_rows))[0]
            cand = cand[bad[e[cand]] == 0]
            _, first = np.unique(e[cand], return_index=True)
            local = e[cand[np.sort(first)]]
            rows = local[~seen[local]]
            n = len(rows)
            G = [dev(T[i, rows]) for i in range(9)]                          # nine float arrays ...
            dd, blk = dev(d[rows]), dev(okf.astype(np.uint8))                # ... the descriptors, the frame's own points: eleven; the pose is the twelfth
            o = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(4)]
            lv, ins = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
            pose = dev(np.concatenate([Rcw.ravel(), tcw, Ow]))
            stream.synchronize()
            assert lib.jsorb_is_in_frustum(stream.cuda_stream, n, *[g.data_ptr() for g in G], pose.data_ptr(), pose.data_ptr() + 36, pose.data_ptr() + 48, *cam,
                                           0, w, 0, h, L, logsf, 0.5, o[2].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), lv.data_ptr(), o[3].data_ptr(),
                                           ins.data_ptr()) == 0
            hmk, hmd = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
            assert lib.jsorb_search_local_points_async(gl.handle, 0, C.byref(sprm), n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), lv.data_ptr(),
                                                       o[3].data_ptr(), ins.data_ptr(), dd.data_ptr(), ur.data_ptr(), blk.data_ptr(), hmk.data_ptr(),
                                                       hmd.data_ptr(), hm["km"].data_ptr(), hm["cnt"].data_ptr()) == 0
            stream.synchronize()
            hm["rows"], hm["n"] = rows, n

        hm["km"], hm["cnt"] = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
        for _ in range(5):
            device_side()
            host_side()
        # the same matches, keypoint by keypoint, as table rows
        a, b = km.cpu().numpy(), hm["km"].cpu().numpy()
        pr = out["point_row"].cpu().numpy()
        assert np.array_equal(np.where(a >= 0, pr[np.maximum(a, 0)], -1), np.where(b >= 0, hm["rows"][np.maximum(b, 0)], -1)) and int(cnt.item()) == int(hm["cnt"].item())
        counts = out["counts"].cpu().numpy().tolist()
        assert counts[4] == 0 and counts[1] == hm["n"]
        td_, th_, spans = [], [], []
        for _ in range(args.reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            ev0.record(stream)
            device_side()
            t1 = time.perf_counter()
            ev1.record(stream)
            ev1.synchronize()
            spans.append(ev0.elapsed_time(ev1) * 1e3)
            t2 = time.perf_counter()
            host_side()
            t3 = time.perf_counter()
            td_.append((t1 - t0) * 1e6)
            th_.append((t3 - t2) * 1e6)
        q = lambda v: {"median_us": round(float(np.median(v)), 1), "p10_us": round(float(np.percentile(v, 10)), 1), "p90_us": round(float(np.percentile(v, 90)), 1)}
        print(json.dumps({"keyframes": n_kf, "entries": E, "table_rows": n_rows, "local": counts[0], "map_points": counts[1], "in_frustum": counts[2],
                          "matches": int(cnt.item()), "device_path": q(td_), "device_gpu_span": q(spans), "host_path": q(th_)}), flush=True)


if __name__ == "__main__":
    main()
