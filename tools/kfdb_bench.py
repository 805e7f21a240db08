"""GPU time of the keyframe database's calls (k_kfdb.hip) on synthetic databases of 100, 1 000 and 5 000 keyframes over a vocabulary of 10^6 words:
jsorb_bow_vector_async of a frame's word ids, jsorb_detect_relocalization_candidates_async, jsorb_detect_loop_candidates_async and
jsorb_keyframe_database_score_async over 20 covisible keyframes.
The data, written down here: the map is a walk through "places" of 3 000 words each (drawn from the 10^6); a keyframe draws 1 200 features from its
place's words with a Zipf-like preference (so about 1 000 distinct words, some repeated), consecutive keyframes share a place for 10 keyframes;
the query is a new frame of the place visited at 40 % of the walk.  Leaf weights uniform in [0.5, 9), 1 % of the words stopped.  No covisibility
neighbours in the timed queries' tables beyond the ten following slots of each keyframe; the loop query's connected set is the last 20 keyframes.
Per call: median, p10 and p90 over --reps of the hipEvent span on the database's stream.  Beside them the host loop's time on the same data and
the same box (tools/micro/kfdb_host_loop.cpp, -O2, median of 20 passes; a relocalisation query without neighbours, whose candidates must be the
device's for the same table).  Prints one JSON line."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_WORDS, PLACE_WORDS, FEATURES, PER_PLACE = 1000000, 3000, 1200, 10


def frame_of(rng, place):
    return place[np.minimum((rng.pareto(1.2, FEATURES) * 300).astype(np.int64), PLACE_WORDS - 1)].astype(np.int32)


def host_loop(tmp, n_kf, start, word, value, q_ids, q_weight):
    exe, src = os.path.join(tmp, "kfdb_host_loop"), os.path.join(tmp, "in.bin")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "micro", "kfdb_host_loop.cpp"), "-o", exe])
    with open(src, "wb") as f:
        f.write(np.array([n_kf, N_WORDS, len(word), len(q_ids)], np.int32).tobytes() + start.tobytes() + word.tobytes() + value.tobytes() +
                q_ids.tobytes() + q_weight.tobytes())
    out = subprocess.run([exe, src, "20"], capture_output=True, text=True, timeout=600)
    m = re.search(r"host_fold_us=([\d.]+) host_query_us=([\d.]+) checksum=(\d+)", out.stdout)
    assert out.returncode == 0 and m, out.stderr + out.stdout
    return float(m.group(1)), float(m.group(2)), int(m.group(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=[100, 1000, 5000])
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from jetson_slam_amd import orb
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    rng = np.random.default_rng(11)
    weight = rng.uniform(0.5, 9.0, N_WORDS) * (rng.random(N_WORDS) > 0.01)
    result = {"tool": "kfdb_bench", "reps": args.reps, "caps": orb.kfdb_build_caps(), "n_words": N_WORDS, "cases": []}

    def timed(call):
        torch.cuda.synchronize()
        for _ in range(10):
            call()
        spans = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            spans.append(a.elapsed_time(b) * 1e3)
        return {"median_us": round(float(np.median(spans)), 2), "p10_us": round(float(np.percentile(spans, 10)), 2),
                "p90_us": round(float(np.percentile(spans, 90)), 2)}

    with tempfile.TemporaryDirectory() as tmp:
        for n_kf in args.sizes:
            db = orb.KeyframeDatabase(weight, n_kf)
            db.set_stream(stream.cuda_stream)
            places = [rng.choice(N_WORDS, PLACE_WORDS, replace=False) for _ in range((n_kf + PER_PLACE - 1) // PER_PLACE)]
            vecs = []
            for k in range(n_kf):
                vecs.append(db.bow_vector(dev(frame_of(rng, places[k // PER_PLACE])), wait=False))
                db.add(k, vecs[-1], wait=False)
            db.sync()
            q_ids = frame_of(rng, places[int(0.4 * n_kf) // PER_PLACE])
            q_dev = dev(q_ids)
            q = db.bow_vector(q_dev)
            nb = np.full((n_kf, 10), -1, np.int32)
            none = dev(nb)
            for k in range(n_kf):
                nb[k] = [j if j < n_kf else -1 for j in range(k + 1, k + 11)]
            nb = dev(nb)
            connected = torch.zeros(n_kf, dtype=torch.uint8, device="cuda")
            connected[-20:] = 1
            cov = dev(np.arange(n_kf - 20, n_kf, dtype=np.int32))
            case = {"keyframes": n_kf, "query_words": int(q[2].cpu()[0]), "mean_keyframe_words": round(float(np.mean([int(v[2].cpu()[0]) for v in vecs[:50]])), 1)}
            ids = iter(range(1, 1 << 30))
            # the C calls themselves, outputs allocated once: nothing but the library's work lies between the two events
            lib, h, n = orb.load_library(), db.handle, len(q_ids)
            vec = [q[0].data_ptr(), q[1].data_ptr(), n, q[2].data_ptr()]
            ow, ov, on = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            cand, nc = torch.empty(n_kf, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            sc, ms = torch.empty(20, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.float32, device="cuda")
            ok = lambda rc: None if rc == 0 else sys.exit("libjsorb rc=%d" % rc)
            case["bow_vector"] = timed(lambda: ok(lib.jsorb_bow_vector_async(h, q_dev.data_ptr(), n, ow.data_ptr(), ov.data_ptr(), on.data_ptr())))
            case["relocalization"] = timed(lambda: ok(lib.jsorb_detect_relocalization_candidates_async(h, *vec, next(ids), nb.data_ptr(), cand.data_ptr(), nc.data_ptr())))
            case["relocalization_stats"] = {k: (float(v) if k == "best_acc" else v) for k, v in db.stats().items()}
            case["score_20"] = timed(lambda: ok(lib.jsorb_keyframe_database_score_async(h, *vec, cov.data_ptr(), 20, sc.data_ptr(), None, ms.data_ptr())))
            case["loop"] = timed(lambda: ok(lib.jsorb_detect_loop_candidates_async(h, *vec, next(ids), connected.data_ptr(), nb.data_ptr(), 0.0, ms.data_ptr(),
                                                                                   cand.data_ptr(), nc.data_ptr())))
            case["loop_stats"] = {k: (float(v) if k == "best_acc" else v) for k, v in db.stats().items()}
            if not args.no_host:
                cand = db.detect_relocalization_candidates(q, next(ids), none, sync=True)
                checksum = 0
                for s in cand:
                    checksum = (checksum * 31 + int(s) + 1) % 1000000007
                counts = np.array([int(v[2].cpu()[0]) for v in vecs])
                start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
                word = np.concatenate([v[0].cpu().numpy()[:c] for v, c in zip(vecs, counts)]).astype(np.int32)
                value = np.concatenate([v[1].cpu().numpy()[:c] for v, c in zip(vecs, counts)]).astype(np.float64)
                fold_us, query_us, host_sum = host_loop(tmp, n_kf, start, word, value, q_ids, weight[q_ids])
                assert host_sum == checksum, "the host loop and the device give different candidates"
                case.update(host_fold_us=fold_us, host_relocalization_us=query_us, candidates_without_neighbours=len(cand))
            result["cases"].append(case)
            db.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
