"""GPU time of jsorb_distinctive_descriptors_async (k_distinct_plan + k_distinct_lanes x 2 + k_distinct_block) on a jsorb_keyframe_matcher for the
points of one C2 keyframe, rows refreshed in place in a descriptor table with `changed`.
The N distribution, written down here: set "frame" is 1000 points with N uniform in [2, 20] (what a keyframe's tracked points look like a few
keyframes into a sequence: most points 2 to 15 observations); set "frame_plus_landmarks" adds 20 points with N uniform in [100, 400] (the few
long-lived landmarks).  The observations are rows drawn at random from 60 keyframes x 1200 clustered descriptors (tests/distinct_cases.clustered).
Per set: median, p10 and p90 over --reps of the hipEvent span of the whole call on the matcher's stream.  Beside it the host loop of
examples/search_in_neighbors.cpp on the same inputs and the same box (tools/micro/distinct_host_loop.cpp, -O2, median of 20 passes), whose winners'
checksum must be the device's.  Prints one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_loop(start, row, kf, tmp):
    exe, src = os.path.join(tmp, "distinct_host_loop"), os.path.join(tmp, "in.bin")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "micro", "distinct_host_loop.cpp"), "-o", exe])
    with open(src, "wb") as f:
        f.write(np.array([len(start) - 1, len(row), len(kf)], np.int32).tobytes() + start.tobytes() + row.tobytes() + kf.tobytes())
    out = subprocess.run([exe, src, "20"], capture_output=True, text=True, timeout=600)
    m = re.search(r"host_loop_us=([\d.]+) checksum=(\d+)", out.stdout)
    assert out.returncode == 0 and m, out.stderr + out.stdout
    return float(m.group(1)), int(m.group(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import distinct_cases as dc
    from jetson_slam_amd import orb
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    m = orb.KeyframeMatcher()
    m.set_stream(stream.cuda_stream)
    lib = orb.load_library()
    rng = np.random.default_rng(7)
    kf = dc.clustered(rng, 60 * 1200, n_bases=400)
    frame = [int(x) for x in rng.integers(2, 21, 1000)]
    sets = (("frame", frame), ("frame_plus_landmarks", frame + [int(x) for x in rng.integers(100, 401, 20)]))
    result = {"tool": "distinct_bench", "reps": args.reps, "caps": orb.distinct_build_caps(), "kf_rows": len(kf), "cases": []}
    kf_d = dev(kf)
    with tempfile.TemporaryDirectory() as tmp:
        for name, ns in sets:
            start = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
            row = rng.integers(0, len(kf), int(start[-1])).astype(np.int32)
            n = len(ns)
            d = [dev(start), dev(row), torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")]
            call = lambda: lib.jsorb_distinctive_descriptors_async(m.handle, n, d[0].data_ptr(), len(row), d[1].data_ptr(), kf_d.data_ptr(), len(kf), None, n,
                                                                   d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr())
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
            best = d[4].cpu().numpy()
            case = {"set": name, "points": n, "observations": int(start[-1]), "stats": m.distinctive_descriptors_stats(),
                    "median_us": round(float(np.median(spans)), 2), "p10_us": round(float(np.percentile(spans, 10)), 2),
                    "p90_us": round(float(np.percentile(spans, 90)), 2)}
            if not args.no_host:
                us, checksum = host_loop(start, row, kf, tmp)
                assert checksum == int(row[start[:-1] + best].astype(np.int64).sum()), "the host loop and the device pick different winners"
                case["host_loop_us"] = us
            result["cases"].append(case)
    m.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
