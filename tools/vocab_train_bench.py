"""GPU time of jsorb_vocabulary_train (k_vocab_train.hip) on descriptors the extractor itself produced from `synth` frames (C5: 720 x 1280, 8
levels), device to device from the handle's buffers, one document per frame; k = 10.  Per size (--sizes, default 1e5 1e6 1e7 descriptors) and
depth (L = 4, 5, 6): the median over --reps calls of the hipEvent span of the whole call on a stream of its own, with the tree's size and the
association passes per level.  The call is synchronous and reads one word per pass, so the span includes the host's part (the tree, the
logarithms).
Beside the smallest size, where oracle/_ref/ref_vocab exists (authoring machines: tools/ref_vocab_goldens.py builds it), the reference's own
create() on the same input at L = 4, one run, wall clock of the process.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def extract_descriptors(orb, torch, want):
    """frames of jetson_slam_amd.synth until `want` descriptors: (device tensor uint8[n, 32], doc_start)"""
    from jetson_slam_amd.synth import synth_image
    lib = orb.load_library()
    h, w = 720, 1280
    g = orb.ORBExtractor(h, w, 1.2, 8, 9, 14, 7, 20, None, 20, 20)
    parts, doc_start, seed = [], [0], 1000
    while doc_start[-1] < want:
        g.extract(synth_image(seed, h, w))
        seed += 1
        n = min(g.n_keypoints(0), want - doc_start[-1])
        part = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        assert lib.jsorb_mem_d2d(ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(lib.jsorb_descriptors_device(g.handle, 0)), ctypes.c_size_t(32 * n)) == 0
        parts.append(part)
        doc_start.append(doc_start[-1] + n)
    lib.jsorb_mem_device_sync()
    return torch.cat(parts).contiguous(), np.asarray(doc_start, np.int32)


def timed(orb, torch, stream, desc, doc_start, L, reps):
    spans, t = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t = orb.train_vocabulary(desc, doc_start, 10, L, seed=1, stream_ptr=ctypes.c_void_p(stream.cuda_stream))
        b.record(stream)
        b.synchronize()
        spans.append(a.elapsed_time(b))
    return float(np.median(spans)), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=float, nargs="+", default=[1e5, 1e6, 1e7])
    ap.add_argument("--depths", type=int, nargs="+", default=[4, 5, 6])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import vocab_train_cases as vc
    from jetson_slam_amd import orb
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    sizes = sorted(int(s) for s in args.sizes)
    t0 = time.time()
    desc, doc_start = extract_descriptors(orb, torch, sizes[-1])
    result = {"tool": "vocab_train_bench", "k": 10, "reps": args.reps, "caps": orb.vocab_train_build_caps(), "frames": len(doc_start) - 1,
              "extract_s": round(time.time() - t0, 1), "cases": []}
    for n in sizes:
        n_docs = int(np.searchsorted(doc_start, n, side="left"))
        ds = np.concatenate([doc_start[:n_docs], [n]]).astype(np.int32)
        d = desc[:n]
        for L in args.depths:
            ms, t = timed(orb, torch, stream, d, ds, L, args.reps)
            result["cases"].append(dict(n=n, L=L, docs=len(ds) - 1, ms=round(ms, 2), nodes=t["n_nodes"], words=t["n_words"], runs=t["n_kmeans_runs"],
                                        passes=t["lloyd_passes"][:L], empty=t["n_empty_clusters"], unconverged=t["n_unconverged"]))
            print(json.dumps(result["cases"][-1]), file=sys.stderr, flush=True)
        if n == sizes[0] and not args.no_host and os.path.exists(vc.driver_path()):
            with tempfile.TemporaryDirectory() as tmp:
                w = dict(feats=d.cpu().numpy(), doc_start=ds, k=10, L=4, weighting=0, seed=1)
                t1 = time.time()
                ref = vc.run_driver(w, tmp)
                result["reference"] = dict(n=n, L=4, s=round(time.time() - t1, 2), survived=ref is not None)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
