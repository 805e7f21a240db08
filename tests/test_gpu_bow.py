"""-m gpu: jsorb_bow_transform* (k_bow_transform) and jsorb_search_by_bow* (k_bow_group + k_bow_match + k_bow_resolve) against the sequential
transcriptions of TemplatedVocabulary::transform and ORBmatcher::SearchByBoW and the kernels' restatements of tests/test_bow_host.py - word ids,
node ids, matches, counts and statistics, bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jetson_slam_amd import vocabulary as V
from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import (ROTATION_KEPT, CONSTRUCTED, REAL_SEED, agree, both_transforms, chain_and_shallow_tree, default_params, flip_bits, frame_side, sampled_voc,
                           search_by_bow_reference, search_by_bow_restated, single_node_case, tied_tree)
from test_gpu_search_local import _dev, _mk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bow_params(orb, prm):
    return orb.make_bow_params(nn_ratio=float(prm["nn_ratio"]), th_low=prm["th_low"], check_orientation=prm["check_orientation"])


def side_of(g, image=0):
    return frame_side(g.keypoints(image), g.descriptors(image))


def host_both(KF, F, prm):
    """the transcription and the restatement (which must agree): (match_kf, nmatches, (node pairs, distances, largest node, ind))"""
    ref = search_by_bow_reference(KF, F, prm)
    st = agree(ref, search_by_bow_restated(KF, F, prm, rng=np.random.default_rng(0)))
    return ref[0], ref[1], st


def concat(kfs):
    """keyframes as the concatenated device arrays of jsorb_search_by_bow_async"""
    start = np.cumsum([0] + [len(k["node"]) for k in kfs]).astype(np.int32)
    cat = lambda key, dt, shape: np.concatenate([np.zeros((0,) + shape[1:], dt)] + [np.asarray(k[key], dt).reshape(shape) for k in kfs])
    return start, _dev(cat("node", np.int32, (-1,))), _dev(cat("valid", np.uint8, (-1,))), _dev(cat("angle", np.float32, (-1,))), _dev(cat("desc", np.uint8, (-1, 32)))


def check_search(orb, g, kfs, F, prm, f_node="given", sync=False, image=0):
    """one device call over the keyframes against both host functions, stats included; returns the host's results per keyframe"""
    import torch
    start, *arrs = concat(kfs)
    fn = _dev(F["node"].astype(np.int32)) if f_node == "given" else None
    if sync:
        mk, cnt = g.search_by_bow_host(start, *arrs, bow_params(orb, prm), f_node=fn, image=image)
    else:
        mk, cnt = g.search_by_bow(start, *arrs, bow_params(orb, prm), f_node=fn, image=image)
        torch.cuda.synchronize()
        mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
    hosts = [host_both(KF, F, prm) if len(KF["node"]) else (np.full(len(F["node"]), -1), 0, (0, 0, 0, (-1, -1, -1))) for KF in kfs]
    for i, h in enumerate(hosts):
        assert np.array_equal(mk[i], h[0]) and int(cnt[i]) == h[1], (i, int(cnt[i]), h[1])
    want = (sum(h[2][0] for h in hosts), sum(h[2][1] for h in hosts), max([h[2][2] for h in hosts] + [0]), hosts[0][2][3] if hosts else (-1, -1, -1))
    assert g.search_by_bow_stats() == want
    return hosts


def poke_frame(orb, g, desc, angle, image=0):
    """overwrite the first len(desc) descriptors and angles of the handle's extract result on the device: a frame side with constructed content"""
    lib = orb.load_library()
    n, N = len(desc), g.n_keypoints(image)
    assert 0 < n <= N
    d = np.ascontiguousarray(desc, np.uint8)
    a = np.ascontiguousarray(angle, np.float32)
    dp, kp = lib.jsorb_descriptors_device(g.handle, image), lib.jsorb_keypoints_device(g.handle, image)
    assert lib.jsorb_mem_h2d(ctypes.c_void_p(dp), ctypes.c_void_p(d.ctypes.data), ctypes.c_size_t(d.nbytes)) == 0
    assert lib.jsorb_mem_h2d(ctypes.c_void_p(kp + 4 * 3 * N), ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes)) == 0
    lib.jsorb_mem_device_sync()


def padded(F, N):
    """a constructed frame side as the first entries of N keypoints; the others are in no node"""
    n = len(F["node"])
    return dict(desc=np.concatenate([F["desc"], np.zeros((N - n, 32), np.uint8)]), angle=np.concatenate([F["angle"], np.zeros(N - n, np.float32)]),
                node=np.concatenate([F["node"], np.full(N - n, -1, np.int32)]).astype(np.int32))


# ---- the transform on descriptors at a device pointer ----
def _vocs():
    rng = np.random.default_rng(0)
    res = {"ragged": (V.random_tree(5, 7, 4, ragged=True, tie=0.4, zero_weight=0.2, max_nodes=400), None), "chain": (chain_and_shallow_tree(), None),
           "one_child": (V.random_tree(6, 1, 3), None)}
    for k in (15, 16, 17, 33):
        res["tied%d" % k] = tied_tree(k, 2)
    return res, rng


@pytest.mark.parametrize("kind", ["ragged", "chain", "one_child", "tied15", "tied16", "tied17", "tied33"])
def test_transform_descriptors(orb, kind):
    import torch
    vocs, rng = _vocs()
    tree, d0 = vocs[kind]
    info_k = int(np.diff(tree["child_start"]).max())
    for levels_up in (0, 1, tree["depth_L"]):
        voc = orb.Vocabulary(tree, levels_up=levels_up)
        assert voc.info() == dict(n_nodes=tree["n_nodes"], n_words=int((tree["word_id"] >= 0).sum()), depth_L=tree["depth_L"], levels_up=levels_up,
                                  max_children=info_k)
        for n in (0, 1, 15, 16, 17, 1000) if levels_up == 1 else (17,):
            desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            if n:
                src = tree["descriptors"][rng.integers(1, tree["n_nodes"], n)] if d0 is None else np.repeat(d0[None], n, 0)
                near = rng.random(n) < 0.7
                desc[near] = flip_bits(rng, src[near], 0, 9)
            word, node = orb.bow_transform_descriptors(voc, _dev(desc) if n else torch.empty((0, 32), dtype=torch.uint8, device="cuda"))
            ref = both_transforms(tree, desc, levels_up)
            assert np.array_equal(word.cpu().numpy(), ref[0]) and np.array_equal(node.cpu().numpy(), ref[1]), (kind, levels_up, n)
        voc.close()


# ---- the handle form: one image, a batch in one launch, and the life of the buffers ----
def test_transform_on_extracted_frames(orb, configs):
    import torch
    c = configs["c1"]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    L = side_of(g)
    tree = sampled_voc(L["desc"])
    voc = orb.Vocabulary(tree, levels_up=1)
    lib = orb.load_library()
    assert g.bow_device_pointers() == (0, 0)
    with pytest.raises(orb.JsorbError):
        g.bow()
    g.bow_transform(voc)
    ref = both_transforms(tree, L["desc"], 1)
    word, node = g.bow()
    assert np.array_equal(word, ref[0]) and np.array_equal(node, ref[1]) and g.bow_transform_stats() == ref[2]
    pw, pn = g.bow_device_pointers()
    assert pw and pn and pw != pn
    # the next extract replaces them: nothing to read until the next transform, which reuses the same buffers
    g.extract(right)
    assert g.bow_device_pointers() == (0, 0)
    with pytest.raises(orb.JsorbError):
        g.bow()
    assert lib.jsorb_bow_transform_async(g.handle, 1, voc.handle) != 0 and lib.jsorb_bow_transform_async(g.handle, -2, voc.handle) != 0
    g.bow_transform(voc)
    R = side_of(g)
    ref = both_transforms(tree, R["desc"], 1)
    word, node = g.bow()
    assert np.array_equal(word, ref[0]) and np.array_equal(node, ref[1]) and g.bow_device_pointers() == (pw, pn)
    # a shallow vocabulary through the handle: the statistics count the leaves above the node level
    chain = chain_and_shallow_tree()
    cv = orb.Vocabulary(chain, levels_up=0)
    g.bow_transform(cv)
    ref = both_transforms(chain, R["desc"], 0)
    word, node = g.bow()
    assert np.array_equal(word, ref[0]) and np.array_equal(node, ref[1]) and g.bow_transform_stats() == ref[2] > 0
    # a batch of 3 images, image = -1: one launch, counts read on the device
    imgs = [left, right, synth_stereo_pair(REAL_SEED + 1, c["h"], c["w"])[0]]
    b = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=4)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    b.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], 3, keep=dev)
    b.bow_transform(voc, image=-1)                   # enqueued behind the lanes, before anything was waited for
    b.sync()
    for i in range(3):
        S = side_of(b, i)
        ref = both_transforms(tree, S["desc"], 1)
        word, node = b.bow(i)
        assert np.array_equal(word, ref[0]) and np.array_equal(node, ref[1]), i
    assert np.array_equal(b.descriptors(0), L["desc"])
    # image 1 alone after a fresh batch: the others have none
    b.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], 3, keep=dev)
    b.sync()
    b.bow_transform(voc, image=1)
    assert np.array_equal(b.bow(1)[1], both_transforms(tree, side_of(b, 1)["desc"], 1)[1]) and b.bow_device_pointers(0) == (0, 0) and b.bow_device_pointers(2) == (0, 0)
    # kernel timing names the launch
    g.enable_kernel_timing(True)
    g.bow_transform(voc)
    assert g.bow_kernel_times()["k_bow_transform"][1] == 1
    g.enable_kernel_timing(False)


# ---- the matcher: left as the keyframe of the right image ----
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_search_by_bow_on_real_frames(orb, configs, name):
    c = configs[name]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    L = side_of(g)
    tree = sampled_voc(L["desc"])
    voc = orb.Vocabulary(tree, levels_up=1)
    g.bow_transform(voc)
    L["node"] = g.bow()[1]
    L["valid"] = (np.random.default_rng(3).random(len(L["node"])) < 0.95).astype(np.uint8)
    g.extract(right)
    g.bow_transform(voc)
    R = side_of(g)
    R["node"] = g.bow()[1]
    assert np.array_equal(R["node"], both_transforms(tree, R["desc"], 1)[1])
    itself = dict(R, valid=np.ones(len(R["node"]), np.uint8))
    empty = dict(desc=np.zeros((0, 32), np.uint8), angle=np.zeros(0, np.float32), node=np.zeros(0, np.int32), valid=np.zeros(0, np.uint8))
    for ratio in (0.7, 0.75):
        for rot in (1, 0):
            prm = default_params(nn_ratio=f32(ratio), check_orientation=rot)
            h = check_search(orb, g, [L, itself, empty], R, prm, f_node="given" if rot else "handle")
            assert h[0][1] >= 15 and h[1][1] > h[0][1] and h[0][2][0] > 20, (ratio, rot, h[0][1])
            h1 = check_search(orb, g, [L], R, prm, f_node="handle" if rot else "given", sync=True)
            assert h1[0][1] == h[0][1]
    check_search(orb, g, [empty, L], R, default_params(), sync=True)      # an empty keyframe first: keyframe 0's kept bins are none
    g.enable_kernel_timing(True)
    check_search(orb, g, [L, itself], R, default_params())
    t = g.bow_kernel_times()
    assert [t[k][1] for k in ("k_bow_group", "k_bow_match", "k_bow_resolve")] == [1, 1, 1]
    g.enable_kernel_timing(False)


# ---- constructed content in the handle's frame: the host cases, the large single node ----
def test_constructed_cases_through_the_device(orb, configs):
    c = configs["c2"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(REAL_SEED, c["h"], c["w"])[0])
    N = g.n_keypoints()
    for name in sorted(CONSTRUCTED):
        (KF, F), prm, want, count = CONSTRUCTED[name]
        poke_frame(orb, g, F["desc"], F["angle"])
        Fp = padded(F, N)
        for sync in (False, True):
            h = check_search(orb, g, [KF], Fp, prm, sync=sync)
            assert list(h[0][0][:len(want)]) == want and h[0][1] == count, name
            assert name not in ROTATION_KEPT or g.search_by_bow_stats()[3] == ROTATION_KEPT[name], name      # the rotation check's edges: kept_bins


@pytest.mark.parametrize("variant", [None, "tiny_bow_wave"])
def test_single_node_of_more_than_300_entries(orb, configs, monkeypatch, variant):
    from jetson_slam_amd import build as jb
    if variant:
        monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant(variant, *jb.VARIANTS[variant])))
    assert orb.bow_build_caps() == ((1, 4096) if variant else (2, 4096))       # the library in use is the build the test means
    c = configs["c2"]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(REAL_SEED, c["h"], c["w"])[0])
    N = g.n_keypoints()
    # every keypoint of the real frame in one node, the frame against itself: a node of N entries
    R = side_of(g)
    R["node"] = np.zeros(N, np.int32)
    R["valid"] = np.ones(N, np.uint8)
    h = check_search(orb, g, [R], R, default_params(th_low=30))
    assert h[0][2][2] == N > 1000
    # the constructed node of more than 300 entries as the first keypoints of the frame (the others in no node)
    voc, KF, F = single_node_case()
    assert N >= len(F["node"])
    poke_frame(orb, g, F["desc"], F["angle"])
    # the node ids through the device as well: levels_up = depth_L, everything in the root
    v = orb.Vocabulary(voc, levels_up=2)
    g.bow_transform(v)
    assert np.array_equal(g.bow()[1][:len(F["node"])], F["node"])
    Fp = padded(F, N)
    for prm in (default_params(), default_params(nn_ratio=f32(0.9), check_orientation=0)):
        h = check_search(orb, g, [KF, KF], Fp, prm)
        assert h[0][2][2] >= 300 and h[0][2][0] == 1 and h[0][1] > 20


# ---- the build that sorts at most 64 keys in LDS: every side of a frame takes k_bow_group's sort in global memory ----
def test_global_memory_sort_build(orb, configs, monkeypatch):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_bow_sort", *jb.VARIANTS["tiny_bow_sort"])))
    assert orb.bow_build_caps() == (2, 64)
    c = configs["c1"]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    L = side_of(g)
    tree = sampled_voc(L["desc"])
    L["node"] = both_transforms(tree, L["desc"], 1)[1]
    L["valid"] = np.ones(len(L["node"]), np.uint8)
    g.extract(right)
    R = side_of(g)
    R["node"] = both_transforms(tree, R["desc"], 1)[1]
    assert len(R["node"]) > 4 * 64 and len(L["node"]) > 4 * 64
    short = {k: v[:50] for k, v in L.items()}        # a side that still fits the LDS next to sides that do not
    empty = {k: v[:0] for k, v in L.items()}
    h = check_search(orb, g, [L, dict(R, valid=np.ones(len(R["node"]), np.uint8)), short, empty], R, default_params())
    assert h[0][1] >= 15 and h[1][1] > h[0][1]
    # keys that are no permutation of a small range: large node ids, keypoints in no node, and one node for everything
    rng = np.random.default_rng(8)
    wild = dict(R, node=np.where(rng.random(len(R["node"])) < 0.2, -1, R["node"] * 7919 + 2 ** 30).astype(np.int32))
    check_search(orb, g, [dict(L, node=(L["node"] * 7919 + 2 ** 30).astype(np.int32))], wild, default_params(nn_ratio=f32(0.75)))
    one = dict(R, node=np.zeros(len(R["node"]), np.int32), valid=np.ones(len(R["node"]), np.uint8))
    check_search(orb, g, [one], one, default_params(th_low=30), sync=True)


# ---- edges and validation ----
def test_edges_and_validation(orb, configs):
    import torch
    c = configs["c1"]
    lib = orb.load_library()
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(REAL_SEED, c["h"], c["w"])[1])
    R = side_of(g)
    N = len(R["angle"])
    R["node"] = (np.arange(N) % 7).astype(np.int32)
    KF = dict(R, valid=np.ones(N, np.uint8))
    prm = default_params()
    p = bow_params(orb, prm)
    assert lib.jsorb_search_by_bow_stats(g.handle, None, None, None, None) != 0      # before any call
    # n_keyframes == 0
    check_search(orb, g, [], R, prm)
    check_search(orb, g, [], R, prm, sync=True)
    # only empty keyframes
    empty = dict(desc=np.zeros((0, 32), np.uint8), angle=np.zeros(0, np.float32), node=np.zeros(0, np.int32), valid=np.zeros(0, np.uint8))
    check_search(orb, g, [empty, empty], R, prm)
    # no keypoint in any node, on either side
    none = dict(R, node=np.full(N, -1, np.int32))
    h = check_search(orb, g, [KF], none, prm)
    assert h[0][1] == 0
    h = check_search(orb, g, [dict(KF, node=none["node"])], R, prm)
    assert h[0][1] == 0
    # N == 0: a flat image has no keypoints
    flat = _mk(orb, c)
    flat.extract(np.full((c["h"], c["w"]), 128, np.uint8))
    assert flat.n_keypoints(0) == 0
    Fz = dict(desc=np.zeros((0, 32), np.uint8), angle=np.zeros(0, np.float32), node=np.zeros(0, np.int32))
    for sync in (False, True):
        h = check_search(orb, flat, [KF, empty], Fz, prm, sync=sync)
        assert h[0][1] == 0
    voc = orb.Vocabulary(V.random_tree(1, 3, 2), levels_up=1)
    flat.bow_transform(voc)
    assert len(flat.bow()[0]) == 0 and flat.bow_transform_stats() == 0
    check_search(orb, flat, [KF], Fz, prm, f_node="handle")
    # validation
    start, *arrs = concat([KF])
    ptrs = [t.data_ptr() for t in arrs]
    fn = _dev(R["node"])
    mk = torch.zeros(2 * N + 64, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    call = lambda prm_=p, f=fn.data_ptr(), nk=1, ks=start, a=ptrs, o=(mk.data_ptr(), cnt.data_ptr()), image=0: \
        lib.jsorb_search_by_bow_async(g.handle, image, ctypes.byref(prm_) if prm_ is not None else None, f, nk, ks.ctypes.data if ks is not None else None, *a, *o)
    assert call() == 0
    assert call(prm_=None) == -1 and call(nk=-1) == -1 and call(nk=257) == -1 and call(ks=None) == -1 and call(image=3) != 0
    for j in range(4):
        assert call(a=ptrs[:j] + [None] + ptrs[j + 1:]) == -1, j
    assert call(a=ptrs[:3] + [ptrs[3] + 8]) == -1                        # misaligned descriptors
    assert call(o=(None, cnt.data_ptr())) == -1 and call(o=(mk.data_ptr(), None)) == -1
    assert call(ks=np.array([5, 2], np.int32)) == -1 and call(ks=np.array([-1, 2], np.int32)) == -1
    assert call(f=None) == -4                                            # no transform of this image since the extract
    two = np.array([N // 2, N // 2, N], np.int32)                        # offsets that do not start at 0: an empty keyframe, then the second half
    assert call(nk=2, ks=two) == 0
    g.sync()
    half = {k: v[N // 2:] for k, v in KF.items()}
    assert np.array_equal(mk.cpu().numpy()[N:2 * N], host_both(half, R, prm)[0]) and (mk.cpu().numpy()[:N] == -1).all()
    fresh = _mk(orb, c)
    assert lib.jsorb_search_by_bow_async(fresh.handle, 0, ctypes.byref(p), None, 0, None, *([None] * 6)) != 0      # no extract yet
    assert lib.jsorb_bow_transform_async(fresh.handle, 0, voc.handle) != 0
    with pytest.raises(orb.JsorbError):
        g.search_by_bow(start, arrs[0].long(), *arrs[1:], p)
    with pytest.raises(orb.JsorbError):
        orb.bow_transform_descriptors(voc, torch.zeros((4, 31), dtype=torch.uint8, device="cuda"))
    assert lib.jsorb_bow_transform_descriptors(None, voc.handle, 4, ctypes.c_void_p(arrs[3].data_ptr() + 8), None, None) == -1
    assert lib.jsorb_bow_transform_descriptors(None, voc.handle, -1, ctypes.c_void_p(arrs[3].data_ptr()), None, None) == -1


# ---- the C++ example through the compat shim gives the count the Python path gives ----
def test_track_reference_keyframe_example(orb, configs, tmp_path):
    from jetson_slam_amd import build as jb
    c = configs["c1"]
    exe = jb.build_example("track_reference_keyframe", str(tmp_path / "track_reference_keyframe"))
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    L = side_of(g)
    tree = sampled_voc(L["desc"])
    lp, rp, vp, op = (str(tmp_path / s) for s in ("keyframe.raw", "current.raw", "vocabulary.bin", "out.bin"))
    left.tofile(lp)
    right.tofile(rp)
    with open(vp, "wb") as f:
        f.write(np.array([tree["n_nodes"], tree["depth_L"], 1], np.int32).tobytes())
        for key in ("child_start", "children", "descriptors", "word_id", "weight"):
            f.write(np.ascontiguousarray(tree[key]).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, vp, op], timeout=300, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    L["node"] = both_transforms(tree, L["desc"], 1)[1]
    L["valid"] = np.ones(len(L["node"]), np.uint8)
    g.extract(right)
    R = side_of(g)
    R["node"] = both_transforms(tree, R["desc"], 1)[1]
    h = check_search(orb, g, [L], R, default_params())
    blob = np.fromfile(op, np.int32)
    N, n_kf = len(R["node"]), len(L["node"])
    assert int(blob[0]) == h[0][1] >= 15 and int(blob[1]) == N and np.array_equal(blob[2:2 + N], h[0][0])
    assert int(blob[2 + N]) == n_kf and np.array_equal(blob[3 + N:3 + N + n_kf], L["node"])
    assert ("nmatches=%d" % h[0][1]) in out.stdout
