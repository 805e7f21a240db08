"""The lanes of the device-resident batch path against the other users of a handle's streams (jsorb_api.hip: the device's lane pool, created
with the device's first handle that takes batches; jsorb_extract.hip: order_lanes_for_new_batch).

Every test works at the C1 geometry (320x240, 3 levels, tile 15) with JSORB_LANE_MIN_MPX=0.01, so that 16 images split into 4 lanes (a second
setting, 0.3, makes 12 images THREE lanes of 4 where 0.01 gives four lanes of 3).  Every batch gets other seeded images, so that a stale result shows, and every result -
keypoints, descriptors, uRight, depth, counts - is compared bit for bit with what a fresh handle pair under JSORB_MAX_LANES=1 computes for the
same images."""
import threading

import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair

H, W, L, TILE, TH = 240, 320, 3, 15, 20
FX, BF = 435.2, 47.906
MB = BF / FX


def _mk(orb, max_batch):
    return orb.ORBExtractor(H, W, 1.2, L, 9, 14, 7, TH, None, TILE, TILE, max_batch=max_batch)


_IMAGES = {}


def _images(seed0, n):
    """n seeded stereo pairs as two uint8 arrays [n, H, W] (made once)"""
    if (seed0, n) not in _IMAGES:
        pairs = [synth_stereo_pair(seed0 + i, H, W) for i in range(n)]
        _IMAGES[(seed0, n)] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    return _IMAGES[(seed0, n)]


def _collect(orb, gl, gr, n):
    out = []
    for i in range(n):
        u, d, st = orb.stereo_result(gl, i)
        out.append((gl.keypoints(i), gl.descriptors(i), gr.keypoints(i), gr.descriptors(i), u.view(np.uint32).copy(), d.view(np.uint32).copy(),
                    np.array([gl.n_keypoints(i), gr.n_keypoints(i), st["n_candidate_pairs"], st["n_corr_match"], st["n_depth"], st["n_final"]])))
    return out


_REFERENCE = {}


def _reference(orb, monkeypatch, seed0, n):
    """what a fresh handle pair on ONE lane computes for the pairs seed0 .. seed0 + n - 1 (computed once, never changed)"""
    import torch
    if (seed0, n) not in _REFERENCE:
        lefts, rights = _images(seed0, n)
        with monkeypatch.context() as m:
            m.setenv("JSORB_MAX_LANES", "1")
            gl, gr = _mk(orb, n), _mk(orb, n)
        ld, rd = torch.from_numpy(lefts).cuda(), torch.from_numpy(rights).cuda()
        gl.extract_batch_device_async(ld.data_ptr(), H * W, W, n, keep=ld)
        gr.extract_batch_device_async(rd.data_ptr(), H * W, W, n, keep=rd)
        orb.stereo_match_batch_async(gl, gr, MB, BF)
        gl.sync(); gr.sync()
        assert gl.launch_forms()["lanes"] == 1
        ref = _collect(orb, gl, gr, n)
        assert min(r[6][0] for r in ref) > 50 and max(r[6][5] for r in ref) > 10, "degenerate input"
        gl.close(); gr.close()
        _REFERENCE[(seed0, n)] = ref
    return _REFERENCE[(seed0, n)]


def _same(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        for k, (a, b) in enumerate(zip(g, r)):
            assert a.shape == b.shape and np.array_equal(a, b), (what, "image", i, "field", k)


def _device_batch(orb, gl, gr, ld, rd, n):
    gl.extract_batch_device_async(ld.data_ptr(), H * W, W, n, keep=ld)
    gr.extract_batch_device_async(rd.data_ptr(), H * W, W, n, keep=rd)
    orb.stereo_match_batch_async(gl, gr, MB, BF)


def _single_frame(orb, gl, gr, seed):
    """one pair through the synchronous single-image calls (the handle's own stream, the frame graph) and the synchronous match"""
    lefts, rights = _images(seed, 1)
    gl.extract(lefts[0]); gr.extract(rights[0])
    assert gl.launch_forms()["lanes"] == 1
    u, d, st = orb.compute_stereo_matches(gl, gr, MB, BF)
    return [(gl.keypoints(0), gl.descriptors(0), gr.keypoints(0), gr.descriptors(0), u.view(np.uint32).copy(), d.view(np.uint32).copy(),
             np.array([gl.n_keypoints(0), gr.n_keypoints(0), st["n_candidate_pairs"], st["n_corr_match"], st["n_depth"], st["n_final"]]))]


@pytest.mark.gpu
@pytest.mark.parametrize("min_mpx,lanes12", [("0.01", 4), ("0.3", 3)])
def test_one_handle_pair_through_batches_gather_and_single_frames(orb, monkeypatch, min_mpx, lanes12):
    """batch of 16 (4 lanes) -> stereo -> batch of 12 (another partition: every new lane waits for all old ones) -> stereo -> gather_counts on the
    main stream -> single frames on the same handles (own stream, graph captured on first use, replayed on the second) -> batch of 16 -> stereo"""
    import torch
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", min_mpx)
    refs = {k: _reference(orb, monkeypatch, *k) for k in ((1000, 16), (1100, 12), (1200, 1), (1201, 1), (1300, 16))}
    gl, gr = _mk(orb, 16), _mk(orb, 16)
    dev = {k: tuple(torch.from_numpy(a).cuda() for a in _images(*k)) for k in ((1000, 16), (1100, 12), (1300, 16))}

    _device_batch(orb, gl, gr, *dev[(1000, 16)], 16)
    gl.sync(); gr.sync()
    assert gl.launch_forms()["lanes"] == 4 and gr.launch_forms()["lanes"] == 4
    _same(_collect(orb, gl, gr, 16), refs[(1000, 16)], "first batch of 16")

    _device_batch(orb, gl, gr, *dev[(1100, 12)], 12)
    counts = torch.full((12 * 3,), -1, dtype=torch.int32, device="cuda")
    orb.gather_counts_async(gl, gr, counts.data_ptr())
    gl.sync(); gr.sync()
    assert gl.launch_forms()["lanes"] == lanes12
    _same(_collect(orb, gl, gr, 12), refs[(1100, 12)], "batch of 12")
    want = np.array([[r[6][0], r[6][1], r[6][5]] for r in refs[(1100, 12)]], np.int32)
    assert np.array_equal(counts.cpu().numpy().reshape(12, 3), want), "gathered counts"

    for seed in (1200, 1201):
        _same(_single_frame(orb, gl, gr, seed), refs[(seed, 1)], "single frame %d" % seed)

    _device_batch(orb, gl, gr, *dev[(1300, 16)], 16)
    gl.sync(); gr.sync()
    assert gl.launch_forms()["lanes"] == 4
    _same(_collect(orb, gl, gr, 16), refs[(1300, 16)], "batch of 16 behind the single frames")
    gl.close(); gr.close()


@pytest.mark.gpu
def test_two_handle_pairs_alive_one_on_a_second_thread(orb, monkeypatch):
    """two handle pairs share the device's lane pool (bench.py --full keeps two sets of handles alive): pair B runs batches from a second host thread
    while pair A captures its frame graph, replays it and runs batches of its own in between"""
    import torch
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.01")
    keys_a = [(2000, 1), (2100, 16), (2001, 1), (2200, 12), (2002, 1)]
    keys_b = [(2300, 16), (2400, 12), (2500, 16), (2600, 16)]
    refs = {k: _reference(orb, monkeypatch, *k) for k in keys_a + keys_b}
    dev = {k: tuple(torch.from_numpy(a).cuda() for a in _images(*k)) for k in keys_a + keys_b if k[1] > 1}
    al, ar, bl, br = _mk(orb, 16), _mk(orb, 16), _mk(orb, 16), _mk(orb, 16)
    torch.cuda.synchronize()
    got_b, err_b = {}, []
    start = threading.Barrier(2)

    def run_b():
        try:
            start.wait(timeout=30)
            for rnd in range(2):
                for k in keys_b:
                    _device_batch(orb, bl, br, *dev[k], k[1])
                    bl.sync(); br.sync()
                    got_b[(rnd, k)] = _collect(orb, bl, br, k[1])
        except Exception as e:      # reported by the main thread
            err_b.append(e)

    t = threading.Thread(target=run_b)
    t.start()
    start.wait(timeout=30)
    got_a = {}
    for rnd in range(2):
        for k in keys_a:
            if k[1] == 1:
                got_a[(rnd, k)] = _single_frame(orb, al, ar, k[0])
            else:
                _device_batch(orb, al, ar, *dev[k], k[1])
                al.sync(); ar.sync()
                got_a[(rnd, k)] = _collect(orb, al, ar, k[1])
    t.join(timeout=120)
    assert not t.is_alive() and not err_b, err_b
    assert len(got_b) == 2 * len(keys_b)
    for (rnd, k), got in list(got_a.items()) + list(got_b.items()):
        _same(got, refs[k], ("pair A" if k in keys_a else "pair B", rnd, k))
    for h in (al, ar, bl, br):
        h.close()


@pytest.mark.gpu
def test_caller_main_stream_with_a_copy_ahead_of_the_batch(orb, monkeypatch):
    """jsorb_set_stream: the caller's stream carries the copy that fills the input; the pool lanes must fork behind it, and the second copy into the
    same buffer must wait for the lanes of the first batch"""
    import torch
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.01")
    keys = [(3000, 16), (3100, 16), (3200, 12)]
    refs = {k: _reference(orb, monkeypatch, *k) for k in keys}
    pinned = {k: tuple(torch.from_numpy(a).pin_memory() for a in _images(*k)) for k in keys}
    gl, gr = _mk(orb, 16), _mk(orb, 16)
    s = torch.cuda.Stream()
    gl.set_stream(s.cuda_stream); gr.set_stream(s.cuda_stream)
    buf_l = torch.zeros((16, H, W), dtype=torch.uint8, device="cuda")
    buf_r = torch.zeros((16, H, W), dtype=torch.uint8, device="cuda")
    ballast = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k in keys:
        n = k[1]
        gl.stream_wait_done(s.cuda_stream); gr.stream_wait_done(s.cuda_stream)      # the last match reads the input buffers in place
        with torch.cuda.stream(s):
            for _ in range(4):
                ballast.fill_(1)            # keeps the stream busy, so that the copies are still pending when the lanes are enqueued
            buf_l[:n].copy_(pinned[k][0], non_blocking=True)
            buf_r[:n].copy_(pinned[k][1], non_blocking=True)
        _device_batch(orb, gl, gr, buf_l, buf_r, n)
        if k == keys[0]:
            continue                        # the second round's copies go out right behind the first batch: no host wait in between
        gl.sync(); gr.sync()
        assert gl.launch_forms()["lanes"] == 4
        _same(_collect(orb, gl, gr, n), refs[k], ("caller stream", k))
    gl.close(); gr.close()


@pytest.mark.gpu
def test_host_uploaded_batches_refill_the_landing_buffers(orb, monkeypatch):
    """host batches land in two buffers that are read in place as level 0, by the stereo match as well: batches 3 and 4 refill the buffers of
    batches 1 and 2 with no host wait in between"""
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.01")
    keys = [(4000, 16), (4100, 16), (4200, 12), (4300, 16)]
    refs = {k: _reference(orb, monkeypatch, *k) for k in keys}
    gl, gr = _mk(orb, 16), _mk(orb, 16)
    alive = []
    for i, k in enumerate(keys):
        lefts, rights = _images(*k)
        alive.append((lefts, rights))
        gl.extract_batch_host_async(lefts)
        gr.extract_batch_host_async(rights)
        orb.stereo_match_batch_async(gl, gr, MB, BF)
        if i in (0, 2):
            continue
        gl.sync(); gr.sync()
        _same(_collect(orb, gl, gr, k[1]), refs[k], ("host batch", i))
    gl.close(); gr.close()
