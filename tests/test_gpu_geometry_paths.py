"""-m gpu: the kernel forms that the SHIPPED library selects from the image geometry, each reached by a geometry that selects it on its own (no
environment switch, no experiments build) and compared bit for bit with the CPU oracle: tile candidates of every level, keypoints, descriptors,
angles, stereo uRight / depth and n_final.  Every geometry runs as single frames (latency layouts) and as a device batch; jsorb_handle_forms
(ORBExtractor.launch_forms) proves which arm each handle took.  tests/test_launch_forms_host.py pins the same rules on the host.

| arm                                                      | selected when                       | geometries here                        |
|----------------------------------------------------------|-------------------------------------|----------------------------------------|
| k_compact (level by level, no scan-line buckets)         | T > 65536                           | 1200x1600 tile 16, 720x1280 L4 tile 8, |
|                                                          |                                     | 1300x256 L10 tile 6                    |
| k_stereo tile-row scan, column-pruned                    | T > 65536 or L * H0 > 12288         | 1537x2048, 1080x1920 L12, the above    |
| k_blur_compact refused for its bucket LDS (T <= 32768)   | L * H0 > 10240                      | 1281x1024 tile 40                      |
| k_blur_compact at 40 KB of bucket counters               | L * H0 = 10240                      | 1280x1024 tile 40                      |
| NMS-MS CPU mode refused                                  | T > 32768                           | 480x752 L12 tile 14                    |
"""
import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair

pytestmark = pytest.mark.gpu

MB, MBF = 0.1, 100.0
FUSE_ALL_BELOW_MPX = 24.0          # jsorb_extract.hip JSORB_FUSE_ALL_BELOW_MPX
CMP_MID_T = 8192


def _mk(orb, H, W, L, tile, max_batch=1, tile_w=None, nms_ms=False, nms_gpu=True):
    return orb.ORBExtractor(H, W, 1.2, L, 9, 14, 7, 20, None, tile, tile_w or tile, False, nms_ms, nms_gpu, max_batch=max_batch)


def _mko(po, H, W, L, tile, tile_w=None, nms_ms=False, nms_gpu=True):
    return po.OracleExtractor(height=H, width=W, n_levels=L, tile_h=tile, tile_w=tile_w or tile, apply_nms_ms=nms_ms, nms_ms_mode_gpu=nms_gpu)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class _Ref:
    """the oracle's results for one stereo pair"""

    def __init__(self, po, geo, left, right, **kw):
        self.ol, self.orr = _mko(po, *geo, **kw), _mko(po, *geo, **kw)
        self.ol.extract(left); self.orr.extract(right)
        self.u, self.d, self.st = po.stereo_match(self.ol, self.orr, MB, MBF)
        L = geo[2]
        self.angles = [np.concatenate([o.level_keypoints(i)[3] for i in range(L)]) for o in (self.ol, self.orr)]

    def matched_levels(self):
        return set(self.ol.keypoints().reshape(6, -1)[4][self.u >= 0].tolist())


def _check_image(g, o, angles, i):
    for a, b in zip(g.tile_candidates(i), o.tiles()):      # every level's tile winners
        assert np.array_equal(a, b)
    assert g.n_keypoints(i) == o.n
    assert np.array_equal(g.keypoints(i), o.keypoints())
    assert np.array_equal(g.descriptors(i), o.descriptors())
    assert _same_bits(g.angles(i), angles)


def _check_pair(orb, gl, gr, ref, i, single):
    _check_image(gl, ref.ol, ref.angles[0], i)
    _check_image(gr, ref.orr, ref.angles[1], i)
    u, d, st = orb.compute_stereo_matches(gl, gr, MB, MBF) if single else orb.stereo_result(gl, i)
    assert _same_bits(u, ref.u) and _same_bits(d, ref.d)
    assert st["n_final"] == ref.st["n_final"]


def _check_forms(orb, g, geo, max_batch, **want):
    """the handle runs what jsorb_plan_forms plans for its geometry (no silent fall-back), and that is the arm this test is about"""
    H, W, L, tile = geo
    f = g.launch_forms()
    plan = orb.plan_forms(H, W, 1.2, L, tile, tile, max_batch=max_batch)
    assert {k: f[k] for k in plan} == plan
    assert f["detect_compact"] == (1 if max_batch > 1 else 0)
    assert {k: f[k] for k in want} == want, (geo, max_batch, f)
    return f


def _expected_schedule(g, n, K):
    """run_pipeline's lane schedule (jsorb_extract.hip lane_order and the per-lane fusion rule), restated"""
    lane_mpx = sum(h * w for h, w in g.level_dims()) * n / K * 1e-6
    order = 0 if (K & 1) or lane_mpx < FUSE_ALL_BELOW_MPX else (1 if g.level_tiles()[0][0] <= 40 else 2)
    f = g.launch_forms()
    blur_first = [K > 1 and (j & 1) == 1 and order == 1 for j in range(K)]
    fuse = [n > 1 and (K > 1 or g.T <= CMP_MID_T) and not blur_first[j] and order != 2 and f["blur_compact_fusable"] == 1 for j in range(K)]
    mask = lambda bits: sum(1 << j for j, b in enumerate(bits) if b)
    return dict(lanes=K, lane_order=order, blur_compact_lanes=mask(fuse), blur_first_lanes=mask(blur_first))


def _run(orb, po, monkeypatch, geo, pairs, single=None, batch=None, lanes=3, n=None):
    """single frames on latency handles, then one device batch of n images (the pairs repeated) on throughput handles, which must run on `lanes`
    lanes; with lanes > 1 and no n, JSORB_LANE_MIN_MPX lets every image have a lane of its own"""
    import torch
    H, W, L, tile = geo
    refs = [_Ref(po, geo, l, r) for l, r in pairs]
    assert len(refs[0].matched_levels()) == L                  # the stereo scan is exercised on every level
    if single is not None:
        gl, gr = _mk(orb, *geo), _mk(orb, *geo)
        _check_forms(orb, gl, geo, 1, **single)
        gl.extract(pairs[0][0]); gr.extract(pairs[0][1])
        _check_pair(orb, gl, gr, refs[0], 0, True)
        assert gl.launch_forms()["lanes"] == 1
        del gl, gr
    if batch is not None:
        n = n or len(pairs)
        idx = [i % len(pairs) for i in range(n)]
        if lanes > 1 and n == len(pairs):                      # read at handle creation: one image per lane at least, min(4, n) lanes
            monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.01")
        else:
            monkeypatch.delenv("JSORB_LANE_MIN_MPX", raising=False)
        gl, gr = _mk(orb, *geo, max_batch=n), _mk(orb, *geo, max_batch=n)
        monkeypatch.delenv("JSORB_LANE_MIN_MPX", raising=False)
        _check_forms(orb, gl, geo, n, **batch)
        lefts = torch.from_numpy(np.stack([pairs[i][0] for i in idx])).cuda()
        rights = torch.from_numpy(np.stack([pairs[i][1] for i in idx])).cuda()
        gl.extract_batch_device_async(lefts.data_ptr(), H * W, W, n, keep=lefts)
        gr.extract_batch_device_async(rights.data_ptr(), H * W, W, n, keep=rights)
        orb.stereo_match_batch_async(gl, gr, MB, MBF)
        gl.sync(); gr.sync()
        sched = gl.launch_forms()
        assert sched["lanes"] == lanes
        assert {k: sched[k] for k in orb.LANE_KEYS} == _expected_schedule(gl, n, lanes)
        for i in range(n):
            _check_pair(orb, gl, gr, refs[idx[i]], i, False)
        return sched


def _pairs(geo, seeds):
    return [synth_stereo_pair(s, geo[0], geo[1]) for s in seeds]


# ---- L * H0 against 12288: scan-line buckets / tile-row scan ----
def test_bucket_limit_holds_at_L_times_H0_12288(orb, po, monkeypatch):
    geo = (1536, 2048, 8, 30)
    _run(orb, po, monkeypatch, geo, _pairs(geo, (41, 42, 43)), single=dict(stereo_buckets=1, compact_form=3), batch=dict(stereo_buckets=1, compact_form=3))


def test_tile_row_scan_above_L_times_H0_12288(orb, po, monkeypatch):
    geo = (1537, 2048, 8, 30)
    s = _run(orb, po, monkeypatch, geo, _pairs(geo, (41, 42, 43)), single=dict(stereo_buckets=0, compact_form=3),
             batch=dict(stereo_buckets=0, compact_form=3, blur_compact_fusable=1))
    assert (s["lane_order"], s["blur_compact_lanes"]) == (0, 0b111)      # no bucket counters: k_blur_compact on every lane


def test_tile_row_scan_with_twelve_levels(orb, po, monkeypatch):
    geo = (1080, 1920, 12, 30)
    _run(orb, po, monkeypatch, geo, _pairs(geo, (44, 45)), single=dict(stereo_buckets=0), batch=dict(stereo_buckets=0), lanes=2)


# ---- T against 65536: level-by-level k_compact and the tile-row scan ----
def test_level_by_level_compaction_above_65536_tiles(orb, po, monkeypatch):
    geo = (1200, 1600, 8, 16)
    _run(orb, po, monkeypatch, geo, _pairs(geo, (46, 47, 48)), single=dict(compact_form=4, stereo_buckets=0, nms_ms_cpu_ok=0),
         batch=dict(compact_form=4, stereo_buckets=0, blur_compact_fusable=0))


def test_flat_compaction_and_buckets_below_65536_tiles(orb, po, monkeypatch):
    geo = (1200, 1600, 8, 17)
    _run(orb, po, monkeypatch, geo, _pairs(geo, (46, 47, 48)), single=dict(compact_form=3, stereo_buckets=1),
         batch=dict(compact_form=3, stereo_buckets=1, blur_compact_fusable=0))


def test_level_by_level_compaction_with_small_tiles(orb, po, monkeypatch):
    geo = (720, 1280, 4, 8)
    _run(orb, po, monkeypatch, geo, _pairs(geo, (49, 50, 51)), single=dict(compact_form=4, stereo_buckets=0), batch=dict(compact_form=4, stereo_buckets=0))


def test_tile_row_scan_with_one_row_tiles(orb, po, monkeypatch):
    """levels 7-9 have tiles of one row and one column: the scan's division by the tile height / width takes its th == 1 / tw == 1 branch"""
    geo = (1300, 256, 10, 6)
    g = _mk(orb, *geo)
    assert [g.level_tiles()[i][:2] for i in (7, 8, 9)] == [(1, 1)] * 3
    del g
    _run(orb, po, monkeypatch, geo, _pairs(geo, (52, 53, 54)), single=dict(compact_form=4, stereo_buckets=0), batch=dict(compact_form=4, stereo_buckets=0))


# ---- T around 32768: NMS-MS CPU mode, k_blur_compact's tables ----
@pytest.mark.parametrize("tile,T", [(14, 32918), (15, 23531)])
def test_nms_ms_modes_around_32768_tiles(orb, po, tile, T):
    geo = (480, 752, 12, tile)
    l, r = synth_stereo_pair(55, 480, 752)
    modes = (True, False)
    if T > 32768:
        with pytest.raises(orb.JsorbError) as ei:
            _mk(orb, *geo, nms_ms=True, nms_gpu=False)
        assert "rc=-3" in str(ei.value) and "NMS-MS CPU mode supports at most 32768 tiles" in str(ei.value)
        modes = (True,)
    for nms_gpu in modes:
        ref = _Ref(po, geo, l, r, nms_ms=True, nms_gpu=nms_gpu)
        gl, gr = _mk(orb, *geo, nms_ms=True, nms_gpu=nms_gpu), _mk(orb, *geo, nms_ms=True, nms_gpu=nms_gpu)
        assert gl.T == T and gl.launch_forms()["nms_ms_cpu_ok"] == (1 if T <= 32768 else 0)
        gl.extract(l); gr.extract(r)
        _check_pair(orb, gl, gr, ref, 0, True)
        assert ref.st["n_final"] > 1000


@pytest.mark.parametrize("tile,fusable", [(14, 0), (15, 1)])
def test_blur_compact_table_limit_around_32768_tiles(orb, po, monkeypatch, tile, fusable):
    geo = (480, 752, 12, tile)
    s = _run(orb, po, monkeypatch, geo, _pairs(geo, (56, 57, 58)), batch=dict(stereo_buckets=1, blur_compact_fusable=fusable))
    assert s["blur_compact_lanes"] == (0b111 if fusable else 0)


# ---- k_blur_compact's bucket counters against 40 KB of LDS ----
def test_blur_compact_at_its_lds_bound_in_one_lane(orb, po, monkeypatch):
    geo = (1280, 1024, 8, 40)                                 # L * H0 = 10240: 40 KB of bucket counters, T = 6904
    s = _run(orb, po, monkeypatch, geo, _pairs(geo, (59, 60)), single=dict(stereo_buckets=1), batch=dict(blur_compact_fusable=1, compact_form=2), lanes=1)
    assert s["blur_compact_lanes"] == 1


def test_blur_compact_refused_above_its_lds_bound(orb, po, monkeypatch):
    geo = (1281, 1024, 8, 40)                                 # L * H0 = 10248
    s = _run(orb, po, monkeypatch, geo, _pairs(geo, (59, 60)), single=dict(stereo_buckets=1), batch=dict(blur_compact_fusable=0, stereo_buckets=1), lanes=1)
    assert s["blur_compact_lanes"] == 0
    _run(orb, po, monkeypatch, geo, _pairs(geo, (61, 62, 63)), batch=dict(blur_compact_fusable=0), lanes=3)


def test_blur_compact_on_every_lane_of_an_odd_lane_count(orb, po, monkeypatch):
    geo = (1280, 1024, 8, 30)                                 # T = 12420, the re-reading 1024-thread compaction inside k_blur_compact
    s = _run(orb, po, monkeypatch, geo, _pairs(geo, (64, 65, 66)), batch=dict(blur_compact_fusable=1, compact_form=3), lanes=3)
    assert (s["lane_order"], s["blur_compact_lanes"]) == (0, 0b111)


# ---- T around 4096 and 8192: the compaction launches of batch handles ----
# One lane compacts inside k_blur_compact (T <= 8192); k_compact's own launch runs on the lanes that take k_blur first, i.e. with an even lane
# count and over 24 MPx of pyramid per lane (the n below), and everywhere above 8192 tiles with one lane.
@pytest.mark.parametrize("geo,single_form,batch_form,n", [((720, 1280, 4, 30), 3, 2, 22), ((480, 752, 4, 20), 0, 1, 58), ((480, 752, 8, 20), 3, 3, 0)])
def test_batch_compaction_forms_around_4096_and_8192_tiles(orb, po, monkeypatch, geo, single_form, batch_form, n):
    pairs = _pairs(geo, (67, 68, 69))
    s = _run(orb, po, monkeypatch, geo, pairs, single=dict(compact_form=single_form), batch=dict(compact_form=batch_form), lanes=1)
    assert s["blur_compact_lanes"] == (0 if batch_form == 3 else 1)
    if n:
        s = _run(orb, po, monkeypatch, geo, pairs, batch=dict(compact_form=batch_form), lanes=2, n=n)
        assert (s["lane_order"], s["blur_first_lanes"], s["blur_compact_lanes"]) == (1, 0b10, 0b01)
    else:
        _run(orb, po, monkeypatch, geo, pairs, batch=dict(compact_form=batch_form), lanes=3)


# ---- ties: K3's horizontal tree against the arg-max by column rank ----
def _tie_image(H, W):
    """bright 2x2 dots every 4 columns: the FAST scores repeat exactly along x, so most tiles hold their maximum at several columns; the
    background and the dots vary down the rows only"""
    y, x = np.mgrid[0:H, 0:W]
    dots = ((x % 4) < 2) & ((y % 6) < 2)
    return np.where(dots, 220 - (y % 6) * 3, 60 + (y * 7) % 50).astype(np.uint8)


@pytest.mark.parametrize("tw", [3, 5, 7, 31, 33, 63, 65, 127])
def test_tie_heavy_tile_rows_follow_the_literal_tree(orb, po, tw):
    import torch
    H, W, th = 160, max(8 * tw, 320), 12
    img = _tie_image(H, W)
    o = _mko(po, H, W, 2, th, tile_w=tw)
    o.extract(img)
    S, tiled, tied = o.level_score(0), 0, 0
    for ty in range(0, H, th):
        for tx in range(0, W, tw):
            blk = S[ty:ty + th, tx:tx + tw]
            if blk.max() > 0:
                tiled += 1
                tied += len(np.unique(np.nonzero(blk == blk.max())[1])) >= 2
    assert tiled >= 20 and 3 * tied >= tiled                   # the input really is tie-heavy
    angles = np.concatenate([o.level_keypoints(i)[3] for i in range(2)])
    g = _mk(orb, H, W, 2, th, tile_w=tw)
    assert g.launch_forms()["tree_replay_levels"] == 0
    g.extract(img)
    _check_image(g, o, angles, 0)
    gb = _mk(orb, H, W, 2, th, tile_w=tw, max_batch=2)          # the compact k_detect form
    assert gb.launch_forms()["tree_replay_levels"] == 0
    dev = torch.from_numpy(np.stack([img, img])).cuda()
    gb.extract_batch_device_async(dev.data_ptr(), H * W, W, 2, keep=dev); gb.sync()
    for i in range(2):
        _check_image(gb, o, angles, i)


# ---- the lane schedule each BASELINE batch shape selects ----
# run_pipeline (jsorb_extract.hip): K = min(4, n / ceil(7 MPx / level-0 pixels)) lanes; lane_order: 0 if K is odd or a lane carries under 24 MPx of
# pyramid, else 1 (tile height <= 40) or 2; lane j runs k_blur first when order == 1 and j is odd, and k_blur_compact when it does not and order != 2.
LANE_SCHEDULES = [
    # config, pairs, lanes, lane order, k_blur_compact lanes, k_blur-first lanes
    ("c2", 128, 4, 1, 0b0101, 0b1010),
    ("c2", 64, 3, 0, 0b111, 0),
    ("c3", 40, 2, 1, 0b01, 0b10),
    ("c5", 24, 3, 0, 0b111, 0),
]


@pytest.mark.parametrize("name,n,K,order,fused,blur_first", LANE_SCHEDULES)
def test_baseline_batch_shapes_pin_their_lane_schedule(orb, configs, monkeypatch, name, n, K, order, fused, blur_first):
    import torch
    for v in ("JSORB_LANE_MIN_MPX", "JSORB_MAX_LANES"):
        monkeypatch.delenv(v, raising=False)
    c = configs[name]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=n)
    assert g.launch_forms()["lanes"] == 0 and g.launch_forms()["lane_order"] == -1
    img = synth_stereo_pair(70, c["h"], c["w"])[0]
    dev = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(img, (n,) + img.shape))).cuda()
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], n, keep=dev); g.sync()
    f = g.launch_forms()
    assert (f["lanes"], f["lane_order"], f["blur_compact_lanes"], f["blur_first_lanes"]) == (K, order, fused, blur_first)
    assert {k: f[k] for k in orb.LANE_KEYS} == _expected_schedule(g, n, K)
    assert g.n_keypoints(n - 1) == g.n_keypoints(0) > 100
