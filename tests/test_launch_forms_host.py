"""The kernel forms a handle selects from its image geometry (jsorb_plan_forms), against an independent restatement of the selection rules.
Host only: jsorb_plan_forms and jsorb_plan_launch touch no device.  tests/test_gpu_geometry_paths.py runs the same geometries on the GPU and checks
through jsorb_handle_forms that a handle runs what is planned here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# ---- the thresholds, restated from the sources they live in ----
REG_T = 4096                 # k_compact.hip compact_form: candidates in registers up to 4096 tiles
CMP_MID_T = 8192             # jsorb_launch.h: batch handles compact with 256-thread workgroups up to here
FLAT_T = 65536               # k_compact_body.h CMP_MAX_CHUNKS * 1024: the flat k_compact (and scan-line buckets) up to here
BLUR_COMPACT_T = 32768       # k_blur.hip blur_compact_fusable: 64 * BLC_MAXCELLS tiles
BUCKET_ROWS = 12288          # jsorb_api.hip build_geometry: L * H0 bucket counters at most
BUCKET_LDS = 40 * 1024       # k_blur.hip blur_compact_fusable: dynamic LDS of the bucket counters next to k_blur's static LDS
NMS_CPU_T = 32768            # jsorb_api.hip: NMS-MS CPU mode
BORDER, BLUR_X_LEAD = 20, 4  # jsorb_device.h JSORB_BORDER, k_blur_body.h


def geometry(H, W, L, tile_h, tile_w, sf=1.2, fixed=False):
    """build_geometry's level sizes and tile grids, in the float32 arithmetic of orb_gpu.cpp"""
    f32 = np.float32
    scale, inv = [f32(1)], [f32(1)]
    for i in range(1, L):
        scale.append(f32(f32(sf) * scale[-1]))
        inv.append(f32(f32(1) / scale[-1]))
    lv = []
    for i in range(L):
        h, w = int(f32(H) * inv[i]), int(f32(W) * inv[i])
        th, tw = (tile_h, tile_w) if fixed or i == 0 else (int(f32(tile_h) * inv[i]), int(f32(tile_w) * inv[i]))
        lv.append(dict(H=h, W=w, th=th, tw=tw, nth=(h - 1) // th + 1, ntw=(w - 1) // tw + 1))
    return lv


def expected_forms(H, W, L, tile, max_batch, detect_lds, sf=1.2):
    lv = geometry(H, W, L, tile, tile, sf)
    T = sum(l["nth"] * l["ntw"] for l in lv)
    latency = max_batch <= 1
    compact = not latency
    buckets = T <= FLAT_T and L * H <= BUCKET_ROWS and W < 32768 and H < 32768
    if T <= REG_T:
        cform = 0 if latency else 1
    elif T <= CMP_MID_T and not latency:
        cform = 2
    elif T <= FLAT_T:
        cform = 3
    else:
        cform = 4
    blur_blocks = any(l["W"] - 2 * BORDER + BLUR_X_LEAD > 0 and l["H"] - 2 * BORDER > 0 for l in lv)
    fusable = blur_blocks and T <= BLUR_COMPACT_T and (L * H * 4 if buckets else 0) <= BUCKET_LDS
    frame_fuse = blur_blocks and not compact and detect_lds + 12 * 1024 <= 64 * 1024
    nms_cpu = T <= NMS_CPU_T and lv[0]["nth"] * lv[0]["ntw"] <= 65535
    return dict(detect_compact=int(compact), compact_form=cform, stereo_buckets=int(buckets), blur_compact_fusable=int(fusable),
                frame_fuses_detect_blur=int(frame_fuse), tree_replay_levels=0, nms_ms_cpu_ok=int(nms_cpu), reserved=0), T


# (H, W, L, tile): the pairs on either side of each threshold (tests/test_gpu_geometry_paths.py runs them on the GPU), the BASELINE shapes, and edges
PAIRS = [
    (1536, 2048, 8, 30), (1537, 2048, 8, 30), (1080, 1920, 12, 30),        # L * H0 vs 12288
    (1200, 1600, 8, 16), (1200, 1600, 8, 17), (720, 1280, 4, 8),           # T vs 65536
    (480, 752, 12, 14), (480, 752, 12, 15),                                # T vs 32768
    (1280, 1024, 8, 40), (1281, 1024, 8, 40), (1280, 1024, 8, 30),         # k_blur_compact's bucket LDS vs 40 KB
    (720, 1280, 4, 30), (480, 752, 4, 20), (480, 752, 8, 20),              # T vs 4096 / 8192
    (1300, 256, 10, 6),                                                    # tile-row scan with one-row tiles on the top levels
    (480, 752, 8, 30), (376, 1241, 8, 25), (720, 1280, 8, 20), (120, 160, 4, 12), (240, 320, 3, 15), (1080, 1920, 8, 30),
]


def _grid():
    rng = np.random.default_rng(77)
    cases = list(PAIRS)
    for _ in range(60):
        cases.append((int(rng.integers(40, 2200)), int(rng.integers(48, 2600)), int(rng.integers(1, 13)), int(rng.choice([6, 8, 12, 16, 20, 25, 30, 40, 58]))))
    return cases


@pytest.mark.parametrize("max_batch", [1, 8])
def test_plan_forms_follow_the_restated_thresholds(max_batch):
    from jetson_slam_amd import orb
    n = 0
    for H, W, L, tile in _grid():
        try:
            plan = orb.plan_launch(H, W, 1.2, L, tile, tile, max_batch=max_batch)
        except orb.JsorbError:
            continue                                             # a level collapses to zero size
        got = orb.plan_forms(H, W, 1.2, L, tile, tile, max_batch=max_batch)
        want, T = expected_forms(H, W, L, tile, max_batch, plan["detect_lds"])
        assert got == want, (H, W, L, tile, max_batch, T)
        n += 1
    assert n >= 60


def test_threshold_pairs_sit_where_the_gpu_tests_expect():
    """The GPU geometry tests name each geometry's arm; these are the tile counts and L * H0 products those names rest on."""
    from jetson_slam_amd import orb

    def T(H, W, L, tile):
        return sum(l["nth"] * l["ntw"] for l in geometry(H, W, L, tile, tile))

    assert (T(1536, 2048, 8, 30), T(1080, 1920, 12, 30)) == (29601, 31635)
    assert (T(1200, 1600, 8, 16), T(1200, 1600, 8, 17), T(720, 1280, 4, 8)) == (67177, 63271, 69240)
    assert (T(480, 752, 12, 14), T(480, 752, 12, 15)) == (32918, 23531)
    assert (T(1280, 1024, 8, 40), T(1280, 1024, 8, 30)) == (6904, 12420)
    assert (T(720, 1280, 4, 30), T(480, 752, 4, 20), T(480, 752, 8, 20)) == (4289, 4018, 8264)
    f = lambda *a, **k: orb.plan_forms(*a, **k)
    assert f(1536, 2048, 1.2, 8, 30, 30)["stereo_buckets"] == 1 and f(1537, 2048, 1.2, 8, 30, 30)["stereo_buckets"] == 0
    assert f(1080, 1920, 1.2, 12, 30, 30)["stereo_buckets"] == 0
    big, small = f(1200, 1600, 1.2, 8, 16, 16, max_batch=4), f(1200, 1600, 1.2, 8, 17, 17, max_batch=4)
    assert (big["compact_form"], big["stereo_buckets"]) == (4, 0) and (small["compact_form"], small["stereo_buckets"]) == (3, 1)
    assert f(480, 752, 1.2, 12, 14, 14)["nms_ms_cpu_ok"] == 0 and f(480, 752, 1.2, 12, 15, 15)["nms_ms_cpu_ok"] == 1
    assert f(1280, 1024, 1.2, 8, 40, 40, max_batch=4)["blur_compact_fusable"] == 1
    assert f(1281, 1024, 1.2, 8, 40, 40, max_batch=4)["blur_compact_fusable"] == 0
    assert [f(*g, max_batch=4)["compact_form"] for g in ((720, 1280, 1.2, 4, 30, 30), (480, 752, 1.2, 4, 20, 20), (480, 752, 1.2, 8, 20, 20))] == [2, 1, 3]
    assert [f(*g)["compact_form"] for g in ((720, 1280, 1.2, 4, 30, 30), (480, 752, 1.2, 4, 20, 20), (480, 752, 1.2, 8, 20, 20))] == [3, 0, 3]
    lv = geometry(1300, 256, 10, 6, 6)
    assert [l["th"] for l in lv[7:]] == [1, 1, 1] and f(1300, 256, 1.2, 10, 6, 6)["stereo_buckets"] == 0


def _tree_winner(score, tw):
    """K3's horizontal reduction on one tile row (jsorb_api.hip tree_winner): ceil-halving rounds, the left slot wins ties"""
    log2 = 0
    while (1 << log2) < tw:
        log2 += 1
    sc, col = list(score), list(range(tw))
    gs = (tw - 1) // 2 + 1
    for _ in range(log2):
        for j in range(gs):
            if j + gs < tw and sc[j] < sc[j + gs]:
                sc[j], col[j] = sc[j + gs], col[j + gs]
        gs = (gs - 1) // 2 + 1
    return col[0]


def test_tree_rank_holds_for_every_tile_width():
    """build_tree_rank succeeds for every tile width the library accepts (1..128), so no level of the shipped build replays the literal
    tree (only the experiments build's JSORB_FORCE_TREE_REPLAY reaches that kernel path)"""
    from jetson_slam_amd import orb
    for tw in range(1, 129):
        f = orb.plan_forms(400, 400, 1.2, 1, 8, tw)
        assert f["tree_replay_levels"] == 0, tw
    f = orb.plan_forms(480, 752, 1.2, 8, 30, 30, fixed_multi_scale_tile_size=True)
    assert f["tree_replay_levels"] == 0


@pytest.mark.parametrize("tw", [2, 3, 5, 6, 7, 8, 9])
def test_arg_max_by_rank_equals_the_literal_tree_on_every_tie_pattern(tw):
    """What the rank form relies on, exhaustively over {0,1,2}^tw: the tree's winner is the arg-max with ties broken by one fixed column
    priority (derived from the pairwise duels, as build_tree_rank does)"""
    import itertools
    beaten = [0] * tw
    for a in range(tw):
        for b in range(a + 1, tw):
            w = _tree_winner([1 if j in (a, b) else 0 for j in range(tw)], tw)
            assert w in (a, b)
            beaten[b if w == a else a] += 1
    assert sorted(beaten) == list(range(tw))                   # a total order
    for sc in itertools.product(range(3), repeat=tw):
        best = max(sc)
        want = 0 if best == 0 else min((c for c in range(tw) if sc[c] == best), key=lambda c: beaten[c])
        assert _tree_winner(sc, tw) == want, sc
