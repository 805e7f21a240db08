"""-m gpu: the exact passes of k_pyramid and k_blur store a byte only where it differs from the one the fast pass stored (k_pyramid.hip exact_finish,
k_blur_body.h exact_pixel).  Images whose undecided pixels are of both kinds - tests/test_fixup_rule_host.py counts them - go through a batch handle
(16-row blur bands, k_blur_compact) and a single-image handle (8-row bands, the fused k_detect_blur), each twice with another image in between on the
same handle: every level plane and every blurred plane bit for bit against the oracle, then keypoints and descriptors.  A skipped store must never
leave a byte of the previous image behind."""
import numpy as np
import pytest

import fixup_fixtures as fx

pytestmark = pytest.mark.gpu

GEO = dict(h=fx.H, w=fx.W, L=fx.LEVELS, tile=16, th=20)


def _handles(orb, po, scale, max_batch):
    c = GEO
    g = orb.ORBExtractor(c["h"], c["w"], scale, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], False, False, True, max_batch=max_batch)
    o = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], scale_factor=scale, tile_h=c["tile"], tile_w=c["tile"], fast_n_min=9, fast_n_max=14,
                           th_fast_max=c["th"], fixed_tile=False, mask=None, apply_nms_ms=False, nms_ms_mode_gpu=True)
    assert g.level_dims() == o.level_dims()
    return g, o


@pytest.fixture(scope="module")
def expected(po):
    """oracle planes, keypoints and descriptors of every image at both scales, computed once"""
    out = {}
    imgs = dict(fx.images(), other=fx.other_image())
    for scale in (1.2, 2.0):
        c = GEO
        o = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], scale_factor=scale, tile_h=c["tile"], tile_w=c["tile"], fast_n_min=9,
                               fast_n_max=14, th_fast_max=c["th"], fixed_tile=False, mask=None, apply_nms_ms=False, nms_ms_mode_gpu=True)
        for name, img in imgs.items():
            o.extract(img)
            out[scale, name] = dict(planes=[o.level_image(lv).copy() for lv in range(c["L"])], blurred=[o.level_blurred(lv).copy() for lv in range(c["L"])],
                                    n=o.n, kp=o.keypoints().copy(), desc=o.descriptors().copy())
    return imgs, out


def _compare(g, want, what, image_idx=0):
    for lv in range(GEO["L"]):
        assert np.array_equal(g.level_image(lv, image_idx), want["planes"][lv]), (what, "level", lv)
        assert np.array_equal(g.level_image(lv, image_idx, blurred=True), want["blurred"][lv]), (what, "blurred", lv)
    assert g.n_keypoints(image_idx) == want["n"], what
    assert np.array_equal(g.keypoints(image_idx), want["kp"]), what
    assert np.array_equal(g.descriptors(image_idx), want["desc"]), what


@pytest.mark.parametrize("scale", [1.2, 2.0])
def test_single_image_handle_stores_exact_bytes_only_where_they_change(orb, po, expected, scale):
    imgs, want = expected
    g, _ = _handles(orb, po, scale, 1)
    names = list(fx.images()) if scale == 1.2 else ["squares", "texture"]      # (scale 2: A is the chain's value everywhere - one pyramid case)
    for name in names:
        for what in (name, "other", name):
            g.extract(imgs[what])
            _compare(g, want[scale, what], (scale, name, what))


@pytest.mark.parametrize("scale", [1.2, 2.0])
def test_batch_handle_stores_exact_bytes_only_where_they_change(orb, po, expected, scale):
    imgs, want = expected
    B = 3
    g, _ = _handles(orb, po, scale, B)
    names = list(fx.images()) if scale == 1.2 else ["squares", "texture"]
    for name in names:
        # the image in slots 0 and 2 with another one between them, then the slots rotated, then the first batch again: every slot sees
        # image, other image, image
        for batch in ((name, "other", name), ("other", name, "other"), (name, "other", name)):
            g.extract_batch_host_async(np.stack([imgs[w] for w in batch])); g.sync()
            for i, what in enumerate(batch):
                _compare(g, want[scale, what], (scale, name, batch, i), i)
