"""The rule by which the exact passes of k_blur and k_pyramid skip a byte store (k_blur_body.h exact_pixel, k_pyramid.hip exact_finish): the fast pass
stored floor(A) and flagged the pixel because floor(256 A) mod 256 is 0 or 255; bit 7 of that fraction byte - the side - travels with the flag, and the
exact lane, which has C, takes the stored byte to be rint(C) - side and stores trunc(C) only where the two differ.  Restated here in numpy
(tests/fixup_fixtures.py) and checked against floor(A) itself on the input families of the two certificate tests; the images of
tests/test_gpu_fixup_stores.py must hold undecided pixels of both kinds for that test to mean something."""
import numpy as np

import fixup_fixtures as fx

F32 = np.float32


def _check(A, C, certified=None):
    """the rule on arrays of fast values A and exact values C; `certified`: False where the kernel never flags (A is the chain itself)
    -> (flagged, changed among flagged)"""
    flagged, side, floor_a, by_rule, floor_c = fx.fraction_rule(A, C)
    if certified is not None:
        assert np.array_equal(A[~certified].view(np.uint32), C[~certified].view(np.uint32))
        flagged = flagged & certified
    assert np.array_equal(by_rule[flagged], floor_a[flagged])          # the fix-up lane knows the stored byte
    assert np.array_equal(floor_a[~flagged], floor_c[~flagged])        # an unflagged pixel needs no fix-up at all
    assert floor_c.min() >= 0 and floor_c.max() <= 255
    return flagged, flagged & (floor_a != floor_c)


def _window_families(rng, n):
    flat = np.arange(256, dtype=np.uint8).reshape(-1, 1, 1).repeat(7, 1).repeat(7, 2)
    return {"random": rng.integers(0, 256, (n, 7, 7), dtype=np.uint8), "flat": flat, "bright": rng.integers(250, 256, (n, 7, 7)).astype(np.uint8),
            "pm1": np.clip(rng.integers(0, 256, (n, 1, 1)) + rng.integers(-1, 2, (n, 7, 7)), 0, 255).astype(np.uint8)}


def test_blur_rule_equals_the_stored_byte_on_every_window_family():
    rng = np.random.default_rng(21)
    for name, P in _window_families(rng, 200000).items():
        for up in (False, True):                                       # even bands walk down, odd bands walk up
            flagged, changed = _check(*fx.blur_windows(P, up))
            if name == "flat":
                assert flagged.all() and int(changed.sum()) == 68      # 68 of the 256 grey levels: the exact byte is one below the fast one
    changed, same = fx.flat_levels()
    assert len(changed) == 68 and len(same) == 188 and 137 in changed


def test_pyramid_rule_equals_the_stored_byte_at_every_level_scale():
    rng = np.random.default_rng(22)
    n = 200000
    scales = []
    s = F32(1)
    for _ in range(7):
        s = F32(s * F32(1.2))
        scales.append(F32(F32(1) / F32(F32(1) / s)))
    scales += [F32(1.5), F32(2.0), F32(3.05)]
    n_flagged = 0
    for s in scales:
        def weights():
            f = (s * rng.integers(0, 2000, n).astype(F32)).astype(F32)
            wl = ((np.floor(f) + F32(1)) - f).astype(F32)
            return wl, (F32(1) - wl).astype(F32)
        wxl, wxr = weights()
        wyt, wyb = weights()
        v = rng.integers(0, 256, n).astype(F32)
        px = lambda lo, hi: [rng.integers(lo, hi, n).astype(F32) for _ in range(4)]
        pm1 = [np.clip(v + rng.integers(-1, 2, n), 0, 255).astype(F32) for _ in range(4)]
        for taps in (px(0, 256), [v, v, v, v], px(250, 256), pm1):
            A, C, cert = fx.pyramid_taps(wxl, wxr, wyt, wyb, *taps)
            flagged, _ = _check(A, C, cert)
            n_flagged += int(flagged.sum())
        if s == F32(2.0):
            assert not cert.any()                                      # every weight pair is (1, 0): nothing to certify, nothing flagged
    assert n_flagged > 10000


def test_gpu_fixtures_hold_undecided_pixels_of_both_kinds():
    """what tests/test_gpu_fixup_stores.py rests on: at least 16 undecided pixels whose byte changes and 16 whose byte does not, for k_blur (on the level-0
    plane alone) and for k_pyramid, and changed pixels in blur bands of both walking directions.  Counted with all bands walking down, flagged /
    changed - blur, level 0: squares 880 / 182, mosaic 40 467 / 20 230, +-1 noise 3 172 / 10, texture 552 / 2; pyramid, levels 1 - 3: squares
    7 049 / 349, mosaic 96 349 / 4 076, +-1 noise 6 975 / 522, texture 3 731 / 163 (4.4 % of the flagged)."""
    imgs = fx.images()
    blur_changed = blur_same = pyr_changed = pyr_same = 0
    per_image = {}
    for name, img in imgs.items():
        chg = np.zeros((fx.H - 40, fx.W - 40), bool)
        flg = np.zeros_like(chg)
        for rb, parity in ((16, 0), (16, 1), (8, 0), (8, 1)):           # batch handles: 16-row bands, single-image handles: 8-row bands
            rows = ((np.arange(fx.H - 40) // rb) & 1) == parity
            A, C = fx.blur_plane(img, up=bool(parity))
            flagged, changed = _check(A, C)
            if rb == 16:
                flg[rows], chg[rows] = flagged[rows], changed[rows]
            if name == "squares":
                assert changed[rows].sum() >= 9, (rb, parity)           # flat cores of the "changed" grey levels in bands walking both ways
        per_image[name] = (int(flg.sum()), int(chg.sum()))
        blur_changed += int(chg.sum()); blur_same += int((flg & ~chg).sum())
        for h, w, s in fx.level_geometry(fx.H, fx.W, fx.LEVELS, 1.2):
            flagged, changed = _check(*fx.pyramid_level(img, h, w, s))
            pyr_changed += int(changed.sum()); pyr_same += int((flagged & ~changed).sum())
    assert min(blur_changed, blur_same, pyr_changed, pyr_same) >= 16, (blur_changed, blur_same, pyr_changed, pyr_same)
    # the mosaic is mostly flat windows (dense exact path), the texture and the squares list a small share of their pixels
    roi = (fx.H - 40) * (fx.W - 40)
    assert per_image["mosaic"][0] > 0.5 * roi and per_image["texture"][0] < 0.05 * roi and per_image["squares"][0] < 0.05 * roi
    assert per_image["mosaic"][1] >= 16 and per_image["squares"][1] >= 16
    # the pyramid of the textured image alone has pixels of both kinds (a share of a few per cent changes)
    ch = sm = 0
    for h, w, s in fx.level_geometry(fx.H, fx.W, fx.LEVELS, 1.2):
        flagged, changed = _check(*fx.pyramid_level(imgs["texture"], h, w, s))
        ch += int(changed.sum()); sm += int((flagged & ~changed).sum())
    assert ch >= 16 and sm >= 16 and ch < 0.2 * (ch + sm), (ch, sm)
    # scale 2.0: A is the chain's value everywhere, nothing is flagged
    for h, w, s in fx.level_geometry(fx.H, fx.W, 3, 2.0):
        A, C, cert = fx.pyramid_level(imgs["texture"], h, w, s)
        assert not cert.any()
        _check(A, C, cert)
