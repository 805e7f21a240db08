"""The case lists of tests/stereo_input_cases.py are not vacuous: from the oracle alone, every list makes the matcher and the extractor do
what tests/test_gpu_stereo_inputs.py wants to see them do on the device - thresholds that change which keypoints match, disparity windows
under, at and far above the true disparities, image families whose keypoint counts lie a factor of 20 apart, and pyramids whose upper
levels have no ROI, a one-row or a one-column ROI.  Every figure is computed here; none is copied from the device."""
import numpy as np
import pytest

import stereo_input_cases as sc


# ---- A: matcher parameters ----
@pytest.mark.parametrize("name", sc.SWEEP_PAIRS)
def test_thresholds_change_what_matches(po, name):
    r = sc.sweep_ref(po, name)
    st = {t: r.match(th=t)[2] for t in sc.THRESHOLDS}
    assert st[(0, 0)]["n_corr_match"] == 0 and st[(0, 0)]["n_candidate_pairs"] > 0          # nothing is closer than 0; the candidates are still counted
    assert len({s["n_candidate_pairs"] for s in st.values()}) == 1                         # the thresholds play no part in the window tests
    assert len({s["n_corr_match"] for s in st.values()}) >= 5
    assert st[(256, 256)]["n_corr_match"] == st[(257, 257)]["n_corr_match"] > st[(100, 100)]["n_corr_match"] > st[(100, 50)]["n_corr_match"] > 0
    for t, s in st.items():                                                                # the sentinel follows th_high
        assert np.all(s["best_dist"][s["best_right"] < 0] == t[0]) and np.all(s["best_dist"][s["best_right"] >= 0] < max(t[0], 1))
    # th_orb = (th_high + th_low) / 2 and th_high are two tests: (50, 100) and (100, 50) share th_orb = 75, (101, 50) rounds down to 75
    assert st[(50, 100)]["n_corr_match"] < st[(100, 50)]["n_corr_match"] == st[(101, 50)]["n_corr_match"]
    assert not np.array_equal(st[(101, 50)]["best_dist"], st[(100, 50)]["best_dist"])


def test_thresholds_of_one_match_only_identical_descriptors(po):
    u, d, st = sc.sweep_ref(po, "adversarial").match(th=(1, 1))
    hit = st["best_right"] >= 0
    assert st["n_corr_match"] > 0 and st["n_depth"] > 0
    assert hit.sum() >= st["n_corr_match"] and np.all(st["best_dist"][hit] == 0)


@pytest.mark.parametrize("name", sc.SWEEP_PAIRS)
def test_windows_below_one_pixel_leave_candidates_and_no_depth(po, name):
    r = sc.sweep_ref(po, name)
    for cal in ((4.0, 2.0), (3.0, 0.75)):
        assert sc.max_d(cal) in (0.5, 0.25)
        st = r.match(cal=cal)[2]
        assert st["n_candidate_pairs"] > 0 and st["n_final"] == 0


def test_window_under_the_true_disparities(po):
    """synth_stereo_pair shifts every row by 6 to 29 px: a window of 6 px keeps candidates and next to no depth"""
    r = sc.sweep_ref(po, "synthetic")
    st, st0 = r.match(cal=(1.0, 6.0))[2], r.match()[2]
    assert sc.max_d((1.0, 6.0)) == 6 and sc.max_d((0.5, 3.0)) == 6
    assert st["n_candidate_pairs"] > 0 and 0 < st["n_final"] * 10 < st0["n_final"]
    for k in sc.STAT_KEYS:                                                 # the same window from another calibration: the same matches, other depths
        assert r.match(cal=(0.5, 3.0))[2][k] == st[k]
    assert st["n_candidate_pairs"] < r.match(cal=(1.0, 7.0))[2]["n_candidate_pairs"] < r.match(cal=(1.0, 29.5))[2]["n_candidate_pairs"]


def test_non_integer_window_edge(po):
    """maxD = 29.5 against the default's 30 on the noise pair: candidates at a disparity of exactly 30 px pass `uR >= uL - maxD` at 30 only, and a
    refined disparity between 29.5 and 30 passes `disparity < maxD` at 30 only"""
    assert sc.max_d((1.0, 29.5)) == 29.5 and sc.max_d((sc.MB, sc.MBF)) == 30
    r = sc.sweep_ref(po, "noise")
    (u, _, st), (u0, _, st0) = r.match(cal=(1.0, 29.5)), r.match()
    assert 0 < st["n_candidate_pairs"] < st0["n_candidate_pairs"]
    assert st["n_corr_match"] == st0["n_corr_match"] and 0 < st["n_depth"] < st0["n_depth"]
    x = r.kp[0].reshape(6, -1)[0].astype(np.float32)
    assert np.all((x - u)[u >= 0] < 29.5) and 29.5 <= np.max((x - u0)[u0 >= 0]) < 30


def test_wide_window_widens_the_search_on_noise(po):
    r = sc.sweep_ref(po, "noise")
    assert abs(sc.max_d((0.01, 10.0)) - 1000) < 1e-3 and abs(sc.max_d((0.1, 100.0)) - 1000) < 1e-3 and sc.max_d((1e-4, 100.0)) > 9e5
    wide, default = r.match(cal=(0.01, 10.0)), r.match()
    assert wide[2]["n_candidate_pairs"] > 2 * default[2]["n_candidate_pairs"]
    x = r.kp[0].reshape(6, -1)[0].astype(np.float32)
    assert np.max((x - wide[0])[wide[0] >= 0]) > 100                        # disparities the default window of 30 px never admits
    assert r.match(cal=(1e-4, 100.0))[2]["n_candidate_pairs"] == wide[2]["n_candidate_pairs"]      # both windows are wider than the image


def test_zero_disparity_branch_survives_every_window_of_six_pixels_or_more(po):
    """the `disparity <= 0 -> 0.01` branch: uRight = (float)((double)uL - 0.01), depth = mbf / 0.01f"""
    r = sc.sweep_ref(po, "adversarial")
    x = r.kp[0].reshape(6, -1)[0]
    want_u = (x.astype(np.float64) - 0.01).astype(np.float32)
    for cal in sc.CALIBRATIONS:
        if sc.max_d(cal) < 6:
            continue
        u, d, _ = r.match(cal=cal)
        hit = (u >= 0) & (u == want_u)
        assert hit.sum() > 0, cal
        assert np.array_equal(d[hit].view(np.uint32), np.full(hit.sum(), np.float32(cal[1]) / np.float32(0.01), np.float32).view(np.uint32)), cal


def test_batch_steps_differ_from_the_defaults_on_every_pair(po):
    for name in sc.SWEEP_PAIRS:
        r = sc.sweep_ref(po, name)
        seen = [r.match()[2]["n_corr_match"]] + [r.match(th=t, cal=c)[2]["n_corr_match"] for t, c in sc.BATCH_STEPS]
        assert len(set(seen)) == 3 and min(seen) > 0, (name, seen)


# ---- B: a change of thresholds between two frames ----
def test_speculative_steps_change_the_result_of_the_frame_they_meet(po):
    """a match adopted with the thresholds of the frame before would not be this frame's match: on every `drop` frame of SPEC_STEPS the oracle's
    result with the old thresholds differs from its result with the new ones"""
    assert [s[2] for s in sc.SPEC_STEPS].count("drop") == 3
    for (_, before, _), (i, now, what) in zip(sc.SPEC_STEPS, sc.SPEC_STEPS[1:]):
        assert (what == "drop") == (before != now)
        if what == "drop":
            r = sc.spec_ref(po, i)
            old, new = r.match(th=before), r.match(th=now)
            assert not sc.same_bits(old[0], new[0]) and old[2]["n_final"] != new[2]["n_final"]
            assert new[2]["n_final"] > 20
    lows = [(b, n) for (_, b, _), (_, n, _) in zip(sc.SPEC_STEPS, sc.SPEC_STEPS[1:]) if b[0] == n[0] and b[1] != n[1]]
    highs = [(b, n) for (_, b, _), (_, n, _) in zip(sc.SPEC_STEPS, sc.SPEC_STEPS[1:]) if b[0] != n[0] and b[1] == n[1]]
    assert lows and highs


# ---- C: image families ----
def test_families_span_sparse_to_dense_and_all_reach_the_matcher(po):
    n_kp = {}
    for kind, seed in sc.FAMILY_PAIRS:
        r = sc.family_ref(po, kind, seed)
        st = r.match()[2]
        assert st["n_final"] >= 20, (kind, seed, st["n_final"])
        n_kp[kind, seed] = [k.size // 6 for k in r.kp]
    assert len(n_kp) == 10
    counts = [n for v in n_kp.values() for n in v]
    assert max(counts) >= 20 * min(counts) and min(counts) > 0
    assert max(counts) * 2 > sc.family_ref(po, "noise", 1).o[0].T              # the dense families fill most tiles


# ---- D: degenerate pyramids ----
def _has_roi(hw):
    return hw[0] > 2 * sc.BORDER and hw[1] > 2 * sc.BORDER


@pytest.mark.parametrize("geo", sc.DEGENERATE, ids=sc.geo_id)
def test_degenerate_geometries_are_legal_and_keypoints_lie_on_levels_with_a_roi(po, geo):
    for r in sc.degenerate_refs(po, geo):
        dims = r.o[0].level_dims()
        for side in (0, 1):
            for lv, n in enumerate(r.level_n[side]):
                assert n == 0 or _has_roi(dims[lv])
                if not _has_roi(dims[lv]):
                    assert not r.planes[side][lv][1].any()                   # a level without a ROI has no blurred pixel either
        r.match()


def test_census_of_the_degenerate_geometries(po):
    census = {geo: [r.level_n[0] for r in sc.degenerate_refs(po, geo)] for geo in sc.DEGENERATE}
    dims = {geo: sc.oracle(po, geo, sc.FAST_D).level_dims() for geo in sc.DEGENERATE}
    # a ROI of one row / one column holds keypoints (the noise pair)
    assert dims[sc.ONE_ROW_ROI][1][0] == 2 * sc.BORDER + 1 and census[sc.ONE_ROW_ROI][1][1] > 0
    assert dims[sc.ONE_COLUMN_ROI][1][1] == 2 * sc.BORDER + 1 and census[sc.ONE_COLUMN_ROI][1][1] > 0
    # an occupied level followed by levels that are all empty because they have no ROI
    tailed = [geo for geo in sc.DEGENERATE
              if any(n[lv] > 0 and lv + 1 < geo[2] and not any(_has_roi(d) for d in dims[geo][lv + 1:]) for n in census[geo] for lv in range(geo[2]))]
    assert len(tailed) >= 3
    # both images of some geometry with ROI-less levels still give the matcher work
    assert all(r.match()[2]["n_final"] > 10 for r in sc.degenerate_refs(po, (100, 140, 6, 1.5, 12)))
    # the shapes the table names
    assert dims[(64, 90, 8, 1.8, 100)][-1] == (1, 1) and sc.oracle(po, (64, 90, 8, 1.8, 100), sc.FAST_D).T == 8
    assert dims[(48, 50, 2, 1.2, 5)][1] == (40, 41)
    assert sc.oracle(po, (45, 300, 1, 1.2, 3), sc.FAST_D).T == 1500
    assert min(geo[1] for geo in sc.DEGENERATE if geo[1] > 2 * sc.BORDER) < 64          # narrower than one pitch unit, with a ROI
    for geo in ((41, 41, 1, 1.2, 8), (5, 9, 1, 1.2, 4), (1, 1, 1, 1.2, 1)):
        assert all(sum(n) == 0 for n in census[geo])
    # the batches of five run on one lane by default; with a lane per 0.01 MPx the larger geometries spread over four lanes, the smaller keep one
    lanes = [sc.expected_lanes(geo, sc.DEGENERATE_BATCH, sc.LANE_RULES["lane_min_mpx_0.01"]) for geo in sc.DEGENERATE]
    assert lanes.count(4) >= 5 and lanes.count(1) >= 5 and 2 in lanes
    assert all(sc.expected_lanes(geo, sc.DEGENERATE_BATCH, sc.LANE_RULES["default"]) == 1 for geo in sc.DEGENERATE)
    # level 0 of a device batch is read in place: rows that start on a dword (width a multiple of 4) and rows that do not both occur
    assert {geo[1] % 4 == 0 for geo in sc.DEGENERATE} == {True, False}


def test_unaligned_ends_sample_the_last_byte_of_an_image_that_ends_inside_a_dword():
    assert (59, 65, 5, 1.25, 9) in sc.DEGENERATE
    for h, w, _, scale, _ in sc.UNALIGNED_ENDS + [(59, 65, 5, 1.25, 9)]:
        (y, wy), (x, wx) = sc.last_tap(h, scale), sc.last_tap(w, scale)
        assert y + 1 == h - 1 and wy > 0 and wx > 0                             # the bottom right tap lies in the image's last row, with weight wy * wx
        tap = (h - 1) * w + x + 1
        # image i of a dense batch starts p bytes behind a dword; the tap lies in the dword that holds the image's last byte, and that dword is not full
        cut = [((h * w + p) // 4) * 4 - p for p in ((i * h * w) % 4 for i in range(sc.DEGENERATE_BATCH)) if (h * w + p) % 4]
        assert cut and any(tap >= c for c in cut)


@pytest.mark.parametrize("geo", sc.REFUSED, ids=sc.geo_id)
def test_collapsed_tiles_are_refused(po, geo):
    with pytest.raises(ValueError):
        sc.oracle(po, geo, sc.FAST_D)
    h, w, L, scale, tile = geo
    s = np.float32(1.0)
    sizes = []
    for _ in range(1, L):
        s = np.float32(scale) * s
        sizes.append(int(np.float32(tile) * (np.float32(1.0) / s)))
    assert min(sizes) == 0                                                  # the reason: a level's tile is 0 px
