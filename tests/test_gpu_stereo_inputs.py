"""-m gpu: the extract + stereo path on the inputs of tests/stereo_input_cases.py, bit for bit against the CPU oracle: tile candidates of every
level, keypoints, descriptors, angles, keypoints per level, uRight and depth, the matcher's four statistics, its L1 distances and, with the
diagnostics on, the arg-min of its candidate search.
  A  the matcher's thresholds and its disparity window are parameters on the device as well: three extracted pairs matched with every
     (th_high, th_low) and every (mb, mbf) of the lists, single frames and a batch
  B  a speculative match enqueued with the thresholds of the frame before is not adopted by a match that names others
  C  every image family of synth.INPUT_FAMILIES and the adversarial pair through the whole path, single frames and a batch on four lanes
  D  pyramids whose levels have no ROI, a one-row or a one-column ROI, images narrower than a pitch unit or smaller than the border, tiles
     larger than the image: single frames with every plane compared, and batches under both lane rules
tests/test_stereo_inputs_host.py shows from the oracle alone that these inputs make the matcher and the extractor take the paths named."""
import numpy as np
import pytest

import stereo_input_cases as sc

pytestmark = pytest.mark.gpu


def _device_batch(orb, gl, gr, lefts, rights):
    """extract the images as one device-resident batch on each handle"""
    import torch
    h, w = lefts[0].shape
    n = len(lefts)
    dl = torch.from_numpy(np.stack(lefts)).cuda()
    dr = torch.from_numpy(np.stack(rights)).cuda()
    gl.extract_batch_device_async(dl.data_ptr(), h * w, w, n, keep=dl)
    gr.extract_batch_device_async(dr.data_ptr(), h * w, w, n, keep=dr)


# ---- A: matcher parameters ----
@pytest.mark.parametrize("name", sc.SWEEP_PAIRS)
def test_matcher_follows_its_thresholds_and_window(orb, po, name):
    r = sc.sweep_ref(po, name)
    gl, gr = sc.product(orb, sc.GEO_A, sc.FAST_A, max_batch=3), sc.product(orb, sc.GEO_A, sc.FAST_A, max_batch=3)
    orb.set_stereo_diagnostics(gl, True)
    gl.extract(r.left); gr.extract(r.right)
    sc.check_image(gl, r, 0); sc.check_image(gr, r, 1)
    for th, cal in sc.sweep_params():
        got = orb.compute_stereo_matches(gl, gr, cal[0], cal[1], th[0], th[1])
        assert got[2]["n_left"] == r.kp[0].size // 6 and got[2]["n_right"] == r.kp[1].size // 6
        sc.check_match(orb, gl, got, r.match(th, cal), th_high=th[0], diagnostics=True)


def test_matcher_parameters_reach_every_image_of_a_batch(orb, po):
    refs = [sc.sweep_ref(po, name) for name in sc.SWEEP_PAIRS]
    gl, gr = sc.product(orb, sc.GEO_A, sc.FAST_A, max_batch=3), sc.product(orb, sc.GEO_A, sc.FAST_A, max_batch=3)
    orb.set_stereo_diagnostics(gl, True)
    for th, cal in sc.BATCH_STEPS:
        r = refs[-1]                                           # the handles of the single-frame sweep serve the batch: a frame with other parameters first
        gl.extract(r.left); gr.extract(r.right)
        sc.check_match(orb, gl, orb.compute_stereo_matches(gl, gr, sc.MB, sc.MBF), r.match(), diagnostics=True)
        _device_batch(orb, gl, gr, [r.left for r in refs], [r.right for r in refs])
        orb.stereo_match_batch_async(gl, gr, cal[0], cal[1], th[0], th[1])
        gl.sync(); gr.sync()
        for i, r in enumerate(refs):
            sc.check_image(gl, r, 0, i); sc.check_image(gr, r, 1, i)
            sc.check_match(orb, gl, orb.stereo_result(gl, i), r.match(th, cal), th_high=th[0], image=i, diagnostics=True)


# ---- B: the speculative match and the thresholds ----
def test_speculative_match_is_not_adopted_across_a_change_of_thresholds(orb, po):
    refs = [sc.spec_ref(po, i) for i in range(len(sc.SPEC_SEEDS))]
    gl, gr = sc.product(orb, sc.GEO_A, sc.FAST_A), sc.product(orb, sc.GEO_A, sc.FAST_A)
    orb.set_speculative_stereo(gl, True); orb.set_speculative_stereo(gr, True)
    adopted = dropped = 0
    for i, th, what in sc.SPEC_STEPS:
        r = refs[i]
        gl.extract(r.left); gr.extract(r.right)
        got = orb.compute_stereo_matches(gl, gr, sc.MB, sc.MBF, th[0], th[1])
        sc.check_image(gl, r, 0); sc.check_image(gr, r, 1)
        sc.check_match(orb, gl, got, r.match(th), th_high=th[0])
        adopted += what == "adopt"
        dropped += what == "drop"
        assert orb.speculative_stereo_stats(gl) == (adopted, dropped), (i, th, what)
    assert adopted == 4 and dropped == 3


# ---- C: image families ----
def test_image_families_single_frames(orb, po, layout):
    gl, gr = sc.product(orb, sc.GEO_A, sc.FAST_A), sc.product(orb, sc.GEO_A, sc.FAST_A)
    orb.set_stereo_diagnostics(gl, True)
    for kind, seed in sc.FAMILY_PAIRS:
        r = sc.family_ref(po, kind, seed)
        gl.extract(r.left); gr.extract(r.right)
        sc.check_image(gl, r, 0); sc.check_image(gr, r, 1)
        sc.check_match(orb, gl, orb.compute_stereo_matches(gl, gr, sc.MB, sc.MBF), r.match(), diagnostics=True)


def test_image_families_as_one_batch_on_four_lanes(orb, po, monkeypatch):
    refs = [sc.family_ref(po, kind, seed) for kind, seed in sc.FAMILY_PAIRS]
    n = len(refs)
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.01")            # read at handle creation: a lane takes as little as one image
    gl, gr = sc.product(orb, sc.GEO_A, sc.FAST_A, max_batch=n), sc.product(orb, sc.GEO_A, sc.FAST_A, max_batch=n)
    monkeypatch.delenv("JSORB_LANE_MIN_MPX")
    orb.set_stereo_diagnostics(gl, True)
    _device_batch(orb, gl, gr, [r.left for r in refs], [r.right for r in refs])
    orb.stereo_match_batch_async(gl, gr, sc.MB, sc.MBF)
    gl.sync(); gr.sync()
    assert gl.launch_forms()["lanes"] == 4 and gr.launch_forms()["lanes"] == 4
    for i, r in enumerate(refs):
        sc.check_image(gl, r, 0, i); sc.check_image(gr, r, 1, i)
        sc.check_match(orb, gl, orb.stereo_result(gl, i), r.match(), image=i, diagnostics=True)


# ---- D: degenerate pyramids ----
@pytest.mark.parametrize("geo", sc.DEGENERATE, ids=sc.geo_id)
def test_degenerate_geometry_single_frames(orb, po, geo, layout):
    gl, gr = sc.product(orb, geo, sc.FAST_D), sc.product(orb, geo, sc.FAST_D)
    assert gl.level_dims() == sc.oracle(po, geo, sc.FAST_D).level_dims()
    assert gl.T == sc.oracle(po, geo, sc.FAST_D).T
    orb.set_stereo_diagnostics(gl, True)
    for r in sc.degenerate_refs(po, geo):
        gl.extract(r.left); gr.extract(r.right)
        sc.check_image(gl, r, 0, planes=True); sc.check_image(gr, r, 1, planes=True)
        sc.check_match(orb, gl, orb.compute_stereo_matches(gl, gr, sc.MB, sc.MBF), r.match(), diagnostics=True)


@pytest.mark.parametrize("lane_rule", sorted(sc.LANE_RULES))
@pytest.mark.parametrize("geo", sc.DEGENERATE, ids=sc.geo_id)
def test_degenerate_geometry_as_a_batch(orb, po, monkeypatch, geo, lane_rule):
    refs = sc.degenerate_refs(po, geo)
    n = sc.DEGENERATE_BATCH
    order = [i % 2 for i in range(n)]                          # the two pairs alternate: no image may keep what its neighbour found
    min_mpx = sc.LANE_RULES[lane_rule]
    monkeypatch.delenv("JSORB_MAX_LANES", raising=False)
    if min_mpx is None:
        monkeypatch.delenv("JSORB_LANE_MIN_MPX", raising=False)
    else:
        monkeypatch.setenv("JSORB_LANE_MIN_MPX", min_mpx)
    gl, gr = sc.product(orb, geo, sc.FAST_D, max_batch=n), sc.product(orb, geo, sc.FAST_D, max_batch=n)
    monkeypatch.delenv("JSORB_LANE_MIN_MPX", raising=False)
    assert gl.level_dims() == refs[0].o[0].level_dims()
    orb.set_stereo_diagnostics(gl, True)
    _device_batch(orb, gl, gr, [refs[k].left for k in order], [refs[k].right for k in order])
    orb.stereo_match_batch_async(gl, gr, sc.MB, sc.MBF)
    gl.sync(); gr.sync()
    assert gl.launch_forms()["lanes"] == gr.launch_forms()["lanes"] == sc.expected_lanes(geo, n, min_mpx)
    for i, k in enumerate(order):
        sc.check_image(gl, refs[k], 0, i, planes=True); sc.check_image(gr, refs[k], 1, i, planes=True)
        sc.check_match(orb, gl, orb.stereo_result(gl, i), refs[k].match(), image=i, diagnostics=True)


@pytest.mark.parametrize("geo", sc.UNALIGNED_ENDS, ids=sc.geo_id)
def test_device_batch_of_images_that_end_inside_a_dword(orb, po, geo):
    """k_pyramid reads level 0 of a device batch in place; the last pixel of level 1 takes its bottom right tap from the image's last byte"""
    refs = sc.degenerate_refs(po, geo)
    n = sc.DEGENERATE_BATCH
    gl, gr = sc.product(orb, geo, sc.FAST_D, max_batch=n), sc.product(orb, geo, sc.FAST_D, max_batch=n)
    _device_batch(orb, gl, gr, [refs[i % 2].left for i in range(n)], [refs[i % 2].right for i in range(n)])
    orb.stereo_match_batch_async(gl, gr, sc.MB, sc.MBF)
    gl.sync(); gr.sync()
    for i in range(n):
        sc.check_image(gl, refs[i % 2], 0, i, planes=True); sc.check_image(gr, refs[i % 2], 1, i, planes=True)
        sc.check_match(orb, gl, orb.stereo_result(gl, i), refs[i % 2].match(), image=i)


def test_only_collapsed_tiles_are_refused(orb):
    for geo in sc.REFUSED:
        with pytest.raises(orb.JsorbError) as ei:
            sc.product(orb, geo, sc.FAST_D)
        assert "tile size collapses to zero" in str(ei.value)
        with pytest.raises(orb.JsorbError):
            sc.product(orb, geo, sc.FAST_D, max_batch=sc.DEGENERATE_BATCH)
    for geo in sc.DEGENERATE:
        sc.product(orb, geo, sc.FAST_D).close()
        sc.product(orb, geo, sc.FAST_D, max_batch=sc.DEGENERATE_BATCH).close()
