"""The inputs of tests/test_stereo_inputs_host.py (oracle only) and tests/test_gpu_stereo_inputs.py (the device against the oracle): what the
extract + stereo path is given beyond its default thresholds, wide disparity windows and one image family.
  A  matcher parameters   three pairs at GEO_A, every (th_high, th_low) of THRESHOLDS and every (mb, mbf) of CALIBRATIONS, BATCH_STEPS as a batch
  B  speculative match    SPEC_STEPS: the thresholds change between two frames of a speculating pair of handles
  C  image families       every family of synth.INPUT_FAMILIES and the adversarial pair, seeds 1 and 2, at GEO_A
  D  degenerate pyramids  DEGENERATE: levels without a blur / detect ROI, one-row and one-column ROIs, images narrower than a pitch unit,
                          tiles larger than the image, levels of 1x1; REFUSED: geometries whose tile collapses
The oracle's results are computed once per process (ref) and only read afterwards.  A geometry is (height, width, levels, scale, tile)."""
import numpy as np

from jetson_slam_amd.synth import INPUT_FAMILIES, synth_adversarial_pair, synth_family_pair, synth_stereo_pair

MB, MBF = 0.1, 3.0
TH_HIGH, TH_LOW = 100, 50
STAT_KEYS = ("n_candidate_pairs", "n_corr_match", "n_depth", "n_final")
BORDER = 20                                           # no score, no blur within 20 px of a level's edge: a level needs H > 40 and W > 40 to have a ROI

# ---- A ----
GEO_A, FAST_A = (240, 320, 4, 1.2, 16), 20
SWEEP_PAIRS = ("synthetic", "adversarial", "noise")
THRESHOLDS = [(100, 50), (100, 100), (60, 20), (256, 256), (257, 257), (1, 1), (0, 0), (101, 50), (50, 100), (30, 90)]
CALIBRATIONS = [(0.1, 3.0), (0.15, 3.0), (0.5, 3.0), (1.0, 6.0), (1.0, 7.0), (1.0, 29.5), (4.0, 2.0), (1.0, 1.0), (3.0, 0.75), (0.01, 10.0), (1e-4, 100.0)]
BATCH_STEPS = [((60, 20), (1.0, 6.0)), ((256, 256), (0.1, 100.0))]          # maxD 6 and maxD 1000


def max_d(cal):
    """maxD = mbf / mb in f32, as the matcher computes it"""
    return np.float32(cal[1]) / np.float32(cal[0])


def sweep_params():
    """every (thresholds, calibration) of part A, the default pair once"""
    return [(t, (MB, MBF)) for t in THRESHOLDS] + [((TH_HIGH, TH_LOW), c) for c in CALIBRATIONS[1:]]


def sweep_pair(name):
    h, w = GEO_A[:2]
    return {"synthetic": lambda: synth_stereo_pair(1, h, w), "adversarial": lambda: synth_adversarial_pair(1, h, w),
            "noise": lambda: synth_family_pair("noise", 3, h, w)}[name]()


# ---- B ----
SPEC_SEEDS = (1, 2, 3, 4)
# (pair, thresholds, what the match must do): the first match arms the pair, a match whose thresholds are those of the frame before is the one
# already enqueued, one whose thresholds differ is not
SPEC_STEPS = [(0, (100, 50), "arm"), (1, (100, 50), "adopt"),
              (2, (60, 20), "drop"), (3, (60, 20), "adopt"),                # both thresholds change
              (0, (60, 50), "drop"), (1, (60, 50), "adopt"),                # th_low only
              (2, (100, 50), "drop"), (3, (100, 50), "adopt")]              # th_high only


def spec_pair(i):
    return synth_stereo_pair(SPEC_SEEDS[i], GEO_A[0], GEO_A[1])


# ---- C ----
FAMILY_PAIRS = [(k, s) for k in INPUT_FAMILIES + ("adversarial",) for s in (1, 2)]


def family_pair(kind, seed):
    h, w = GEO_A[:2]
    return synth_adversarial_pair(seed, h, w) if kind == "adversarial" else synth_family_pair(kind, seed, h, w)


# ---- D ----
FAST_D = 15
DEGENERATE = [
    (100, 140, 6, 1.5, 12),      # levels 3-5 (29x41, 19x27, 13x18) have no ROI
    (96, 109, 6, 1.5, 10),       # the smallest level of test_random_parameter_fuzz's default cases (12x14)
    (50, 200, 4, 1.2, 8),        # level 1 is 41 px high: a one-row ROI; levels 2-3 have none
    (200, 50, 4, 1.2, 8),        # level 1 is 41 px wide: a one-column ROI; levels 2-3 have none
    (45, 300, 1, 1.2, 3),        # a 5-row ROI, tile 3, T = 1500
    (42, 63, 1, 1.2, 6),         # narrower than one 64-byte pitch unit
    (48, 50, 2, 1.2, 5),         # level 1 is 40x41: no ROI
    (59, 65, 5, 1.25, 9),        # levels 2-4 have no ROI
    (61, 61, 3, 1.5, 7),         # levels 1-2 have no ROI
    (64, 90, 8, 1.8, 100),       # tile larger than the image, T = 8, levels down to 1x2 and 1x1
    (41, 41, 1, 1.2, 8),         # a single interior pixel
    (5, 9, 1, 1.2, 4),           # smaller than the border
    (1, 1, 1, 1.2, 1),
]
REFUSED = [(48, 70, 8, 1.5, 12), (64, 64, 6, 2.0, 16), (60, 66, 4, 3.0, 10)]          # the tile of a level collapses to zero
ONE_ROW_ROI, ONE_COLUMN_ROI = (50, 200, 4, 1.2, 8), (200, 50, 4, 1.2, 8)
DEGENERATE_BATCH = 5


def degenerate_pairs(geo):
    h, w = geo[:2]
    return [synth_stereo_pair(3, h, w), synth_family_pair("noise", 3, h, w)]


# Device batches whose images end inside a dword (H * W is no multiple of 4) and whose last level-1 pixel takes its bottom right tap from the last
# bytes of the image: k_pyramid reads level 0 in place through a bounds-checked descriptor, which has to reach to the end of that dword
# (the batch of (59, 65, 5, 1.25, 9) above found level 1, row 46, columns 49-51 wrong)
UNALIGNED_ENDS = [(59, 65, 2, 1.25, 9), (59, 66, 2, 1.25, 9), (59, 69, 2, 1.25, 9), (58, 65, 2, 1.25, 9), (59, 129, 2, 1.25, 9)]


def last_tap(n0, scale):
    """(tap, weight of the next tap) of the last pixel of level 1 along an axis of n0 level-0 pixels, in the resampler's f32 arithmetic"""
    inv = np.float32(1.0) / np.float32(scale)
    s = np.float32(1.0) / inv
    f = s * np.float32(int(np.float32(n0) * inv) - 1)
    return int(np.floor(f)), float(f - np.floor(f))


LANE_RULES = {"default": None, "lane_min_mpx_0.01": "0.01"}     # JSORB_LANE_MIN_MPX when the handle is created


def expected_lanes(geo, n, min_mpx):
    """plan_lanes (jsorb_extract.hip) restated: a lane takes at least min_mpx (default 7) MPx of level-0 pixels, four lanes at most"""
    per_lane = max(1, int(np.ceil(float(min_mpx or 7.0) * 1e6 / (geo[0] * geo[1]))))
    return max(1, min(4, n // per_lane))


def geo_id(geo):
    return "%dx%d-L%d-%g-t%d" % geo


# ---- the two sides ----
def oracle(po, geo, fast_th):
    h, w, L, scale, tile = geo
    return po.OracleExtractor(height=h, width=w, n_levels=L, scale_factor=scale, tile_h=tile, tile_w=tile, th_fast_max=fast_th)


def product(orb, geo, fast_th, max_batch=1):
    h, w, L, scale, tile = geo
    return orb.ORBExtractor(h, w, scale, L, 9, 14, 7, fast_th, None, tile, tile, max_batch=max_batch)


class Ref:
    """the oracle's extract of one stereo pair and its matches, one per (thresholds, calibration)"""

    def __init__(self, po, geo, fast_th, left, right):
        self.po, self.geo, self.left, self.right = po, geo, left, right
        self.o = [oracle(po, geo, fast_th), oracle(po, geo, fast_th)]
        self.o[0].extract(left); self.o[1].extract(right)
        L = geo[2]
        self.angles = [np.concatenate([o.level_keypoints(i)[3] for i in range(L)]) for o in self.o]
        self.level_n = [[o.l.orc_level_n_keypoints(o.h, i) for i in range(L)] for o in self.o]
        self.planes = [[(o.level_image(i), o.level_blurred(i)) for i in range(L)] for o in self.o]
        self.kp = [o.keypoints() for o in self.o]
        self.desc = [o.descriptors() for o in self.o]
        self.tiles = [o.tiles() for o in self.o]
        self._matches = {}

    def match(self, th=(TH_HIGH, TH_LOW), cal=(MB, MBF)):
        """(uRight, depth, statistics with best_right, best_dist and l1) of the oracle"""
        key = (tuple(th), tuple(cal))
        if key not in self._matches:
            self._matches[key] = self.po.stereo_match(self.o[0], self.o[1], cal[0], cal[1], th[0], th[1])
        return self._matches[key]


_REFS = {}


def ref(po, geo, fast_th, name, make):
    """the Ref of the pair `name` (make() -> (left, right)) at a geometry, built on first use"""
    key = (geo, fast_th, name)
    if key not in _REFS:
        _REFS[key] = Ref(po, geo, fast_th, *make())
    return _REFS[key]


def sweep_ref(po, name):
    return ref(po, GEO_A, FAST_A, ("sweep", name), lambda: sweep_pair(name))


def spec_ref(po, i):
    return ref(po, GEO_A, FAST_A, ("spec", i), lambda: spec_pair(i))


def family_ref(po, kind, seed):
    return ref(po, GEO_A, FAST_A, ("family", kind, seed), lambda: family_pair(kind, seed))


def degenerate_refs(po, geo):
    pairs = degenerate_pairs(geo)
    return [ref(po, geo, FAST_D, ("degenerate", k), lambda k=k: pairs[k]) for k in range(2)]


# ---- comparisons, bit for bit ----
def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_image(g, r, side, image=0, planes=False):
    """handle g holds what the oracle found in image `side` (0 left, 1 right) of the pair r"""
    L = r.geo[2]
    if planes:
        for lv in range(L):
            assert np.array_equal(g.level_image(lv, image), r.planes[side][lv][0]), lv
            assert np.array_equal(g.level_image(lv, image, blurred=True), r.planes[side][lv][1]), lv
    for a, b in zip(g.tile_candidates(image), r.tiles[side]):
        assert np.array_equal(a, b)
    assert g.n_keypoints(image) == r.kp[side].size // 6
    assert g.level_n_keypoints(image) == r.level_n[side]
    assert np.array_equal(g.keypoints(image), r.kp[side])
    assert np.array_equal(g.descriptors(image), r.desc[side])
    assert same_bits(g.angles(image), r.angles[side])


def check_match(orb, gl, got, want, th_high=TH_HIGH, image=0, diagnostics=False):
    """got = (uRight, depth, statistics) of the device for image `image` of the left handle gl, want = Ref.match(...)"""
    u, d, st = got
    ou, od, ost = want
    assert same_bits(u, ou) and same_bits(d, od)
    assert [st[k] for k in STAT_KEYS] == [ost[k] for k in STAT_KEYS]
    l1 = orb.stereo_l1(gl, image)
    assert l1.dtype == ost["l1"].dtype and np.array_equal(l1, ost["l1"])
    if diagnostics:
        best_right, best_dist, _ = orb.stereo_diagnostics(gl, image)
        assert np.array_equal(best_right, ost["best_right"])
        assert np.array_equal(best_dist, ost["best_dist"])
        assert np.all(best_dist[best_right < 0] == th_high)             # the no-match sentinel is the parameter itself
