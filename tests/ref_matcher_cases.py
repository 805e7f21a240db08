"""What tools/ref_matcher_goldens.py and tests/test_ref_matcher.py / tests/test_gpu_ref_matcher.py share: per matcher entry point the cases of
tests/golden/ref_matcher_<name>.npz (the random generators and constructed cases of the host tests, imported, with what the reference cannot be
given changed in the input - see the tool's docstring), and how a stored case goes through the Python transcription and the numpy restatement of
that matcher and is compared with what the reference's own ORBmatcher.cpp returned.

Not a test module.  A case is a dict: the sides and prm in the vocabulary of the matcher's host test, `out` (the reference's outputs, from
oracle/pyref_matcher.py's driver) and `counters` (the transcription's trace on the same inputs)."""
from collections import OrderedDict

import numpy as np

import fuse_replay
import test_bow_host as tb
import test_fuse_host as tf
import test_search_kf_host as tk
import test_loop_host as tl
import test_search_init_host as ti
import test_search_last_frame_host as tlf
import test_search_local_host as tloc
import test_triangulation_host as tt

f32 = np.float32
LOCAL_CAP = 128                               # the shipped library's per-point candidate list of k_local_candidates (tests/test_gpu_search_local.py)
TH_LOW, TH_HIGH = 50, 100                     # ORBmatcher.cpp:24-25: compiled into the reference


def fold_angles(a):
    """into [0, 360): outside it the reference indexes outside its histogram (its assert is compiled in and would abort)"""
    a = np.asarray(a, np.float32)
    out = np.mod(a, f32(360)).astype(np.float32)
    out[out >= f32(360)] = f32(0)
    return out


def wrap_levels(level, n_levels):
    """a level outside the pyramid (the generators draw a few: outside the contract of include/jsorb.h) makes the reference read outside
    mvScaleFactors; such entries are taken modulo the number of levels"""
    level = np.asarray(level).astype(np.int64)
    bad = (level < 0) | (level >= n_levels)
    return np.where(bad, np.mod(level, n_levels), level).astype(np.int32)


def block_of(name):
    """'random1.07' -> 'random1', 'real0.01' -> 'real0' (a block on the extracted frame); None for a constructed case"""
    return name.split(".")[0] if name.startswith(("random", "real")) else None


SYNTH = dict(config="c1", seed=11)            # frame 0 of the "real" cases: the left image of synth_stereo_pair(seed) at tests/conftest.py's CONFIGS[config] (484 keypoints)
# frame 1 of the real cases (950 keypoints), and the handle every other case of the frame-handle files is written over (on_handle below).
# 8 levels: every pyramid the generators draw is a prefix of the handle's.
POKE = dict(h=240, w=320, L=8, tile=15, th=20, seed=2, fx=435.2, bf=47.906)


class OracleFrame:
    """the oracle's extraction of the SYNTH image behind the accessors of the product's ORBExtractor that the GPU tests' frame builders use
    (tests/frame_builders.py: frame_of): tools/ref_matcher_goldens.py builds the real cases from it on the CPU, the GPU tests extract the
    same image on the device and require the same frame before they match against it"""

    def __init__(self, po, frame=0):
        from conftest import CONFIGS
        from jetson_slam_amd.synth import synth_stereo_pair
        self.c = dict(CONFIGS[SYNTH["config"]], seed=SYNTH["seed"]) if frame == 0 else POKE
        self.e = po.OracleExtractor(height=self.c["h"], width=self.c["w"], n_levels=self.c["L"], tile_h=self.c["tile"], tile_w=self.c["tile"],
                                    th_fast_max=self.c["th"])
        self.e.extract(synth_stereo_pair(self.c["seed"], self.c["h"], self.c["w"])[0])

    def keypoints(self, image=0):
        return self.e.keypoints().copy()

    def keypoints_undistorted(self, image=0):
        kp, n = self.e.keypoints(), self.e.n
        return kp[:n].astype(np.float32), kp[n:2 * n].astype(np.float32)

    def descriptors(self, image=0):
        return self.e.descriptors().copy()

    def get_scale_factors(self):
        return self.e.scales()


def is_real(name):
    return name.startswith("real")


# The generators' random cases and the constructed cases reach the device too: their frame is written over the keypoints of an extracted frame
# (tests/test_gpu_search_kf.py: poke_keypoints), which takes integer coordinates and exactly the handle's keypoint count.  So the frame of every
# such case is stored as the handle will hold it - coordinates rounded, the unused keypoints in a far corner on octave 2 with the all-ones
# descriptor (constructed_on_device's padding) - and the reference, the host yardsticks and the device all see that frame.
_poke_n = []


def poke_count(po):
    """the keypoint count of the POKE handle's extraction (the oracle's, which the device reproduces bit for bit)"""
    if not _poke_n:
        from jetson_slam_amd.synth import synth_stereo_pair
        e = po.OracleExtractor(height=POKE["h"], width=POKE["w"], n_levels=POKE["L"], tile_h=POKE["tile"], tile_w=POKE["tile"], th_fast_max=POKE["th"])
        e.extract(synth_stereo_pair(POKE["seed"], POKE["h"], POKE["w"])[0])
        _poke_n.append(int(e.n))
    return _poke_n[0]


def on_handle(po, F):
    """the frame side F as the POKE handle can hold it: rounded coordinates, padded to the handle's keypoint count, the grid rebuilt"""
    N, n0 = poke_count(po), len(F["kx"])
    assert N > n0
    pad = N - n0
    cat = lambda a, fill, dt: np.concatenate([np.asarray(a, dt).reshape((n0,) + np.shape(a)[1:]), np.full((pad,) + np.shape(a)[1:], fill, dt)])
    G = dict(F)
    G["kx"] = cat(np.round(np.asarray(F["kx"], np.float32)), POKE["w"] - 3.0, np.float32)
    G["ky"] = cat(np.round(np.asarray(F["ky"], np.float32)), POKE["h"] - 3.0, np.float32)
    G["octave"] = cat(F["octave"], 2, np.asarray(F["octave"]).dtype if n0 else np.int64)
    G["desc"] = cat(np.asarray(F["desc"], np.uint8).reshape(n0, 32), 255, np.uint8)
    if "angle" in F:
        G["angle"] = cat(F["angle"], 0, np.float32)
    if F.get("u_right") is not None:
        G["u_right"] = cat(F["u_right"], -1, np.float32)
    if F.get("blocked") is not None:
        G["blocked"] = cat(F["blocked"], 0, np.uint8)
    G["grid"], G["start"], G["items"] = tloc.build_grid(G["kx"], G["ky"], F["min_x"], F["min_y"], F["inv_w"], F["inv_h"], F["cols"], F["rows"])
    return G


class Matcher:
    driver = None
    required = ()                             # the counters the host test requires to be non-zero on a random block

    @staticmethod
    def verify(po, c):
        """what tools/ref_matcher_goldens.py requires of a case and its stored reference output before it writes it (and the CPU test again)"""

    @staticmethod
    def prepare(c):
        """a loaded case as the yardsticks and the driver take it"""
        return c


# ------------------------------------------------------------------ SearchByProjection(F, map points, th)
class SearchLocal(Matcher):
    driver = "search_local"
    required = ("matches", "multi_round")     # tests/test_search_local_host.py: n_matched and n_rounds_gt1

    @staticmethod
    def build(po):
        out = OrderedDict()
        for b, (th, stereo) in enumerate([(1.0, False), (3.0, True), (5.0, True)]):
            rng = np.random.default_rng(7100 + b)
            for c in range(10):
                F, P = tloc.random_case(rng, th, stereo, chain=c % 5 == 0)
                P["level"] = wrap_levels(P["level"], len(F["scale"]))
                out["random%d.%02d" % (b, c)] = dict(F=on_handle(po, F), P=P, prm=dict(th=f32(th), nn_ratio=f32(1.0 if c % 5 == 0 else 0.8)))
        # the extracted frame the device can be given (monocular: uRight on the device comes from its own stereo match), 800 points, blocked keypoints
        from frame_builders import frame_of, points_near_keypoints
        for b, (th, frame) in enumerate(((1.0, 0), (3.0, 0), (5.0, 0), (3.0, 1))):
            g = OracleFrame(po, frame)
            blocked = (np.random.default_rng(7149).random(g.e.n) < 0.05).astype(np.uint8)
            for k in range(2):
                rng = np.random.default_rng(7150 + 10 * b + k)
                F = frame_of(g, g.c, blocked=blocked)
                P, _ = points_near_keypoints(rng, F, 800 if frame == 0 else 1000, g.c["L"])
                P["desc"][1::50] = P["desc"][0::50][:len(P["desc"][1::50])]      # identical descriptors: exact-tie distances
                out["real%d.%02d" % (b, k)] = dict(F=F, P=P, prm=dict(th=f32(th), nn_ratio=f32(0.8)), frame=np.int64(frame))
        return out

    @staticmethod
    def transcription(po, c):
        return tloc.search_by_projection(c["F"], c["P"], c["prm"]["th"], c["prm"]["nn_ratio"], TH_HIGH)

    @staticmethod
    def restatement(po, c):
        return tloc.search_local_restated(c["F"], c["P"], c["prm"]["th"], c["prm"]["nn_ratio"], TH_HIGH)

    @staticmethod
    def counters(po, c, tr):
        rounds = tloc.search_local_restated(c["F"], c["P"], c["prm"]["th"], c["prm"]["nn_ratio"], TH_HIGH)[4]
        n_cand = [len(k) for k in tloc.candidate_lists(c["F"], c["P"], c["prm"]["th"])]
        return dict(matches=tr[3], multi_round=int(rounds > 2), rounds=rounds, candidates=int(sum(n_cand)), overflow=int(sum(n > LOCAL_CAP for n in n_cand)))

    @staticmethod
    def same(c, res):
        """kp_match (a keypoint blocked before the call is -2 in the reference's output and -1 here) and the count"""
        want = np.where(c["out"]["kp_match"] == -2, -1, c["out"]["kp_match"])
        assert np.array_equal(res[2], want) and res[3] == int(c["out"]["nmatches"])
        # the per-point view of the same thing: point i's keypoint is the one that holds i
        held = {int(i): k for k, i in enumerate(want) if i >= 0}
        assert all(int(res[0][i]) == held.get(i, -1) for i in range(len(res[0])))


# ------------------------------------------------------------------ SearchByProjection(CurrentFrame, LastFrame, th, bMono)
class SearchLastFrame(Matcher):
    driver = "search_last_frame"
    required = ("matches", "culled", "shared")

    @staticmethod
    def build(po):
        out = OrderedDict()
        for b in range(3):
            rng = np.random.default_rng(7200 + b)
            for c in range(10):
                F, P, prm = tlf.random_case(rng, mono=(b == 2), dense=c % 4 == 0)
                P["octave"] = wrap_levels(P["octave"], len(F["scale"]))
                prm = dict(prm, th_high=TH_HIGH, retry_below=0)
                out["random%d.%02d" % (b, c)] = dict(F=on_handle(po, F), P=P, prm=prm)
        # the extracted frame the device can be given (monocular), 600 points, every direction
        from frame_builders import last_frame_of, params, points_of
        for b, (th, frame) in enumerate(((7.0, 0), (15.0, 0), (7.0, 1))):
            g = OracleFrame(po, frame)
            for k, direction in enumerate((0, 1, -1)):
                rng = np.random.default_rng(7250 + 10 * b + k)
                F = last_frame_of(g, g.c)
                prm = params(g.c, F, th, direction=direction, retry_below=0, seed=10 * b + k + 1)
                P, _ = points_of(rng, F, prm, 600 if frame == 0 else 1000, g.c["L"])
                out["real%d.%02d" % (b, k)] = dict(F=F, P=P, prm=prm, frame=np.int64(frame))
        return out

    @staticmethod
    def transcription(po, c):
        return tlf.search_by_projection_last(po, c["F"], c["P"], c["prm"], f32(c["prm"]["th"]))

    @staticmethod
    def restatement(po, c):
        return tlf.search_last_restated(po, c["F"], c["P"], c["prm"], f32(c["prm"]["th"]))

    @staticmethod
    def counters(po, c, tr):
        m = tr[0][tr[0] >= 0]
        culled = sum(1 for i in np.nonzero(tr[0] >= 0)[0] if tr[2][tr[0][i]] == -1)      # matched points whose keypoint the cull emptied
        return dict(matches=tr[3], culled=int(culled), shared=len(m) - len(set(m.tolist())), candidates=tr[4], ind=np.asarray(tr[5], np.int64))

    @staticmethod
    def same(c, res):
        assert np.array_equal(res[2], c["out"]["kp_match"]) and res[3] == int(c["out"]["nmatches"])


# ------------------------------------------------------------------ SearchForInitialization
class SearchInit(Matcher):
    driver = "search_init"
    required = ("matches", "displaced", "hidden", "culled")

    @staticmethod
    def _clean(po, F1, F2, prev, prm, fold=True):
        """(an extracted frame's angles lie in (-180, 180] and stay as they are: differences within (-360, 540) fall inside the histogram)"""
        F1 = dict(F1, octave=np.where(np.asarray(F1["octave"]) < 0, 1, F1["octave"]).astype(np.int32), angle=fold_angles(F1["angle"]))
        return dict(F1=F1, F2=on_handle(po, dict(F2, angle=fold_angles(F2["angle"]))) if fold else F2, prev=np.asarray(prev, np.float32),
                    prm=dict(prm, th_low=TH_LOW, window=f32(int(prm["window"]))))

    @classmethod
    def build(cls, po):
        out = OrderedDict()
        for b in range(3):
            rng = np.random.default_rng(7300 + b)
            for c in range(12):
                out["random%d.%02d" % (b, c)] = cls._clean(po, *ti.random_case(rng, big=c % 4 == 0))
        prm0 = ti.default_params(check_orientation=0)
        # the one-keypoint chains of the host test with distances that stay within the reference's TH_LOW = 50 (the host test runs them at 256)
        for n in (5, 45):
            out["chain decreasing %d" % n] = cls._clean(po, *ti.one_target(list(range(n, 0, -1))), prm0)
        for n in (5, 65):
            out["chain increasing %d" % n] = cls._clean(po, *ti.one_target([min(1 + k, 50) for k in range(n)]), prm0)
            out["chain equal %d" % n] = cls._clean(po, *ti.one_target([30] * n), prm0)
        for n in (3, 70):
            out["domino %d" % n] = cls._clean(po, *ti.domino(n))
        F1, F2, prev, prm = ti.domino(20)
        prev = prev.copy()
        prev[0, 0] = 20
        out["domino broken at its start"] = cls._clean(po, F1, F2, prev, prm)
        # the extracted frame the device can be given: F1 drawn from its keypoints (duplicate targets: displaced and hidden points)
        for b, (prm, frame) in enumerate([(ti.default_params(), 0), (ti.default_params(window=f32(12), nn_ratio=f32(0.6)), 0), (ti.default_params(), 1)]):
            g = OracleFrame(po, frame)
            xu, yu = g.keypoints_undistorted()
            F2 = ti.frame_from_extract(g.keypoints(), g.descriptors(), xu, yu, g.c["w"], g.c["h"])
            for k in range(2):
                F1, prev = ti.f1_drawn_from(np.random.default_rng(7350 + 10 * b + k), F2, 500 if frame == 0 else 900)
                out["real%d.%02d" % (b, k)] = dict(cls._clean(po, F1, F2, prev, prm, fold=False), frame=np.int64(frame))
        return out

    @staticmethod
    def transcription(po, c):
        return ti.search_for_initialization(c["F1"], c["F2"], c["prev"], c["prm"])

    @staticmethod
    def restatement(po, c):
        return ti.search_init_restated(c["F1"], c["F2"], c["prev"], c["prm"])

    @staticmethod
    def counters(po, c, tr):
        t = tr[4]
        return dict(matches=tr[2], **{k: int(t[k]) for k in ("candidates", "displaced", "hidden", "choice_changed", "ratio_flip", "culled", "displaced_kept",
                                                            "displaced_culled", "claims")},
                    ind=np.asarray(t["ind"], np.int64), **dict(zip(("rounds", "overflow"), (lambda st: (st[0], st[2]))(
                        ti.search_init_restated(c["F1"], c["F2"], c["prev"], c["prm"])[4]))))

    @staticmethod
    def same(c, res):
        o = c["out"]
        assert np.array_equal(res[0], o["matches12"]) and res[2] == int(o["nmatches"])
        assert np.array_equal(np.asarray(res[3], np.float32).view(np.uint32), np.asarray(o["prev"], np.float32).reshape(2, -1).view(np.uint32))


# ------------------------------------------------------------------ SearchByBoW(KeyFrame, Frame)
def _bow_clean(KF, F, prm):
    return dict(KF=dict(KF, angle=fold_angles(KF["angle"])), F=dict(F, angle=fold_angles(F["angle"])), prm=dict(prm, th_low=TH_LOW))


class SearchByBow(Matcher):
    driver = "search_by_bow"
    required = ("matches", "culled", "second_choice", "ratio_fail")

    @staticmethod
    def build(po):
        out = OrderedDict()
        for b in range(3):
            rng = np.random.default_rng(7400 + b)
            for c in range(3):                # 300 - 800 keypoints a side
                voc = tb.random_voc(rng)
                levels_up = int(rng.integers(0, voc["depth_L"] + 1))
                n_f, n_k = (800, 800) if c == 0 else (int(rng.integers(300, 800)) for _ in range(2))
                KF, F = tb.random_sides(rng, voc, levels_up, n_f, n_k)
                prm = tb.default_params(nn_ratio=f32(rng.choice([0.7, 0.75, 0.9])), check_orientation=int(c % 3 != 2))
                out["random%d.%02d" % (b, c)] = _bow_clean(KF, F, prm)
        for name, ((KF, F), prm, want, count) in tb.CONSTRUCTED.items():
            out[name] = _bow_clean(KF, F, prm)
        voc, KF, F = tb.single_node_case()
        out["one large node"] = _bow_clean(KF, F, tb.default_params())
        return out

    @staticmethod
    def transcription(po, c):
        return tb.search_by_bow_reference(c["KF"], c["F"], c["prm"])

    @staticmethod
    def restatement(po, c):
        return tb.search_by_bow_restated(c["KF"], c["F"], c["prm"], rng=np.random.default_rng(1), network=True)

    @staticmethod
    def counters(po, c, tr):
        t = tr[2]
        return dict(matches=tr[1], ind=np.asarray(t["ind"], np.int64),
                    **{k: int(t[k]) for k in ("node_pairs", "distances", "largest_node", "claims", "culled", "second_choice", "ratio_fail")})

    @staticmethod
    def same(c, res):
        assert np.array_equal(res[0], c["out"]["match_kf"]) and res[1] == int(c["out"]["nmatches"])


# ------------------------------------------------------------------ SearchByBoW(KeyFrame, KeyFrame)
class SearchByBowKf(Matcher):
    driver = "search_by_bow_kf"
    required = tl.BOW_GATES + ("matches", "overflow")

    @staticmethod
    def build(po):
        out = OrderedDict()
        for b in range(2):                    # a block: 2 calls of one keyframe against 3 loop candidates (one drawn set of keypoints, cut in three)
            rng = np.random.default_rng(7500 + b)
            for call in range(2):
                n1, cut = (380, [600, 900, 1200]) if call == 0 else (int(rng.integers(300, 400)), [310, 650, 1000])
                KF1, KF2 = tl.random_bow_sides(rng, n1, cut[-1], n_nodes=3 if call == 0 else int(rng.choice([12, 40])))
                prm = tl.bow_params(nn_ratio=f32(rng.choice([0.6, 0.75, 0.9])), check_orientation=int(call == 0))
                for k, (lo, hi) in enumerate(zip([0] + cut, cut)):
                    out["random%d.%02d" % (b, 3 * call + k)] = dict(KF1=dict(KF1, angle=fold_angles(KF1["angle"])), prm=dict(prm, th_low=TH_LOW),
                                                                    KF2={key: (fold_angles(v) if key == "angle" else v)[lo:hi] for key, v in KF2.items()})
        for name, ((KF1, KF2), prm, want, count) in tl.BOW_CONSTRUCTED.items():
            out[name] = dict(KF1=dict(KF1, angle=fold_angles(KF1["angle"])), KF2=dict(KF2, angle=fold_angles(KF2["angle"])), prm=dict(prm, th_low=TH_LOW))
        return out

    @staticmethod
    def transcription(po, c):
        return tl.bow_kf_reference(c["KF1"], c["KF2"], c["prm"])

    @staticmethod
    def restatement(po, c):
        return tl.bow_kf_restated(c["KF1"], c["KF2"], c["prm"], rng=np.random.default_rng(1), network=True)

    @staticmethod
    def counters(po, c, tr):
        t = tr[2]
        d = {k: int(t[k]) for k in tl.BOW_GATES + ("node_pairs", "distances", "largest_node", "claims")}
        return dict(d, matches=tr[1], overflow=int(t["largest_node"] > 64 * tl.LB_NODE_REGS), ind=np.asarray(t["ind"], np.int64))

    @staticmethod
    def same(c, res):
        assert np.array_equal(res[0], c["out"]["matches12"]) and res[1] == int(c["out"]["nmatches"])


# ------------------------------------------------------------------ SearchForTriangulation
class SearchForTriangulation(Matcher):
    driver = "search_for_triangulation"
    required = ("matches", "gate_skips", "line_fails", "line_passes", "culled", "ties_replaced", "pruned", "shared", "big_node")

    @staticmethod
    def _clean(KF1, KF2, geom, prm):
        nl = int(prm["n_levels"])
        return dict(KF1=dict(KF1, angle=fold_angles(KF1["angle"])), KF2=dict(KF2, angle=fold_angles(KF2["angle"]), octave=wrap_levels(KF2["octave"], nl)),
                    geom=dict(geom), prm=dict(prm, th_low=TH_LOW))

    @classmethod
    def build(cls, po):
        out = OrderedDict()
        for b in range(2):                    # a block: one call of a keyframe against 4 neighbours, each with a geometry of its own
            rng = np.random.default_rng(7600 + b)
            n1 = int(rng.integers(300, 400))
            kw = dict(n_nodes=[12, 3][b], only_stereo=0, check_orientation=1, free=0.8, stereo=0.3, noise=1.0, n_levels=8)
            KF1, KF2, geom, prm = tt.random_case(rng, n1, int(rng.integers(300, 400)), near_epipole=0.3, forward=True, **kw)
            out["random%d.00" % b] = cls._clean(KF1, KF2, geom, prm)
            for k in range(1, 4):             # the other neighbours observe KF1's landmarks under a pose of their own (tests/test_gpu_triangulation.py: observe)
                n2 = int(rng.integers(300, 400))
                _, K2, g2, _ = tt.random_case(rng, 0, n2, near_epipole=0.3 * (k == 2), forward=bool(k == 2), **kw)
                src = rng.integers(0, n1, n2)
                K2 = dict(K2, desc=tb.flip_bits(rng, KF1["desc"][src], 0, 9), node=KF1["node"][src].copy())
                if k == 3:                    # ... or lie on the line x2 = 0 of the constructed cases, which most candidates pass
                    K2["x"] = np.where(rng.random(n2) < 0.7, 0.0, 5.0).astype(np.float32)
                    g2 = tt.geometry(tt.F_LINE, *tt.FAR)
                out["random%d.%02d" % (b, k)] = cls._clean(KF1, K2, g2, prm)
        for name, (KF1, KF2, geom, prm, want, count) in tt.CONSTRUCTED.items():
            out[name] = cls._clean(KF1, KF2, geom, prm)
        return out

    @staticmethod
    def transcription(po, c):
        return tt.search_for_triangulation_reference(c["KF1"], c["KF2"], c["geom"], c["prm"])

    @staticmethod
    def restatement(po, c):
        return tt.search_for_triangulation_restated(c["KF1"], c["KF2"], c["geom"], c["prm"], network=True)

    @staticmethod
    def counters(po, c, tr):
        t = tr[3]
        taken = tr[0][tr[0] >= 0]
        d = {k: int(t[k]) for k in ("node_pairs", "distances", "line_tests", "largest_node", "gate_skips", "line_fails", "line_passes", "culled",
                                    "ties_replaced", "pruned")}
        return dict(d, matches=tr[1], shared=len(taken) - len(set(taken.tolist())), big_node=int(t["largest_node"] > tt.TR_LANES),
                    ind=np.asarray(t["ind"], np.int64))

    @staticmethod
    def same(c, res):
        pairs = np.asarray(c["out"]["pairs"], np.int64).reshape(-1, 2)
        m12 = np.full(len(c["KF1"]["node"]), -1, np.int64)
        m12[pairs[:, 0]] = pairs[:, 1]
        assert np.array_equal(res[0], m12) and res[1] == int(c["out"]["nmatches"]) == len(pairs)
        assert (np.diff(pairs[:, 0]) > 0).all()               # vMatchedPairs is in ascending idx1


# ------------------------------------------------------------------ Fuse(pKF, vpMapPoints, th) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
# The device projects with K14 / K16's fused steps, the reference with separate float products and sums through cv::Mat: the two agree bit for
# bit only where every product and partial sum is exact in float.  So these cases are built on exact inputs - rotations that are signed
# permutations, camera depths that are powers of two, fx = fy = 256, dyadic cx, cy, bf, translations, normals and Sim3 scales, projections on a
# quarter-pixel grid - and prove_exact() checks it per case, step by step, never trusting the construction.
F64 = np.float64
LEVEL_MARGIN = 2.0 ** -10
ROT_Z = [np.array(r, np.float32) for r in ([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, -1, 0, 1, 0, 0, 0, 0, 1], [-1, 0, 0, 0, -1, 0, 0, 0, 1], [0, 1, 0, -1, 0, 0, 0, 0, 1])]


class LevelMargin(AssertionError):
    """a pair whose predicted level could depend on the logf in use; .indices: the positions (in the proof's own point order) to draw again"""

    def __init__(self, message, indices):
        super().__init__(message)
        self.indices = np.asarray(indices, np.int64)


def check_levels(prm, maxd, dist, reached, index_of):
    """ceil(logf(maxd / dist) / logScaleFactor) clamped, with two different logf: the float64 quotient moved by +-2^-10 must clamp to the same level
    for every pair that reaches PredictScale (`reached`); index_of maps a position of these arrays to the caller's point index"""
    with np.errstate(all="ignore"):
        ratio = (np.asarray(maxd, np.float32) / np.where(reached, dist, f32(1))).astype(np.float32).astype(F64)
        q = np.log(np.where(reached & (ratio > 0), ratio, 1.0)) / float(f32(prm["log_sf"]))
    nl = len(prm["scale"])
    lo, hi = np.clip(np.ceil(q - LEVEL_MARGIN), 0, nl - 1), np.clip(np.ceil(q + LEVEL_MARGIN), 0, nl - 1)
    bad = reached & (lo != hi)
    if bad.any():
        raise LevelMargin("a level within 2^-10 of a step of ceil", np.asarray(index_of)[bad])
    return int(reached.sum())


def _ex(r, what):
    """r (float64, computed from float32 values) is a float32: the float32 rounding of this step is the identity"""
    r = np.asarray(r, F64)
    ok = (r.astype(np.float32).astype(F64) == r) | ~np.isfinite(r)
    assert ok.all(), "inexact in float32: %s (%d values, first %r)" % (what, int((~ok).sum()), r[~ok].ravel()[0])
    return r


def mind_for(mindi):
    """mfMinDistance values whose GetMinDistanceInvariance (0.8f * mfMinDistance, one float product) is exactly mindi: x -> 0.8f x maps
    neighbouring floats at most one ulp apart, so every float is reached"""
    mindi = np.asarray(mindi, np.float32)
    m = (mindi.astype(F64) / float(f32(0.8))).astype(np.float32)
    for _ in range(8):
        got = (f32(0.8) * m).astype(np.float32)
        done = (got == mindi) | ~np.isfinite(mindi)
        if done.all():
            return m
        m = np.where(done, m, np.nextafter(m, np.where(got < mindi, f32(np.inf), f32(-np.inf)).astype(np.float32))).astype(np.float32)
    raise AssertionError("no mfMinDistance found")


def maxd_for(maxdi):
    """an mfMaxDistance with 1.2f * mfMaxDistance == maxdi exactly, searched among the neighbours of maxdi / 1.2f (not every float is reached)"""
    m0 = f32(float(maxdi) / float(f32(1.2)))
    for step in range(-16, 17):
        m = m0
        for _ in range(abs(step)):
            m = np.nextafter(m, f32(np.inf) if step > 0 else f32(-np.inf))
        if f32(f32(1.2) * m) == f32(maxdi):
            return f32(m)
    raise AssertionError("no mfMaxDistance found")


def fuse_case(prm, kfs, poses, P, mps=None, obs=(), targets=None, lst=None, Scw=None, replace_loop=0):
    """a case of the fuse files (fuse_replay's vocabulary) from tests/test_fuse_host.py's keyframes, poses and points: by default every keyframe is
    a target with empty slots, every point is in the list, nothing is observed"""
    n = len(P["Px"])
    P = dict(P)
    if "mind" not in P:
        P["mind"] = mind_for(P["mindi"])
    P["mindi"], P["maxdi"] = (f32(0.8) * np.asarray(P["mind"], np.float32)).astype(np.float32), (f32(1.2) * np.asarray(P["maxd"], np.float32)).astype(np.float32)
    P.setdefault("bad", np.zeros(n, np.uint8))
    P = {k: np.asarray(v, np.uint8 if k in ("bad", "desc") else np.float32) for k, v in P.items()}
    P["desc"] = P["desc"].reshape(n, 32)
    KF = []
    for j, (K, (R, t, O)) in enumerate(zip(kfs, poses)):
        N = len(K["x"])
        KF.append(dict(x=K["x"], y=K["y"], octave=K["octave"], desc=K["desc"], uright=K["uright"] if K["uright"] is not None else np.full(N, -1, np.float32),
                       Rcw=np.asarray(R, np.float32),
                       tcw=np.asarray(t, np.float32), Ow=np.asarray(O, np.float32),
                       mps=np.full(N, -1, np.int32) if mps is None or mps[j] is None else np.asarray(mps[j], np.int32)))
    c = dict(KF=KF, P=P, prm={k: (np.asarray(v) if isinstance(v, np.ndarray) else v) for k, v in prm.items()}, obs=np.asarray(obs, np.int32).reshape(-1, 3),
             targets=np.asarray(range(len(kfs)) if targets is None else targets, np.int32), list=np.asarray(range(n) if lst is None else lst, np.int32))
    # a map as the reference keeps it: an observation's slot holds the observer, and a live point in a slot observes it (the head tests' "a point
    # leaves a keyframe only by becoming bad" rests on that)
    for p, k, i in c["obs"]:
        assert KF[k]["mps"][i] == p and not P["bad"][p], ("observation without its slot", p, k, i)
    seen = set(map(tuple, c["obs"].tolist()))
    for k, K in enumerate(KF):
        for i, p in enumerate(K["mps"]):
            assert p < 0 or P["bad"][p] or (int(p), k, i) in seen, ("slot without its observation", p, k, i)
    if Scw is not None:
        c["Scw"], c["replace_loop"] = np.asarray(Scw, np.float32).reshape(len(c["targets"]), 16), np.int64(replace_loop)
    return with_grids(c)


def named(c, driver, cname):
    """the case with its file and name under keys the files do not store (STATED_DIFFERENCES is looked up by them)"""
    c["_driver"], c["_name"] = driver, cname
    return c


def with_grids(c):
    """every keyframe's mGrid and its CSR, built from its keypoints (AssignFeaturesToGrid: tests/test_search_local_host.py's build_grid) under
    keys the files do not store: 4 000 cell starts a keyframe would be most of a file"""
    prm = c["prm"]
    for K in c["KF"]:
        if "grid" not in K:
            K["grid"], K["_start"], K["_items"] = tloc.build_grid(K["x"], K["y"], prm["min_x"], prm["min_y"], prm["inv_w"], prm["inv_h"], int(prm["cols"]), int(prm["rows"]))
    return c


def scw_of(pose, s=1.0):
    """Scw = [s R | s t; 0 0 0 1] row-major for a pose (Rcw, tcw, Ow) and a scale"""
    R, t, _ = pose
    S = np.eye(4, dtype=np.float32)
    S[:3, :3], S[:3, 3] = f32(s) * np.asarray(R, np.float32).reshape(3, 3), f32(s) * np.asarray(t, np.float32)
    return S.ravel()


def list_points(c, idxs=None, desc=None):
    """the list's points as tests/test_fuse_host.py's P (a NULL entry: point 0's values, to be skipped)"""
    lst = np.asarray(c["list"], np.int64)
    if idxs is not None:
        lst = lst[list(idxs)]
    sel = np.maximum(lst, 0)
    n_pts = len(c["P"]["Px"])
    P = {k: (np.asarray(v)[sel] if n_pts else np.asarray(v)[:0]) for k, v in c["P"].items()}
    if desc is not None:
        P["desc"] = np.asarray(desc, np.uint8).reshape(len(lst), 32)
    return P


def kf_side(c, k):
    K = c["KF"][k]
    return dict(K, start=K["_start"], items=K["_items"], uright=K["uright"] if (np.asarray(K["uright"]) >= 0).any() else None), (K["Rcw"], K["tcw"], K["Ow"])


def fuse_prm(c):
    return dict(c["prm"], cols=int(c["prm"]["cols"]), rows=int(c["prm"]["rows"]), th_low=int(c["prm"]["th_low"]), check=int(c["prm"]["check"]))


def fuse_search(po, c, kind="transcription", mutant=None, trace=None):
    """fuse_replay's search over the host yardsticks: the sequential transcription (with its probes and gate trace) or the restatement of the kernels"""
    prm = fuse_prm(c)

    def search(ts, idxs, desc, skip):
        P = list_points(c, idxs, desc)
        bi, bd = np.full((len(ts), len(idxs)), -1, np.int64), np.full((len(ts), len(idxs)), -1, np.int64)
        st, probes = [0, 0, 0, 0], {}
        for r, t in enumerate(ts):
            K, pose = kf_side(c, int(c["targets"][t]))
            if kind == "transcription":
                pr = {}
                res = tf.fuse_reference(po, K, pose, P, prm, skip[r], probe=pr, mutant=mutant)
                tr = res[3]
                one = (tr["windows"], tr["walked"], tr["distances"], tr["largest"]) if len(K["x"]) else (0, 0, 0, 0)
                probes.update({(t, idxs[i]): rows for i, rows in pr.items()})
                if trace is not None:
                    trace.update({g: trace.get(g, 0) + tr[g] for g in tf.GATES})
            else:
                res = tf.fuse_restated(po, K, pose, P, prm, skip[r])
                one = res[3]
            bi[r], bd[r] = res[0], res[1]
            st = [st[0] + one[0], st[1] + one[1], st[2] + one[2], max(st[3], one[3])]
        return bi, bd, st, probes
    return search


def prove_exact(c):
    """Every float32 step in which the contract's route (K14 / K16: fused) and the reference's route (separate products and sums, left to right)
    differ is exact for every (target keyframe, list point) pair that reaches it: evaluated in float64 from the float32 inputs, each intermediate
    must be a float32.  Then both routes compute the same real numbers and so the same bits.  Steps both routes compute with the same operations
    (ur, the chi-square sums, the cell range, maxd / dist) need no exactness.  Also: Scw decomposes exactly into the stored pose, and no pair's
    level can depend on the logf in use (returns the number of pairs that reach PredictScale)."""
    prm, lst = c["prm"], np.asarray(c["list"], np.int64)
    P = list_points(c)
    live = lst >= 0
    x, y, z = (np.asarray(P[k], np.float32).astype(F64)[live] for k in ("Px", "Py", "Pz"))
    nx, ny, nz = (np.asarray(P[k], np.float32).astype(F64)[live] for k in ("Nx", "Ny", "Nz"))
    fx, fy, cx, cy = (float(prm[k]) for k in ("fx", "fy", "cx", "cy"))
    n_level_pairs = 0
    for t, k in enumerate(c["targets"]):
        K = c["KF"][int(k)]
        R, tc, Ow = (np.asarray(K[a], np.float32).astype(F64).ravel() for a in ("Rcw", "tcw", "Ow"))
        if c.get("Scw") is not None:
            S = np.asarray(c["Scw"], np.float32).astype(F64).reshape(-1, 4, 4)[t]
            s2 = _ex(_ex(_ex(S[0, 0] * S[0, 0], "scw") + _ex(S[0, 1] * S[0, 1], "scw"), "scw") + _ex(S[0, 2] * S[0, 2], "scw"), "scw")
            s = _ex(np.sqrt(s2), "scw")
            Rd, td = _ex(S[:3, :3] / s, "Rcw = sRcw / scw"), _ex(S[:3, 3] / s, "tcw / scw")
            Od = np.zeros(3)
            for r in range(3):                                   # Ow = -Rcw^T tcw: a row of the transpose times the vector, left to right
                acc = _ex(-Rd[0, r] * td[0], "Ow")
                for q in (1, 2):
                    acc = _ex(acc + _ex(-Rd[q, r] * td[q], "Ow"), "Ow")
                Od[r] = acc
            assert np.array_equal(Rd.ravel(), R) and np.array_equal(td, tc) and np.array_equal(Od + 0.0, Ow + 0.0), "Scw is not the stored pose"
        with np.errstate(all="ignore"):
            Pc = []
            for r in range(3):                                   # (x R0 + y R1) + z R2, then + t: the partial sums of both routes
                a, b, d = _ex(x * R[3 * r], "x R"), _ex(y * R[3 * r + 1], "y R"), _ex(z * R[3 * r + 2], "z R")
                Pc.append(_ex(_ex(_ex(a + b, "x R + y R") + d, "R P") + tc[r], "R P + t"))
            front = Pc[2] > 0
            invz = _ex(np.where(front, 1.0 / np.where(front, Pc[2], 1.0), 0.0), "1 / Pcz")
            uv = []
            for Pa, f, cc in ((Pc[0], fx, cx), (Pc[1], fy, cy)):
                Pa = np.where(front, Pa, 0.0)
                _ex(Pa * f, "Pc * f")                             # K14 rounds this product before its fma
                xn = _ex(Pa * invz, "X * invz")                  # the reference's x = X * invz, u = fx * x + cx
                uv.append(_ex(_ex(f * xn, "f * x") + cc, "f * x + c"))
            u, v = uv
            inside = front & (u >= float(prm["min_x"])) & (u <= float(prm["max_x"])) & (v >= float(prm["min_y"])) & (v <= float(prm["max_y"]))
            o = [np.where(inside, _ex(a - Ow[r], "P - Ow"), 0.0) for r, a in enumerate((x, y, z))]
            d2 = _ex(_ex(_ex(o[0] * o[0], "ox^2") + _ex(o[1] * o[1], "oy^2"), "ox^2 + oy^2") + _ex(o[2] * o[2], "oz^2"), "dist^2")
            _ex(_ex(_ex(o[0] * nx, "ox nx") + _ex(o[1] * ny, "oy ny"), "ox nx + oy ny") + _ex(o[2] * nz, "oz nz"), "PO . Pn")
            # the level: ceil(logf(maxd / dist) / logScaleFactor) clamped, with two different logf - both candidates of a quotient near an integer
            # must clamp to the same level
            n_level_pairs += check_levels(prm, np.asarray(P["maxd"], np.float32)[live], np.sqrt(d2).astype(np.float32), inside, lst[live])
    return n_level_pairs


def sequential_run(po, c):
    """the transcription searched keyframe by keyframe on the live map - the reference's own order - and the gates its pairs stopped at"""
    trace = {}
    seq, _, _ = fuse_replay.replay(c, fuse_search(po, c, "transcription", None, trace), "sequential")
    return seq, trace


class Fuse(Matcher):
    driver = "fuse"
    required = tf.GATES + ("matches", "replace_to_kf", "replace_to_list", "added", "bad_in_kf", "head_flips", "descriptor_changes")
    NAMES_FROM_HOST_TEST = ("tie_within_a_cell", "tie_across_columns", "tie_across_rows", "column_before_row", "strictly_better_later_wins",
                            "th_low_accepted", "th_low_plus_one_not", "octaves_around_level_2", "octave_above_the_level", "u_at_max_x_is_out",
                            "u_at_min_x_is_in", "v_at_max_y_is_out", "v_at_min_y_is_in", "depth_zero_and_negative", "dot_at_half_the_distance",
                            "dot_below_half_the_distance", "window_over_the_left_edge", "window_over_the_right_edge", "window_over_the_top_edge",
                            "window_over_the_bottom_edge", "mono_dropped_at_6_5", "stereo_kept_at_6_5", "stereo_dropped_at_8_75",
                            "mono_beats_nothing_stereo_wins", "chi_square_at_float_7_8", "contraction_e2", "window_of_0", "window_of_1", "window_of_15",
                            "window_of_16", "window_of_17", "window_of_33", "no_keypoints", "no_points")
    check = 1
    main_shape = dict(th=3)
    prepare = staticmethod(with_grids)

    # ---- random blocks ----
    @classmethod
    def random_block(cls, rng, n_targets=5, n=150, N=300, stereo=0.5, th=3, n_world=None):
        """One direction of SearchInNeighbors on a small world: `n_targets` target keyframes, the current keyframe (index n_targets) and one more
        observer.  Every camera looks along world z - a turn about z by a multiple of 90 degrees and a shift in x, y by multiples of 1/16 - so a
        world point has the same power-of-two depth in every keyframe.  World points project on a quarter-pixel grid into a base camera; a
        keyframe's keypoints are projections of world points (a quarter pixel or a few sigma off), with a descriptor a few bits from the world
        point's; the list is the current keyframe's map points.  Slots of the targets hold nothing, another point with fewer / as many / more
        observations, or a bad one; a share of the list points fails each gate."""
        prm = tf.default_params(check=cls.check, th=f32(th))
        n_levels = len(prm["scale"])
        n_kf = n_targets + 2
        W = n_world or 2 * n
        poses = []
        for j in range(n_kf):
            R = ROT_Z[0] if j in (0, n_targets) else ROT_Z[int(rng.integers(0, 4))]
            t = np.array([rng.integers(-6, 7) / 16.0, rng.integers(-6, 7) / 16.0, 0], np.float32)
            poses.append((R, t, (-(R.reshape(3, 3).T @ t) + f32(0)).astype(np.float32)))
        wz = rng.choice([2.0, 4.0, 8.0], W)
        wu, wv = rng.integers(4 * 20, 4 * 300, W) / 4.0, rng.integers(4 * 20, 4 * 220, W) / 4.0
        Pc = np.stack([(wu - 160.0) * wz / 256.0, (wv - 120.0) * wz / 256.0, wz])
        wdesc = rng.integers(0, 256, (W, 32), dtype=np.uint8)
        wdesc[:, 16:] = 0                                           # (128 random bits tell two world points apart by about 64; the rest compresses)
        wlevel = rng.integers(1, n_levels - 1, W)

        def project(j, Pw):
            R, t, _ = poses[j]
            c = R.reshape(3, 3).astype(F64) @ Pw + t.astype(F64)[:, None]
            return 256.0 * c[0] / c[2] + 160.0, 256.0 * c[1] / c[2] + 120.0
        R0, t0, _ = poses[n_targets]                               # the base camera is the current keyframe
        Pw = R0.reshape(3, 3).astype(F64).T @ (Pc - t0.astype(F64)[:, None])
        kfs, src = [], []
        for j in range(n_kf):
            u, v = project(j, Pw)
            vis = np.nonzero((u > 2) & (u < 318) & (v > 2) & (v < 238))[0]
            w = rng.choice(vis, N if j < n_targets else N // 2, replace=len(vis) < N)
            case = rng.random(len(w))
            off = np.where(case < 0.08, 2.6 * prm["scale"][wlevel[w]].astype(F64), rng.integers(-2, 3, len(w)) / 4.0)      # 2.6 sigma off: beyond 5.99, within 7.8
            kx, ky = u[w] + off, v[w] + rng.integers(-2, 3, len(w)) / 4.0
            octave = wlevel[w] - rng.integers(0, 2, len(w))
            octave = np.where((case >= 0.08) & (case < 0.16), wlevel[w] + 1, octave)             # above the level window
            st = rng.random(len(w)) < stereo
            ur = np.where(st, kx - 32.0 / wz[w] + np.where((case >= 0.16) & (case < 0.22), 3.0, 0.0), -1.0)      # a disparity that no longer fits
            desc = wdesc[w].copy()
            flips = np.where(case >= 0.90, rng.integers(52, 90, len(w)), rng.integers(0, 40, len(w)))
            for i in range(len(w)):
                b = rng.choice(256, int(flips[i]), replace=False)
                np.bitwise_xor.at(desc[i], b // 8, (1 << (7 - b % 8)).astype(np.uint8))
            kfs.append(tf.keyframe(kx, ky, octave, desc, prm, ur.astype(np.float32) if stereo > 0 else None))
            src.append(w)
        # the list: the current keyframe's first n keypoints hold the list points (ids 0 .. n-1), each the world point of its keypoint
        cur = n_targets
        lw = src[cur][:n]
        n = len(lw)
        case = rng.random(n)
        Pl = Pw[:, lw].copy()
        Pl[2] = np.where(case < 0.05, -Pl[2], Pl[2])                                               # behind every camera
        nrm = np.zeros((3, n))
        pick = rng.integers(0, 3, n)
        nrm[:, pick == 0], nrm[:, pick == 1], nrm[:, pick == 2] = [[0], [0], [1]], [[0.25], [-0.25], [0.75]], [[0], [0.5], [0.75]]
        nrm[:, (case >= 0.05) & (case < 0.10)] = [[0], [0], [-1]]                                 # turned away
        Ow = poses[cur][2].astype(F64)
        dist = np.sqrt(((Pl - Ow[:, None]) ** 2).sum(0))
        P = dict(Px=Pl[0].astype(np.float32), Py=Pl[1].astype(np.float32), Pz=Pl[2].astype(np.float32), Nx=nrm[0].astype(np.float32),
                 Ny=nrm[1].astype(np.float32), Nz=nrm[2].astype(np.float32), desc=wdesc[lw].copy())
        # the other points (ids n ..): what target slots hold; P's arrays cover them with values no search reads
        mps = [np.full(len(K["x"]), -1, np.int32) for K in kfs]
        mps[cur][:n] = np.arange(n)
        obs = [(i, cur, i) for i in range(n)]
        others_bad = []
        for j in list(range(n_targets)) + [n_targets + 1]:
            for kp, w in enumerate(src[j]):
                r = rng.random()
                if r < 0.45 or mps[j][kp] >= 0:
                    continue                                        # an empty slot (or one a point of an earlier keyframe took)
                pid = n + len(others_bad)
                others_bad.append(r > 0.92)
                mps[j][kp] = pid
                if others_bad[-1]:
                    continue                                        # a bad point sits in the slot and observes nothing
                obs.append((pid, j, kp))
                if r > 0.70:                                        # seen from a second keyframe too: the keypoint of the same world point, if free
                    for j2 in rng.permutation(n_kf):
                        hit = np.nonzero(src[j2] == w)[0]
                        if j2 != j and len(hit) and mps[j2][hit[0]] < 0:
                            mps[j2][hit[0]] = pid
                            obs.append((pid, int(j2), int(hit[0])))
                            break
        for i in range(n):                                          # list points seen from the extra observer as well (more observations than a slot's point)
            hit = np.nonzero(src[n_targets + 1] == lw[i])[0]
            if len(hit) and mps[n_targets + 1][hit[0]] < 0 and rng.random() < 0.7:
                mps[n_targets + 1][hit[0]] = i
                obs.append((i, n_targets + 1, int(hit[0])))
        m = len(others_bad)
        full = {k: np.concatenate([np.asarray(v), np.zeros((m,) + np.shape(v)[1:], np.asarray(v).dtype)]) for k, v in P.items()}
        full["bad"] = np.concatenate([(case >= 0.97).astype(np.uint8), np.array(others_bad, np.uint8)])      # a few bad list points
        obs = [o for o in obs if not full["bad"][o[0]]]            # (a bad point keeps its slots and observes nothing, as after SetBadFlag's clear)
        lst = np.arange(n)
        lst = np.where((case >= 0.94) & (case < 0.97), -1, lst)                                    # NULL entries (the reference's vector holds every slot)
        full["Pz"][n:] = 4.0
        full["Nz"][n:] = 1.0
        # distance ranges: maxd predicts the world point's level; redrawn until no pair's level depends on the logf in use
        level = wlevel[lw].astype(F64)
        jitter = rng.uniform(-0.35, 0.35, n)
        far, near = (case >= 0.10) & (case < 0.13), (case >= 0.13) & (case < 0.16)
        c = None
        for attempt in range(200):
            maxd = (dist * 1.2 ** (level - 0.5 + jitter)).astype(np.float32)
            maxd[far] = (dist[far] * 0.7).astype(np.float32)                                      # 1.2 maxd < dist
            mind = (maxd / f32(prm["scale"][-1])).astype(np.float32)
            mind[near] = (dist[near] * 1.5).astype(np.float32)                                    # 0.8 mind > dist
            full["maxd"], full["mind"] = np.concatenate([maxd, np.ones(m, np.float32)]), np.concatenate([mind, np.ones(m, np.float32)])
            c = fuse_case(prm, kfs, poses, full, mps, obs, targets=np.arange(n_targets), lst=lst)
            try:
                prove_exact(c)
                break
            except LevelMargin as e:                                # (.indices: point ids; the list points are ids 0 .. n-1)
                jitter[e.indices] = rng.uniform(-0.35, 0.35, len(e.indices))
        else:
            raise AssertionError("no distance ranges found")
        return c

    @classmethod
    def build(cls, po):
        out = OrderedDict()
        # (descriptors do not compress: one call of the workload's shape per block - 5 targets x 150 points x 300 keypoints, half of them stereo -
        # and small ones for th 4, all-stereo and all-monocular keyframes, the point counts around a workgroup's 16 and one call that crosses
        # FUSE_KF_CHUNK = 32 keyframes)
        edge = dict(th=3, n_targets=2, N=40, n_world=40)
        shapes = [cls.main_shape, dict(th=4, stereo=1.0, n_targets=3, n=50, N=100), dict(th=3, stereo=0.0, n_targets=3, n=50, N=100), dict(edge, n=1), dict(edge, n=15),
                  dict(edge, n=16), dict(edge, n=17), dict(th=3, n_targets=33, n=32, N=32, n_world=48)]
        for b in range(2):
            rng = np.random.default_rng(7700 + b + 10 * cls.check)
            for k, kw in enumerate(shapes):
                if b and k == 0:
                    kw = dict(kw, n=kw.get("n", 150) - 10, N=kw.get("N", 300) - 40)      # (the second block's large call: other sizes)
                out["random%d.%02d" % (b, k)] = cls.finish(cls.random_block(rng, **kw))
        out.update(cls.constructed(po))
        return out

    @classmethod
    def finish(cls, c):
        return c

    # ---- constructed cases ----
    @classmethod
    def constructed(cls, po):
        out = OrderedDict()
        for name in cls.NAMES_FROM_HOST_TEST:
            K, pose, P, prm, want = tf.CONSTRUCTED[name]
            P = dict(P)
            n = len(P["Px"])
            if not name.startswith("dot_"):                          # the host test's normals point along the ray (inexact products): straight ahead here
                P["Nx"], P["Ny"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
                P["Nz"] = np.where(np.asarray(P["Pz"]) < 0, -1, 1).astype(np.float32)
            if name == "depth_zero_and_negative":                    # (maxd = 0.9 dist is 0 at the origin, which ends at IsInImage anyway)
                P["maxd"] = np.where(np.asarray(P["maxd"]) > 0, P["maxd"], 1).astype(np.float32)
            out[name] = cls.finish(fuse_case(dict(prm, check=cls.check), [K], [pose], P))
            out[name]["want"] = np.asarray(want, np.int64)
        prm = tf.default_params(check=cls.check, th=f32(3 if cls.check else 4))
        at = lambda uv, **kw: dict(tf.points_at(uv, prm, **kw), Nx=np.zeros(len(uv), np.float32), Ny=np.zeros(len(uv), np.float32), Nz=np.ones(len(uv), np.float32))
        # the distance range: dist3D equal to each invariance bound is inside, one ulp beyond is not.  (0, 0, 4) is at distance 4 exactly.
        P = at([(160, 120)] * 4)
        d = f32(4)
        P["mind"] = mind_for(np.array([d, np.nextafter(d, f32(8)), 0, 0], np.float32))
        top = maxd_for(d)
        P["maxd"] = np.array([top, top, top, np.nextafter(top, f32(0))], np.float32)
        assert f32(f32(1.2) * P["maxd"][3]) < d
        out["dist3D_at_both_bounds"] = cls.finish(fuse_case(prm, [tf.kps([(160, 120, 0, 10)], prm)], [tf.IDENTITY], P))
        out["dist3D_at_both_bounds"]["want"] = np.array([0, -1, 0, -1], np.int64)
        if cls.check:
            kx, ky = chi_square_at_float_5_99()
            out["chi_square_at_float_5_99"] = cls.finish(fuse_case(prm, [tf.kps([(kx, ky, 0, 10)], prm)], [tf.IDENTITY], at([(100, 100)])))
            out["chi_square_at_float_5_99"]["want"] = np.array([0], np.int64)
        # u == max_x and v == max_y exactly, with a keypoint that would be taken were the gate closed: on level 1 (radius 3.6, sigma2 1.44) the keypoint
        # 2.6 px inside passes the chi-square test, which on level 0 hides what u_at_max_x_is_out is about
        for nm, kp, uv in (("u_at_max_x_with_a_candidate", (317.4, 100, 1, 10), (320, 100)), ("v_at_max_y_with_a_candidate", (100, 237.4, 1, 10), (100, 240))):
            out[nm] = cls.finish(fuse_case(prm, [tf.kps([kp], prm)], [tf.IDENTITY], at([uv, (uv[0] - (nm[0] == "u"), uv[1] - (nm[0] == "v"))], level=1)))
            out[nm]["want"] = np.array([-1, 0], np.int64)
        # an empty keyframe among the targets
        K = tf.kps([(100, 100, 0, 10)], prm)
        out["empty_keyframe_between_two"] = cls.finish(fuse_case(prm, [K, tf.kps([], prm), K], [tf.IDENTITY] * 3, at([(100, 100), (101, 100)])))
        out.update(cls.tail_cases(prm, at))
        return out

    @classmethod
    def tail_cases(cls, prm, at):
        """every branch of :938-958 on identity poses (all keyframes see a point at the same pixel), keypoints at distance bits from the zero descriptor"""
        out = OrderedDict()
        I = tf.IDENTITY
        holder = lambda d, n=4, st=(): tf.kps([(40 + 20 * i, 200, 0, d[i] if i < len(d) else 200) + ((30.0 + 20 * i,) if i in st else ()) for i in range(n)], prm)
        # 1. one target keyframe, eight list entries
        T = tf.kps([(100, 100, 0, 10), (120, 100, 0, 10), (140, 100, 0, 10), (160, 100, 0, 10), (180, 100, 0, 10), (200, 100, 0, 10), (220, 100, 0, 10)], prm)
        cur = holder([0] * 8, 8, st=(2,))                          # keypoint 2 of the current keyframe is a stereo one: its observation counts 2
        oth = holder([0] * 8, 8)
        oth2 = holder([0] * 8, 8)
        P = at([(100, 100), (120, 100), (140, 100), (160, 100), (180, 100), (200, 100), (220, 100), (100, 100)] + [(10, 10)] * 4)
        P["bad"] = np.array([0, 0, 0, 0, 0, 1, 0, 0] + [0, 0, 0, 1], np.uint8)
        # ids 8, 9, 10: the points in T's slots 0, 1, 2 with more / as many / fewer observations than the list point; 11: a bad one in slot 3
        # (point 9 is also in keyframe 3, where point 1 is already: that slot is emptied when 1 takes 9's place)
        mps = [[8, 9, 10, 11, -1, -1, 6], list(range(8)), [8, -1, -1, -1, -1, -1, -1, -1], [8, 1, 9, -1, -1, -1, -1, -1]]
        obs = [(i, 1, i) for i in range(8) if i != 5] + [(8, 0, 0), (8, 2, 0), (8, 3, 0), (9, 0, 1), (9, 3, 2), (1, 3, 1), (10, 0, 2), (6, 0, 6)]
        out["tail_every_branch"] = cls.finish(fuse_case(prm, [T, cur, oth, oth2], [I] * 4, P, mps, obs, targets=[0], lst=[0, 1, 2, 3, 4, 5, 6, -1]))
        # 2. a point enters keyframe 1 through the Replace of keyframe 0: its head test there flips to skip, though the search finds a keypoint
        A, B = tf.kps([(100, 100, 0, 10)], prm), tf.kps([(100, 100, 0, 12), (40, 40, 0, 10)], prm)
        P2 = at([(100, 100), (10, 10)])
        out["enters_a_later_keyframe_by_replace"] = cls.finish(fuse_case(prm, [A, B, holder([0])], [I] * 3, P2, [[1], [-1, 1], [0, -1, -1, -1]],
                                                                       [(0, 2, 0), (1, 0, 0), (1, 1, 1)], targets=[0, 1], lst=[0]))
        # 3. what the issue is about: point 0 (descriptor bits 0, seen from the current keyframe 2 and from 3) finds in keyframe 0 the keypoint of
        # point 1 (as many observations: point 1 is replaced by point 0), inherits its observations (bits 20 in keyframe 0, bits 22 in 4) and its
        # descriptor becomes bits 20, the first of the two with the least median distance.  In keyframe 1 the old descriptor chooses keypoint 0
        # (bits 5), the new one keypoint 1 (bits 24).
        out.update(cls.descriptor_cases(prm, at))
        return out

    @classmethod
    def descriptor_cases(cls, prm, at, **kw):
        I = tf.IDENTITY
        k0, k1 = tf.kps([(100, 100, 0, 20)], prm), tf.kps([(100, 100, 0, 5), (101, 100, 0, 24)], prm)
        cur, far, far2 = tf.kps([(100, 100, 0, 0)], prm), tf.kps([(100, 100, 0, 60)], prm), tf.kps([(100, 100, 0, 22)], prm)
        P = at([(100, 100), (10, 10)])
        c = fuse_case(prm, [k0, k1, cur, far, far2], [I] * 5, P, [[1], [-1, -1], [0], [0], [1]], [(0, 2, 0), (0, 3, 0), (1, 0, 0), (1, 4, 0)], targets=[0, 1],
                      lst=[0], **kw)
        # the same with a third target that the changed point must be searched in again, and a second list point whose descriptor never changes
        k2 = tf.kps([(100, 100, 0, 3), (99, 100, 0, 26), (140, 100, 0, 10)], prm)
        P2 = at([(100, 100), (10, 10), (140, 100)])
        kw2 = dict(kw, Scw=np.concatenate([kw["Scw"], kw["Scw"][:16]])) if kw else kw
        c2 = fuse_case(prm, [k0, k1, k2, cur, far, far2], [I] * 6, P2, [[1], [-1, -1], [-1, -1, -1], [0, ], [0], [1]],
                       [(0, 3, 0), (0, 4, 0), (1, 0, 0), (1, 5, 0)], targets=[0, 1, 2], lst=[0, 2], **kw2)
        return OrderedDict([("descriptor_changes_between_keyframes", cls.finish(c)), ("descriptor_changes_three_keyframes", cls.finish(c2))])

    @staticmethod
    def verify(po, c):
        """the exactness proof; the sequential replay of the transcription is the reference's run, event for event; and the reference's probe log -
        the pixel, distance, level and radius its own ORBmatcher.cpp handed over - equals the contract's values bit for bit.  (Where Pcz == 0 the
        reference reaches IsInImage with a non-finite pixel and the contract stops before: those rows are not the contract's.)"""
        prove_exact(c)
        seq, _, _ = fuse_replay.replay(c, fuse_search(po, c), "sequential")
        fuse_replay.same_map(seq, c["out"])
        ref = split_probe(c["_driver"], c.get("_name"), c["out"]["probe"])      # (asserts how many non-finite rows a Pcz == 0 leaves: STATED_DIFFERENCES)
        assert ref.shape == seq["probe"].shape and ref.tobytes() == seq["probe"].tobytes(), "u, v, dist3D, level or radius differ from the contract's"

    # ---- the yardsticks ----
    @staticmethod
    def transcription(po, c):
        return fuse_replay.replay(c, fuse_search(po, c, "transcription"), "research")

    @staticmethod
    def restatement(po, c):
        return fuse_replay.replay(c, fuse_search(po, c, "restatement"), "research")

    @staticmethod
    def counters(po, c, tr):
        """the gate trace and the tail's branches of the sequential replay, and the statistics of the device calls of the contract's replay"""
        seq, trace = sequential_run(po, c)
        ev = seq["events"]
        lst = set(int(p) for p in c["list"] if p >= 0)
        rep = ev[ev[:, 0] == fuse_replay.EV_REPLACE]
        batched = fuse_replay.replay(c, fuse_search(po, c, "transcription"), "batched")
        flips = int((tr[2][0] >= 0).sum()) - int(tr[0]["nmatches"])      # pairs the search has a keypoint for and the live head test skips
        d = {g: int(trace.get(g, 0)) for g in tf.GATES}
        d.update(matches=int(seq["nmatches"]), replace_to_kf=int(sum(int(r[1]) in lst for r in rep)), replace_to_list=int(sum(int(r[2]) in lst for r in rep)),
                 added=int((ev[:, 0] == fuse_replay.EV_ADD_MAP_POINT).sum()), bad_in_kf=int(seq["nmatches"]) - len(rep) - int((ev[:, 0] == fuse_replay.EV_ADD_MAP_POINT).sum()),
                 head_flips=flips, descriptor_changes=int((ev[:, 0] == fuse_replay.EV_DESCRIPTOR).sum()),
                 calls=np.asarray(tr[1], np.int64).reshape(-1, 4), differs_without_research=int(not _same(batched[0], seq)))
        return d

    @staticmethod
    def same(c, res):
        fuse_replay.same_map(res[0], c["out"])
        if "want" in c:                                            # a constructed case of the host test: the best_idx it is about
            assert np.array_equal(res[2][0][0], c["want"])


def _same(a, b):
    try:
        fuse_replay.same_map(a, b)
        return True
    except AssertionError:
        return False


def chi_square_at_float_5_99():
    """a monocular keypoint next to u = v = 100 whose ex*ex + ey*ey is exactly (float)5.99 = 5.98999977..., below the double 5.99: kept"""
    rng = np.random.default_rng(21)
    u, v, want = f32(100), f32(100), f32(5.99)
    for _ in range(200000):
        kx = f32(100 - rng.uniform(0.5, 1.5))
        ex = f32(u - kx)
        ey0 = f32(np.sqrt(f32(want - f32(ex * ex))))
        for step in range(-3, 4):
            ky = f32(v - ey0)
            for _ in range(abs(step)):
                ky = np.nextafter(ky, f32(np.inf) if step > 0 else f32(-np.inf))
            ey = f32(v - ky)
            if f32(f32(ex * ex) + f32(ey * ey)) == want:
                return kx, ky
    raise AssertionError("no keypoint found")


class FuseSim3(Fuse):
    driver = "fuse_sim3"
    required = tuple(g for g in tf.GATES if g != "chi") + ("matches", "replace_to_list", "added", "bad_in_kf", "descriptor_changes")
    NAMES_FROM_HOST_TEST = tuple(n for n in Fuse.NAMES_FROM_HOST_TEST if "_6_5" not in n and "8_75" not in n and "chi_" not in n and "contraction" not in n
                                 and n != "mono_beats_nothing_stereo_wins") + ("no_reprojection_gate",)
    check = 0
    main_shape = dict(th=4, n=110, N=220)                           # (loop closing runs th = 4)

    @classmethod
    def finish(cls, c):
        """through the overload with Scw: per target Scw = s [R | t] with s = 1, 2, 1/2 in turn, SearchAndFuse's Replace loop after every call; the
        list holds no NULL entry"""
        if "Scw" in c:
            return c
        lst = np.asarray(c["list"])
        c["list"] = np.where(lst < 0, np.flatnonzero(np.asarray(c["P"]["bad"]) != 0)[0] if (lst < 0).any() else 0, lst).astype(np.int32)
        c["Scw"] = np.stack([scw_of((c["KF"][int(k)]["Rcw"], c["KF"][int(k)]["tcw"], None), (1.0, 2.0, 0.5)[t % 3]) for t, k in enumerate(c["targets"])]
                            + [np.zeros(16, np.float32)])[:len(c["targets"])]
        c["replace_loop"] = np.int64(1)
        return c

    @classmethod
    def tail_cases(cls, prm, at):
        out = OrderedDict()
        I = tf.IDENTITY
        S = np.concatenate([scw_of(I, 2.0), scw_of(I, 0.5)])
        out.update(cls.descriptor_cases(prm, at, Scw=S, replace_loop=1))
        # the same map without the caller's loop: vpReplacePoint is all the overload returns
        c = cls.descriptor_cases(prm, at, Scw=S, replace_loop=0)["descriptor_changes_between_keyframes"]
        out["replace_points_without_the_loop"] = c
        return out


# ------------------------------------------------------------------ SearchBySim3
def sim3_case(prm, K1, K2, poses, P, slots1, slots2, matches12, s12, R12, t12, obs=(), bad=None):
    """a case of the search_by_sim3 file: two keyframes (tests/test_fuse_host.py's keyframe) with their poses (Rcw, tcw), one point table (Px ..
    Pz, maxd, mind, desc, bad), the keyframes' slots and the pre-filled vpMatches12 as point ids (-1: NULL), the observations GetIndexInKeyFrame
    reads as (point, keyframe, keypoint) rows, and the similarity"""
    n = len(P["Px"])
    P = dict(P)
    if "mind" not in P:
        P["mind"] = mind_for(P["mindi"])
    P["mindi"], P["maxdi"] = (f32(0.8) * np.asarray(P["mind"], np.float32)).astype(np.float32), (f32(1.2) * np.asarray(P["maxd"], np.float32)).astype(np.float32)
    P["bad"] = np.zeros(n, np.uint8) if bad is None else np.asarray(bad, np.uint8)
    P = {k: np.asarray(v, np.uint8 if k in ("bad", "desc") else np.float32) for k, v in P.items() if k in ("Px", "Py", "Pz", "maxd", "mind", "mindi", "maxdi", "desc", "bad")}
    P["desc"] = P["desc"].reshape(n, 32)
    KF = [dict(x=K["x"], y=K["y"], octave=K["octave"], desc=K["desc"], Rcw=np.asarray(R, np.float32).ravel(), tcw=np.asarray(t, np.float32),
               mps=np.asarray(sl, np.int32).reshape(len(K["x"]))) for K, (R, t), sl in zip((K1, K2), poses, (slots1, slots2))]
    c = dict(KF=KF, P=P, prm={k: v for k, v in prm.items()}, obs=np.asarray(obs, np.int32).reshape(-1, 3), matches12=np.asarray(matches12, np.int32).reshape(len(K1["x"])),
             s12=f32(s12), R12=np.asarray(R12, np.float32).ravel(), t12=np.asarray(t12, np.float32))
    return with_grids(c)


def sim3_sides(c, mutant=None):
    """the case as the contract's two sides (tests/test_loop_host.py: sim3_side): per slot its point's arrays, the search flag - a live point whose
    slot is not matched already (:1119-1129, :1139-1143, :1219-1223) - and the pose with the similarity into the other camera as the reference
    derives it (:1106-1108), in float32 like its cv::Mat products"""
    P, m12 = c["P"], np.asarray(c["matches12"])
    n1, n2 = len(c["KF"][0]["x"]), len(c["KF"][1]["x"])
    in_kf2 = {int(p): int(i) for p, k, i in np.asarray(c["obs"]).reshape(-1, 3) if k == 1}
    matched2 = np.zeros(n2, bool)
    for p in m12[m12 >= 0]:
        idx2 = in_kf2.get(int(p), -1)
        if 0 <= idx2 < n2 and mutant != "ignore_matched2":
            matched2[idx2] = True
    s, R12, t12 = f32(c["s12"]), np.asarray(c["R12"], np.float32).reshape(3, 3), np.asarray(c["t12"], np.float32)
    sR12 = (s * R12).astype(np.float32)
    sR21 = (f32(f32(1) / s) * R12.T).astype(np.float32)
    t21 = np.array([f32(f32(f32(-sR21[r, 0] * t12[0]) + f32(-sR21[r, 1] * t12[1])) + f32(-sR21[r, 2] * t12[2])) for r in range(3)], np.float32)
    sides = []
    for k, (sR, t, taken) in enumerate(((sR21, t21, m12 >= 0), (sR12, t12, matched2))):
        K = c["KF"][k]
        slots = np.asarray(K["mps"], np.int64)
        sel = np.maximum(slots, 0)
        Ps = {a: np.asarray(P[a])[sel] if len(P["Px"]) else np.asarray(P[a])[:0] for a in ("Px", "Py", "Pz", "maxd", "mindi", "maxdi", "desc")}
        search = (slots >= 0) & (np.asarray(P["bad"])[sel] == 0 if len(P["Px"]) else np.zeros(len(slots), bool)) & ~taken
        sides.append(tl.sim3_side(dict(K, start=K["_start"], items=K["_items"]), Ps, search, dict(Rw=K["Rcw"], tw=K["tcw"], sR=sR.ravel(), t=t)))
    return sides


def prove_exact_sim3(c):
    """prove_exact for the two directions of SearchBySim3: the chain own = Rw P + tw, Pc = sR own + t (and sR21, t21 themselves), the pixel and
    dist3D^2 = |Pc|^2 are exact in float32 for every searched slot that reaches them, and no level depends on the logf in use"""
    prm = c["prm"]
    s, R12, t12 = float(c["s12"]), np.asarray(c["R12"], F64).reshape(3, 3), np.asarray(c["t12"], F64)
    _ex(1.0 / s, "1 / s12"), _ex(s * R12, "s12 R12")
    sR21 = _ex((1.0 / s) * R12.T, "sR21")
    for r in range(3):
        _ex(_ex(_ex(-sR21[r, 0] * t12[0], "t21") + _ex(-sR21[r, 1] * t12[1], "t21"), "t21") + _ex(-sR21[r, 2] * t12[2], "t21"), "t21")
    pairs = 0
    for side, S in enumerate(sim3_sides(c)):
        live = S["search"] != 0
        x, y, z = (S["P"][k].astype(F64)[live] for k in ("Px", "Py", "Pz"))
        with np.errstate(all="ignore"):
            def chain(R, t, x, y, z, what):
                out = []
                for r in range(3):
                    a, b, d = _ex(x * R[3 * r], what), _ex(y * R[3 * r + 1], what), _ex(z * R[3 * r + 2], what)
                    out.append(_ex(_ex(_ex(a + b, what) + d, what) + t[r], what))
                return out
            own = chain(S["Rw"].astype(F64), S["tw"].astype(F64), x, y, z, "Rw P + tw")
            Pc = chain(S["sR"].astype(F64), S["t"].astype(F64), *own, "sR own + t")
            front = Pc[2] > 0
            invz = _ex(np.where(front, 1.0 / np.where(front, Pc[2], 1.0), 0.0), "1 / Pcz")
            uv = []
            for Pa, f, cc in ((Pc[0], float(prm["fx"]), float(prm["cx"])), (Pc[1], float(prm["fy"]), float(prm["cy"]))):
                Pa = np.where(front, Pa, 0.0)
                _ex(Pa * f, "Pc * f")
                uv.append(_ex(_ex(f * _ex(Pa * invz, "X * invz"), "f * x") + cc, "f * x + c"))
            u, v = uv
            inside = front & (u >= float(prm["min_x"])) & (u <= float(prm["max_x"])) & (v >= float(prm["min_y"])) & (v <= float(prm["max_y"]))
            o = [np.where(inside, a, 0.0) for a in Pc]
            d2 = _ex(_ex(_ex(o[0] * o[0], "x^2") + _ex(o[1] * o[1], "y^2"), "x^2 + y^2") + _ex(o[2] * o[2], "z^2"), "dist^2")
            slots = np.asarray(c["KF"][side]["mps"], np.int64)
            pairs += check_levels(prm, S["P"]["maxd"][live], np.sqrt(d2).astype(np.float32), inside, slots[live])
    return pairs


class SearchBySim3(Matcher):
    driver = "search_by_sim3"
    required = tl.SIM3_GATES + ("disagree", "matches", "prefilled", "matched2")
    prepare = staticmethod(with_grids)

    @staticmethod
    def random_case(rng, n1=150, n2=170, s12=1.0, th=7.5):
        """tests/test_loop_host.py's random_sim3_case on exact inputs: both cameras look along world z (a turn about z by a multiple of 90 degrees, a
        shift by multiples of 1/16), R12 such a turn too, t12 a shift in x, y, s12 a power of two; a slot's point is back-projected from a keypoint of
        the OTHER keyframe (a quarter pixel off or more) at depth 2, 4 or 8 in that camera; three quarters of the slots are paired mutually"""
        prm = tl.sim3_params(th=f32(th))
        n_levels = len(prm["scale"])
        shift = lambda: np.array([rng.integers(-4, 5) / 16.0, rng.integers(-4, 5) / 16.0, 0.0])
        R12, t12 = ROT_Z[int(rng.integers(0, 4))].astype(F64).reshape(3, 3), shift()
        sR12, sR21 = s12 * R12, (1.0 / s12) * R12.T
        t21 = -sR21 @ t12
        Rw = [ROT_Z[int(rng.integers(0, 4))].astype(F64).reshape(3, 3) for _ in range(2)]
        tw = [shift(), shift()]
        Ks = []
        for N in (n1, n2):
            Ks.append(tf.keyframe(rng.integers(4 * 4, 4 * 316, N) / 4.0, rng.integers(4 * 4, 4 * 236, N) / 4.0, rng.integers(0, n_levels, N),
                                  np.concatenate([rng.integers(0, 256, (N, 16), dtype=np.uint8), np.zeros((N, 16), np.uint8)], 1), prm))
        m = min(n1, n2)
        pi = rng.permutation(n2)[:m]
        target = [rng.integers(0, max(n2, 1), n1), rng.integers(0, max(n1, 1), n2)]
        mutual = rng.random(m) < 0.75
        target[0][:m][mutual] = pi[mutual]
        target[1][pi[mutual]] = np.arange(m)[mutual]
        parts = []
        for side, (sR, t) in enumerate(((sR21, t21), (sR12, t12))):
            O, n = Ks[1 - side], len(target[side])
            if len(O["x"]) == 0:
                O = dict(x=np.full(1, 160, np.float32), y=np.full(1, 120, np.float32), octave=np.zeros(1, np.int64), desc=np.zeros((1, 32), np.uint8))
            tg = target[side] % len(O["x"])
            px = O["x"][tg].astype(F64) + rng.integers(-2, 3, n) / 4.0
            py = O["y"][tg].astype(F64) + rng.integers(-2, 3, n) / 4.0
            z = rng.choice([2.0, 4.0, 8.0], n)
            case = rng.random(n)
            z = np.where(case < 0.05, -z, z)
            px = np.where((case >= 0.05) & (case < 0.10), px + 400, px)
            Pc = np.stack([(px - 160.0) * z / 256.0, (py - 120.0) * z / 256.0, z])
            own = np.linalg.inv(sR) @ (Pc - t[:, None])
            Pw = Rw[side].T @ (own - tw[side][:, None])
            dist = np.sqrt((Pc * Pc).sum(0))
            level = O["octave"][tg].astype(np.int64) + rng.integers(0, 2, n)
            level = np.clip(np.where((case >= 0.20) & (case < 0.30), level + 3, level), 0, n_levels - 1).astype(F64)
            desc = O["desc"][tg].copy()
            flips = np.where(case >= 0.88, rng.integers(101, 140, n), rng.integers(0, 45, n))
            for i in range(n):
                b = rng.choice(256, int(flips[i]), replace=False)
                np.bitwise_xor.at(desc[i], b // 8, (1 << (7 - b % 8)).astype(np.uint8))
            parts.append(dict(Pw=Pw, dist=dist, level=level, case=case, desc=desc))
        n = n1 + n2
        P = dict(Px=np.concatenate([p["Pw"][0] for p in parts]).astype(np.float32), Py=np.concatenate([p["Pw"][1] for p in parts]).astype(np.float32),
                 Pz=np.concatenate([p["Pw"][2] for p in parts]).astype(np.float32), desc=np.concatenate([p["desc"] for p in parts]))
        dist, level, case = (np.concatenate([p[k] for p in parts]) for k in ("dist", "level", "case"))
        state = rng.random(n)
        slots = np.where(state < 0.05, -1, np.arange(n))                                          # NULL slots
        bad = ((state >= 0.05) & (state < 0.10)).astype(np.uint8)                                   # bad points
        slots1, slots2 = slots[:n1], slots[n1:]
        # the pre-filled vpMatches12: points of keyframe 2's slots (GetIndexInKeyFrame in range: that slot is not searched), three extra points
        # that keyframe 2 does not observe (-1) and three that it observes at an index of at least N2
        extra = 6 if n1 >= 12 and n2 else 0
        matches12 = np.full(n1, -1, np.int64)
        obs = [(int(p), 1, j) for j, p in enumerate(slots2) if p >= 0 and not bad[p]]
        if extra:
            pre = rng.choice(n1, 12, replace=False)
            ok2 = [j for j, p in enumerate(slots2) if p >= 0 and not bad[p]]
            matches12[pre[:6]] = [slots2[j] for j in rng.choice(ok2, 6, replace=False)] if len(ok2) >= 6 else n + np.arange(6) % 3
            matches12[pre[6:]] = n + np.arange(6)
            obs += [(n + 3 + j, 1, n2 + j) for j in range(3)]
            P = {k: np.concatenate([v, np.zeros((extra,) + v.shape[1:], v.dtype)]) for k, v in P.items()}
            bad = np.concatenate([bad, np.zeros(extra, np.uint8)])
        jitter = rng.uniform(-0.35, 0.35, n)
        far, near = (case >= 0.10) & (case < 0.13), (case >= 0.13) & (case < 0.16)
        poses = [(Rw[0], tw[0]), (Rw[1], tw[1])]
        for attempt in range(200):
            maxd = (dist * 1.2 ** (level - 0.5 + jitter)).astype(np.float32)
            maxd[far] = (dist[far] * 0.7).astype(np.float32)
            mind = (maxd / f32(prm["scale"][-1])).astype(np.float32)
            mind[near] = (dist[near] * 1.5).astype(np.float32)
            P["maxd"], P["mind"] = np.concatenate([maxd, np.ones(extra, np.float32)]), np.concatenate([mind, np.ones(extra, np.float32)])
            c = sim3_case(prm, Ks[0], Ks[1], poses, P, slots1, slots2, matches12, s12, R12, t12, obs, bad)
            try:
                prove_exact_sim3(c)
                return c
            except LevelMargin as e:                                # (.indices: point ids, which are the positions of jitter)
                jitter[e.indices] = rng.uniform(-0.35, 0.35, len(e.indices))
        raise AssertionError("no distance ranges found")

    @classmethod
    def build(cls, po):
        out = OrderedDict()
        for b, s12 in enumerate((1.0, 2.0, 0.5)):
            rng = np.random.default_rng(7900 + b)
            out["random%d.00" % b] = cls.random_case(rng, s12=s12)
            for k, n1 in enumerate((1, 15, 16, 17)):                # the slot counts of tests/test_gpu_loop.py around a workgroup's 16
                out["random%d.%02d" % (b, k + 1)] = cls.random_case(rng, n1=n1, n2=60, s12=s12)
        out.update(cls.constructed())
        return out

    @staticmethod
    def constructed():
        """both cameras at the origin, the similarity the identity: a slot's point at depth 4 behind pixel (u, v) is searched around (u, v) in the other
        keyframe.  A keyframe is rows (x, y, octave, bits of its descriptor), a side's points rows (u, v, level, bits) or None per slot.  `want`: the new
        entries of vpMatches12 as keypoints of keyframe 2."""
        prm = tl.sim3_params()
        out = OrderedDict()

        def case(k1, p1, k2, p2, want, pre=None, extra_obs=(), n_extra=0):
            rows = [r for r in list(p1) + list(p2)]
            live = [tuple(r) + (4.0,)[len(r) - 4:] if r is not None else (10, 10, 0, 0, 4.0) for r in rows]      # (an optional fifth entry: the depth)
            P = tf.points_at([r[:2] for r in live], prm, z=[r[4] for r in live], level=[r[2] for r in live], dbits=[r[3] for r in live])
            P["maxd"] = np.where(np.isfinite(P["maxd"]) & (P["maxd"] > 0), P["maxd"], 1).astype(np.float32)
            P["mindi"] = (P["maxd"] * f32(0.1)).astype(np.float32)
            P = {k: np.concatenate([np.asarray(v), np.zeros((n_extra,) + np.shape(v)[1:], np.asarray(v).dtype)]) for k, v in P.items()}
            P["maxd"][len(rows):], P["mindi"][len(rows):] = 1, 0
            ids = np.array([i if r is not None else -1 for i, r in enumerate(rows)])
            slots1, slots2 = ids[:len(p1)], ids[len(p1):]
            obs = [(int(q), 1, j) for j, q in enumerate(slots2) if q >= 0] + list(extra_obs)
            I = (np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
            c = sim3_case(prm, tf.kps(k1, prm), tf.kps(k2, prm), [I, I], P, slots1, slots2, np.full(len(p1), -1) if pre is None else pre, 1.0,
                          np.eye(3), np.zeros(3), obs)
            c["want"] = np.asarray(want, np.int64)
            return c
        A, B = (100, 100, 0, 10), (200, 100, 0, 10)
        # slot 0 of keyframe 1 finds keypoint 0 of keyframe 2 and is found by it
        out["mutual"] = case([A], [(100, 100, 0, 0)], [A], [(100, 100, 0, 0)], [0])
        # ... finds it, but that keypoint's point finds keypoint 1 of keyframe 1: agreement one way only
        out["agrees_one_way_only"] = case([A, B], [(100, 100, 0, 0), None], [A], [(200, 100, 0, 0)], [-1, -1])
        # bestDist == TH_HIGH is a match, one more is not (descriptor bits 0 against 100 and 101)
        out["th_high_accepted"] = case([(100, 100, 0, 100)], [(100, 100, 0, 0)], [(100, 100, 0, 100)], [(100, 100, 0, 0)], [0])
        out["th_high_plus_one_not"] = case([(100, 100, 0, 100)], [(100, 100, 0, 0)], [(100, 100, 0, 101)], [(100, 100, 0, 0)], [-1])
        # equal distances at two walk positions: the first wins, and only its point agrees
        out["tie_first_in_walk_order"] = case([A], [(100, 100, 0, 0)], [(101, 100, 0, 10), (99, 100, 0, 10)], [(100, 100, 0, 0), None], [0])
        # octaves L-1, L and L+1 around level 2 (the points of keyframe 2 find their keypoint of keyframe 1 at level 0)
        k1 = [(60, 100, 0, 10), (100, 100, 0, 10), (140, 100, 0, 10)]
        out["octaves_around_the_level"] = case(k1, [(60, 100, 2, 0), (100, 100, 2, 0), (140, 100, 2, 0)], [(60, 100, 1, 10), (100, 100, 2, 10), (140, 100, 3, 10)],
                                               [(60, 100, 0, 0), (100, 100, 0, 0), (140, 100, 0, 0)], [0, 1, -1])
        # u == max_x exactly is outside (half open), one pixel less inside, with a keypoint that a closed gate would give
        out["u_at_max_x_with_a_candidate"] = case([(40, 100, 0, 10), (40, 140, 0, 10)], [(320, 100, 0, 0), (319, 140, 0, 0)], [(317.4, 100, 0, 10), (317.4, 140, 0, 10)],
                                                  [(40, 100, 0, 0), (40, 140, 0, 0)], [-1, 1])
        out["u_at_min_x_is_in"] = case([(300, 100, 0, 10), (300, 140, 0, 10)], [(0, 100, 0, 0), (-0.25, 140, 0, 0)], [(2, 100, 0, 10), (2, 140, 0, 10)],
                                       [(300, 100, 0, 0), (300, 140, 0, 0)], [0, -1])       # (a quarter pixel outside: rejected)
        # Pcz == 0 and Pcz < 0 have no candidate (:1150; at 0 the reference's pixel is not finite: STATED_DIFFERENCES)
        three = [(100, 100, 0, 10), (200, 100, 0, 10), (60, 60, 0, 10)]
        out["depth_zero_and_negative"] = case(three, [(100, 100, 0, 0), (200, 100, 0, 0, 0.0), (60, 60, 0, 0, -4.0)], three,
                                              [(100, 100, 0, 0), (200, 100, 0, 0), (60, 60, 0, 0)], [0, -1, -1])
        # dist3D equal to each invariance bound is inside, one ulp beyond is not: four slots behind the principal point (dist 4), told apart by
        # their descriptors (bits 0, 30, 60, 90), each agreeing with the keypoint of keyframe 2 that has its bits
        k4 = [(160 + i, 120, 0, 30 * i) for i in range(4)]
        c = case(k4, [(160, 120, 0, 30 * i) for i in range(4)], k4, [(160 + i, 120, 0, 30 * i) for i in range(4)], [0, -1, 2, -1])
        top = maxd_for(f32(4))
        c["P"]["mind"][:4] = mind_for(np.array([4, np.nextafter(f32(4), f32(8)), 0, 0], np.float32))
        c["P"]["maxd"][:4] = [top, top, top, np.nextafter(top, f32(0))]
        c["P"]["mindi"], c["P"]["maxdi"] = (f32(0.8) * c["P"]["mind"]).astype(np.float32), (f32(1.2) * c["P"]["maxd"]).astype(np.float32)
        out["dist3D_at_both_bounds"] = c
        # vbAlreadyMatched2 through GetIndexInKeyFrame: vpMatches12[1] holds the point of keyframe 2's slot 0, so that slot is not searched and slot 0
        # of keyframe 1 finds no agreement; with an index of at least N2, or none, nothing is blocked
        two = [A, (40, 40, 0, 200)]
        out["already_matched2_in_range"] = case(two, [(100, 100, 0, 0), None], [A], [(100, 100, 0, 0)], [-1, -1], pre=[-1, 2])
        out["already_matched2_index_at_least_n2"] = case(two, [(100, 100, 0, 0), None], [A], [(100, 100, 0, 0)], [0, -1], pre=[-1, 3], extra_obs=[(3, 1, 1)], n_extra=1)
        out["already_matched2_not_in_keyframe"] = case(two, [(100, 100, 0, 0), None], [A], [(100, 100, 0, 0)], [0, -1], pre=[-1, 3], n_extra=1)
        out["empty_sides"] = case([], [], [A], [(100, 100, 0, 0)], [])
        return out

    @staticmethod
    def verify(po, c):
        prove_exact_sim3(c)
        probe = []
        S1, S2 = sim3_sides(c)
        tl.sim3_reference(po, S1, S2, fuse_prm_sim3(c), probe)
        ref = split_probe("search_by_sim3", c.get("_name"), c["out"]["probe"])
        got = np.array(probe, np.float32).reshape(-1, 5)
        assert ref.shape == got.shape and ref.tobytes() == got.tobytes(), "u, v, dist3D, level or radius differ from the contract's"

    @staticmethod
    def transcription(po, c, mutant=None):
        S1, S2 = sim3_sides(c, mutant)
        return tl.sim3_reference(po, S1, S2, fuse_prm_sim3(c), mutant=mutant)

    @staticmethod
    def restatement(po, c):
        S1, S2 = sim3_sides(c)
        return tl.sim3_restated(po, S1, S2, fuse_prm_sim3(c))

    @staticmethod
    def counters(po, c, tr):
        t = tr[4]
        S1, S2 = sim3_sides(c)
        d = {k: int(t[k]) for k in tl.SIM3_GATES + ("disagree", "windows", "walked", "distances", "largest")}
        return dict(d, matches=int(tr[3]), prefilled=int((np.asarray(c["matches12"]) >= 0).sum()),
                    matched2=int(((np.asarray(c["KF"][1]["mps"]) >= 0) & (S2["search"] == 0)).sum() - int((np.asarray(c["P"]["bad"])[np.maximum(c["KF"][1]["mps"], 0)] != 0)[np.asarray(c["KF"][1]["mps"]) >= 0].sum())))

    @staticmethod
    def expected_m12(c):
        """the stored vpMatches12 after the call as keypoints of keyframe 2 for the new entries (-1 elsewhere: the pre-filled ones are left as they were)"""
        out, pre, slots2 = np.asarray(c["out"]["matches12"], np.int64), np.asarray(c["matches12"], np.int64), np.asarray(c["KF"][1]["mps"], np.int64)
        where = {int(p): j for j, p in enumerate(slots2) if p >= 0}
        assert np.array_equal(out[pre >= 0], pre[pre >= 0])
        return np.array([where[int(p)] if q < 0 and p >= 0 else -1 for p, q in zip(out, pre)], np.int64)

    @classmethod
    def same(cls, c, res):
        assert np.array_equal(res[2], cls.expected_m12(c)) and res[3] == int(c["out"]["nmatches"])
        if "want" in c:
            assert np.array_equal(res[2], c["want"])


def fuse_prm_sim3(c):
    return dict(c["prm"], cols=int(c["prm"]["cols"]), rows=int(c["prm"]["rows"]), th_high=int(c["prm"]["th_high"]))


# ------------------------------------------------------------------ SearchByProjection(Frame, KeyFrame, sAlreadyFound, th, ORBdist)
# Where the library's contract differs from the reference's text ON PURPOSE: the files store the reference's output, and this table holds what
# the reference gives and what the contract gives, so that the tests assert both sides.  Anything else that differs is a finding.
#   search_kf, Pcz < 0: the reference has no depth test there (:1994-2006) and projects through the centre; the contract has no candidate.
#   Pcz == 0 (every projecting matcher): the reference goes on with an infinite or NaN pixel and finds nothing (in search_kf a NaN pixel passes
#   both bounds tests; the stored case ends at the distance gate, its point lying in the camera centre); the contract stops at the depth.  The outputs are
#   the same; the reference's probe log has `nonfinite_probe_rows` rows that the contract's does not.
STATED_DIFFERENCES = {
    ("search_kf", "depth_negative_projects_through_the_centre"): dict(reference=dict(kp_match=[0, -1], nmatches=1), contract=dict(kp_match=[-1, -1], nmatches=0),
                                                                     nonfinite_probe_rows=0),
    ("search_kf", "depth_zero"): dict(reference=dict(kp_match=[-1], nmatches=0), contract=dict(kp_match=[-1], nmatches=0), nonfinite_probe_rows=0),
    ("fuse", "depth_zero_and_negative"): dict(nonfinite_probe_rows=1),
    ("fuse_sim3", "depth_zero_and_negative"): dict(nonfinite_probe_rows=1),
    ("search_by_sim3", "depth_zero_and_negative"): dict(nonfinite_probe_rows=1),
}


def split_probe(name, cname, probe):
    """the reference's probe log without its non-finite rows, after asserting that there are exactly as many as STATED_DIFFERENCES says (none for a
    case that is not listed)"""
    ref = np.asarray(probe, np.float32).reshape(-1, 5)
    finite = np.isfinite(ref).all(1)
    want = STATED_DIFFERENCES.get((name, cname), {}).get("nonfinite_probe_rows", 0)
    assert int((~finite).sum()) == want, (name, cname, int((~finite).sum()), want)
    return ref[finite]


def kf_live(c):
    """the slots the contract's caller hands to the device - a live point that is not in sAlreadyFound (:1988-1990) - as tests/test_search_kf_host.py's
    P, and their slot numbers"""
    P = c["P"]
    idx = np.nonzero(np.asarray(P["state"]) == 1)[0]
    return {k: np.asarray(P[k])[idx] for k in ("Px", "Py", "Pz", "maxd", "maxdi", "mindi", "angle", "desc")}, idx


def kf_prm(c):
    return dict(c["prm"], orb_dist=int(c["prm"]["orb_dist"]), check_orientation=int(c["prm"]["check_orientation"]))


def kf_frame(c):
    F = c["F"]
    return dict(F, cols=int(F["cols"]), rows=int(F["rows"]))


def prove_exact_kf(c):
    """prove_exact for the frame's pose: Rcw P + tcw, the pixel (fx * xc) * invzc + cx against K14's fma(Pcx * fx, invz, cx), and |P - Ow|^2 are exact
    in float32 for every live slot that reaches them (the closed bounds gate); no level depends on the logf in use"""
    prm = c["prm"]
    P, idx = kf_live(c)
    x, y, z = (P[k].astype(F64) for k in ("Px", "Py", "Pz"))
    R, tc, Ow = (np.asarray(prm[a], np.float32).astype(F64).ravel() for a in ("Rcw", "tcw", "Ow"))
    for r in range(3):                                               # Ow = -Rcw^T tcw (:1974)
        acc = _ex(-R[r] * tc[0], "Ow")
        for q in (1, 2):
            acc = _ex(acc + _ex(-R[3 * q + r] * tc[q], "Ow"), "Ow")
        assert acc + 0.0 == Ow[r] + 0.0, "Ow is not -Rcw^T tcw"
    with np.errstate(all="ignore"):
        Pc = []
        for r in range(3):
            a, b, d = _ex(x * R[3 * r], "x R"), _ex(y * R[3 * r + 1], "y R"), _ex(z * R[3 * r + 2], "z R")
            Pc.append(_ex(_ex(_ex(a + b, "x R + y R") + d, "R P") + tc[r], "R P + t"))
        front = Pc[2] > 0
        invz = _ex(np.where(front, 1.0 / np.where(front, Pc[2], 1.0), 0.0), "1 / Pcz")
        uv = []
        for Pa, f, cc in ((Pc[0], float(prm["fx"]), float(prm["cx"])), (Pc[1], float(prm["fy"]), float(prm["cy"]))):
            Pa = np.where(front, Pa, 0.0)
            uv.append(_ex(_ex(_ex(f * Pa, "f * xc") * invz, "f * xc * invzc") + cc, "f * xc * invzc + c"))
        u, v = uv
        inside = front & (u >= float(prm["min_x"])) & (u <= float(prm["max_x"])) & (v >= float(prm["min_y"])) & (v <= float(prm["max_y"]))
        o = [np.where(inside, _ex(a - Ow[r], "P - Ow"), 0.0) for r, a in enumerate((x, y, z))]
        d2 = _ex(_ex(_ex(o[0] * o[0], "ox^2") + _ex(o[1] * o[1], "oy^2"), "ox^2 + oy^2") + _ex(o[2] * o[2], "oz^2"), "dist^2")
    return check_levels(dict(prm, scale=c["F"]["scale"]), P["maxd"], np.sqrt(d2).astype(np.float32), inside, idx)


class SearchKf(Matcher):
    driver = "search_kf"
    required = ("matches", "lost_first", "blocked_drops", "culled", "rejects", "not_searched")

    @staticmethod
    def case_on(rng, F, n_src, n, th=10, orb_dist=100, depths=(2.0, 4.0, 8.0)):
        """a keyframe's slots against frame F (integer keypoints, of which the first n_src are drawn from): the frame looks along world z (a turn
        about z by a multiple of 90 degrees, a shift by multiples of 1/16), fx = fy = 256; a slot's point is back-projected from a keypoint - drawn
        with replacement: several points want one keypoint - up to a pixel off on a quarter-pixel grid at depth 2, 4 or 8, its descriptor a few bits
        away (some beyond ORBdist), its angle one rotation off with 30 % outliers, its distance range predicting the octave +-1 (some out of
        range); a share of the slots is NULL, bad or already found.  No point lies behind the camera: that is a stated difference, constructed."""
        nl = len(F["scale"])
        R = ROT_Z[int(rng.integers(0, 4))]
        t = np.array([rng.integers(-4, 5) / 16.0, rng.integers(-4, 5) / 16.0, 0.0])
        R64 = R.astype(F64).reshape(3, 3)
        Ow = (-(R64.T @ t) + 0.0).astype(np.float32)
        prm = dict(th=f32(th), orb_dist=np.int64(orb_dist), check_orientation=np.int64(1), fx=f32(256), fy=f32(256), cx=f32(160), cy=f32(120), min_x=f32(0),
                   max_x=f32(320), min_y=f32(0), max_y=f32(240), Rcw=R.copy(), tcw=t.astype(np.float32), Ow=Ow, log_sf=f32(np.log(f32(1.2))))
        src = rng.integers(0, n_src, n)
        case = rng.random(n)
        u = F["kx"][src].astype(F64) + rng.integers(-4, 5, n) / 4.0 + np.where(case < 0.04, 400, 0)      # some outside the image
        v = F["ky"][src].astype(F64) + rng.integers(-4, 5, n) / 4.0
        z = rng.choice(depths, n)
        Pc = np.stack([(u - 160.0) * z / 256.0, (v - 120.0) * z / 256.0, z])
        Pw = R64.T @ (Pc - t[:, None])
        dist = np.sqrt((Pc * Pc).sum(0))
        desc = F["desc"][src].copy()
        flips = np.where(case >= 0.92, rng.integers(int(orb_dist) + 1, 140, n), rng.integers(0, 40, n))
        for i in range(n):
            b = rng.choice(256, int(flips[i]), replace=False)
            np.bitwise_xor.at(desc[i], b // 8, (1 << (7 - b % 8)).astype(np.uint8))
        off = np.where(rng.random(n) < 0.3, rng.uniform(0, 360, n), 12.0)
        angle = fold_angles((F["angle"][src].astype(F64) + off).astype(np.float32))
        level = np.clip(F["octave"][src].astype(np.int64) + rng.integers(-1, 2, n), 0, nl - 1).astype(F64)
        st = rng.random(n)
        state = np.where(st < 0.05, 0, np.where(st < 0.10, 2, np.where(st < 0.15, 3, 1))).astype(np.uint8)
        P = dict(Px=Pw[0].astype(np.float32), Py=Pw[1].astype(np.float32), Pz=Pw[2].astype(np.float32), angle=angle, desc=desc, state=state)
        jitter = rng.uniform(-0.35, 0.35, n)
        far, near = (case >= 0.04) & (case < 0.08), (case >= 0.08) & (case < 0.12)
        for attempt in range(200):
            maxd = (dist * 1.2 ** (level - 0.5 + jitter)).astype(np.float32)
            maxd[far] = (dist[far] * 0.7).astype(np.float32)
            mind = (maxd / f32(F["scale"][-1])).astype(np.float32)
            mind[near] = (dist[near] * 1.5).astype(np.float32)
            P.update(maxd=maxd, mind=mind, mindi=(f32(0.8) * mind).astype(np.float32), maxdi=(f32(1.2) * maxd).astype(np.float32))
            c = dict(F=F, P=dict(P), prm=prm)
            try:
                prove_exact_kf(c)
                return c
            except LevelMargin as e:                                # (.indices: slot numbers)
                jitter[e.indices] = rng.uniform(-0.35, 0.35, len(e.indices))
        raise AssertionError("no distance ranges found")

    @staticmethod
    def random_frame(rng, N=300):
        """integer keypoints over 320 x 240 on all 8 octaves, clustered so that windows hold several"""
        cx, cy = rng.integers(20, 300, 40), rng.integers(20, 220, 40)
        w = rng.integers(0, 40, N)
        kx, ky = np.clip(cx[w] + rng.integers(-8, 9, N), 4, 316), np.clip(cy[w] + rng.integers(-8, 9, N), 4, 236)
        desc = np.concatenate([rng.integers(0, 256, (N, 16), dtype=np.uint8), np.zeros((N, 16), np.uint8)], 1)
        return tk.make_frame(kx, ky, rng.integers(0, 8, N), fold_angles(rng.uniform(0, 360, N)), desc, blocked=(rng.random(N) < 0.12).astype(np.uint8))

    @classmethod
    def build(cls, po):
        out = OrderedDict()
        for b in range(2):                     # the generator's frames, stored as the POKE handle holds them
            rng = np.random.default_rng(8000 + b)
            for k, (n, th, od) in enumerate(((350, 10, 100), (200, 3, 64), (1, 10, 100), (15, 10, 100), (16, 3, 100), (17, 10, 64))):
                F0 = cls.random_frame(rng)
                out["random%d.%02d" % (b, k)] = cls.case_on(rng, on_handle(po, F0), len(F0["kx"]), n, th, od)
        from frame_builders import last_frame_of
        for b, frame in enumerate((0, 1)):     # the extracted frames the device can be given
            g = OracleFrame(po, frame)
            rng = np.random.default_rng(8050 + b)
            for k, (th, od) in enumerate(((10, 100), (3, 64))):
                F = last_frame_of(g, g.c)
                F["blocked"] = (np.random.default_rng(8049).random(g.e.n) < 0.08).astype(np.uint8)
                F["bounds"] = (f32(0), f32(320), f32(0), f32(240))
                out["real%d.%02d" % (b, k)] = dict(cls.case_on(rng, F, g.e.n, 500 if frame == 0 else 700, th, od), frame=np.int64(frame))
        out.update(cls.constructed(po))
        return out

    @staticmethod
    def constructed(po):
        """the identity pose, fx = fy = 256: a point at depth 4 behind pixel (u, v).  A frame is rows (x, y, octave, bits of its descriptor[, angle]), a
        slot (u, v, level, bits[, angle[, state[, depth]]])."""
        out = OrderedDict()

        def case(frame, slots, want, th=10, orb_dist=100, blocked=None):
            fr = [tuple(r) + (0.0,) * (5 - len(r)) for r in frame]
            F = tk.make_frame([r[0] for r in fr], [r[1] for r in fr], [r[2] for r in fr], [r[4] for r in fr], np.stack([tk.bits_set(int(r[3])) for r in fr]),
                              blocked=np.zeros(len(fr), np.uint8) if blocked is None else np.asarray(blocked, np.uint8))
            prm = tk.identity_params(F, th=th, orb_dist=orb_dist, fx=256.0, fy=256.0)
            sl = [tuple(r) + (0.0, 1, 4.0)[len(r) - 4:] for r in slots]
            P = tk.points_at([r[0] for r in sl], [r[1] for r in sl], prm, [r[4] for r in sl], np.stack([tk.bits_set(int(r[3])) for r in sl] + [np.zeros(32, np.uint8)])[:len(sl)],
                             level=0)
            z = np.array([r[6] for r in sl], np.float32)
            P["Px"], P["Py"], P["Pz"] = (P["Px"] * z / f32(4)).astype(np.float32), (P["Py"] * z / f32(4)).astype(np.float32), z
            d = np.sqrt(P["Px"].astype(F64) ** 2 + P["Py"].astype(F64) ** 2 + P["Pz"].astype(F64) ** 2)
            P["maxd"] = np.where(d > 0, d * 1.2 ** (np.array([r[2] for r in sl], F64) - 0.5), 1).astype(np.float32)
            P["mind"] = (P["maxd"] * f32(0.1)).astype(np.float32)
            P["mindi"], P["maxdi"] = (f32(0.8) * P["mind"]).astype(np.float32), (f32(1.2) * P["maxd"]).astype(np.float32)
            P["state"] = np.array([r[5] for r in sl], np.uint8)
            prm = dict(prm, orb_dist=np.int64(orb_dist), check_orientation=np.int64(prm["check_orientation"]))
            return dict(F=on_handle(po, {k: v for k, v in F.items() if k != "bounds"}), P=P, prm=prm, want=np.asarray(want, np.int64))
        kp = (100, 100, 0, 10)
        # the bounds gate is closed at :2003-2006: u == max_x, u == min_x, v == max_y are inside (the keypoints 3 px inside them are found)
        out["u_at_max_x_is_in"] = case([(317, 100, 0, 10)], [(320, 100, 0, 0), (320.25, 100, 0, 0)], [0])
        out["u_at_min_x_is_in"] = case([(3, 100, 0, 10)], [(0, 100, 0, 0), (-0.25, 100, 0, 0)], [0])
        out["v_at_max_y_is_in"] = case([(100, 237, 0, 10)], [(100, 240, 0, 0), (100, 240.25, 0, 0)], [0])
        # GetFeaturesInArea(u, v, r, L-1, L+1): octaves L-1, L, L+1 are candidates, L+2 is not (level 2 here)
        out["octaves_around_the_level"] = case([(40, 100, 1, 10), (100, 100, 2, 10), (160, 100, 3, 10), (220, 100, 4, 10)],
                                               [(40, 100, 2, 0), (100, 100, 2, 0), (160, 100, 2, 0), (220, 100, 2, 0)], [0, 1, 2, -1])
        # bestDist == ORBdist is a match, one more is not
        out["orb_dist_accepted"] = case([(100, 100, 0, 64), (200, 100, 0, 65)], [(100, 100, 0, 0), (200, 100, 0, 0)], [0, -1], orb_dist=64)
        # equal distances: the first in walk order; a keypoint an earlier point took is no candidate: the later point takes its second best
        out["tie_first_in_walk_order"] = case([(101, 100, 0, 10), (99, 100, 0, 10)], [(100, 100, 0, 0)], [0, -1])
        out["claimed_keypoint_is_no_candidate"] = case([(100, 100, 0, 3), (101, 100, 0, 30)], [(100, 100, 0, 0), (100, 100, 0, 0)], [0, 1])
        out["blocked_keypoint_is_no_candidate"] = case([(100, 100, 0, 3), (101, 100, 0, 30)], [(100, 100, 0, 0)], [-1, 0], blocked=[1, 0])
        # 12 points in rotation bin 0; point 12 (rotation 180: one entry < 0.1 * 12) takes keypoint 12 at distance 0 and is culled afterwards;
        # point 13 wants keypoint 12 too, finds it taken and takes keypoint 13 at distance 5 (tests/test_search_kf_host.py: culled_keypoint_case)
        fr = [(20 + 20 * k, 30, 0, 0) for k in range(12)] + [(300, 200, 0, 0), (301, 200, 0, 5)]
        sl = [(20 + 20 * k, 30, 0, 0, 0.0) for k in range(12)] + [(300, 200, 0, 0, 180.0), (300, 200, 0, 0, 0.0)]
        out["culled_keypoint_stays_hidden"] = case(fr, sl, list(range(12)) + [-1, 13], th=5)
        # NULL, bad and already found slots are not searched
        out["slot_states"] = case([kp, (200, 100, 0, 10), (40, 40, 0, 10), (250, 200, 0, 10)],
                                  [(100, 100, 0, 0, 0.0, 0), (200, 100, 0, 0, 0.0, 2), (40, 40, 0, 0, 0.0, 3), (250, 200, 0, 0, 0.0, 1)], [-1, -1, -1, 3])
        # dist3D equal to each invariance bound is inside, one ulp beyond is not ((0, 0, 4): dist 4)
        c = case([(160, 120, 0, 10)], [(160, 120, 0, 0)] * 4, [0])
        top = maxd_for(f32(4))
        c["P"]["mind"] = mind_for(np.array([4, np.nextafter(f32(4), f32(8)), 0, 0], np.float32))
        c["P"]["maxd"] = np.array([top, top, top, np.nextafter(top, f32(0))], np.float32)
        c["P"]["mindi"], c["P"]["maxdi"] = (f32(0.8) * c["P"]["mind"]).astype(np.float32), (f32(1.2) * c["P"]["maxd"]).astype(np.float32)
        c["prm"]["check_orientation"] = np.int64(0)
        out["dist3D_at_both_bounds"] = c                            # slot 0 takes the keypoint, 2 finds it taken; 1 and 3 are outside the range
        # the stated differences: a point behind the camera is projected through the centre by the reference ((-0.9375, -0.3125, -4) lands on
        # (220, 140), where (0.9375, 0.3125, 4) does); a point in the camera plane gets a NaN pixel
        out["depth_negative_projects_through_the_centre"] = case([(220, 140, 0, 10), (250, 200, 0, 10)], [(220, 140, 0, 0, 0.0, 1, -4.0), (10, 10, 0, 200)], [-1, -1])
        out["depth_zero"] = case([(160, 120, 0, 10)], [(160, 120, 0, 0, 0.0, 1, 0.0)], [-1])
        out["empty_keyframe"] = case([kp], [], [-1])
        return out

    @staticmethod
    def verify(po, c):
        cname = c.get("_name")
        prove_exact_kf(c)
        P, idx = kf_live(c)
        probe = []
        tk.search_by_projection_kf(po, kf_frame(c), P, kf_prm(c), probe)
        got = np.array(probe, np.float32).reshape(-1, 5)
        if ("search_kf", cname) in STATED_DIFFERENCES and "reference" in STATED_DIFFERENCES[("search_kf", cname)]:
            return                                                  # (the reference searches a slot the contract does not: the logs differ by it)
        ref = split_probe("search_kf", cname, c["out"]["probe"])
        assert ref.shape == got.shape and ref.tobytes() == got.tobytes(), "u, v, dist3D, level or radius differ from the contract's"

    @staticmethod
    def transcription(po, c, mutant=None):
        P, idx = kf_live(c)
        return tk.search_by_projection_kf(po, kf_frame(c), P, kf_prm(c), mutant=mutant) + (idx,)

    @staticmethod
    def restatement(po, c):
        P, idx = kf_live(c)
        return tk.search_kf_restated(po, kf_frame(c), P, kf_prm(c))[:6] + (idx,)

    @staticmethod
    def counters(po, c, tr):
        P, idx = kf_live(c)
        F, prm = kf_frame(c), kf_prm(c)
        keys = tk.candidate_keys(po, F, P, prm)
        res = tk.resolve_kf(keys, F, P, prm)
        items = np.asarray(F["items"], np.int64)
        lost = sum(1 for i in range(len(keys)) if len(keys[i]) and (int(keys[i].min()) >> 18) <= prm["orb_dist"] and tr[0][i] != items[int(keys[i].min()) & tk.POS])
        win = tk.windows(po, F, P, prm)
        drops = sum(int(sum(F["blocked"][k] != 0 for k in tk.get_features_in_area(F, w[0], w[1], w[2], w[3] - 1, w[3] + 1))) for w in win if w is not None)
        return dict(matches=int(tr[3]), lost_first=int(lost), blocked_drops=int(drops), culled=int((tr[0] >= 0).sum()) - int(tr[3]),
                    rejects=int(sum(w is None for w in win)), not_searched=int(len(c["P"]["state"]) - len(idx)), rounds=int(res[6]), candidates=int(res[4]),
                    overflow=int(res[7]), ind=np.asarray(res[5], np.int64))

    @staticmethod
    def kp_match_of(res):
        """the yardstick's kp_match (positions among the searched slots) as slot numbers"""
        km, idx = np.asarray(res[2], np.int64), res[-1]
        return np.where(km >= 0, idx[np.maximum(km, 0)] if len(idx) else -1, -1)

    @classmethod
    def same(cls, c, res):
        cname = c.get("_name")
        ref_km = np.where(np.asarray(c["out"]["kp_match"]) == -2, -1, c["out"]["kp_match"])
        stated = STATED_DIFFERENCES.get(("search_kf", cname), {})
        n0 = len(c["want"]) if "want" in c else None
        if "reference" in stated:                                   # both sides of a stated difference: what the reference gave, what the contract gives
            k = len(stated["reference"]["kp_match"])
            assert ref_km[:k].tolist() == stated["reference"]["kp_match"] and int(c["out"]["nmatches"]) == stated["reference"]["nmatches"]
            assert cls.kp_match_of(res)[:k].tolist() == stated["contract"]["kp_match"] and res[3] == stated["contract"]["nmatches"]
            assert (cls.kp_match_of(res)[k:] == -1).all() and (ref_km[k:] == -1).all()
            return
        assert np.array_equal(cls.kp_match_of(res), ref_km) and res[3] == int(c["out"]["nmatches"])
        if n0 is not None:
            assert ref_km[:n0].tolist() == c["want"].tolist() and (ref_km[n0:] == -1).all()


MATCHERS = OrderedDict([("search_local", SearchLocal), ("search_last_frame", SearchLastFrame), ("search_init", SearchInit), ("search_by_bow", SearchByBow),
                        ("search_by_bow_kf", SearchByBowKf), ("search_for_triangulation", SearchForTriangulation), ("fuse", Fuse), ("fuse_sim3", FuseSim3), ("search_by_sim3", SearchBySim3), ("search_kf", SearchKf)])
