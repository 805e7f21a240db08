"""What tools/ref_matcher_goldens.py and tests/test_ref_matcher.py / tests/test_gpu_ref_matcher.py share: per matcher entry point the cases of
tests/golden/ref_matcher_<name>.npz (the random generators and constructed cases of the host tests, imported, with what the reference cannot be
given changed in the input - see the tool's docstring), and how a stored case goes through the Python transcription and the numpy restatement of
that matcher and is compared with what the reference's own ORBmatcher.cpp returned.

Not a test module.  A case is a dict: the sides and prm in the vocabulary of the matcher's host test, `out` (the reference's outputs, from
oracle/pyref_matcher.py's driver) and `counters` (the transcription's trace on the same inputs)."""
from collections import OrderedDict

import numpy as np

import test_bow_host as tb
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


MATCHERS = OrderedDict([("search_local", SearchLocal), ("search_last_frame", SearchLastFrame), ("search_init", SearchInit), ("search_by_bow", SearchByBow),
                        ("search_by_bow_kf", SearchByBowKf), ("search_for_triangulation", SearchForTriangulation)])
