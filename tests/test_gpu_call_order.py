"""-m gpu: the ORDER in which the library's kernels read an extract's results - not the kernels, which the other files pin bit for bit.

include/jsorb.h promises: work the library enqueued on a handle that reads an extract's results completes before the next extract overwrites
them, with no wait needed from the caller.  The matchers (jsorb_search_*_async, jsorb_search_by_bow_async), jsorb_bow_transform_async and
jsorb_init_reference_set run on the handle's MAIN stream behind the lanes of the extract they read; a following batch of K > 1 lanes runs on
the device's pool streams, none of which is the main stream, and has to be ordered behind them explicitly (order_lanes_for_new_batch,
mark_main_stream in csrc/jsorb_handle.h).  Every case here is the sequence

    extract A (batch of 16 = 4 lanes, or one synchronous frame)  ->  plug  ->  reader under test  ->  batch B of K lanes  ->  wait

with NO host wait between the plug and the end of batch B's enqueue (every call of the sequence has run once before, waited for, so that no
first-use allocation or code loading stalls the host inside it).  The plug is jsorb_search_by_bow_async over image 0 with every keypoint in
node 0 against JSORB_BOW_MAX_KEYFRAMES copies of the frame itself: one wave per keyframe walks all N x N pairs, so it holds the main stream for
about a millisecond and the reader behind it cannot have run before batch B was enqueued.  That is asserted, not assumed: an event recorded
behind the reader must still be pending when the enqueue of batch B has returned, else the case FAILS and asks for a longer plug (PLUG_CALLS).
Expected values: every image of A and B extracted alone and synchronously by the same library (that path is pinned to the oracle by
tests/test_gpu_parity.py), fed to the host transcriptions of tests/test_*_host.py.  A reader always has to return the transcription on A's data;
batch B has to equal B's reference; the plug's 256 rows have to equal the transcription; and the same reader run again on B, waited for, has
to equal the transcription on B (nothing stale left behind).  Each case asserts the lane count the handle really used.

Geometry: the API fuzz's (200 x 320, 4 levels, tile 16, JSORB_LANE_MIN_MPX=0.2): 16 images = 4 lanes, 8 = 2 lanes, 3 = 1 lane.

Measured once on an MI355X with events (measure_plug_and_batch below), at this geometry (439 keypoints in image 0): one plug call 1 140 - 1 183 us,
batch B of 16 images on 4 lanes 106 - 112 us of GPU time (and 82 - 86 us of host time to enqueue it).  One plug is 10 x batch B; PLUG_CALLS = 2 are
enqueued per case (21 x), so batch B's descriptor stores certainly land inside the plug unless something orders them behind it.
On the library before mark_main_stream existed, the 28 own-stream cases with K > 1, three of the four stream-change cases and the own-stream chain
failed (wrong match results); the 44 one-lane and caller-stream cases passed."""
import ctypes

import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import both_transforms, frame_side, sampled_voc, search_by_bow_reference
from test_bow_host import default_params as bow_defaults
from test_gpu_bow import bow_params, concat
from test_gpu_search_init import frame_of as init_frame_of
from test_gpu_search_init import init_params
from test_gpu_search_last_frame import last_frame_of, points_of
from test_gpu_search_last_frame import params as last_params
from test_gpu_search_local import _dev, _mk, frame_of, points_near_keypoints
from test_search_init_host import default_params as init_defaults
from test_search_init_host import f1_drawn_from, f1_from_frame, search_for_initialization
from test_search_last_frame_host import track_with_motion_model
from test_search_local_host import search_by_projection

pytestmark = pytest.mark.gpu
C = dict(h=200, w=320, L=4, tile=16, th=20, fx=300.0, bf=40.0)
MB, MBF = C["bf"] / C["fx"], C["bf"]
NA = 16                                           # images of a set; max_batch of the handles
IMAGES_OF_LANES = {4: 16, 2: 8, 1: 3}             # batch B per lane count (JSORB_LANE_MIN_MPX=0.2: 4 images of 200 x 320 carry a lane)
TARGETS = (0, 2, 7, 15)                           # images a reader may be aimed at: the first and the last image of a batch of 3, 8 and 16
PLUG_KEYFRAMES = 256                              # JSORB_BOW_MAX_KEYFRAMES
PLUG_CALLS = 2                                    # plugs enqueued in front of the reader: 2 x 1.16 ms against 0.11 ms of batch B (docstring)
N_POINTS = 300


def mk16(orb):
    return orb.ORBExtractor(C["h"], C["w"], 1.2, C["L"], 9, 14, 7, C["th"], None, C["tile"], C["tile"], max_batch=NA)


class World:
    """images, device copies, per-image references and lazily computed transcriptions, shared by every case and never changed"""

    def __init__(self, orb, po):
        import torch
        self.orb, self.po, self.lib = orb, po, orb.load_library()
        self.img, self.dev, self.kp, self.desc, self.frames, self._memo = {}, {}, {}, {}, {}, {}
        gl, gr = _mk(orb, C), _mk(orb, C)         # the single-frame handles the references come from
        for s, seed in (("A", 1100), ("B", 1200)):
            pairs = [synth_stereo_pair(seed + i, C["h"], C["w"]) for i in range(NA)]
            self.img[s] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
            self.dev[s] = tuple(torch.from_numpy(a).cuda() for a in self.img[s])
            for i in range(NA):
                self.kp[s, i], self.desc[s, i] = gl.extract(self.img[s][0][i])
                if i in TARGETS:
                    right = frame_side(*gr.extract(self.img[s][1][i]))
                    u, _, _ = orb.compute_stereo_matches(gl, gr, MB, MBF)
                    self.frames[s, i] = dict(local=frame_of(gl, C, u_right=u), last=last_frame_of(gl, C), init=init_frame_of(gl, C),
                                             side=frame_side(self.kp[s, i], self.desc[s, i]), right=right, u=u)
        torch.cuda.synchronize()
        self.tree = sampled_voc(self.desc["A", 0])
        self.voc = orb.Vocabulary(self.tree, levels_up=1)

    def n(self, s, i):
        return len(self.kp[s, i]) // 6

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def bow_side(self, s, i, view="side"):
        """descriptors, angles, node ids (host transform: the device one is pinned to it by tests/test_gpu_bow.py), every keypoint valid"""
        def make():
            S = dict(self.frames[s, i][view])
            S["node"] = both_transforms(self.tree, S["desc"], 1)[1].astype(np.int32)
            S["valid"] = np.ones(len(S["node"]), np.uint8)
            return S
        return self.memo(("bow_side", s, i, view), make)


@pytest.fixture(scope="module")
def world(orb, po):
    W = World(orb, po)
    # B is another scene than A: other counts, other descriptors (asserted once, here)
    assert [W.n("A", i) for i in range(NA)] != [W.n("B", i) for i in range(NA)]
    for i in range(NA):
        assert W.n("A", i) > 100 and W.n("B", i) > 100
        assert W.n("A", i) != W.n("B", i) or not np.array_equal(W.desc["A", i], W.desc["B", i]), i
    for i in TARGETS:
        assert W.n("A", i) != W.n("B", i), ("pick another seed: equal keypoint counts", i)
        m = min(W.n("A", i), W.n("B", i))
        assert (W.desc["A", i][:m] != W.desc["B", i][:m]).any(axis=1).mean() > 0.9
    return W


def _full(shape, v, dtype):
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (shape,), v, dtype=dtype, device="cuda")


def _chk(g, rc):
    assert rc == 0, (rc, g._lib.jsorb_last_error(g.handle))


# ---- the plug: the single-node shape of test_single_node_of_more_than_300_entries, JSORB_BOW_MAX_KEYFRAMES keyframes that are the frame itself ----
class Plug:
    def __init__(self, W, s, calls=PLUG_CALLS):
        import torch
        self.W, self.s = W, s
        S = W.frames[s, 0]["side"]
        N = len(S["angle"])
        self.side = dict(S, node=np.zeros(N, np.int32), valid=np.ones(N, np.uint8))
        self.prm = bow_defaults(th_low=30)
        self.start, *self.arrs = W.memo(("plug_dev", s), lambda: concat([self.side] * PLUG_KEYFRAMES))
        self.f_node = _full(N, 0, torch.int32)
        self.out = [(_full((PLUG_KEYFRAMES, N), -7, torch.int32), _full(PLUG_KEYFRAMES, -7, torch.int32)) for _ in range(calls)]
        self.p = bow_params(W.orb, self.prm)

    def enqueue(self, g, k):
        mk, cnt = self.out[k]
        _chk(g, g._lib.jsorb_search_by_bow_async(g.handle, 0, ctypes.byref(self.p), self.f_node.data_ptr(), PLUG_KEYFRAMES, self.start.ctypes.data,
                                                 *[t.data_ptr() for t in self.arrs], mk.data_ptr(), cnt.data_ptr()))

    def check(self):
        ref = self.W.memo(("plug_ref", self.s), lambda: search_by_bow_reference(self.side, self.side, self.prm))
        assert ref[1] > 0
        for k, (mk, cnt) in enumerate(self.out):
            mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
            assert (cnt == ref[1]).all(), ("plug", k, np.unique(cnt), ref[1])
            assert (mk == np.asarray(ref[0])[None, :]).all(), ("plug", k)


# ---- the readers.  prepare(): device inputs and caller-owned outputs (torch, before the sequence); enqueue(): C ABI calls only; check(): after the wait ----
class ByBow:
    """jsorb_search_by_bow_async with real nodes of the sampled vocabulary: the keyframes are the right view of the frame and the frame itself"""
    handle_nodes = False

    def __init__(self, W, s, i):
        import torch
        self.W, self.s, self.i = W, s, i
        self.F = W.bow_side(s, i)
        self.kfs = [W.bow_side(s, i, "right"), self.F]
        self.prm = bow_defaults()
        self.p = bow_params(W.orb, self.prm)
        self.start, *self.arrs = concat(self.kfs)
        self.f_node = _dev(self.F["node"])
        N = len(self.F["node"])
        self.mk, self.cnt = _full((2, N), -7, torch.int32), _full(2, -7, torch.int32)

    def enqueue(self, g, image):
        lib = g._lib
        if self.handle_nodes:
            _chk(g, lib.jsorb_bow_transform_async(g.handle, image, self.W.voc.handle))
        _chk(g, lib.jsorb_search_by_bow_async(g.handle, image, ctypes.byref(self.p), None if self.handle_nodes else self.f_node.data_ptr(), 2,
                                              self.start.ctypes.data, *[t.data_ptr() for t in self.arrs], self.mk.data_ptr(), self.cnt.data_ptr()))

    def check(self, g=None):
        mk, cnt = self.mk.cpu().numpy(), self.cnt.cpu().numpy()
        for k, KF in enumerate(self.kfs):
            ref = self.W.memo(("bow_ref", self.s, self.i, k), lambda: search_by_bow_reference(KF, self.F, self.prm))
            assert int(cnt[k]) == ref[1] and np.array_equal(mk[k], ref[0]), (type(self).__name__, self.s, self.i, k, int(cnt[k]), ref[1])
        assert int(cnt[1]) > 0 and int(cnt[0]) > 0                # a matcher that matched nothing would prove nothing


class ByBowHandleNodes(ByBow):
    """jsorb_bow_transform_async, then jsorb_search_by_bow_async with f_node = NULL: the handle's own node ids"""
    handle_nodes = True


class Local:
    """jsorb_search_local_points_async, monocular (u_right = NULL)"""
    stereo = False

    def __init__(self, W, s, i):
        import torch
        self.W, self.s, self.i = W, s, i
        F = W.frames[s, i]["local"]
        self.F = F if self.stereo else dict(F, u_right=None)
        self.P = W.memo(("local_P", s, i, self.stereo), lambda: points_near_keypoints(np.random.default_rng(3), self.F, N_POINTS, C["L"])[0])
        P = self.P
        self.inp = [_dev(P[k]) for k in ("u", "v", "invz", "level", "view_cos", "in_frustum", "desc")]
        N = len(F["kx"])
        self.out = [_full(N_POINTS, -1, torch.int32), _full(N_POINTS, -1, torch.int32), _full(N, -1, torch.int32), _full(1, 0, torch.int32)]
        self.p = W.orb.JsorbSearchParams(1.0, 0.8, 100, float(F["mbf"]), float(F["min_x"]), float(F["min_y"]), float(F["inv_w"]), float(F["inv_h"]),
                                         F["cols"], F["rows"])

    def enqueue(self, g, image):
        lib = g._lib
        ur = lib.jsorb_stereo_uright_device(g.handle, image) if self.stereo else None      # the handle's own stereo result, in place
        assert ur or not self.stereo
        _chk(g, lib.jsorb_search_local_points_async(g.handle, image, ctypes.byref(self.p), N_POINTS, *[t.data_ptr() for t in self.inp], ur, None,
                                                    *[t.data_ptr() for t in self.out]))

    def check(self, g=None):
        ref = self.W.memo(("local_ref", self.s, self.i, self.stereo), lambda: search_by_projection(self.F, self.P, 1.0))
        m, d, km, cnt = (t.cpu().numpy() for t in self.out)
        assert int(cnt[0]) == ref[3] > 0, (type(self).__name__, self.s, self.i, int(cnt[0]), ref[3])
        assert np.array_equal(m, ref[0]) and np.array_equal(d, ref[1]) and np.array_equal(km, ref[2]), (type(self).__name__, self.s, self.i)


class LocalStereo(Local):
    """jsorb_search_local_points_async with u_right = jsorb_stereo_uright_device of the handle: the next stereo match rewrites it as well"""
    stereo = True


class LastFrame:
    """jsorb_search_last_frame_async (monocular, the retry enqueued)"""

    def __init__(self, W, s, i):
        import torch
        self.W, self.s, self.i = W, s, i
        F = self.F = W.frames[s, i]["last"]
        self.prm = last_params(C, F, 7, seed=5)
        self.P = W.memo(("last_P", s, i), lambda: points_of(np.random.default_rng(6), F, self.prm, N_POINTS, C["L"])[0])
        P, prm = self.P, self.prm
        self.inp = [_dev(P[k]) for k in ("Px", "Py", "Pz", "octave", "angle", "desc")]
        N = len(F["kx"])
        self.out = [_full(N_POINTS, -1, torch.int32), _full(N_POINTS, -1, torch.int32), _full(N, -1, torch.int32), _full(1, 0, torch.int32)]
        self.p = W.orb.make_last_frame_params(prm["Rcw"], prm["tcw"], (prm["fx"], prm["fy"], prm["cx"], prm["cy"]),
                                              (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]), (F["inv_w"], F["inv_h"]), th=float(prm["th"]),
                                              direction=prm["direction"], mbf=float(F["mbf"]), check_orientation=prm["check_orientation"],
                                              retry_below=prm["retry_below"], th_high=prm["th_high"], cols=F["cols"], rows=F["rows"])

    def enqueue(self, g, image):
        _chk(g, g._lib.jsorb_search_last_frame_async(g.handle, image, ctypes.byref(self.p), N_POINTS, *[t.data_ptr() for t in self.inp], None,
                                                     *[t.data_ptr() for t in self.out]))

    def check(self, g=None):
        ref = self.W.memo(("last_ref", self.s, self.i), lambda: track_with_motion_model(self.W.po, self.F, self.P, self.prm))
        m, d, km, cnt = (t.cpu().numpy() for t in self.out)
        assert int(cnt[0]) == ref[3] > 0, ("LastFrame", self.s, self.i, int(cnt[0]), ref[3])
        assert np.array_equal(m, ref[0]) and np.array_equal(d, ref[1]) and np.array_equal(km, ref[2]), ("LastFrame", self.s, self.i)


class Init:
    """jsorb_search_for_initialization_async: F1 drawn from the frame's own keypoints, prev_matched updated in place"""

    def __init__(self, W, s, i):
        import torch
        self.W, self.s, self.i = W, s, i
        F2 = self.F2 = W.frames[s, i]["init"]
        self.F1, self.prev = W.memo(("init_F1", s, i), lambda: f1_drawn_from(np.random.default_rng(1), F2, N_POINTS))
        self.prm = init_defaults()
        self.p = init_params(W.orb, F2, self.prm)
        self.inp = [_dev(self.F1["octave"]), _dev(self.F1["angle"]), _dev(self.F1["desc"]), _dev(self.prev)]
        N = len(F2["kx"])
        self.out = [_full(N_POINTS, -1, torch.int32), _full(N, -1, torch.int32), _full(1, 0, torch.int32)]

    def enqueue(self, g, image):
        _chk(g, g._lib.jsorb_search_for_initialization_async(g.handle, image, ctypes.byref(self.p), N_POINTS, *[t.data_ptr() for t in self.inp],
                                                             *[t.data_ptr() for t in self.out]))

    def check(self, g=None):
        ref = self.W.memo(("init_ref", self.s, self.i), lambda: search_for_initialization(self.F1, self.F2, self.prev, self.prm))
        m12, m21, cnt = (t.cpu().numpy() for t in self.out)
        assert int(cnt[0]) == ref[2] > 0, ("Init", self.s, self.i, int(cnt[0]), ref[2])
        assert np.array_equal(m12, ref[0]) and np.array_equal(m21, ref[1]), ("Init", self.s, self.i)
        assert np.array_equal(self.inp[3].cpu().numpy().view(np.uint32), ref[3].view(np.uint32)), ("Init prev_matched", self.s, self.i)


class KeptFrame:
    """jsorb_init_reference_set: the copies of the frame's descriptors, octaves, angles and mvKeysUn into the handle's kept buffers.  Checked by
    jsorb_search_initial_frame against image 0 of whatever the handle holds by then (`against`: the set that image comes from)"""

    def __init__(self, W, s, i):
        self.W, self.s, self.i = W, s, i
        self.F1, self.prev = f1_from_frame(W.frames[s, i]["init"])
        self.prm = init_defaults()

    def enqueue(self, g, image):
        _chk(g, g._lib.jsorb_init_reference_set(g.handle, image))

    def check(self, g, against):
        F2 = self.W.frames[against, 0]["init"]
        assert g.initial_frame_n() == len(self.F1["octave"])
        m12, pm, cnt = g.search_initial_frame(init_params(self.W.orb, F2, self.prm), image=0)
        ref = self.W.memo(("kept_ref", self.s, self.i, against), lambda: search_for_initialization(self.F1, F2, self.prev, self.prm))
        assert cnt == ref[2] > 0, ("KeptFrame", self.s, self.i, against, cnt, ref[2])
        assert np.array_equal(m12, ref[0]) and np.array_equal(pm.view(np.uint32), ref[3].view(np.uint32)), ("KeptFrame", self.s, self.i, against)


READERS = dict(by_bow=ByBow, bow_transform_then_by_bow=ByBowHandleNodes, local_mono=Local, local_stereo_uright=LocalStereo, last_frame=LastFrame,
               for_initialization=Init, init_reference_set=KeptFrame)


# ---- the sequence ----
def _extract(W, gl, gr, s, n, single=False):
    """set s on the pair (gr and the stereo match only when gr is given): a batch of n images, or image 0 through the synchronous single-frame call"""
    if single:
        gl.extract(W.img[s][0][0])
        if gr is not None:
            gr.extract(W.img[s][1][0])
    else:
        gl.extract_batch_device_async(W.dev[s][0].data_ptr(), C["h"] * C["w"], C["w"], n, keep=W.dev[s][0])
        if gr is not None:
            gr.extract_batch_device_async(W.dev[s][1].data_ptr(), C["h"] * C["w"], C["w"], n, keep=W.dev[s][1])
    if gr is not None:
        W.orb.stereo_match_batch_async(gl, gr, MB, MBF)


def _check_extract(W, gl, gr, s, n, lanes):
    assert gl.launch_forms()["lanes"] == lanes, ("the batch did not run on the lane count under test", gl.launch_forms()["lanes"], lanes)
    for j in range(n):
        assert gl.n_keypoints(j) == W.n(s, j), (s, j, gl.n_keypoints(j), W.n(s, j))
        assert np.array_equal(gl.keypoints(j), W.kp[s, j]) and np.array_equal(gl.descriptors(j), W.desc[s, j]), (s, j)
    if gr is not None:
        for j in (0, n - 1):
            u, _, _ = W.orb.stereo_result(gl, j)
            assert np.array_equal(u.view(np.uint32), W.frames[s, j]["u"].view(np.uint32)), (s, j)


def run_sequence(W, monkeypatch, reader, lanes, first, stream_kind):
    """first: "batch_last" / "batch_first" (A as a batch of 16 on 4 lanes, the reader on its last / first image) or "single" (A[0] through the
    synchronous call).  stream_kind: "own", "user" (jsorb_set_stream to a torch stream before anything), "switch" (jsorb_set_stream between the
    reader and batch B: the new main stream has to continue after the reader)"""
    import torch
    orb, lib = W.orb, W.lib
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.2")
    cls = READERS[reader]
    stereo = cls is LocalStereo
    gl, gr = mk16(orb), (mk16(orb) if stereo else None)
    user = torch.cuda.Stream() if stream_kind != "own" else None
    single = first == "single"
    nA, nB = (1 if single else NA), IMAGES_OF_LANES[lanes]
    image = nA - 1 if first == "batch_last" else 0
    plug, rd, warm = Plug(W, "A"), cls(W, "A", image), cls(W, "A", image)
    torch.cuda.synchronize()                      # the inputs and the cleared outputs are in place before anything is enqueued on the handles
    try:
        if stream_kind == "user":
            gl.set_stream(user.cuda_stream)
        # 0. every call of the sequence once, waited for: the handle's first-use allocations, the pool's streams and the loading of the kernels'
        #    code cost the host milliseconds, which must not be spent while the plug is running
        _extract(W, gl, gr, "B", nB)
        gl.sync()
        if gr is not None:
            gr.sync()
        # 1. A, waited for: the host needs its counts to size the readers' arguments
        _extract(W, gl, gr, "A", nA, single)
        gl.sync()
        if gr is not None:
            gr.sync()
        _check_extract(W, gl, gr, "A", nA, 1 if single else 4)
        plug.enqueue(gl, 0)
        warm.enqueue(gl, image)
        gl.sync()
        # 2. .. 4.: no host wait
        for k in range(PLUG_CALLS):
            plug.enqueue(gl, k)
        rd.enqueue(gl, image)
        behind_reader = torch.cuda.Event()
        behind_reader.record(torch.cuda.ExternalStream(lib.jsorb_get_stream(gl.handle)))
        if stream_kind == "switch":
            gl.set_stream(user.cuda_stream)
        _extract(W, gl, gr, "B", nB)
        reader_pending = not behind_reader.query()
        # 5.
        gl.sync()
        if gr is not None:
            gr.sync()
        torch.cuda.synchronize()
        # 6.
        assert reader_pending, "the reader had finished before batch B was enqueued: the case proves nothing - a longer plug is needed (PLUG_CALLS)"
        _check_extract(W, gl, gr, "B", nB, lanes)
        if cls is KeptFrame:
            rd.check(gl, "B")
        else:
            rd.check()
        plug.check()
        # the same reader on B, waited for: nothing of A is left behind
        image_b = min(image, nB - 1)
        again = cls(W, "B", image_b)
        torch.cuda.synchronize()
        again.enqueue(gl, image_b)
        gl.sync()
        torch.cuda.synchronize()
        if cls is KeptFrame:
            again.check(gl, "B")
        else:
            again.check()
    finally:
        if user is not None:
            gl.set_stream(None)
        gl.close()
        if gr is not None:
            gr.close()


# lanes of batch B x what A was: a batch read at its last image (the last lane's slice) or at its first, or one synchronous frame
SHAPES = [(4, "batch_last"), (4, "single"), (2, "batch_first"), (2, "single"), (1, "batch_last")]


@pytest.mark.parametrize("stream_kind", ["own", "user"])
@pytest.mark.parametrize("lanes,first", SHAPES)
@pytest.mark.parametrize("reader", sorted(READERS))
def test_reader_is_ordered_before_the_next_batch(world, monkeypatch, reader, lanes, first, stream_kind):
    run_sequence(world, monkeypatch, reader, lanes, first, stream_kind)


@pytest.mark.parametrize("lanes,first", [(4, "batch_last"), (1, "single")])
@pytest.mark.parametrize("reader", ["by_bow", "init_reference_set"])
def test_reader_is_ordered_before_a_new_main_stream(world, monkeypatch, reader, lanes, first):
    run_sequence(world, monkeypatch, reader, lanes, first, "switch")


@pytest.mark.parametrize("stream_kind", ["own", "user"])
def test_transitions_between_single_frames_and_lane_counts(world, monkeypatch, stream_kind):
    """single -> batch K=4 -> batch K=2 -> batch K=1 -> single -> batch K=4 on one handle pair, a short reader (no plug) in every gap and no host
    wait between a reader and the extract that follows it.  At the end of each step: the extract (and the stereo match) against the references,
    and the reader of the step before against the transcription on ITS data."""
    import torch
    W, orb = world, world.orb
    monkeypatch.setenv("JSORB_LANE_MIN_MPX", "0.2")
    rng = np.random.default_rng(2024)
    gl, gr = mk16(orb), mk16(orb)
    user = torch.cuda.Stream() if stream_kind == "user" else None
    kinds = [Local, LocalStereo, LastFrame, Init, ByBow]
    chain = []                                    # (lanes, set, images, image the reader is aimed at, reader); lanes 0: the synchronous single frame
    for lanes, s in [(0, "A"), (4, "B"), (2, "A"), (1, "B"), (0, "B"), (4, "A")]:
        n = IMAGES_OF_LANES[lanes] if lanes else 1
        image = int(rng.choice([0, n - 1]))
        chain.append((lanes, s, n, image, kinds[int(rng.integers(0, len(kinds)))](W, s, image)))
    torch.cuda.synchronize()                      # every reader's inputs and cleared outputs are in place
    try:
        if user is not None:
            gl.set_stream(user.cuda_stream)
        pending = None
        for lanes, s, n, image, rd in chain:
            _extract(W, gl, gr, s, n, single=not lanes)      # right behind the previous step's reader
            gl.sync()
            gr.sync()
            torch.cuda.synchronize()
            _check_extract(W, gl, gr, s, n, lanes or 1)
            if pending is not None:
                pending.check()
            rd.enqueue(gl, image)
            pending = rd
        gl.sync()
        torch.cuda.synchronize()
        pending.check()
    finally:
        if user is not None:
            gl.set_stream(None)
        gl.close()
        gr.close()


# ---- not a test: the two durations the docstring quotes (python -c "import test_gpu_call_order as t; t.measure_plug_and_batch()" on a GPU) ----
def measure_plug_and_batch(orb=None, po=None, reps=5):
    import os
    import torch
    if orb is None:
        torch.cuda.init()
        from jetson_slam_amd import orb
        from oracle import pyoracle as po
        po.build()
    os.environ["JSORB_LANE_MIN_MPX"] = "0.2"
    W = World(orb, po)
    g = mk16(orb)
    user = torch.cuda.Stream()
    g.set_stream(user.cuda_stream)                # the lanes fork from and join the caller's stream: events on it bracket a batch
    plug = Plug(W, "A", calls=1)
    torch.cuda.synchronize()
    res = dict(plug_us=[], batch_us=[], enqueue_batch_host_us=[], n_keypoints_image0=W.n("A", 0))
    import time
    for _ in range(reps + 1):
        _extract(W, g, None, "A", NA)
        g.sync()
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record(user)
        plug.enqueue(g, 0)
        b.record(user)
        t0 = time.perf_counter()
        _extract(W, g, None, "B", NA)
        t1 = time.perf_counter()
        c.record(user)
        g.sync()
        torch.cuda.synchronize()
        assert g.launch_forms()["lanes"] == 4
        res["plug_us"].append(round(a.elapsed_time(b) * 1e3, 1))
        res["batch_us"].append(round(b.elapsed_time(c) * 1e3, 1))
        res["enqueue_batch_host_us"].append(round((t1 - t0) * 1e6, 1))
    g.set_stream(None)
    g.close()
    for k in ("plug_us", "batch_us", "enqueue_batch_host_us"):
        res[k] = res[k][1:]                       # the first round allocates
    print("CALL_ORDER_MEASURED", res)
    return res
