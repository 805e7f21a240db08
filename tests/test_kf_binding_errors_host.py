"""No GPU: the JsorbError texts of KeyframeMatcher's four argument builders (_args, _fuse_args, _bow_kf_args, _sim3_args), fed stand-in tensor
objects (tests/kf_refusal_cases.py: binding_rows), against the "bindings" rows of tests/golden/kf_matcher_refusals.json - recorded from the
commit before the builders shared their side checker, never from the tree."""
import json

import pytest

import kf_refusal_cases as cases


@pytest.fixture(scope="module")
def recorded():
    with open(cases.GOLDEN) as f:
        return json.load(f)["bindings"]


@pytest.fixture(scope="module")
def raised(orb):
    return cases.binding_rows(orb)


def test_every_row_raises_the_recorded_text(recorded, raised):
    assert sorted(raised) == sorted(recorded)        # the same rows: none dropped, none new without a recording
    for row in recorded:
        assert raised[row] == recorded[row], (row, raised[row], recorded[row])


@pytest.mark.parametrize("what, sides", [("tri", ("kf1", "kf2")), ("fuse", ("points", "kfs")), ("bow_kf", ("kf1", "cands")), ("sim3", ("s1", "s2"))])
def test_the_recording_has_a_row_per_message_and_side(recorded, what, sides):
    for side in sides:
        for fault, text in (("not_a_tensor", "must be a device tensor"), ("not_on_the_device", "must be a device tensor"), ("dtype", "must be a contiguous"),
                            ("shape", "must be a contiguous"), ("not_contiguous", "must be a contiguous")):
            row = recorded["%s/%s/%s" % (what, side, fault)]
            assert row.startswith("JsorbError: ") and text in row, (what, side, fault, row)
        assert any(k.startswith("%s/%s/misaligned_" % (what, side)) and v.endswith("must be 16-byte aligned") for k, v in recorded.items())
    assert recorded[what + "/ok"] == "ok" and "params must come from make_" in recorded[what + "/params_class"]


def test_the_recording_has_the_call_level_rows(recorded):
    for what in ("tri", "fuse", "bow_kf"):
        for row in ("kf_start_2d", "kf_start_empty"):
            assert recorded["%s/%s" % (what, row)].endswith("kf_start must be a host array of n_keyframes + 1 offsets")
    for row in ("tri/F12_count", "tri/epipole_count"):
        assert recorded[row].endswith("F12 must hold 9 and epipole 2 floats per keyframe")
    for row in ("fuse/Rcw_count", "fuse/tcw_count", "fuse/Ow_count"):
        assert recorded[row].endswith("Rcw must hold 9, tcw 3 and Ow 3 floats per keyframe")
    for row in ("fuse/skip_not_on_the_device", "fuse/skip_dtype", "fuse/skip_count", "fuse/skip_not_contiguous"):
        assert recorded[row].endswith("skip must be a contiguous uint8 / bool device tensor of n_keyframes x n_points entries")
    assert recorded["fuse/skip_ok"] == "ok" and recorded["fuse/uright_none"] == "ok"
    for side, name in (("s1", "side1"), ("s2", "side2")):
        for k, size in (("Rw", 9), ("tw", 3), ("sR", 9), ("t", 3)):
            assert recorded["sim3/%s/pose_%s" % (side, k)] == "JsorbError: search_by_sim3: %s['%s'] must hold %d floats" % (name, k, size)
    assert recorded["sim3/params_before_self"].startswith("JsorbError: ")      # raised with None as self: before self is touched


# ---- the host arrays a builder converts stay alive through the C call ----
class RecordingLib:
    """stands in for the library: every entry point first allocates numpy arrays of the sizes the converted inputs have (what numpy's
    small-block cache would hand a freed copy's memory to), then reads the memory behind the host addresses it was passed"""

    def __init__(self, reads):
        self.reads, self.seen = reads, {}

    def __getattr__(self, name):
        def call(m, *args):
            import ctypes as C
            import numpy as np
            churn = [np.full(n, -7, dt) for _, dt, n in self.reads.values() for _ in range(8)]
            for key, (index, dt, n) in self.reads.items():
                self.seen[key] = np.frombuffer(C.string_at(args[index], n * np.dtype(dt).itemsize), dt).copy()
            del churn
            return 0
        return call


@pytest.mark.parametrize("host", [False, True])
def test_converted_host_arrays_outlive_the_builder(orb, monkeypatch, host):
    """kf_start as a list and the per-keyframe geometry as float64 (both accepted: np.ascontiguousarray copies them): what the C call reads
    behind the addresses is still the input, although the runner allocates its outputs between the builder and the call"""
    import numpy as np
    import torch
    K = orb.KeyframeMatcher
    i32, u8, f32 = torch.int32, torch.uint8, torch.float32
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"synchronize": lambda self: None})())

    def side(keys, n, dtypes):
        return {k: cases.FakeTensor(dtypes.get(k, f32), (n, 32) if k.endswith("desc") else (n,)) for k in keys}

    ks = [0, 2, 4, 5]
    rng = np.random.default_rng(5)
    F12, epi, R, t, O = (rng.normal(size=(3, w)) for w in (9, 2, 9, 3, 3))          # float64
    m = K.__new__(K)
    m._m = None
    tri_dt = dict(node=i32, octave=i32, free=u8, stereo=u8, desc=u8)
    calls = [
        ("search_for_triangulation", dict(kf_start=(10, np.int32, 4), F12=(19, np.float32, 27), epipole=(20, np.float32, 6)),
         lambda f: f(side(K.KF1_KEYS, 3, tri_dt), ks, side(K.KF2_KEYS, 5, tri_dt), F12, epi, orb.make_triangulation_params([1.0]))),
        ("fuse", dict(kf_start=(13, np.int32, 4), Rcw=(19, np.float32, 27), tcw=(20, np.float32, 9), Ow=(21, np.float32, 9)),
         lambda f: f(side(K.POINT_KEYS, 3, dict(desc=u8)), ks, side(K.FUSE_KF_KEYS, 5, dict(octave=i32, desc=u8)), R, t, O,
                     orb.make_fuse_params((1, 1, 0, 0), (0, 1, 0, 1), (1, 1), 0.18, [1.0]))),
        ("search_by_bow_kf", dict(kf_start=(7, np.int32, 4)),
         lambda f: f(side(K.BOW_KF_KEYS, 3, dict(node=i32, valid=u8, desc=u8)), ks, side(K.BOW_KF_KEYS, 5, dict(node=i32, valid=u8, desc=u8)),
                     orb.make_bow_params())),
    ]
    want = dict(kf_start=np.array(ks, np.int32), F12=F12, epipole=epi, Rcw=R, tcw=t, Ow=O)
    for name, reads, call in calls:
        m._lib = RecordingLib(reads)
        method = getattr(m, name + "_host") if host else getattr(m, name)
        call(method if host else (lambda *a, _f=method: _f(*a, wait=False)))
        assert sorted(m._lib.seen) == sorted(reads), name
        for key, got in m._lib.seen.items():
            assert np.array_equal(got, np.asarray(want[key]).astype(got.dtype).reshape(-1)), (name, key, got)
