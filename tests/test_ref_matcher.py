"""CPU: the matchers' two host yardsticks against the reference's OWN src/ORBmatcher.cpp.

tests/golden/ref_matcher_<name>.npz (tools/ref_matcher_goldens.py) hold, per entry point, the inputs of the host tests' random generators and
constructed cases and what the reference's matcher - compiled unmodified against the stand-in headers of oracle/ref_matcher/ - returned for them.
Here the sequential Python transcription and the numpy restatement of the kernels of each matcher (tests/test_*_host.py) run on the stored inputs
and must give the stored outputs bit for bit: match vectors, counts, vbPrevMatched.  Where oracle/_ref/libref_matcher.so exists (the reference
tree was present when the project was built) the drivers run again and must return what the files hold; only that part skips without it.
tests/test_gpu_ref_matcher.py holds the device to the same files."""
import os

import numpy as np
import pytest

import fuse_replay
import ref_matcher_cases as cases
from oracle import pyref_matcher as rm

NAMES = list(cases.MATCHERS)


@pytest.fixture(scope="module")
def goldens():
    return {name: {k: cases.named(cases.MATCHERS[name].prepare(c), cases.MATCHERS[name].driver, k) for k, c in rm.load_golden(name).items()} for name in NAMES}


@pytest.mark.parametrize("kind", ["transcription", "restatement"])
@pytest.mark.parametrize("name", NAMES)
def test_host_yardstick_equals_the_reference(po, goldens, name, kind):
    m = cases.MATCHERS[name]
    n_matches = 0
    for cname, c in goldens[name].items():
        try:
            m.same(c, getattr(m, kind)(po, c))
        except AssertionError as e:
            raise AssertionError("%s / %s: the %s differs from the reference's ORBmatcher.cpp" % (name, cname, kind)) from e
        n_matches += int(c["out"]["nmatches"])
    assert n_matches > 100                     # not vacuous: the reference matched


@pytest.mark.parametrize("name", NAMES)
def test_fixture_coverage(po, goldens, name):
    """the stored trace counters are the transcription's on the stored inputs, and every counter the host test of the matcher requires to be
    non-zero is non-zero on every random block; every file has at least two random blocks and stays under 500 KB"""
    m = cases.MATCHERS[name]
    blocks = {}
    for cname, c in goldens[name].items():
        got = m.counters(po, c, m.transcription(po, c))
        assert set(got) == set(c["counters"]) and all(np.array_equal(np.asarray(got[k]), c["counters"][k]) for k in got), cname
        if cases.block_of(cname):
            tot = blocks.setdefault(cases.block_of(cname), dict.fromkeys(m.required, 0))
            for k in m.required:
                tot[k] += int(c["counters"][k])
    assert len(blocks) >= 2
    for bname, tot in blocks.items():
        assert all(v > 0 for v in tot.values()), (name, bname, tot)
    assert os.path.getsize(rm.golden_path(name)) < 500 * 1000


@pytest.mark.parametrize("name", NAMES)
def test_reference_library_still_returns_the_stored_outputs(goldens, name):
    """keeps the fixtures and the recipe (oracle/Makefile: ref_matcher, oracle/ref_matcher/) from drifting apart"""
    if not rm.available():
        pytest.skip("oracle/_ref/libref_matcher.so is built only where the reference tree is present")
    m = cases.MATCHERS[name]
    for repeat in range(2):                    # the last-frame matcher keeps static buffers: the drivers are called again, sizes interleaved
        for cname, c in goldens[name].items():
            out = rm.run(m.driver, c)
            assert set(out) == set(c["out"]), cname
            for k, v in out.items():
                a, b = np.asarray(v), np.asarray(c["out"][k])
                assert a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes(), (name, cname, k)


# ---- the two Fuse overloads: the replay on a live map, the descriptor question, the sensitivity of the fixtures ----
FUSE_NAMES = [n for n in NAMES if n.startswith("fuse")]
DESCRIPTOR_CASES = ("descriptor_changes_between_keyframes", "descriptor_changes_three_keyframes")


@pytest.mark.parametrize("name", FUSE_NAMES)
def test_fuse_cases_are_exact_and_the_sequential_replay_is_the_reference(po, goldens, name):
    """per case: every float step in which the contract's fused route and the reference's route differ is exact, no level depends on the logf in
    use, the transcription searched keyframe by keyframe on the live map gives the reference's event log, map and nFused, and the reference's own
    u, v, dist3D, level and radius (its probe log) are the contract's bit for bit"""
    m = cases.MATCHERS[name]
    reached = 0
    for cname, c in goldens[name].items():
        try:
            m.verify(po, c)
        except AssertionError as e:
            raise AssertionError("%s / %s" % (name, cname)) from e
        reached += len(c["out"]["probe"])
    assert reached > 2000


@pytest.mark.parametrize("kind", ["transcription", "restatement"])
@pytest.mark.parametrize("name", FUSE_NAMES)
def test_one_batched_search_needs_the_search_again_after_a_descriptor_change(po, goldens, name, kind):
    """MapPoint::Replace ends with ComputeDistinctiveDescriptors on the surviving point (MapPoint.cpp:243), and SearchInNeighbors / SearchAndFuse
    search that point in the next keyframe with its new descriptor.  So one search of all keyframes from the descriptors as they were before the
    call, replayed, is NOT the reference's loop - on the constructed cases and on every random block - and it is once the points whose
    descriptor changed are searched again in the keyframes not yet replayed (include/jsorb.h)."""
    m = cases.MATCHERS[name]
    differs = set()
    for cname, c in goldens[name].items():
        search = cases.fuse_search(po, c, kind)
        batched = fuse_replay.replay(c, search, "batched")[0]
        again = fuse_replay.replay(c, search, "research")[0]
        fuse_replay.same_map(again, c["out"])
        if not cases._same(batched, c["out"]):
            differs.add(cname)
            assert int(c["counters"]["descriptor_changes"]) > 0, cname      # nothing else makes the batched replay differ
        assert int(cname in differs) == int(c["counters"]["differs_without_research"]), cname
    assert set(DESCRIPTOR_CASES) <= differs
    assert {"random0", "random1"} <= {cases.block_of(n) for n in differs}
    # the constructed case by hand: the old descriptor (bits 0) takes keypoint 0 of keyframe 1, the new one (bits 20) keypoint 1
    c = goldens[name][DESCRIPTOR_CASES[0]]
    search = cases.fuse_search(po, c, kind)
    old, new = fuse_replay.replay(c, search, "batched")[2][0], fuse_replay.replay(c, search, "research")[2][0]
    assert old[:, 0].tolist() == [0, 0] and new[:, 0].tolist() == [0, 1]


# one decision of the transcription flipped: the stored cases that must notice (at least one each).  Not listed, because no output can change:
#   Pcz >= 0 in place of Pcz > 0 - at Pcz == 0 the pixel is infinite or NaN and IsInImage fails either way (the reference's own text is Pcz < 0: skip);
#   a contracted ur = fma(-bf, invz, u) - on inputs built for bit equality bf * invz is exact (a power-of-two depth), so both forms round once;
#     the case that tells them apart (tests/test_fuse_host.py: contraction_ur, depth 3) cannot be a reference fixture, because 1/3 already makes the
#     reference's own u differ from the contract's.  It stays pinned by the host and GPU tests of the matcher only.
# (dist <= bestDist IS listed for both overloads: Fuse has no ratio test, so a tie changes bestIdx.)
FUSE_MUTANTS = {"tie_le": ("tie_within_a_cell",), "th_low_strict": ("th_low_accepted",), "closed_image": ("u_at_max_x_with_a_candidate", "v_at_max_y_with_a_candidate"),
                "level_above": ("octave_above_the_level",), "float_threshold": ("chi_square_at_float_7_8",)}


# (the overload with Scw has no chi-square gate: the float threshold does not exist there)
@pytest.mark.parametrize("name,mutant", [(n, m) for n in FUSE_NAMES for m in sorted(FUSE_MUTANTS) if (n, m) != ("fuse_sim3", "float_threshold")])
def test_fuse_fixtures_notice_one_flipped_decision(po, goldens, name, mutant):
    failed = []
    ordered = sorted(goldens[name], key=lambda n: (cases.block_of(n) is not None, n))      # the constructed cases first
    for cname in ordered:
        c = goldens[name][cname]
        got = fuse_replay.replay(c, cases.fuse_search(po, c, "transcription", mutant), "sequential")[0]
        if not cases._same(got, c["out"]):
            failed.append(cname)
            if set(FUSE_MUTANTS[mutant]) <= set(failed):
                break
    assert failed and set(FUSE_MUTANTS[mutant]) <= set(failed), (name, mutant, failed)


@pytest.mark.parametrize("mutant", ["depth_ge", "contract_ur"])
@pytest.mark.parametrize("name", FUSE_NAMES)
def test_fuse_mutants_that_change_no_output(po, goldens, name, mutant):
    """the two explanations above as a check: Pcz >= 0 and a contracted ur leave every stored case as it is (should the fixtures become sensitive to
    one of them, it belongs into FUSE_MUTANTS)"""
    for cname, c in goldens[name].items():
        got = fuse_replay.replay(c, cases.fuse_search(po, c, "transcription", mutant), "sequential")[0]
        fuse_replay.same_map(got, c["out"])


# SearchBySim3: one decision flipped (tests/test_loop_host.py's transcription; "ignore_matched2" drops :1125-1127 from the sides) and the stored
# cases that must notice.  Pcz >= 0 changes no output, as for Fuse.
SIM3_MUTANTS = {"tie_le": ("tie_first_in_walk_order",), "th_high_strict": ("th_high_accepted",), "closed_image": ("u_at_max_x_with_a_candidate",),
                "level_above": ("octaves_around_the_level",), "no_agreement": ("agrees_one_way_only",), "ignore_matched2": ("already_matched2_in_range",)}


@pytest.mark.parametrize("mutant", sorted(SIM3_MUTANTS))
def test_sim3_fixtures_notice_one_flipped_decision(po, goldens, mutant):
    m = cases.MATCHERS["search_by_sim3"]
    failed = []
    for cname, c in goldens["search_by_sim3"].items():
        try:
            m.same(c, m.transcription(po, c, mutant))
        except AssertionError:
            failed.append(cname)
    assert set(SIM3_MUTANTS[mutant]) <= set(failed), (mutant, failed)


def test_sim3_cases_are_exact_and_the_probes_are_the_contracts(po, goldens):
    """per case: the chain through both cameras, the pixel and dist3D^2 are exact in float32 on both routes, no level depends on the logf in use, and
    the reference's own u, v, dist3D, level and radius (its probe log) are the contract's bit for bit"""
    m = cases.MATCHERS["search_by_sim3"]
    for cname, c in goldens["search_by_sim3"].items():
        try:
            m.verify(po, c)
        except AssertionError as e:
            raise AssertionError(cname) from e
    assert sum(len(c["out"]["probe"]) for c in goldens["search_by_sim3"].values()) > 1000


# SearchByProjection(Frame, KeyFrame): one decision of tests/test_search_kf_host.py's transcription flipped and the stored cases that must notice
KF_MUTANTS = {"half_open": ("u_at_max_x_is_in", "v_at_max_y_is_in"), "level_window": ("octaves_around_the_level",), "claim_ignored": ("claimed_keypoint_is_no_candidate",),
              "cull_first": ("culled_keypoint_stays_hidden",), "tie_le": ("tie_first_in_walk_order",)}


@pytest.mark.parametrize("mutant", sorted(KF_MUTANTS))
def test_search_kf_fixtures_notice_one_flipped_decision(po, goldens, mutant):
    m = cases.MATCHERS["search_kf"]
    failed = []
    for cname, c in goldens["search_kf"].items():
        try:
            m.same(c, m.transcription(po, c, mutant))
        except AssertionError:
            failed.append(cname)
    assert set(KF_MUTANTS[mutant]) <= set(failed), (mutant, failed)
    assert mutant == "half_open" or any(cases.block_of(n) for n in failed), (mutant, failed)      # (no random pixel lies on a bound)


def test_search_kf_cases_are_exact_and_the_probes_are_the_contracts(po, goldens):
    """per case: the projection through the frame's pose and dist3D^2 are exact in float32 on both routes, no level depends on the logf in use, and the
    reference's own dist3D, level, u, v and radius (what it hands to PredictScale and Frame::GetFeaturesInArea) are the contract's bit for bit"""
    m = cases.MATCHERS["search_kf"]
    for cname, c in goldens["search_kf"].items():
        try:
            m.verify(po, c)
        except AssertionError as e:
            raise AssertionError(cname) from e
    assert sum(len(c["out"]["probe"]) for c in goldens["search_kf"].values()) > 2000


def test_stated_differences_are_stored_cases(goldens):
    """every entry of STATED_DIFFERENCES names a stored case (its two sides are asserted by the matcher's same() and by split_probe in verify());
    a depth of zero or below is in every file of a projecting matcher"""
    for (name, cname), d in cases.STATED_DIFFERENCES.items():
        assert cname in goldens[name], (name, cname)
        rows = np.asarray(goldens[name][cname]["out"]["probe"], np.float32).reshape(-1, 5)
        assert int((~np.isfinite(rows).all(1)).sum()) == d["nonfinite_probe_rows"], (name, cname)
    assert {n for n, _ in cases.STATED_DIFFERENCES} == {"search_kf", "fuse", "fuse_sim3", "search_by_sim3"}
