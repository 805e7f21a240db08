"""Both host statements of tests/distinct_cases.py against what the reference's own MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:273-338,
compiled unmodified: tools/ref_mappoint/) left in mDescriptor, as tests/golden/ref_matcher_mappoint_distinctive.npz records it; where the reference tree is
present the driver is built and run again and must reproduce the file.  Six mutants of the transcription must each fail a recorded case.  No GPU."""
import numpy as np
import pytest

import distinct_cases as dc

WORLD_KEYS = ("kf_start", "kf_desc", "kf_bad", "obs_start", "obs_kf", "obs_idx")


@pytest.fixture(scope="module")
def golden():
    return dc.load_golden()


def test_the_file_holds_the_worlds_the_tests_generate(golden):
    worlds = dc.fixture_worlds()
    assert list(golden) == list(worlds)
    for name, w in worlds.items():
        for k in WORLD_KEYS:
            assert np.array_equal(golden[name][k], w[k]) and golden[name][k].dtype == w[k].dtype, (name, k)
        if name.startswith("random"):
            assert (golden[name]["counters"] > 0).all(), name


def test_transcription_and_restatement_give_the_reference_bytes(golden):
    for name, g in golden.items():
        want, bo, bm = dc.world_reference(g)
        assert np.array_equal(g["out_has"], (bo >= 0).astype(np.uint8)) and np.array_equal(g["out_desc"], want), name
        start, row = dc.csr(g)
        for caps in (dc.SHIPPED, dc.TINY):
            r = dc.restatement(start, row, g["kf_desc"], desc_out=np.zeros_like(want), caps=caps)
            assert np.array_equal(r["desc_out"], g["out_desc"]) and np.array_equal(r["best_obs"] >= 0, g["out_has"] != 0), (name, caps)
        # an old descriptor stays where the reference leaves mDescriptor alone
        old = np.full_like(want, 0x77)
        kept = dc.restatement(start, row, g["kf_desc"], desc_out=old)["desc_out"]
        assert (kept[g["out_has"] == 0] == 0x77).all() and np.array_equal(kept[g["out_has"] != 0], g["out_desc"][g["out_has"] != 0]), name
    names = list(dc.constructed())
    g = golden["constructed"]
    _, bo, bm = dc.world_reference(g)
    for p, n in enumerate(names):
        if dc.constructed()[n][1] is not None:
            assert (bo[p], bm[p]) == dc.constructed()[n][1:], n


def test_the_driver_reproduces_the_file(golden, tmp_path):
    reference = dc.reference_tree()
    if reference is None:
        return                                   # no reference tree here: the file stands for it (the tests above hold both statements to it)
    dc.build_driver(reference)
    for name, g in golden.items():
        has, desc = dc.run_driver(g, str(tmp_path))
        assert np.array_equal(has, g["out_has"]) and np.array_equal(desc, g["out_desc"]), name


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_every_mutant_fails_a_recorded_case(golden, mutant):
    failed = 0
    for name, g in golden.items():
        start, row = dc.csr(g)
        for p in np.nonzero(np.diff(start) > 0)[0]:
            if start[p + 1] - start[p] > 100:
                continue                         # (the small points decide; the two largest only cost time)
            rows = row[start[p]:start[p + 1]]
            failed += not np.array_equal(g["kf_desc"][rows[dc.mutant_point(g["kf_desc"][rows], mutant)]], g["out_desc"][p])
    assert failed > 0, mutant
