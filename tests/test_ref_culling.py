"""-m "not gpu": the two yardsticks of tests/kf_culling_cases.py against the reference's own src/LocalMapping.cpp, src/KeyFrame.cpp and
src/MapPoint.cpp - the worlds recorded in tests/golden/ref_matcher_culling.npz (tools/ref_culling_goldens.py), and, where the reference tree is
present, the driver rebuilt and compared live."""
import numpy as np
import pytest

import kf_culling_cases as kc

WORLDS = kc.golden_worlds()
GOLDEN = kc.load_golden()


def test_the_file_holds_the_worlds_and_nothing_else():
    assert list(GOLDEN) == list(WORLDS) and len(WORLDS) >= kc.GOLDEN_WORLDS + 12
    assert sum(n.startswith("seed_") for n in WORLDS) == kc.GOLDEN_WORLDS and all(len(W["G"]["state"]) <= 16 for W in WORLDS.values())
    n_culled = n_bad = n_records = n_deferred = 0
    for name, rec in GOLDEN.items():
        assert sorted(rec) == ["crc", "raw"] and rec["raw"].dtype == np.int32
        r = kc.run_restated(WORLDS[name])
        n_culled, n_bad, n_records, n_deferred = n_culled + r["counts"][2], n_bad + r["counts"][5], n_records + r["counts"][8], n_deferred + r["counts"][3]
    assert n_culled >= 30 and n_bad >= 8 and n_records >= 20 and n_deferred >= 1, (n_culled, n_bad, n_records, n_deferred)


@pytest.mark.parametrize("name", list(WORLDS))
def test_both_yardsticks_reproduce_the_reference(name):
    W = WORLDS[name]
    kc.same_as_recorded(W, kc.run_restated(W), GOLDEN[name]["raw"])
    kc.same_as_recorded(W, kc.run_literal(W), GOLDEN[name]["raw"])


def test_the_driver_rebuilt_gives_the_recorded_arrays(tmp_path):
    ref = kc.reference_tree()
    if ref is None:
        pytest.skip("the reference tree is not here")
    kc.build_driver(ref)
    for name, W in WORLDS.items():
        rec = kc.run_driver(W, str(tmp_path))
        for k in ("raw", "crc"):
            assert np.array_equal(rec[k], GOLDEN[name][k]), (name, k)
