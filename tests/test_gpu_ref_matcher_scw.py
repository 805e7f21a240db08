"""-m gpu: every case of tests/golden/ref_matcher_search_scw.npz - what the reference's own ORBmatcher::SearchByProjection(pKF, Scw, vpPoints,
vpMatched, th) (ORBmatcher.cpp:277-390) returned on an authoring machine - through jsorb_search_by_projection_sim3 on the device, in the
synchronous and the asynchronous form, with the shipped caps and under the tiny_scw_cap build: vpMatched after the call and the return value must be
the reference's.  Only the committed fixture is read here."""
import numpy as np
import pytest

import scw_cases as sc
from oracle import pyref_matcher as rm
from test_gpu_search_scw import check_scw, matcher, tiny  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stored():
    return rm.load_golden(sc.GOLDEN)


def through_the_device(po, orb, m, stored, cap):
    total = 0
    for name, c in stored.items():
        host = None
        for sync in (False, True):
            host = check_scw(po, orb, m, c, sync=sync, cap=cap, host=host)      # (asserts vpMatched after the call against the transcription's)
        ref = host[0]
        assert np.array_equal(ref[0], c["out"]["matched"]) and ref[1] == int(c["out"]["nmatches"]), name
        total += ref[1]
    return total


def test_stored_reference_cases_through_the_device(po, orb, matcher, stored):
    assert through_the_device(po, orb, matcher, stored, sc.SC_CAP) >= 300


def test_stored_reference_cases_under_the_lowered_caps(po, orb, tiny, stored):
    assert through_the_device(po, orb, tiny, stored, sc.TINY[0]) >= 300
