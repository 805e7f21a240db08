"""-m gpu: jsorb_distinctive_descriptors* against what the reference's own MapPoint::ComputeDistinctiveDescriptors left in mDescriptor
(tests/golden/ref_matcher_mappoint_distinctive.npz, from src/MapPoint.cpp compiled unmodified: tools/ref_mappoint/): every recorded world through the device in
both forms, with the shipped library and under the tiny_distinct build; the rows of the points the reference leaves alone keep their bytes."""
import numpy as np
import pytest

import distinct_cases as dc
from test_gpu_distinct import check, matcher, tiny      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return dc.load_golden()


def through(m, caps, golden):
    for name, g in golden.items():
        start, row = dc.csr(g)
        old = np.full_like(g["out_desc"], 0x77)
        want = np.where((g["out_has"] != 0)[:, None], g["out_desc"], old)
        for sync in (False, True):
            got = check(m, start, row, g["kf_desc"], caps, old=old, sync=sync)
            assert np.array_equal(got["desc_out"], want) and np.array_equal(got["best_obs"] >= 0, g["out_has"] != 0), name


def test_reference_outputs_through_the_device(orb, matcher, golden):      # noqa: F811
    through(matcher, dc.SHIPPED, golden)


def test_reference_outputs_tiny(orb, tiny, golden):                     # noqa: F811
    through(tiny, dc.TINY, golden)
