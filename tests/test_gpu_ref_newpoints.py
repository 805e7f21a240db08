"""-m gpu: jsorb_create_new_map_points on the worlds recorded from the reference's own LocalMapping.cpp (tests/golden/ref_matcher_newpoints.npz):
bit-equal to the recording in everything the reference holds of the new points and the keyframes' map points, and to the transcription in the
rest (tests/test_ref_newpoints.py holds the transcription to the same recording)."""
import pytest

import new_points_cases as nc
from test_gpu_new_points import FORMS, DeviceWorld

pytestmark = pytest.mark.gpu
GOLDEN = nc.load_golden()
WORLDS = nc.golden_worlds(GOLDEN)


@pytest.mark.parametrize("name", list(WORLDS))
def test_the_device_reproduces_the_reference(orb, name):
    W = WORLDS[name]
    dw, m, want = DeviceWorld(orb, W), orb.KeyframeMatcher(), nc.restate(W)
    for form in FORMS:
        if form != FORMS[0]:
            dw.load()
        got = dw.create(m, form)
        nc.same_as_recorded(W, got, GOLDEN[name]["raw"], (name, form))
        nc.same(want, got, (name, form))
