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

import ref_matcher_cases as cases
from oracle import pyref_matcher as rm

NAMES = list(cases.MATCHERS)


@pytest.fixture(scope="module")
def goldens():
    return {name: rm.load_golden(name) for name in NAMES}


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
