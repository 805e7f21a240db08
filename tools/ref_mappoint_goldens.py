"""tests/golden/ref_matcher_mappoint_distinctive.npz from the reference's own MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:273-338).

Authoring-only, like tools/ref_matcher_goldens.py: needs the reference tree.  Builds tools/ref_mappoint/driver.cpp with the reference's
src/MapPoint.cpp, src/ORBmatcher.cpp and DBoW2's FeatureVector.cpp (all unmodified) into oracle/_ref/ (which git ignores), runs every world of
tests/distinct_cases.py (imported, not copied) through it and stores the worlds and what the reference left in mDescriptor - inputs and outputs only.
Before anything is written the transcription and the restatement must give the reference's bytes, every constructed case its stated winner, and every
coverage counter of every random block must be non-zero.

Usage: python tools/ref_mappoint_goldens.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import distinct_cases as dc                          # noqa: E402  (tests/distinct_cases.py: what both this tool and the tests run)


def main():
    reference = dc.reference_tree()
    assert reference, "the reference tree is missing (JSORB_REFERENCE)"
    dc.build_driver(reference)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, w in dc.fixture_worlds().items():
            has, desc = dc.run_driver(w, tmp)
            want, bo, bm = dc.world_reference(w)
            assert np.array_equal(has, (bo >= 0).astype(np.uint8)) and np.array_equal(desc, want), "%s: the transcription is not the reference" % name
            start, row = dc.csr(w)
            res = dc.restatement(start, row, w["kf_desc"], desc_out=np.zeros_like(want))
            assert np.array_equal(res["desc_out"], desc) and np.array_equal(res["best_obs"], bo), "%s: the restatement is not the reference" % name
            counters = dc.coverage(w, bo)
            if name.startswith("random"):
                zero = [k for k, v in counters.items() if v == 0]
                assert not zero, "%s: coverage counters are zero: %s" % (name, zero)
            else:
                cases = dc.constructed()
                for p, n in enumerate(cases):
                    assert cases[n][1] is None or (bo[p], bm[p]) == cases[n][1:], n
            out[name] = dict(w, out_has=has, out_desc=desc, counter_names=np.array(sorted(counters)), counters=np.array([counters[k] for k in sorted(counters)], np.int64))
    path = dc.save_golden(out)
    print("%s: %d worlds, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
