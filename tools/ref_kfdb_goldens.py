"""tests/golden/ref_matcher_kfdb.npz from the reference's own KeyFrameDatabase (src/KeyFrameDatabase.cpp:44-313), BowVector and L1Scoring.

Authoring-only, like tools/ref_mappoint_goldens.py: needs the reference tree.  Builds tools/ref_kfdb/driver.cpp with the reference's
src/KeyFrameDatabase.cpp and DBoW2's BowVector.cpp and ScoringObject.cpp (all unmodified) into oracle/_ref/ (which git ignores), plays every world of
tests/kfdb_cases.py (imported, not copied) through it and stores the worlds and what the reference computed - inputs and outputs only.  Before
anything is written the transcription and the restatement (for both builds' caps) must equal the reference on every world, doubles as bits, every
constructed case must decide what it names, and every coverage counter of every random block must be non-zero.

Usage: python tools/ref_kfdb_goldens.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kfdb_cases as kc                              # noqa: E402  (tests/kfdb_cases.py: what both this tool and the tests run)


def main():
    reference = kc.reference_tree()
    assert reference, "the reference tree is missing (JSORB_REFERENCE)"
    kc.build_driver(reference)
    cases = kc.constructed()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, w in kc.fixture_worlds().items():
            ref = kc.run_driver(w, tmp)
            t = kc.Transcription(w)
            mine = kc.run(w, t)
            assert kc.same(ref, mine) is None, "%s: the transcription is not the reference (%s)" % (name, kc.same(ref, mine))
            for caps in (kc.SHIPPED, kc.TINY):
                res = kc.run(w, kc.Restatement(w, caps))
                assert kc.same(ref, res) is None, "%s: the restatement is not the reference (%s)" % (name, kc.same(ref, res))
                assert kc.same(mine, res, ("stats", "best_acc")) is None and mine["order"] == res["order"], name
            if name.startswith("random"):
                zero = [k for k, v in t.count.items() if v == 0]
                assert not zero, "%s: coverage counters are zero: %s" % (name, zero)
            else:
                cases[name[2:]][1](mine)
            out[name] = dict(w, counters=np.array([t.count[k] for k in kc.COUNTERS], np.int64), **{"out_" + k: ref[k] for k in kc.OUT_KEYS})
    path = kc.save_golden(out)
    print("%s: %d worlds, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
