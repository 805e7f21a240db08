#!/usr/bin/env python
"""Authors tests/golden/ref_matcher_covis.npz: the worlds of tests/covis_cases.golden_worlds() run through the reference's own src/KeyFrame.cpp
(tools/ref_covis/driver.cpp over stand-in headers; the binary goes to oracle/_ref/, which git ignores).  Needs the reference tree
(JSORB_REFERENCE, default /root/reference); nothing of its text ends up in the repository - the file holds recorded arrays only.

    python tools/ref_covis_goldens.py            # build the driver, run the worlds, check both yardsticks against them, write the file
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import covis_cases as cc      # noqa: E402


def main():
    ref = cc.reference_tree()
    if ref is None:
        sys.exit("the reference tree is not here")
    cc.build_driver(ref)
    recorded = {}
    with tempfile.TemporaryDirectory() as tmp:
        for w in cc.golden_worlds():
            rec = cc.run_driver(w, tmp)
            r = cc.run_restated(w)
            assert not cc.overflowed(r), w["name"]
            cc.same_as_recorded(w, r, rec)
            cc.same_as_recorded(w, cc.run_literal(w), rec)
            recorded[w["name"]] = rec
    path = cc.write_golden(recorded)
    print("%s: %d worlds, %d steps, %d bytes" % (path, len(recorded), sum(len(r["lens"]) for r in recorded.values()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
