"""Fixtures from the live reference: tests/golden/ref_matcher_<name>.npz, one per matcher entry point.

Authoring-only, like tools/ptx_chain.py: it needs oracle/_ref/libref_matcher.so, the reference's own src/ORBmatcher.cpp compiled against the
stand-in headers of oracle/ref_matcher/ (python __graft_entry__.py builds it where the reference tree is present).  The inputs are the random
generators and constructed cases of the host tests (imported from tests/, not copied); each file holds them as the drivers take them, what the
reference returned, and the trace counters of the Python transcription on the same inputs.  A "random block" is a run of consecutive cases from
one seeded generator; every counter the host test of that matcher requires to be non-zero must be non-zero on every block, or the tool fails.

What the reference cannot be given is changed in the INPUT, never left out of a comparison (DESIGN.md section 6 lists it):
 - its thresholds are compiled in (TH_LOW = 50, TH_HIGH = 100) and its asserts are on: cases drawn with other thresholds run with these;
 - a level or octave outside the pyramid makes it read outside mvScaleFactors: such values are taken modulo the number of levels;
 - the device holds integer keypoint coordinates and a fixed keypoint count: the generators' frames of the three frame-handle matchers are
   stored with rounded coordinates, padded to the count of the handle they are written over (tests/ref_matcher_cases.py: on_handle);
 - an angle difference outside [0, 360) makes it index outside its histogram: such angles are folded into [0, 360).
 - the projecting matchers (both Fuse overloads, SearchBySim3, SearchByProjection(Frame, KeyFrame)) compute pixel, distance and level on the device with K14 / K16's fused steps and in
   the reference with separate float products and sums: their cases are built on inputs for which every such step is exact in float32 (rotations
   that are signed permutations, power-of-two depths and scales, fx = fy = 256, a quarter-pixel grid), and the tool PROVES it per case
   (ref_matcher_cases.prove_exact*), requires that no level depends on the logf in use, and that the reference's own u, v, dist3D, level and radius
   (the harness's probe log) equal the contract's bit for bit, before it writes the case (Matcher.verify).
 - where the library's contract differs from the reference's text on purpose (a depth of zero or below), the file stores the reference's output
   and ref_matcher_cases.STATED_DIFFERENCES holds both sides.

Usage: python tools/ref_matcher_goldens.py [name ...]      (no name: all)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as po                    # noqa: E402
from oracle import pyref_matcher as rm               # noqa: E402
import ref_matcher_cases as cases                    # noqa: E402  (tests/ref_matcher_cases.py: what both this tool and the tests run)

f32 = np.float32


def main(names):
    po.build()
    assert rm.available(), "oracle/_ref/libref_matcher.so is missing: run python __graft_entry__.py where the reference tree is present"
    for name in names or cases.MATCHERS:
        m = cases.MATCHERS[name]
        out, blocks = {}, {}
        for cname, case in m.build(po).items():
            case = cases.named(m.prepare(dict(case)), m.driver, cname)
            case["out"] = rm.run(m.driver, case)
            m.verify(po, case)
            case["counters"] = {k: np.asarray(v, np.int64) for k, v in m.counters(po, case, m.transcription(po, case)).items()}
            out[cname] = case
            if cases.block_of(cname):
                tot = blocks.setdefault(cases.block_of(cname), dict.fromkeys(m.required, 0))
                for k in m.required:
                    tot[k] += int(case["counters"][k])
        for bname, tot in blocks.items():
            zero = [k for k, v in tot.items() if v == 0]
            assert not zero, "%s %s: counters the host test requires to be non-zero are zero: %s" % (name, bname, zero)
        path = rm.save_golden(name, out)
        print("%-28s %3d cases %7d bytes  %s" % (name, len(out), os.path.getsize(path), os.path.relpath(path, ROOT)))
        assert os.path.getsize(path) < 500 * 1000, path


if __name__ == "__main__":
    main(sys.argv[1:])
