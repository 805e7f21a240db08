"""Records tests/golden/ref_matcher_culling.npz: the worlds of tests/kf_culling_cases.golden_worlds() through the reference's own
src/LocalMapping.cpp, src/KeyFrame.cpp and src/MapPoint.cpp, compiled unmodified against the stand-in headers of tools/ref_culling
(kf_culling_cases.build_driver).  Data only: the driver's int32 output per world and the CRC of its input.  AUTHORING TOOLING: needs the
reference tree (JSORB_REFERENCE, default /root/reference).
Usage: python tools/ref_culling_goldens.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kf_culling_cases as kc  # noqa: E402


def main():
    ref = kc.reference_tree()
    if ref is None:
        sys.exit("the reference tree is not here")
    kc.build_driver(ref)
    recorded = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, W in kc.golden_worlds().items():
            recorded[name] = kc.run_driver(W, tmp)
            for run in (kc.run_literal, kc.run_restated):
                kc.same_as_recorded(W, run(W), recorded[name]["raw"])
    path = kc.write_golden(recorded)
    print("%s: %d worlds, %d bytes" % (path, len(recorded), os.path.getsize(path)))


if __name__ == "__main__":
    main()
