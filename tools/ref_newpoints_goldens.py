"""Records tests/golden/ref_matcher_newpoints.npz: the worlds of tests/new_points_cases.golden_worlds() through the reference's own
src/LocalMapping.cpp, src/KeyFrame.cpp and src/MapPoint.cpp, compiled unmodified against tools/ref_newpoints' opencv2/core/core.hpp and the
stand-in headers of tools/ref_culling (new_points_cases.build_driver), with ORBmatcher::SearchForTriangulation stubbed by the rule of
ORBmatcher.cpp:686-690 over recorded candidates.  Data only: the driver's output per world (the created points with their fields, every
keyframe's map points, the cos_stereo its libm gave) and the CRC of its input.  AUTHORING TOOLING: needs the reference tree (JSORB_REFERENCE).
Usage: python tools/ref_newpoints_goldens.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import new_points_cases as nc  # noqa: E402


def main():
    ref = nc.reference_tree()
    if ref is None:
        sys.exit("the reference tree is not here")
    nc.build_driver(ref)
    recorded = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, W in nc.golden_worlds().items():
            recorded[name] = nc.run_driver(W, tmp)
        for name, W in nc.golden_worlds(recorded).items():
            n = nc.same_as_recorded(W, nc.restate(W), recorded[name]["raw"], name)
            print(name, "created", n)
    path = nc.write_golden(recorded)
    print("%s: %d worlds, %d bytes" % (path, len(recorded), os.path.getsize(path)))


if __name__ == "__main__":
    main()
