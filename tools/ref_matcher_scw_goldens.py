"""The fixture of the one matcher oracle/ref_matcher/harness.cpp has no driver for: tests/golden/ref_matcher_search_scw.npz, from the reference's own
ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:277-390).

Authoring-only, like tools/ref_matcher_goldens.py.  oracle/_ref/libref_matcher.so already holds the whole of the reference's ORBmatcher.cpp and the
stand-in KeyFrame / MapPoint members; this tool compiles tools/ref_matcher_scw_driver.cpp against it into oracle/_ref/ (which git ignores) with
oracle/Makefile's REF_FLAGS and -ffp-contract=off, runs every case of tests/scw_cases.py (imported, not copied) through it and stores the inputs,
what the reference returned and the transcription's trace counters.  Before a case is written: the exactness proof (scw_cases.prove), and the
transcription and the restatement must give the reference's vpMatched and return value.  The harness's probe log cannot be switched on from
outside harness.cpp, so only outputs are compared and stored.  The tool refuses to write the file unless every coverage counter is non-zero on
every random block, and reports (does not assert) how many output values the contracted-FMA build of the reference changes.

Usage: python tools/ref_matcher_scw_goldens.py"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as po                    # noqa: E402
from oracle import pyref_matcher as rm               # noqa: E402
import scw_cases as sc                               # noqa: E402  (tests/scw_cases.py: what both this tool and the tests run)


def build_driver(reference):
    """oracle/Makefile's REF_FLAGS, -ffp-contract=off for both: the driver itself computes nothing; the second one links the fused library"""
    ora = os.path.join(ROOT, "oracle")
    shadow = os.path.join(ora, "ref_matcher")
    flags = ["-std=c++14", "-O2", "-fno-fast-math", "-fPIC", "-shared", "-w", "-I" + shadow, "-I" + os.path.join(reference, "include"), "-I" + reference,
             "-include", os.path.join(shadow, "MapPoint.h"), "-include", os.path.join(shadow, "KeyFrame.h"), "-include", os.path.join(shadow, "Frame.h"),
             "-ffp-contract=off"]
    for fused in (False, True):
        assert rm.available(fused), "oracle/_ref/libref_matcher*.so is missing: run python __graft_entry__.py where the reference tree is present"
        subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-o", sc.driver_path(fused), os.path.join(ROOT, "tools", "ref_matcher_scw_driver.cpp"),
                               "-L" + os.path.join(ora, "_ref"), "-lref_matcher" + ("_fused" if fused else ""), "-Wl,-rpath,$ORIGIN"])


def main():
    po.build()
    build_driver(os.environ.get("JSORB_REFERENCE", "/root/reference"))
    out, fused_changes, values = {}, 0, 0
    for name, c in sc.fixture_cases().items():
        proved = sc.prove(c)
        c["out"] = sc.run_driver(c)
        ref, res = sc.both(po, c)
        assert np.array_equal(ref[0], c["out"]["matched"]) and ref[1] == int(c["out"]["nmatches"]), "%s: the transcription is not the reference" % name
        if "want" in c:
            assert np.array_equal(c["want"], c["out"]["matched"]) and int(c["want_count"]) == int(c["out"]["nmatches"]), name
        c["counters"] = dict(sc.trace_of(ref[4]), proved=np.int64(proved), rounds=np.int64(res[sc.SC_CAP][4][0]), overflow_at_2=np.int64(res[sc.TINY[0]][4][2]))
        if name.startswith("random"):                # a random block: one call
            zero = [k for k in sc.COVERAGE if c["counters"][k] == 0] + [k for k in ("overflow_at_2",) if c["counters"][k] == 0]
            assert not zero and c["counters"]["rounds"] >= 4, "%s: coverage counters are zero: %s (rounds %d)" % (name, zero, c["counters"]["rounds"])
        f = sc.run_driver(c, fused=True)
        fused_changes += int((f["matched"] != c["out"]["matched"]).sum()) + int(f["nmatches"] != c["out"]["nmatches"])
        values += len(f["matched"]) + 1
        out[name] = c
    path = rm.save_golden(sc.GOLDEN, out)
    size, limit = os.path.getsize(path), os.path.getsize(rm.golden_path("fuse_sim3"))
    print("%-28s %3d cases %7d bytes  %s" % (sc.GOLDEN, len(out), size, os.path.relpath(path, ROOT)))
    print("the contracted-FMA build of the reference changes %d of %d output values" % (fused_changes, values))
    assert size <= limit, (size, limit)


if __name__ == "__main__":
    main()
