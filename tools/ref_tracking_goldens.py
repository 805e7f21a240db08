"""Records tests/golden/ref_matcher_tracking.npz: the worlds of tests/tracking_cases.worlds(), each with use_gpu_ = 1 and with use_gpu_ = 0, through the
front half of the reference's own Tracking::TrackLocalMap - src/Tracking.cpp, src/KeyFrame.cpp and src/MapPoint.cpp compiled unmodified against
the stand-in headers of tools/ref_tracking (tracking_cases.build_driver).  Data only: the driver's int32 output per world and the CRC of its input;
the worlds regenerate from their names and seeds.  AUTHORING TOOLING: needs the reference tree (JSORB_REFERENCE, default /root/reference).

It refuses to write unless the seeded graphs show every drop reason of the local map (n_null, n_duplicates, n_bad, n_seen), a neighbour, a child
and a parent appended, the list's end and a parent as end reasons, a bad top voter, a tie for the maximum vote and an unregistered entry.  The third
end reason, more than 80 keyframes, cannot occur in a graph of at most 64 slots: it is required of the recorded worlds as a whole.
Usage: python tools/ref_tracking_goldens.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import tracking_cases as tc  # noqa: E402

LIMIT = 478508                                   # the largest ref_matcher_*.npz committed before this one


def gate(worlds):
    seeded, whole = dict.fromkeys(tc.COVERAGE, 0), dict.fromkeys(tc.COVERAGE, 0)
    for name, T in worlds.items():
        for k, v in tc.coverage(T).items():
            whole[k] += v
            if name.startswith("seed_"):
                seeded[k] += v
    print("the seeded graphs:", seeded)
    print("every world:", whole)
    missing = [k for k in tc.COVERAGE if not (whole if k == "end_reason_1" else seeded)[k]]
    if missing:
        sys.exit("not written: nothing shows %s" % ", ".join(missing))


def main():
    ref = tc.reference_tree()
    if ref is None:
        sys.exit("the reference tree is not here")
    worlds = tc.worlds()
    gate(worlds)
    tc.build_driver(ref)
    recorded = {}
    with tempfile.TemporaryDirectory() as tmp:
        for T in worlds.values():
            for V in (T, tc.host_variant(T)):
                recorded[V["name"]] = tc.run_driver(V, tmp)
                tc.unpack(V, recorded[V["name"]]["raw"])
    path = tc.write_golden(recorded)
    size = os.path.getsize(path)
    if size >= LIMIT:
        os.remove(path)
        sys.exit("not written: %d bytes, the limit is %d" % (size, LIMIT))
    print("%s: %d worlds, %d bytes" % (path, len(recorded), size))


if __name__ == "__main__":
    main()
