"""tests/golden/ref_matcher_bow_transform.npz from the reference's own TemplatedVocabulary::loadFromTextFile, saveToTextFile and both forms of
transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259, :1338-1449).

Authoring-only, like tools/ref_vocab_goldens.py: needs the reference tree.  Builds tools/ref_bow/driver.cpp with DBoW2's sources (unmodified) into
oracle/_ref/ (which git ignores), plays every world of tests/bow_ref_cases.py (imported, not copied; the worlds are generated from their names,
so only the reference's outputs are stored - and the frame world's descriptors, which the CPU oracle extracts here) through it, each in a process
of its own, and stores what the reference computed.  Nothing is written unless the reference survives every world, the worlds that may skip
nothing hold no surviving sentinel, and the coverage the worlds were built for is there: stopped words, shallow leaves, the root case, a word
once / twice / many times, an all-stopped and an empty set, the /nd branch.

Usage: python tools/ref_bow_goldens.py"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bow_ref_cases as bc                           # noqa: E402  (tests/bow_ref_cases.py: what both this tool and the tests run)


def main():
    reference = bc.reference_tree()
    assert reference, "the reference tree is missing (JSORB_REFERENCE)"
    bc.build_driver(reference)
    from oracle import pyoracle
    pyoracle.build()
    descs = bc.frame_descriptors(pyoracle)
    bc._cache["frame"] = bc.frame_world(descs)
    out = {}
    seen = dict(stopped=0, shallow=0, root=0, skipped_vector=0, vector=0)
    with tempfile.TemporaryDirectory() as tmp:
        for name in bc.RECORDED:
            w = bc.world(name)
            rec = bc.run_driver(w, tmp)
            assert rec is not None, "%s: the reference died" % name
            if "t_nid" in rec:
                live = rec["t_weight_bits"].view(np.float64) > 0
                kept = rec["t_nid"] == bc.SENTINEL
                assert name not in bc.NO_SHALLOW or not kept.any(), "%s: a shallow leaf" % name
                seen["stopped"] += int((~live).sum())
                seen["shallow"] += int((kept & live).sum())
                seen["root"] += sum(1 for lu in w["levelsup"] if w["tree"]["depth_L"] - lu <= 0)
                seen["skipped_vector"] += int((rec["v_ran"] == 0).sum())
                seen["vector"] += int((rec["v_ran"] == 1).sum())
            out[name] = rec
    out["frame"]["in_desc_left"], out["frame"]["in_desc_right"] = descs
    assert all(v > 0 for v in seen.values()), seen
    path = bc.save_golden(out)
    size = os.path.getsize(path)
    assert size < bc.MAX_BYTES, size
    print("%s: %d worlds, %d bytes; %s" % (path, len(out), size, seen))


if __name__ == "__main__":
    main()
