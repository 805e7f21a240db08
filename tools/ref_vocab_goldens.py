"""tests/golden/ref_matcher_vocab_create.npz from the reference's own TemplatedVocabulary::create (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-996).

Authoring-only, like tools/ref_kfdb_goldens.py: needs the reference tree.  Builds tools/ref_vocab/driver.cpp with DBoW2's sources (unmodified) into
oracle/_ref/ (which git ignores), plays every recorded world of tests/vocab_train_cases.py (imported, not copied; the worlds are generated from
their names, so only the reference's outputs are stored) through it, each in a process of its own, and stores what the reference computed.  Ni is
recovered from the reference's weights and checked (math.log(NDocs / Ni) must give the weight's bits).  Nothing is written unless the reference
survives every recorded world, the transcription counts no empty cluster and no unconverged run in any of them, the transcription and the
level-wise restatement equal the reference on every world, and every coverage counter is non-zero over the worlds together.

Usage: python tools/ref_vocab_goldens.py"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vocab_train_cases as vc                       # noqa: E402  (tests/vocab_train_cases.py: what both this tool and the tests run)

MAX_BYTES = 500000


def main():
    reference = vc.reference_tree()
    assert reference, "the reference tree is missing (JSORB_REFERENCE)"
    vc.build_driver(reference)
    out, total, weightings = {}, vc.new_cov(), set()
    with tempfile.TemporaryDirectory() as tmp:
        for name in vc.RECORDED:
            w = vc.world_any(name)
            ref = vc.run_driver(w, tmp)
            assert ref is not None, "%s: the reference died" % name
            mine = vc.transcribe(**w)
            assert mine["n_empty_clusters"] == 0 and mine["n_unconverged"] == 0, "%s: an empty cluster or an unconverged run" % name
            ni = vc.ni_from_weights(ref, w)
            if ni is not None:
                ref["Ni"] = ni
            for how in (mine, vc.levelwise(**w)):
                assert vc.same_as_reference(ref, how) is None, "%s: not the reference (%s)" % (name, vc.same_as_reference(ref, how))
            for key, v in mine["coverage"].items():
                total[key] += v
            weightings.add(w["weighting"])
            out[name] = {key: ref[key] for key in ref}
    zero = [key for key, v in total.items() if v == 0 and key != "empty_cluster"]
    assert not zero, "coverage counters are zero: %s" % zero
    assert weightings == {0, 1, 2, 3}, weightings
    path = vc.save_golden(out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print("%s: %d worlds, %d bytes; coverage %s" % (path, len(out), size, total))


if __name__ == "__main__":
    main()
