"""tests/golden/ref_matcher_vocab_create.npz against the reference's own TemplatedVocabulary::create, compiled unmodified (tools/ref_vocab/): where
the reference tree is present the driver is built and run again, every world in a process of its own, and must reproduce the file.  No GPU."""
import numpy as np

import vocab_train_cases as vc


def test_the_file_is_small_and_holds_the_recorded_worlds():
    import os
    g = vc.load_golden()
    assert list(g) == vc.RECORDED and os.path.getsize(vc.golden_path()) < 500000
    for name, ref in g.items():
        w = vc.world_any(name)
        assert ref["n_nodes"] == len(ref["parent"]) >= 2 and ref["descriptors"].shape == (ref["n_nodes"], 32), name
        assert ("Ni" in ref) == (w["weighting"] in (vc.TF_IDF, vc.IDF)), name


def test_the_driver_reproduces_the_file(tmp_path):
    reference = vc.reference_tree()
    if reference is None:
        return                                   # no reference tree here: the file stands for it (tests/test_vocab_train_host.py holds both statements to it)
    vc.build_driver(reference)
    for name, ref in vc.load_golden().items():
        w = vc.world_any(name)
        got = vc.run_driver(w, str(tmp_path))
        assert got is not None, name
        ni = vc.ni_from_weights(got, w)
        if ni is not None:
            got["Ni"] = ni
        assert vc.same_as_reference(ref, got) is None and (ni is None or np.array_equal(ni, ref["Ni"])), (name, vc.same_as_reference(ref, got))
