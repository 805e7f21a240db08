"""-m gpu: jsorb_vocabulary_train against what the reference's own TemplatedVocabulary::create computed (tests/golden/ref_matcher_vocab_create.npz,
DBoW2 compiled unmodified: tools/ref_vocab/): every recorded world bit for bit in parent, child_start, children, descriptors, word_id, Ni (where the
weights show it), the weights against math.log on the running machine, the draws consumed and the run count, with no empty cluster and no
unconverged run - with the shipped library and under the tiny_vocab_train build."""
import math

import numpy as np
import pytest

import vocab_train_cases as vc
from test_gpu_vocab_train import lib_orb, train  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return vc.load_golden()


def test_recorded_worlds(lib_orb, golden):  # noqa: F811
    assert list(golden) == vc.RECORDED
    for name, ref in golden.items():
        w = vc.world_any(name)
        got = train(lib_orb, w)
        assert vc.same_as_reference(ref, got) is None, (name, vc.same_as_reference(ref, got))
        assert got["n_empty_clusters"] == 0 and got["n_unconverged"] == 0, name
        n_docs = len(w["doc_start"]) - 1
        for v in np.nonzero(got["word_id"] >= 0)[0]:
            if w["weighting"] in (vc.TF, vc.BINARY):
                assert got["weight"][v] == 1.0
            else:
                assert got["weight"][v] == (math.log(float(n_docs) / float(got["Ni"][v])) if got["Ni"][v] > 0 else 0.0), (name, v)
