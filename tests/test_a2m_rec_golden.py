"""The project's restatement of the HumanAct12 recognition GRU (tests/a2m_rec_ref.py) against the reference's own MotionDiscriminator /
MotionDiscriminatorForFID (tests/golden/a2m_rec.npz, written by tools/make_golden_a2m_rec.py on the seeded stand-in weights): float32 on both sides,
the same formulas, so within 1e-5 absolute (tests/test_t2m_golden.py's bound); and the float64 restatement alone satisfies the class rule there."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import a2m_rec_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "a2m_rec.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_float32_restatement_matches_the_reference(gold, fam):
    j, lens, h0 = gold["case_joints"], [int(n) for n in gold["case_lengths"]], gold["case_h0"]
    with torch.no_grad():
        lo, ac = R.forward(R.modules(R.weights(fam), torch.float32), torch.from_numpy(j), lens, torch.from_numpy(h0))
    el = float(np.abs(lo.numpy() - gold[f"case_logits_{fam}"]).max())
    ea = float(np.abs(ac.numpy() - gold[f"case_act_{fam}"]).max())
    print(f"{fam}: logits {el:.2e}  activations {ea:.2e}")
    assert el <= 1e-5 and ea <= 1e-5


def test_fixture_inputs_are_the_seeded_case(gold):
    j, lens, h0 = R.make_case(17, 13)
    assert np.array_equal(j, gold["case_joints"]) and lens == [int(n) for n in gold["case_lengths"]] and np.array_equal(h0, gold["case_h0"])


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_float64_restatement_satisfies_the_class_rule(gold, fam):
    (rl, _), _ = R.reference(R.weights(fam), gold["case_joints"], [int(n) for n in gold["case_lengths"]], gold["case_h0"])
    R.check_gaps(rl)
    R.check_classes(gold[f"case_logits_{fam}"], rl)
