"""The project's restatement of the UESTC recognition ST-GCN (tests/uestc_rec_ref.py) and the synthetic graph operand (mld_hip.synthetic.uestc_graph)
against the reference's own STGCN (tests/golden/uestc_rec.npz, written by tools/make_golden_uestc_rec.py on the seeded stand-in weights with the
reference's own ``A``): ``A`` exactly (a handful of divisions by small integers, rounded to float32 once on both sides); float32 on both sides with the
same formulas for the net, so within 1e-5 absolute (tests/test_t2m_golden.py's bound); and the float64 restatement alone satisfies the class rule."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import uestc_rec_ref as R  # noqa: E402
from mld_hip import synthetic as syn  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uestc_rec.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def test_synthetic_graph_is_the_references(gold):
    A = syn.uestc_graph()
    assert A.shape == (3, 24, 24) and A.dtype == np.float32
    assert np.array_equal(A, gold["A"])
    assert np.array_equal(R.weights()["A"], gold["A"])
    assert np.allclose(A.sum(axis=(0, 1)), 1.0, atol=1e-6)      # column-normalised over the three groups


def test_state_dict_is_the_documented_group():
    sd = R.weights()
    assert len(sd) == 149 and not any(k.endswith("num_batches_tracked") for k in sd)
    assert {k: v.shape for k, v in sd.items()} == syn.uestc_rec_shapes()
    assert sd["st_gcn_networks.4.residual.0.weight"].shape == (128, 64, 1, 1) and sd["st_gcn_networks.7.tcn.2.weight"].shape == (256, 256, 9, 1)
    assert "st_gcn_networks.5.residual.0.weight" not in sd and sd["fcn.weight"].shape == (40, 256, 1, 1)


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_float32_restatement_matches_the_reference(gold, fam):
    with torch.no_grad():
        yh, ft = R.forward(R.tensors(R.weights(fam), torch.float32), torch.from_numpy(gold["case_motion"]))
    ey = float(np.abs(yh.numpy() - gold[f"case_yhat_{fam}"]).max())
    ef = float(np.abs(ft.numpy() - gold[f"case_feat_{fam}"]).max())
    print(f"{fam}: yhat {ey:.2e}  features {ef:.2e}")
    assert ey <= 1e-5 and ef <= 1e-5


def test_fixture_inputs_are_the_seeded_case(gold):
    assert np.array_equal(R.make_case(5, 13), gold["case_motion"])


@pytest.mark.parametrize("fam", list(R.FAMILIES))
def test_float64_restatement_satisfies_the_class_rule(gold, fam):
    (rl, e32), (rf, f32) = R.reference(R.weights(fam), gold["case_motion"])
    assert e32 > 0 and f32 > 0
    R.check_gaps(rl)
    R.check_classes(gold[f"case_yhat_{fam}"], rl)


def test_strided_view_of_feature_rows_is_the_same_input(gold):
    m = gold["case_motion"]
    rows, view = R.feature_rows(m)
    assert view.shape == (5, 24, 6, 13) and view.stride() == (150 * 13, 1, 25, 150) and torch.equal(view, torch.from_numpy(m))
