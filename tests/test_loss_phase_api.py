"""loss.loss_phase on its PyTorch route (CPU tensors, no library) against the float64 restatement (tests/loss_phase_ref.py), and
the public names of the phase network's loss / reconstruction path."""
import numpy as np
import pytest
import torch

from tests import loss_phase_ref as R


def _case(B=4, T=7, F=9, D=6, seed=2):
    c = R.planted_case(B, (T, F), seed)
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    g = torch.Generator().manual_seed(seed)
    emb = torch.nn.functional.normalize(torch.randn(B, T, F, D, generator=g), dim=-1)
    one_hot = torch.nn.functional.one_hot(torch.randint(0, 3, (B, T, F), generator=g), 3)[..., :2].double()
    output = [emb, t["masks"][..., 0], t["masks"][..., 1], t["pA"], t["pB"]]
    label = [one_hot, t["x"], t["s1"], t["s2"], t["q1"], t["q2"]]
    return output, label


def test_loss_phase_on_cpu_matches_the_restatement():
    from onssen_amd import loss as L
    output, label = _case()
    got = L.loss_phase(output, label)
    assert L.last_phase_path == "aten"
    ref = R.loss_phase_ref(output, label)
    assert tuple(got.shape) == (4, 4) and got.dtype == torch.float32
    # every term is a float32 sum of a few hundred float32 terms: 1e-5 of the size of each (embedding term; 2 sum x for the others)
    le = R.loss_dc_literal(output[0], label[0], label[1])
    bound = 1e-5 * (0.975 * le.abs() + 0.025 * 2 * 2 * label[1].double().flatten(1).sum(1))
    print("loss_phase on CPU: max |got - ref| / bound", float(((got.double() - ref).abs() / bound).max()))
    assert ((got.double() - ref).abs() <= bound).all()


def test_tie_takes_the_swapped_assignment_on_the_pytorch_route():
    from onssen_amd import loss as L
    output, label = _case()
    lm, lp = L._phase_terms(*output[1:], *label[1:])
    rm, rp, perm = R.terms(*output[1:], *label[1:])
    assert perm.tolist()[:3] == [0, 1, 1]
    # row 2 (mask_A == mask_B): the phase term of the swapped assignment, which differs from the straight one's by far more
    rp_other = R.terms(*output[1:], *label[1:4], label[5], label[4])[1]
    assert abs(float(rp[2] - rp_other[2])) > 0.5
    assert abs(float(lp[2]) - float(rp[2])) < 1e-4 * float(label[1][2].sum()) < abs(float(lp[2]) - float(rp_other[2]))
    np.testing.assert_allclose(lm.numpy(), rm.numpy(), rtol=1e-5)


def test_labels_get_no_gradient_and_estimates_do():
    from onssen_amd import loss as L
    output, label = _case()
    output = [t.clone().requires_grad_(True) for t in output]
    label = [label[0]] + [t.clone().requires_grad_(True) for t in label[1:]]
    L.loss_phase(output, label).mean().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in output)
    assert all(t.grad is None for t in label[2:])            # (mag_mix reaches loss_dc's (B,B) product as upstream's does)


def test_wrong_counts_raise():
    from onssen_amd import loss as L
    output, label = _case()
    with pytest.raises(AssertionError, match="5 tensors"):
        L.loss_phase(output + [output[-1]], label)
    with pytest.raises(AssertionError, match="5 tensors"):
        L.loss_phase(output[:4], label)
    with pytest.raises(AssertionError, match="6 tensors"):
        L.loss_phase(output, label[:5])


def test_public_names():
    from onssen_amd import evaluate, features, loss, separation
    assert callable(loss.loss_phase) and callable(features.phase_istft) and callable(separation.separate_phase)
    assert issubclass(evaluate.tester_phase, evaluate.tester)
    with pytest.raises(ValueError, match="ragged"):
        evaluate.tester_phase(dict(model=torch.nn.Identity(), device="cpu", test_loader=[])).eval(batch=2)
