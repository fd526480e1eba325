"""Training through unfolded MISI iterations end to end on the device: ``loss.loss_wa_misi`` (``separation.misi`` as a chain of
autograd nodes, the half-step's backward csrc/misi_bwd.inc) against torch float64 autograd of the whole chain
(tests/misi_grad_ref.py), the kinds that take it, and a few optimiser steps on a "chimera-wa" batch."""
import numpy as np
import pytest
import torch

from tests import misi_bwd_checks as K
from tests import misi_grad_ref as G
from tests import wa_pit_cases as W

pytestmark = pytest.mark.gpu

B, T, F, HOP = 2, 13, 129, 64
FO = dict(batch_size=B, frame_length=T, sampling_rate=8000, window_size=256, hop_size=HOP, db_threshold=40.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)


def chimera_io(dev, c, masks):
    """A chimera output whose masks are the planes of ``masks`` (B,T,F,2), and the label of the "chimera-wa" loader."""
    return [torch.zeros(c.B, c.T, c.F, 20, device=dev), masks[..., 0], masks[..., 1]], [to(dev, c.ri), to(dev, c.src)]


def test_zero_iterations_are_loss_wa_bit_for_bit(dev):
    from onssen_amd.loss import loss_wa, loss_wa_misi
    c = G.chain_case()
    got = []
    for run in (lambda o, l: loss_wa(o, l, hop_size=HOP), lambda o, l: loss_wa_misi(o, l, 0, hop_size=HOP)):
        masks = to(dev, c.masks).requires_grad_(True)
        loss = run(*chimera_io(dev, c, masks))
        loss.backward()
        got.append((loss.detach().clone(), masks.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert float(got[0][1].abs().max()) > 0


@pytest.mark.parametrize("iters", [1, 2])
def test_mask_gradient_through_unfolded_iterations(dev, iters):
    """d loss / d masks of ``loss_wa_misi`` against torch float64 autograd through mask_istft and K x (half-step, phase_istft), with
    the loss's sign pattern and assignment taken from the estimates the device formed.  Bound: 4 x the host-side build's figure
    (G.CHAIN_MEASURED_REL: K = 1 3.32e-07, K = 2 1.69e-07 relative to max |ref|), ceiling 1e-4 max |ref|."""
    from onssen_amd import features, separation
    from onssen_amd.loss import loss_wa_misi
    c = G.chain_case()
    masks = to(dev, c.masks).requires_grad_(True)
    out, label = chimera_io(dev, c, masks)
    loss = loss_wa_misi(out, label, iters, hop_size=HOP)
    assert loss.grad_fn is not None
    loss.backward()
    with torch.no_grad():
        mix = features.mask_istft(label[0], None, HOP, c.n)[:, 0]
        est = separation.misi(label[0], masks, mix, iters, HOP)
    assert not est.requires_grad
    est, mix = est.cpu().numpy(), mix.cpu().numpy()
    V, _, _, gy, _ = W.reference(est, c.src, None, np.full(B, 1.0 / B))
    assert abs(float(loss.detach()) - V.mean()) <= 1e-6 * V.mean()          # the tracked chain formed the same estimates
    got = masks.grad.cpu().numpy()
    assert np.isfinite(got).all()
    err, top = K.chain_error(got, c, iters, mix, gy)
    print(f"loss_wa_misi K = {iters}: max |got - ref| {err:.3e}, max |ref| {top:.3e} ({err / top:.3e} relative; bound "
          f"{G.CHAIN_REL_BOUND:.3e}, ceiling 1e-4)")
    assert top > 0 and err <= 1e-4 * top and err <= G.CHAIN_REL_BOUND * top


def test_upit_with_three_speakers_and_the_phase_kind_take_a_backward_step(dev):
    from onssen_amd.loss import loss_wa_misi
    c3 = G.chain_case(C=3)
    m3 = to(dev, c3.masks).requires_grad_(True)
    loss_wa_misi([m3[..., s] for s in range(3)], [to(dev, c3.ri), to(dev, c3.src)], 1, hop_size=HOP, kind="upit").backward()
    assert torch.isfinite(m3.grad).all() and float(m3.grad.abs().max()) > 0
    c = G.chain_case()
    masks, ph = to(dev, c.masks).requires_grad_(True), to(dev, c.phases).requires_grad_(True)
    out, label = chimera_io(dev, c, masks)
    loss_wa_misi(out + [ph[0], ph[1]], label, 1, hop_size=HOP, kind="phase").backward()
    for g in (masks.grad, ph.grad):
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    with pytest.raises(ValueError, match="nothing to redistribute"):
        loss_wa_misi([masks[..., 0]], [label[0], label[1][:, :1]], 1, hop_size=HOP, kind="enhance")


def test_a_few_adam_steps_lower_the_loss(dev):
    """20 Adam steps (lr 1e-3) at one unfolded iteration on ONE synthetic "chimera-wa" batch: the last loss is strictly below the
    first (the measured ratio is in DESIGN section 25; it is not a threshold)."""
    from onssen_amd import nn as onn
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.loss import loss_wa_misi
    (feat,), label = next(iter(SyntheticWsj02mix("chimera-wa", FO, "tr", device=dev, num_batches=1)))
    assert tuple(label[0].shape) == (B, T, F, 2) and tuple(label[1].shape) == (B, 2, HOP * (T - 1))
    torch.manual_seed(0)
    model = onn.chimera(F, 32, 2, dropout=0.0).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = loss_wa_misi(model([feat]), label, 1, hop_size=HOP)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"loss_wa_misi (K = 1) over 20 Adam steps: first {losses[0]:.6f}, last {losses[-1]:.6f}, ratio {losses[-1] / losses[0]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
