"""Waveform-approximation training end to end on the device: the differentiable inverse transforms of ``features``, ``loss.loss_wa``
on the outputs of the mask models against the float64 restatement (tests/istft_grad_ref.py, tests/wa_pit_cases.py), a few
optimiser steps on a "chimera-wa" batch, and a graph capture of the loss with its backward."""
import numpy as np
import pytest
import torch

from onssen_amd.synthetic import synth_mixture_k
from oracle import np_oracle as O
from tests import istft_grad_ref as R
from tests import wa_pit_cases as W

pytestmark = pytest.mark.gpu

B, T, F, HOP, N = 2, 40, 129, 64, 64 * 39
FO = dict(batch_size=B, frame_length=T, sampling_rate=8000, window_size=256, hop_size=HOP, db_threshold=40.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)


@pytest.fixture(scope="module")
def batch():
    """ri (B,T,F,2) f32 of two-speaker mixtures of N samples, feat (B,T,F) their log-magnitude, src (B,2,N) the sources."""
    sigs = [synth_mixture_k(70 + b, N, num_speaker=2) for b in range(B)]
    mix = np.stack([s[0] for s in sigs]).astype(np.float32)
    src = np.stack([np.stack(s[1:]) for s in sigs]).astype(np.float32)
    X = [O.stft(m, 256, HOP) for m in mix]
    ri = np.ascontiguousarray(np.stack([np.stack([x.real, x.imag], -1) for x in X]), dtype=np.float32)
    feat = np.stack([O.log_magnitude(x) for x in X])
    assert ri.shape == (B, T, F, 2)
    return ri, feat, src


def reference_gradient(mode, ri, op, phases, est_dev, src, C):
    """d mean_b V_b / d (operand, phases) in float64: the sign pattern and the assignment are taken from the estimate the device
    formed (a float64 estimate could fall on the other side of an |est - ref| of a few 1e-8), the adjoint is the restatement's."""
    _, _, _, gy, _ = W.reference(est_dev, src, None, np.full(B, 1.0 / B))
    g_op, g_ph = np.zeros((B, T, F, C)), np.zeros((C, B, T, F, 2))
    for b in range(B):
        g_op[b], g_ph[:, b] = R.adjoint(ri[b], op[b], mode, HOP, gy[b], None if phases is None else phases[:, b])
    return g_op, g_ph


def check(what, got, ref):
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: max |got - ref| {err:.3e}, max |ref| {top:.3e} ({err / top:.2e} relative; bound {R.GRAD_REL_BOUND:.2e}, ceiling 1e-5)")
    assert top > 0 and err <= 1e-5 * top and err <= R.GRAD_REL_BOUND * top


def test_mask_istft_with_grad_has_the_bits_of_the_plain_call(dev, batch):
    """(Fails on the parent commit: its result has no grad_fn.)"""
    from onssen_amd import features
    ri, _, _ = batch
    rng = np.random.default_rng(1)
    masks = to(dev, rng.random((B, T, F, 2)).astype(np.float32))
    plain = features.mask_istft(to(dev, ri), masks)
    tracked = features.mask_istft(to(dev, ri), masks.clone().requires_grad_(True))
    assert tracked.grad_fn is not None and not plain.requires_grad
    assert torch.equal(tracked.detach(), plain)
    mags = to(dev, rng.random((B, T, F)).astype(np.float32))
    assert torch.equal(features.mag_istft(to(dev, ri), mags.clone().requires_grad_(True)).detach(), features.mag_istft(to(dev, ri), mags))
    ph = to(dev, R.case(256, 64, 21, 2).phases[:, :, :1].repeat(T, axis=2))
    tracked = features.phase_istft(to(dev, ri), masks, ph.clone().requires_grad_(True))
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), features.phase_istft(to(dev, ri), masks, ph))
    with pytest.raises(RuntimeError, match="spectrum is data"):
        features.mask_istft(to(dev, ri).requires_grad_(True), masks)
    with pytest.raises(ValueError, match="out= cannot be combined"):
        features.phase_istft(to(dev, ri), masks.clone().requires_grad_(True), ph, out=torch.empty(B, 2, N, device=dev))
    with torch.no_grad():           # nothing changes without autograd: the plain path, out= included
        out = torch.empty(B, 2, N, device=dev)
        assert features.phase_istft(to(dev, ri), masks.clone().requires_grad_(True), ph, out=out) is out


def test_loss_wa_on_a_chimera_output(dev, batch):
    from onssen_amd import features, nn as onn
    from onssen_amd.loss import loss_wa
    ri, feat, src = batch
    torch.manual_seed(0)
    model = onn.chimera(F, 64, 2, 20, dropout=0.0).to(dev).train()
    emb, mA, mB = model([to(dev, feat)])
    masks = torch.stack([mA, mB], -1).detach().requires_grad_(True)          # the masks as a leaf: their gradient is what is checked
    loss = loss_wa([emb.detach(), masks[..., 0], masks[..., 1]], [to(dev, ri), to(dev, src)], hop_size=HOP)
    loss.backward()
    with torch.no_grad():
        est = features.mask_istft(to(dev, ri), masks, HOP, N).cpu().numpy()
    V, _, _, _, _ = W.reference(est, src, None, np.ones(B))
    assert abs(float(loss.detach()) - V.mean()) <= 1e-6 * V.mean()
    g_ref, _ = reference_gradient(R.MASK, ri, masks.detach().cpu().numpy(), None, est, src, 2)
    check("chimera++ d loss / d masks", masks.grad.cpu().numpy(), g_ref)
    # and through the network itself: every parameter of the mask branch gets a finite, non-zero gradient
    loss_wa(model([to(dev, feat)]), [to(dev, ri), to(dev, src)], hop_size=HOP).backward()
    g = model.fc_mi.weight.grad if hasattr(model, "fc_mi") else next(p.grad for p in model.parameters() if p.grad is not None)
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0


def test_loss_wa_through_phase_istft(dev, batch):
    from onssen_amd import features
    from onssen_amd.loss import loss_wa
    ri, _, src = batch
    rng = np.random.default_rng(2)
    m = rng.random((B, T, F, 2)).astype(np.float32)
    p = rng.standard_normal((2, B, T, F, 2))
    p = (p / np.linalg.norm(p, axis=-1, keepdims=True)).astype(np.float32)
    masks, ph = to(dev, m).requires_grad_(True), to(dev, p).requires_grad_(True)
    emb = torch.zeros(B, T, F, 20, device=dev)
    loss_wa([emb, masks[..., 0], masks[..., 1], ph[0], ph[1]], [to(dev, ri), to(dev, src)], hop_size=HOP, kind="phase").backward()
    with torch.no_grad():
        est = features.phase_istft(to(dev, ri), masks, ph, HOP, N).cpu().numpy()
    g_m, g_p = reference_gradient(R.PHASE, ri, m, p, est, src, 2)
    check("phase d loss / d masks", masks.grad.cpu().numpy(), g_m)
    check("phase d loss / d phases", ph.grad.cpu().numpy(), g_p)


def test_loss_wa_through_mag_istft(dev, batch):
    from onssen_amd import features
    from onssen_amd.loss import loss_wa
    ri, _, src = batch
    rng = np.random.default_rng(3)
    m = (rng.random((B, T, F)) * np.hypot(ri[..., 0], ri[..., 1])).astype(np.float32)
    mag = to(dev, m).requires_grad_(True)
    ref = src[:, :1]
    loss_wa([mag], [to(dev, ri), to(dev, np.ascontiguousarray(ref))], hop_size=HOP, kind="enhance").backward()
    with torch.no_grad():
        est = features.mag_istft(to(dev, ri), mag, HOP, N).cpu().numpy()
    g_m, _ = reference_gradient(R.MAG, ri, m[..., None], None, est, ref, 1)
    check("enhance d loss / d magnitude", mag.grad.cpu().numpy(), g_m[..., 0])


def test_a_few_adam_steps_lower_the_loss(dev):
    """20 Adam steps (lr 1e-3) on ONE synthetic "chimera-wa" batch: the last loss is strictly below the first (the measured ratio
    is in DESIGN section 23; it is not a threshold)."""
    from onssen_amd import nn as onn
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.loss import loss_wa
    (feat,), label = next(iter(SyntheticWsj02mix("chimera-wa", FO, "tr", device=dev, num_batches=1)))
    assert tuple(label[0].shape) == (B, T, F, 2) and tuple(label[1].shape) == (B, 2, HOP * (T - 1))
    torch.manual_seed(0)
    model = onn.chimera(F, 64, 2, 20, dropout=0.0).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = loss_wa(model([feat]), label, hop_size=HOP)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"loss_wa over 20 Adam steps: first {losses[0]:.6f}, last {losses[-1]:.6f}, ratio {losses[-1] / losses[0]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


def test_loss_wa_in_a_graph_capture(dev, batch):
    """Forward and backward of ``loss_wa`` captured into one graph replay to the bits of the eager call."""
    from onssen_amd.loss import loss_wa
    ri, _, src = batch
    rng = np.random.default_rng(4)
    values = to(dev, rng.random((B, T, F, 2)).astype(np.float32))
    emb, label = torch.zeros(B, T, F, 20, device=dev), [to(dev, ri), to(dev, src)]
    run = lambda m: loss_wa([emb, m[..., 0], m[..., 1]], label, hop_size=HOP)
    first = values.clone().requires_grad_(True)
    eager = run(first)
    eager.backward()
    want_loss, want_grad = eager.detach().clone(), first.grad.clone()
    del eager
    masks = values.clone().requires_grad_(True)        # a leaf of its own: its gradient buffer is allocated inside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up off the default stream, as capture asks
        run(masks).backward()
    torch.cuda.current_stream().wait_stream(side)
    masks.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = run(masks)
        loss.backward()
    for _ in range(2):
        masks.grad.zero_()
        loss.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want_loss) and torch.equal(masks.grad, want_grad)
