"""The phase network end to end on the GPU: loss_phase on the HIP kernels (value, assignment, gradients, graph capture), the
phase-aware iSTFT against the oracle, separate_phase against its parts, and a short training run through the HIP loss.
Bounds as in tests/test_emu_loss_phase.py and tests/phase_istft_cases.py (reasoned there), for the shapes used here."""
import numpy as np
import pytest
import torch

from onssen_amd import loss as L
from tests import loss_phase_ref as R
from tests.phase_istft_cases import SHAPES, atol, case, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _loss_case(B, T, F, dev, views, D=8):
    c = {k: torch.from_numpy(v).to(dev) for k, v in R.planted_case(B, (T, F), seed=B + T).items()}
    g = torch.Generator().manual_seed(T)
    emb = torch.nn.functional.normalize(torch.randn(B, T, F, D, generator=g), dim=-1).to(dev).requires_grad_(True)
    one_hot = torch.nn.functional.one_hot(torch.randint(0, 3, (B, T, F), generator=g), 3)[..., :2].double().to(dev)
    pA, pB = c["pA"].clone().requires_grad_(True), c["pB"].clone().requires_grad_(True)
    if views == "network":                  # two planes of one non-leaf (B,T,F,2) buffer, as the network hands them over
        leaf = c["masks"].clone().requires_grad_(True)
        buf = (leaf * 1.0).reshape(B, T, F * 2).reshape(B, T, F, 2)
        mA, mB, wrt = buf[:, :, :, 0], buf[:, :, :, 1], [leaf]
    else:                                   # two unrelated tensors
        mA, mB = (c["masks"][..., k].contiguous().requires_grad_(True) for k in (0, 1))
        wrt = [mA, mB]
    label = [one_hot, c["x"], c["s1"], c["s2"], c["q1"], c["q2"]]
    masks_grad = lambda gs: gs[0] if views == "network" else torch.stack([gs[0], gs[1]], -1)
    return c, [emb, mA, mB, pA, pB], label, wrt, masks_grad


@pytest.mark.parametrize("views", ["network", "separate"])
@pytest.mark.parametrize("B,T,F", [(3, 5, 129), (2, 100, 257)])
def test_loss_terms_value_and_gradients(dev, B, T, F, views):
    """onssen_loss_phase_f32 / _grad_f32 through their autograd node against the float64 restatement on the device."""
    c, output, label, wrt, masks_grad = _loss_case(B, T, F, dev, views)
    _, mA, mB, pA, pB = output
    lm, lp = L._phase_terms_hip(mA, mB, pA, pB, *label[1:], True)
    args = (c["masks"][..., 0], c["masks"][..., 1], c["pA"], c["pB"], c["x"], c["s1"], c["s2"], c["q1"], c["q2"])
    rm, rp, perm = R.terms(*args)
    assert perm.tolist() == [0, 1, 1][:B]
    bound = 1e-5 * 2.0 * c["x"].double().flatten(1).sum(1)
    print("mask term  |out - ref| / bound", ((lm.detach().double() - rm).abs() / bound).tolist())
    print("phase term |out - ref| / bound", ((lp.detach().double() - rp).abs() / bound).tolist())
    assert ((lm.detach().double() - rm).abs() <= bound).all() and ((lp.detach().double() - rp).abs() <= bound).all()
    g_mask = torch.linspace(-1.3, 0.9, B, device=dev)
    g_phase = torch.linspace(0.7, -1.1, B, device=dev)
    grads = torch.autograd.grad([lm, lp], wrt + [pA, pB], [g_mask, g_phase])
    dA, dB, dpA, dpB = R.grads(*args, perm, g_mask, g_phase)
    assert torch.equal(masks_grad(grads), torch.stack([dA, dB], -1).float())             # sign * float32(g x): exact
    xg = g_phase.double().abs().reshape(-1, 1, 1) * c["x"].double()
    for got, ref, p in ((grads[-2], dpA, c["pA"]), (grads[-1], dpB, c["pB"])):
        pb = 1e-5 * xg / R._norm(p.double()).clamp_min(R.EPS)
        err = (got.double() - ref).abs().amax(-1)
        print("phase gradient max |err| / bound", float((err / pb).max()))
        assert torch.isfinite(got).all() and (err <= pb).all()


@pytest.mark.parametrize("views", ["network", "separate"])
def test_loss_phase_public_route(dev, views):
    """loss.loss_phase on device tensors: the HIP route, the (B,B) value as 0.975 loss_dc + 0.025 (mask + phase), gradients for
    every estimate, none for the labels; the same value under no_grad and from a captured graph."""
    B, T, F = 3, 5, 129
    c, output, label, wrt, masks_grad = _loss_case(B, T, F, dev, views)
    got = L.loss_phase(output, label)
    assert L.last_phase_path == "hip" and tuple(got.shape) == (B, B)
    args = (c["masks"][..., 0], c["masks"][..., 1], c["pA"], c["pB"], c["x"], c["s1"], c["s2"], c["q1"], c["q2"])
    rm, rp, perm = R.terms(*args)
    with torch.no_grad():
        le = L.loss_dc([output[0]], label[:2]).double()                   # (pinned by its own tests)
    want = le * 0.975 + rm * 0.025 + rp * 0.025
    sx = c["x"].double().flatten(1).sum(1)
    # the two new terms to their bound, plus three float32 roundings of the sum
    bound = 0.025 * 2 * 1e-5 * 2.0 * sx + 4 * np.finfo(np.float32).eps * (le.abs() + 0.025 * (rm.abs() + rp.abs()))
    print("loss_phase |got - want| / bound", float(((got.detach().double() - want).abs() / bound).max()))
    assert ((got.detach().double() - want).abs() <= bound).all()
    grads = torch.autograd.grad(got.mean(), [output[0]] + wrt + [output[3], output[4]])
    assert all(torch.isfinite(g).all() for g in grads)
    # d mean / d term[b] = 0.025 B / B^2, formed by autograd in float32: the masks' gradient to a few roundings of that factor
    g = torch.full((B,), 0.025 / B, device=dev, dtype=torch.float64)
    dA, dB, dpA, dpB = R.grads(*args, perm, g, g)
    ref_m = torch.stack([dA, dB], -1)
    assert ((masks_grad(grads[1:-2]).double() - ref_m).abs() <= 4 * np.finfo(np.float32).eps * ref_m.abs()).all()
    for got_p, ref, p in ((grads[-2], dpA, c["pA"]), (grads[-1], dpB, c["pB"])):
        pb = 1e-5 * (g.reshape(-1, 1, 1) * c["x"].double()) / R._norm(p.double()).clamp_min(R.EPS)
        assert ((got_p.double() - ref).abs().amax(-1) <= pb).all()
    detached = [t.detach() for t in output]
    with torch.no_grad():
        eager = L.loss_phase(detached, label)
        assert L.last_phase_path == "hip" and torch.equal(eager, got.detach())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            L.loss_phase(detached, label)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = L.loss_phase(detached, label)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


@pytest.mark.parametrize("n_fft,hop,n,C", [s + (2,) for s in SHAPES] + [SHAPES[0] + (3,)])
def test_phase_istft_matches_oracle(dev, n_fft, hop, n, C):
    from onssen_amd.features import phase_istft
    _, ri, masks, phases = case(n_fft, hop, n, C)
    d = lambda a: torch.from_numpy(a).to(dev)
    ph = d(phases)
    out = phase_istft(d(ri), d(masks), ph, hop, n)
    ref = reference(ri, masks, phases, hop, n)
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"n_fft {n_fft} hop {hop} C {C}: max |out - ref| {err:.3e}, bound {atol(ref):.3e}")
    assert tuple(out.shape) == (2, C, n) and err <= atol(ref)
    listed = phase_istft(d(ri), d(masks), [ph[c].clone() for c in range(C)], hop, n)      # C tensors of their own
    assert torch.equal(listed, out)


def _tiny_model(dev):
    from onssen_amd import nn as onn
    torch.manual_seed(4)
    return onn.phase_net(129, hidden_dim=32, num_layers=1, embedding_dim=8, dropout=0).to(dev)


def test_separate_phase_is_its_parts(dev):
    from onssen_amd.features import phase_istft, stft_logmag
    from onssen_amd.separation import separate_phase
    from onssen_amd.synthetic import synth_mixture
    model = _tiny_model(dev).eval()
    wav = torch.from_numpy(np.stack([synth_mixture(50 + b, 2048) for b in range(2)])).to(dev)
    out = separate_phase(model, wav, 256, 64)
    with torch.no_grad():
        logmag, ri = stft_logmag(wav, 256, 64)
        _, mA, mB, pA, pB = model([logmag, ri])
        want = phase_istft(ri, torch.stack([mA, mB], -1), [pA, pB], 64, 2048)
    assert tuple(out.shape) == (2, 2, 2048) and torch.isfinite(out).all() and float(out.abs().max()) > 0
    assert torch.equal(out, want)


def test_training_through_the_hip_loss(dev):
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    model = _tiny_model(dev).train()
    fo = dict(batch_size=2, frame_length=20, sampling_rate=8000, window_size=256, hop_size=64, db_threshold=40)
    input, label = next(iter(SyntheticWsj02mix("phase", fo, "tr", dev, num_batches=1)))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for step in range(21):
        opt.zero_grad()
        loss = torch.mean(L.loss_phase(model(input), label))
        assert L.last_phase_path == "hip"
        losses.append(float(loss.detach()))
        if step == 20:
            break
        loss.backward()
        if step == 0:
            missing = [n for n, p in model.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
            assert not missing, missing
        opt.step()
    print("loss_phase on one batch, 20 Adam steps:", losses[0], "->", losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
