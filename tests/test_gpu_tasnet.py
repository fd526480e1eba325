"""ConvTasNet on the device: the HIP forward against the g8 fixtures (reference outputs) and against tests/tasnet_ref.py at the
recipe shape, determinism and graph replay, weight changes, the ATen training path and the SI-SDR tester.  Every comparison
prints what it measured."""
import glob
import os

import numpy as np
import pytest
import torch

from onssen_amd import nn as onn
from tests import tasnet_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLD, "g8_tasnet_*.npz"))
                  if not f.endswith(("_loss.npz", "_train.npz", "_names.npz")))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _model(cfg, sd, dev):
    m = onn.ConvTasNet(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def _errors(out, ref):
    """max |err|, worst relative L2 per (speaker, utterance)"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if ref.ndim == 2:
        out, ref = out[:, None], ref[:, None]
    rel = np.linalg.norm(out - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-30)
    return float(np.abs(out - ref).max()), float(rel.max())


def _run(m, x):
    with torch.no_grad():
        out = m([x])
    torch.cuda.synchronize()
    return np.stack([o.cpu().numpy() for o in out])


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[10:-4])
def test_fixture(path, prec, dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    cfg, sd, x, out64, _ = tasnet_ref.load_fixture(path)
    out = _run(_model(cfg, sd, dev), torch.from_numpy(x).to(dev))
    assert out.shape == out64.shape
    amax, rel = _errors(out, out64)
    print(f"{os.path.basename(path)} {prec}: max |err| {amax:.2e} (max |ref| {np.abs(out64).max():.2f}), rel L2 {rel:.2e}")
    if prec == "bf16":
        assert rel <= 3e-2
    else:
        assert amax <= 2e-5 * max(1.0, float(np.abs(out64).max())) and rel <= 1e-5


_RECIPE_REF = {}


def _recipe_case(name):
    if name not in _RECIPE_REF:
        sd = tasnet_ref.make_state(tasnet_ref.RECIPE, seed=11)
        rng = np.random.default_rng(12)
        shape = {"3x32000": (3, 32000), "3x32003": (3, 32003), "1d_37152": (37152,)}[name]
        x = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        _RECIPE_REF[name] = (sd, x, np.stack(tasnet_ref.forward(sd, x, tasnet_ref.RECIPE)))
    return _RECIPE_REF[name]


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["3x32000", "3x32003", "1d_37152"])
def test_recipe_shape(name, prec, dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    sd, x, ref = _recipe_case(name)
    out = _run(_model(tasnet_ref.RECIPE, sd, dev), torch.from_numpy(x).to(dev))
    assert out.shape == ref.shape
    amax, rel = _errors(out, ref)
    print(f"recipe {name} {prec}: max |err| {amax:.2e} (max |ref| {np.abs(ref).max():.3f}), worst rel L2 {rel:.2e}")
    if prec == "bf16":
        assert rel <= 3e-2
    else:
        assert rel <= 1e-5 and amax <= 2e-5 * max(1.0, float(np.abs(ref).max()))


def test_same_bits_eager_and_graph(dev):
    sd, x, _ = _recipe_case("3x32000")
    m = _model(tasnet_ref.RECIPE, sd, dev)
    xd = torch.from_numpy(x).to(dev)
    a, b = _run(m, xd), _run(m, xd)
    assert np.array_equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        m([xd])                                          # warm: images and workspace exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = m([xd])
    g.replay()
    torch.cuda.synchronize()
    c = np.stack([o.cpu().numpy() for o in out])
    assert np.array_equal(a, c)


def test_weight_edit_between_forwards(dev):
    cfg, sd, x, _, _ = tasnet_ref.load_fixture(FIXTURES[0])
    m = _model(cfg, sd, dev)
    xd = torch.from_numpy(x).to(dev)
    _run(m, xd)
    with torch.no_grad():
        m.separation[0][1].dwconv.weight.mul_(-1.5)
        m.gen_masks.bias.add_(0.3)
    out = _run(m, xd)
    sd2 = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    ref = np.stack(tasnet_ref.forward(sd2, x, cfg))
    amax, _ = _errors(out, ref)
    print(f"after an in-place weight edit: max |err| {amax:.2e}")
    assert amax <= 2e-5 * max(1.0, float(np.abs(ref).max()))


def _aten(m, xd):
    with torch.no_grad():
        out = m._autograd_forward(xd if xd.dim() == 2 else xd[None])
    return np.stack([o.cpu().numpy() for o in out])


def test_eval_after_training_steps(dev):
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    cfg, sd, x, _, _ = tasnet_ref.load_fixture(FIXTURES[0])
    m = _model(cfg, sd, dev)
    xd = torch.from_numpy(x).to(dev)
    _run(m, xd)                                          # an eval forward packs the images of step 0
    m.train()
    opt = build_optimizer(m.parameters(), {"name": "adam", "lr": 1e-2})
    S_out = _run(m, xd).shape[-1]
    refs = [torch.randn(x.shape[0], S_out, device=dev, generator=torch.Generator(dev).manual_seed(s)) for s in range(2)]
    for _ in range(3):
        loss = dist.train_step(m, opt, L.si_snr_loss, [xd], refs)
        assert np.isfinite(loss)
    m.eval()
    out = _run(m, xd)
    ref = _aten(m, xd)
    amax, rel = _errors(out, ref)
    print(f"eval after 3 fused-Adam steps vs the ATen forward of the updated weights: max |err| {amax:.2e}, rel L2 {rel:.2e}")
    assert rel <= 1e-5


def test_training_path_gradients_and_step(dev):
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    z = np.load(os.path.join(GOLD, "g8_tasnet_train.npz"))
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(os.path.join(GOLD, "g8_tasnet_train.npz"))
    m = _model(cfg, sd, dev).train()
    est = m([torch.from_numpy(z["x"]).float().to(dev)])
    loss = L.si_snr_loss(est, [torch.from_numpy(r).float().to(dev) for r in z["refs"]])
    loss.backward()
    print(f"training loss {float(loss.detach()):.6f} vs fixture {float(z['loss'][0]):.6f}")
    assert abs(float(loss.detach()) - float(z["loss"][0])) <= 1e-4 * max(1.0, abs(float(z["loss"][0])))
    # relative to max(|g| of the parameter, 1e-3 of the largest gradient): the zero-mean SI-SNR does not see a constant offset, so
    # decoder.bias has an exactly zero gradient in exact arithmetic (1e-17 in the fp64 fixture, fp32 round-off here)
    gmax = max(float(np.abs(z[k]).max()) for k in z.files if k.startswith("grad__"))
    worst = 0.0
    for k, p in m.named_parameters():
        if "grad__" + k not in z.files:                  # PReLU_2 / norm_2: unused by the forward, no gradient upstream either
            assert p.grad is None
            continue
        g = z["grad__" + k]
        err = np.abs(p.grad.cpu().numpy() - g).max() / max(np.abs(g).max(), 1e-3 * gmax)
        worst = max(worst, err)
    print(f"worst relative gradient error {worst:.2e}")
    assert worst <= 2e-3
    # one data-parallel step with the recipe's optimizer
    opt = build_optimizer(m.parameters(), {"name": "adam", "lr": 0.001})
    before = m.gen_masks.weight.detach().clone()
    val = dist.train_step(m, opt, L.si_snr_loss, [torch.from_numpy(z["x"]).float().to(dev)],
                          [torch.from_numpy(r).float().to(dev) for r in z["refs"]])
    assert np.isfinite(val) and not torch.equal(before, m.gen_masks.weight.detach())


def test_tester_tasnet_matches_reference_sdr(dev, tmp_path):
    from onssen_amd.data import wsj0_2mix_dataloader
    from onssen_amd.evaluate import tester_tasnet
    from onssen_amd.evaluate import batch_SDR_torch
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(FIXTURES[0])
    m = _model(cfg, sd, dev)
    fo = {"data_path": "synthetic", "batch_size": 1, "sampling_rate": 8000, "chunk_size": 400, "n_utterances": 3,
          "min_samples": 300, "max_samples": 500}
    loader = wsj0_2mix_dataloader("conv-tasnet", fo, "tt", dev)
    t = tester_tasnet({"model": m, "test_loader": loader, "device": dev})
    got = t.eval()
    sdrs = []
    for inp, lab in loader:
        mix, = inp
        ref_sig, = lab
        est = tasnet_ref.forward(sd, mix.cpu().numpy()[0], cfg)
        S = ref_sig.shape[-1]
        e = torch.from_numpy(np.stack([o[:S] for o in est])[None]).float().to(dev)
        sdrs.append(float(batch_SDR_torch(e, ref_sig.to(dev)).mean()))
    print(f"tester_tasnet {got:.4f} dB, on tasnet_ref outputs {np.mean(sdrs):.4f} dB")
    assert abs(got - float(np.mean(sdrs))) <= 1e-3


def test_errors(dev, monkeypatch):
    monkeypatch.delenv("ONSSEN_CPU_AUTOGRAD", raising=False)
    cfg, sd, x, _, _ = tasnet_ref.load_fixture(FIXTURES[0])
    m = _model(cfg, sd, dev)
    with pytest.raises(RuntimeError, match="ROCm device"):
        with torch.no_grad():                            # the inference path: no CPU fallback
            m.cpu()([torch.from_numpy(x)])
    with pytest.raises(RuntimeError, match="ROCm device"):
        m.cpu().train()([torch.from_numpy(x)])          # the training path: no CPU autograd without the test switch
    m = m.to(dev).eval()
    with pytest.raises(RuntimeError, match="1/2D"):
        m([torch.zeros(1, 2, 300, device=dev)])
    bad = onn.ConvTasNet(N=8, L=70, B=4, H=8, P=3, X=1, R=1).to(dev).eval()
    with pytest.raises(RuntimeError, match="L = 70"):
        with torch.no_grad():
            bad([torch.zeros(2, 300, device=dev)])
