"""ConvTasNet training on the device: the HIP training path (forward + backward of the network behind one autograd node)
against the reference's gradient fixture and against fp64 ATen autograd at the recipe shape, the routing to ATen, training
curves of both paths, allocator stability, gradient accumulation, two graphs alive, eval after training and bit-exact
repeatability.  Every comparison prints what it measured.

Gradient metric and ceiling: the project's contract (tests/test_gpu_tasnet.py): per parameter
max |g - g_ref| / max(max |g_ref|, 1e-3 of the model's largest gradient) <= 2e-3."""
import copy
import os

import numpy as np
import pytest
import torch

from onssen_amd import nn as onn
from tests import tasnet_ref

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRAIN = os.path.join(GOLD, "g8_tasnet_train.npz")
CEILING = 2e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _model(cfg, sd, dev):
    m = onn.ConvTasNet(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).train()


def _grads(m):
    return {k: p.grad.detach().double().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}


def _grad_error(got, ref):
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    worst, where = 0.0, None
    for k, g in ref.items():
        err = float(np.abs(got[k].reshape(g.shape) - g).max()) / max(float(np.abs(g).max()), 1e-3 * gmax)
        if err >= worst:
            worst, where = err, k
    return worst, where


def _fixture(dev):
    z = np.load(TRAIN)
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(TRAIN)
    x = torch.from_numpy(z["x"]).float().to(dev)
    refs = [torch.from_numpy(r).float().to(dev) for r in z["refs"]]
    gref = {k[6:]: z[k] for k in z.files if k.startswith("grad__")}
    return z, cfg, sd, x, refs, gref


def _check_fixture_grads(m, z, x, refs, gref, path):
    from onssen_amd import loss as L
    loss = L.si_snr_loss(m([x]), refs)
    loss.backward()
    assert m.last_train_path == path
    print(f"loss {float(loss.detach()):.6f} vs fixture {float(z['loss'][0]):.6f} ({path})")
    assert abs(float(loss.detach()) - float(z["loss"][0])) <= 1e-4 * max(1.0, abs(float(z["loss"][0])))
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k not in gref), k          # PReLU_2 / norm_2: no gradient, as upstream
    err, where = _grad_error(_grads(m), gref)
    print(f"worst relative gradient error {err:.2e} ({where}), ceiling {CEILING:.0e}")
    assert err <= CEILING


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_fixture_gradients_on_the_hip_path(dev, prec, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    z, cfg, sd, x, refs, gref = _fixture(dev)
    _check_fixture_grads(_model(cfg, sd, dev), z, x, refs, gref, "hip")


def _three_way(dev, cfg, n, S, seed, monkeypatch):
    """Gradients of the HIP path and of fp32 ATen autograd, each against fp64 ATen autograd on the device.

    The batch is a training batch: the mixture is the sum of its references.  References that are independent of the mixture
    make the yardstick itself useless: SI-SNR's gradient goes with 1 / <estimate, reference>, and with an estimate orthogonal to
    the reference up to chance (SI-SNR -46.8 dB, cos 4.6e-3) that dot product of 32 000 fp32 terms is all cancellation -- the
    first form of this test, with independent noise as references, measured 6.67e-3 for the HIP path AND 6.67e-3 for fp32 ATen
    autograd (ratio 1.00, the same parameter) at the recipe shape: the error of the fp32 loss, not of either backward."""
    from onssen_amd import loss as L
    sd = tasnet_ref.make_state(cfg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    hop = cfg["L"] // 2
    S_out = ((S - cfg["L"]) // hop) * hop + cfg["L"]
    src = (0.1 * rng.standard_normal((cfg["num_spks"], n, S))).astype(np.float32)
    x = src.sum(axis=0)
    refs = np.ascontiguousarray(src[:, :, :S_out])
    out = {}
    for name, dtype, opt in (("hip", torch.float32, "hip"), ("aten32", torch.float32, "aten"), ("aten64", torch.float64, "aten")):
        monkeypatch.setenv("ONSSEN_TASNET_TRAIN", opt)
        m = _model(cfg, sd, dev).to(dtype)
        loss = L.si_snr_loss(m([torch.from_numpy(x).to(dev).to(dtype)]), [torch.from_numpy(r).to(dev).to(dtype) for r in refs])
        loss.backward()
        assert m.last_train_path == opt
        out[name] = (_grads(m), float(loss.detach()))
        del m, loss
    e_hip, w_hip = _grad_error(out["hip"][0], out["aten64"][0])
    e_aten, w_aten = _grad_error(out["aten32"][0], out["aten64"][0])
    print(f"{n} x {S}: loss hip {out['hip'][1]:.6f} aten32 {out['aten32'][1]:.6f} aten64 {out['aten64'][1]:.6f}; gradient error "
          f"against fp64 ATen: HIP {e_hip:.2e} ({w_hip}), fp32 ATen {e_aten:.2e} ({w_aten}), ratio {e_hip / max(e_aten, 1e-30):.2f}")
    return e_hip


def test_recipe_shape_gradients_against_fp64(dev, monkeypatch):
    cfg = dict(tasnet_ref.RECIPE, activate="sigmoid")          # the shipped config's activation
    assert _three_way(dev, cfg, 3, 32000, 21, monkeypatch) <= CEILING


def test_cln_causal_gradients_against_fp64(dev, monkeypatch):
    cfg = dict(N=128, L=16, B=64, H=128, P=3, X=4, R=2, norm="cln", num_spks=2, activate="relu", causal=True)
    assert _three_way(dev, cfg, 2, 8000, 22, monkeypatch) <= CEILING


def test_unaligned_channel_counts_against_fp64(dev, monkeypatch):
    """No channel count a multiple of 4, an odd hop: every row of every operand starts off a 16-byte boundary."""
    cfg = dict(N=21, L=6, B=13, H=25, P=3, X=2, R=2, norm="gln", num_spks=3, activate="softmax", causal=False)
    assert _three_way(dev, cfg, 2, 1501, 23, monkeypatch) <= CEILING


def test_routing_to_aten(dev, monkeypatch):
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    z, cfg, sd, x, refs, gref = _fixture(dev)
    monkeypatch.setenv("ONSSEN_TASNET_TRAIN", "aten")
    _check_fixture_grads(_model(cfg, sd, dev), z, x, refs, gref, "aten")
    monkeypatch.delenv("ONSSEN_TASNET_TRAIN")
    # an input that requires a gradient
    m = _model(cfg, sd, dev)
    xg = x.clone().requires_grad_(True)
    assert any("input" in w for w in m.hip_train_limits(xg))
    L.si_snr_loss(m([xg]), refs).backward()
    assert m.last_train_path == "aten" and xg.grad is not None
    err, _ = _grad_error(_grads(m), gref)
    assert err <= CEILING
    # train-mode BatchNorm
    bn = dict(cfg, norm="bn")
    mb = _model(bn, tasnet_ref.make_state(bn, seed=3), dev)
    assert any("bn" in w for w in mb.hip_train_limits())
    opt = build_optimizer(mb.parameters(), {"name": "adam", "lr": 1e-3})
    val = dist.train_step(mb, opt, L.si_snr_loss, [x], refs)
    assert mb.last_train_path == "aten" and np.isfinite(val)


def test_training_curves_memory_and_eval(dev, monkeypatch):
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    z, cfg, sd, x, refs, _ = _fixture(dev)
    curves, models = {}, {}
    for path in ("hip", "aten"):
        monkeypatch.setenv("ONSSEN_TASNET_TRAIN", path)
        m = _model(cfg, sd, dev)
        opt = build_optimizer(m.parameters(), {"name": "adam", "lr": 1e-3})
        vals, mem = [], {}
        for step in range(1, 21):
            vals.append(dist.train_step(m, opt, L.si_snr_loss, [x], refs))
            assert m.last_train_path == path
            if step in (3, 20):
                torch.cuda.synchronize()
                mem[step] = torch.cuda.memory_allocated()
        curves[path], models[path] = vals, m
        print(f"{path}: " + " ".join(f"{v:.4f}" for v in vals) + f"; allocated after step 3 / 20: {mem[3]} / {mem[20]}")
        assert all(np.isfinite(vals)) and vals[-1] < vals[0]
        if path == "hip":
            assert mem[20] == mem[3]
    assert abs(curves["hip"][0] - curves["aten"][0]) <= 1e-5 * max(1.0, abs(curves["aten"][0]))
    # eval after those steps: the HIP forward against the ATen forward of the updated weights
    m = models["hip"].eval()
    with torch.no_grad():
        out = torch.stack(m([x])).double()
        ref = torch.stack([o.reshape(out.shape[1:]) for o in m._autograd_forward(x)]).double()
    rel = float(((out - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-30)).max())
    print(f"eval after 20 HIP training steps vs the ATen forward of the updated weights: rel L2 {rel:.2e}")
    assert rel <= 1e-5


def test_gradient_accumulation_and_two_graphs(dev):
    from onssen_amd import loss as L
    z, cfg, sd, x, refs, _ = _fixture(dev)
    x2 = torch.flip(x, dims=[1]) * 0.7
    refs2 = [torch.flip(r, dims=[1]) for r in refs[::-1]]
    m = _model(cfg, sd, dev)
    single = []
    for xx, rr in ((x, refs), (x2, refs2)):
        m.zero_grad(set_to_none=True)
        L.si_snr_loss(m([xx]), rr).backward()
        single.append({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    want = {k: single[0][k] + single[1][k] for k in single[0]}

    def check(tag):
        worst = 0.0
        for k, p in m.named_parameters():
            if k not in want:
                assert p.grad is None
                continue
            scale = max(float(single[0][k].abs().max()), float(single[1][k].abs().max()), 1e-30)
            worst = max(worst, float((p.grad - want[k]).abs().max()) / scale)
        print(f"{tag}: worst |accumulated - (g1 + g2)| / max(|g1|, |g2|) = {worst:.2e}")
        assert worst <= 1e-6

    # two backward calls without zero_grad: the second adds to the first
    m.zero_grad(set_to_none=True)
    L.si_snr_loss(m([x]), refs).backward()
    L.si_snr_loss(m([x2]), refs2).backward()
    check("forward, backward, forward, backward")
    # two forwards, then their two backwards: each graph owns its saved activations
    m.zero_grad(set_to_none=True)
    l1 = L.si_snr_loss(m([x]), refs)
    l2 = L.si_snr_loss(m([x2]), refs2)
    assert m.last_train_path == "hip"
    slots = [s for v in m._train_saved.values() for s in v]
    assert len(slots) == 2 and slots[0].buf.data_ptr() != slots[1].buf.data_ptr()
    l1.backward()
    l2.backward()
    check("forward, forward, backward, backward")
    assert all(s.owner == 0 for s in slots)


def test_two_identical_steps_give_identical_weights(dev):
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    z, cfg, sd, x, refs, _ = _fixture(dev)
    finals = []
    for _ in range(2):
        m = _model(cfg, sd, dev)
        opt = build_optimizer(m.parameters(), {"name": "adam", "lr": 1e-3})
        for _ in range(2):
            dist.train_step(m, opt, L.si_snr_loss, [x], refs)
        assert m.last_train_path == "hip"
        finals.append(copy.deepcopy({k: v.detach().cpu() for k, v in m.state_dict().items()}))
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
