"""The SI-SNR permutation-invariant training loss on the device: ``loss.sisnr_pit`` and ``loss.si_snr_loss`` under
``tasnet_loss = "hip"`` against the NumPy fp64 restatement (tests/sisnr_pit_ref.py; bounds as tests/test_emu_sisnr_pit.py),
ragged and degenerate rows, views of one (k, n, S) tensor against separate tensors, a tiny ConvTasNet trained one step per loss
route, and graph capture of loss forward + backward.  Every comparison prints what it measured."""
import copy

import numpy as np
import pytest
import torch

from onssen_amd import loss as L
from onssen_amd import nn as onn
from tests import sisnr_pit_ref as R
from tests import tasnet_ref

pytestmark = pytest.mark.gpu

BASE = dict(N=20, L=4, B=12, H=24, P=3, X=2, R=1, num_spks=2)        # the geometry of tests/test_emu_tasnet_train.py
CEILING = 2e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


@pytest.fixture
def hip_loss(monkeypatch):
    monkeypatch.setenv("ONSSEN_TASNET_LOSS", "hip")


def _rows(a, dev, pad=0, offset=0):
    """(N, S) on the device with rows S + pad floats apart, ``offset`` floats into its buffer; NaN everywhere else."""
    N, S = a.shape
    raw = torch.full((N * (S + pad) + offset + 4,), float("nan"), device=dev)
    view = raw.as_strided((N, S), (S + pad, 1), offset)
    view.copy_(torch.from_numpy(a))
    return view


def _loss_and_grad(ests, refs):
    xs = [e.detach().requires_grad_(True) for e in ests]
    loss = L.si_snr_loss(xs, refs)
    loss.backward()
    assert L.last_si_snr_path == "hip"
    return loss.detach(), torch.stack([x.grad for x in xs])


def _check(dev, ests, refs, ref, tag, pad=0, offset=0):
    de, dr = [_rows(e, dev, pad, offset) for e in ests], [_rows(r, dev, pad, offset) for r in refs]
    value, perm = L.sisnr_pit(de, dr, return_perm=True)
    assert value.dtype == torch.float32 and perm.dtype == torch.int64
    loss, grad = _loss_and_grad(de, dr)
    R.check_values(value.cpu().numpy(), perm.cpu().numpy(), float(loss), ref, tag)
    R.check_grad(grad.cpu().numpy(), ref, tag)
    return value, loss, grad


# ---- items 1 and 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_value_perm_loss_and_gradient(dev, hip_loss, k):
    for N, S in ((3, 65), (1, 513), (3, 1030)):
        ests, refs, ref = R.planted_clear(k, N, S, seed=2000 * k + S + N)
        plain = _check(dev, ests, refs, ref, f"k={k} N={N} S={S}")
        odd = _check(dev, ests, refs, ref, f"k={k} N={N} S={S}, rows S + 3 apart, base off by one float", pad=3, offset=1)
        for a, b in zip(plain, odd):
            assert torch.equal(a, b)


def test_high_si_snr_per_row_gradients_and_long_rows(dev, hip_loss):
    ests, refs = R.planted(2, 3, 1030, seed=5, noise=1e-3)
    gv = np.array([0.5, -2.0, 0.25], np.float32)
    ref = R.reference(ests, refs, g_value=gv, g_total=0.0)
    assert ref["value"].min() > 55.0
    xs = [torch.from_numpy(e).to(dev).requires_grad_(True) for e in ests]
    value, perm = L.sisnr_pit(xs, [torch.from_numpy(r).to(dev) for r in refs], return_perm=True)
    (value * torch.from_numpy(gv).to(dev)).sum().backward()
    R.check_values(value.detach().cpu().numpy(), perm.cpu().numpy(), ref["loss"], ref, "60 dB")
    R.check_grad(torch.stack([x.grad for x in xs]).cpu().numpy(), ref, "60 dB, per-row incoming gradients")
    ests, refs, ref = R.planted_clear(2, 1, R.S_ABOVE_CHUNK_GROWTH, seed=9)
    _check(dev, ests, refs, ref, f"S={R.S_ABOVE_CHUNK_GROWTH}")


# ---- item 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,S,lengths", [(2, 1030, (1030, 513, 5)), (4, 520, (512, 1, 519))])
def test_ragged_rows_are_the_one_row_calls_bit_for_bit(dev, k, S, lengths):
    N = len(lengths)
    ests, refs = R.planted(k, N, S, seed=40 + k)
    de, dr = [_rows(e, dev, 3, 1) for e in ests], [_rows(r, dev, 3, 1) for r in refs]
    for t in de + dr:
        for b, n in enumerate(lengths):
            t[b, n:] = float("nan")                      # what lies beyond a row's length is never used
    gv = torch.linspace(0.5, 1.5, N, device=dev)
    xs = [e.detach().requires_grad_(True) for e in de]
    value, perm = L.sisnr_pit(xs, dr, lengths=list(lengths), return_perm=True)
    (value * gv).sum().backward()
    grad = torch.stack([x.grad for x in xs])
    assert torch.isfinite(value).all() and torch.isfinite(grad).all()
    v2, p2 = L.sisnr_pit(de, dr, lengths=torch.tensor(lengths, dtype=torch.int32, device=dev), return_perm=True)
    assert torch.equal(value.detach(), v2) and torch.equal(perm, p2)          # host integers or a device tensor: the same call
    if min(lengths) >= 5:
        ref = R.reference(ests, refs, lengths, g_value=gv.cpu().numpy(), g_total=0.0)
        R.check_values(value.detach().cpu().numpy(), perm.cpu().numpy(), ref["loss"], ref, f"ragged k={k} {lengths}")
        R.check_grad(grad.cpu().numpy(), ref, f"ragged k={k} {lengths}")
    for b, n in enumerate(lengths):
        x1 = [torch.from_numpy(e[b:b + 1, :n].copy()).to(dev).requires_grad_(True) for e in ests]
        v1, p1 = L.sisnr_pit(x1, [torch.from_numpy(r[b:b + 1, :n].copy()).to(dev) for r in refs], return_perm=True)
        (v1 * gv[b:b + 1]).sum().backward()
        assert torch.equal(v1.detach(), value.detach()[b:b + 1]) and torch.equal(p1, perm[b:b + 1])
        assert torch.equal(torch.stack([x.grad[0] for x in x1]), grad[:, b, :n])
        assert not grad[:, b, n:].any()


# ---- item 4 ---------------------------------------------------------------------------------------------------------------
def test_degenerate_rows(dev, hip_loss):
    rng = np.random.default_rng(2)
    S = 257
    s = rng.standard_normal((1, S)).astype(np.float32)
    x = (s + 0.3 * rng.standard_normal((1, S))).astype(np.float32)
    zero, const = np.zeros((1, S), np.float32), np.full((1, S), 0.3, np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)                       # noqa: E731
    for name, est, ref in (("all-zero estimate", zero, s), ("constant estimate", const, s), ("all-zero reference", x, zero)):
        loss, grad = _loss_and_grad([t(est)], [t(ref)])
        print(f"{name}: loss {float(loss)!r}, max |gradient| {float(grad.abs().max())!r}")
        assert float(loss) == 160.0 and not grad.any()
    loss, grad = _loss_and_grad([t((2.0 * s).astype(np.float32))], [t(s)])
    print(f"exact multiple: value {-float(loss)!r} dB, max |gradient| {float(grad.abs().max()):.3e}")
    assert np.isfinite(float(loss)) and -float(loss) >= 120.0 and torch.isfinite(grad).all()


# ---- views of one tensor, separate tensors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N,S", [(2, 3, 150), (3, 1, 513), (4, 3, 64)])
def test_views_of_one_tensor_and_separate_tensors_same_bits(dev, hip_loss, k, N, S):
    ests, refs = R.planted(k, N, S, seed=70 + k)
    dr = [torch.from_numpy(r).to(dev) for r in refs]
    base = torch.from_numpy(ests).to(dev).requires_grad_(True)
    views = [base[i] for i in range(k)]
    assert L._pit_stacked_base(views) is base
    loss = L.si_snr_loss(views, dr)
    loss.backward()
    loss2, grad2 = _loss_and_grad([torch.from_numpy(e.copy()).to(dev) for e in ests], dr)
    assert torch.equal(loss.detach(), loss2) and torch.equal(base.grad, grad2)
    R.check_grad(base.grad.cpu().numpy(), R.reference(ests, refs), f"k={k} N={N} S={S}, the (k, N, S) tensor's gradient")


# ---- a tiny model, one training step per loss route ------------------------------------------------------------------------
def _model(cfg, sd, dev, dtype=torch.float32):
    m = onn.ConvTasNet(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).to(dtype).train()


def _grads(m):
    return {k: p.grad.detach().double().cpu().numpy() for k, p in m.named_parameters() if p.grad is not None}


def _batch(cfg, n, S, seed, dev):
    """A training batch: the mixture is the sum of its references (tests/test_gpu_tasnet_train.py: _three_way)."""
    rng = np.random.default_rng(seed)
    hop = cfg["L"] // 2
    S_out = ((S - cfg["L"]) // hop) * hop + cfg["L"]
    src = (0.1 * rng.standard_normal((cfg["num_spks"], n, S))).astype(np.float32)
    return torch.from_numpy(src.sum(axis=0)).to(dev), [torch.from_numpy(np.ascontiguousarray(r[:, :S_out])).to(dev) for r in src]


def test_tiny_model_one_step_per_loss_route(dev, monkeypatch):
    from onssen_amd import dist
    from onssen_amd.utils import build_optimizer
    from tests.tasnet_train_emu import grad_error
    cfg = dict(BASE, norm="gln", activate="relu", causal=False)
    sd = tasnet_ref.make_state(cfg, seed=5)
    x, refs = _batch(cfg, 2, 150, 31, dev)
    first, finals = {}, {}
    for route in ("aten", "hip", "hip"):
        monkeypatch.setenv("ONSSEN_TASNET_LOSS", route)
        m = _model(cfg, sd, dev)
        opt = build_optimizer(m.parameters(), {"name": "adam", "lr": 1e-3})
        vals = [dist.train_step(m, opt, L.si_snr_loss, [x], refs) for _ in range(2)]
        assert m.last_train_path == "hip" and L.last_si_snr_path == route
        first[route] = vals[0]
        finals.setdefault(route, []).append(copy.deepcopy({k: v.detach().cpu() for k, v in m.state_dict().items()}))
    print(f"first-step loss: aten route {first['aten']:.7f}, hip route {first['hip']:.7f}")
    assert abs(first["hip"] - first["aten"]) <= 1e-5 * max(1.0, abs(first["aten"]))
    for k in finals["hip"][0]:                                       # two identical steps give identical weights
        assert torch.equal(finals["hip"][0][k], finals["hip"][1][k]), k
    # parameter gradients of the hip-loss route against the fp64 ATen route
    monkeypatch.setenv("ONSSEN_TASNET_LOSS", "hip")
    m = _model(cfg, sd, dev)
    L.si_snr_loss(m([x]), refs).backward()
    assert m.last_train_path == "hip" and L.last_si_snr_path == "hip"
    m64 = _model(cfg, sd, dev, torch.float64)
    L.si_snr_loss(m64([x.double()]), [r.double() for r in refs]).backward()
    assert m64.last_train_path == "aten" and L.last_si_snr_path == "aten"
    err, where = grad_error(_grads(m), _grads(m64))
    print(f"hip network + hip loss against fp64 ATen: worst relative gradient error {err:.2e} ({where}), ceiling {CEILING:.0e}")
    assert err <= CEILING


# ---- graph capture ---------------------------------------------------------------------------------------------------------
def test_graph_capture_of_loss_forward_and_backward(dev, hip_loss):
    k, N, S = 2, 3, 1030
    data = [R.planted(k, N, S, seed=80 + i) for i in range(3)]
    base = torch.from_numpy(data[0][0]).to(dev).requires_grad_(True)
    refs = [torch.from_numpy(r).to(dev) for r in data[0][1]]

    def step():
        loss = L.si_snr_loss([base[i] for i in range(k)], refs)
        grad, = torch.autograd.grad(loss, base)
        return loss, grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s, grad_s = step()
    assert L.last_si_snr_path == "hip"
    for ests, rr in data[1:]:
        with torch.no_grad():
            base.copy_(torch.from_numpy(ests))
            for dst, r in zip(refs, rr):
                dst.copy_(torch.from_numpy(r))
        graph.replay()
        torch.cuda.synchronize()
        got = (loss_s.clone(), grad_s.clone())
        want = step()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        R.check_grad(got[1].cpu().numpy(), R.reference(ests, rr), "replayed graph")
