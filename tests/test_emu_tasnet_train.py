"""Conv-TasNet training through the C ABI on the host-side emulation build (tests/emu): the training forward against the eval
forward (bit for bit), the backward against fp64 autograd of the module's unchanged ATen path and against the reference's own
gradients (tests/golden/g8_tasnet_train.npz), determinism, and the refusals.  Geometry as tests/test_emu_tasnet.py: T = 74 frames
and channel counts 20 / 12 / 24, ragged against every tile, plus one case with channel counts 21 / 13 / 25 and L = 6 (no 16-byte
row alignment anywhere).  Every comparison prints what it measured.

Gradient metric and ceiling: the project's contract for these gradients (tests/test_gpu_tasnet.py): per parameter
max |g - g_ref| / max(max |g_ref|, 1e-3 of the model's largest gradient) <= 2e-3.  fp32 ATen autograd on the CPU is printed
beside the HIP path as the yardstick of what fp32 gives on the same case."""
import os

import numpy as np
import pytest

from tests import tasnet_emu, tasnet_ref
from tests.emu_build import load_emu
from tests.tasnet_train_emu import Step, aten_grads, grad_error, param_names

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BASE = dict(N=20, L=4, B=12, H=24, P=3, X=2, R=1, num_spks=2)
CASES = [
    dict(norm="gln", activate="relu", causal=False),
    dict(norm="gln", activate="softmax", causal=True),
    dict(norm="cln", activate="sigmoid", causal=False),
    dict(norm="cln", activate="relu", causal=True, P=5),
    dict(norm="gln", activate="sigmoid", causal=False, num_spks=3),
    dict(norm="cln", activate="softmax", causal=False, N=21, L=6, B=13, H=25),       # no channel count a multiple of 4, odd hop
]
IDS = lambda c: "-".join(f"{k}={v}" for k, v in c.items())          # noqa: E731
CEILING = 2e-3


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _x(n=2, S=150, seed=0):
    return (0.5 * np.random.default_rng(seed).standard_normal((n, S))).astype(np.float32)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_training_forward_is_the_eval_forward_bit_for_bit(lib, case, prec):
    cfg = dict(BASE, **case)
    sd = tasnet_ref.make_state(cfg, seed=5)
    for n in (1, 2):
        x = _x(n)
        st = Step(lib, sd, cfg, x, prec)
        ref = tasnet_emu.forward(lib, sd, cfg, x, prec)
        assert np.isfinite(st.out).all() and np.array_equal(st.out, ref)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_matches_fp64_autograd(lib, case, n, monkeypatch):
    monkeypatch.setenv("ONSSEN_CPU_AUTOGRAD", "1")
    import torch
    cfg = dict(BASE, **case)
    sd = tasnet_ref.make_state(cfg, seed=5)
    x = _x(n, seed=3)
    st = Step(lib, sd, cfg, x, "f32")
    d_out = np.random.default_rng(11).standard_normal(st.out.shape).astype(np.float32)
    got = st.backward(d_out)
    _, ref, _ = aten_grads(cfg, sd, x.astype(np.float64), torch.float64, d_out=d_out.astype(np.float64))
    _, g32, _ = aten_grads(cfg, sd, x, torch.float32, d_out=d_out)
    assert set(ref) == set(param_names(cfg))
    e_hip, where = grad_error(got, ref)
    e_aten, _ = grad_error(g32, ref)
    print(f"{IDS(case)} n={n}: HIP {e_hip:.2e} (worst: {where}), fp32 ATen {e_aten:.2e}, ceiling {CEILING:.0e}")
    assert all(np.isfinite(v).all() for v in got.values())
    assert float(np.abs(got["decoder.bias"]).max()) > 0.0          # a random d_out reaches every parameter
    assert e_hip <= CEILING


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_reference_gradient_fixture(lib, prec, monkeypatch):
    """g8_tasnet_train.npz: training forward on the emulation, si_snr_loss and its gradient with respect to the estimates in
    torch, the HIP backward -> every grad__* of the fixture."""
    monkeypatch.setenv("ONSSEN_CPU_AUTOGRAD", "1")
    import torch
    from onssen_amd import loss as L
    path = os.path.join(GOLD, "g8_tasnet_train.npz")
    z = np.load(path)
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(path)
    x = z["x"].astype(np.float32)
    st = Step(lib, sd, cfg, x, prec)
    refs = [torch.from_numpy(r).float() for r in z["refs"]]
    est = torch.from_numpy(st.out.copy()).requires_grad_(True)
    loss = L.si_snr_loss([est[s] for s in range(est.shape[0])], refs)
    loss.backward()
    print(f"{prec}: loss {float(loss.detach()):.6f} vs fixture {float(z['loss'][0]):.6f}")
    assert abs(float(loss.detach()) - float(z["loss"][0])) <= 1e-4 * max(1.0, abs(float(z["loss"][0])))
    got = st.backward(est.grad.numpy())
    ref = {k[6:]: z[k] for k in z.files if k.startswith("grad__")}
    assert set(ref) == set(param_names(cfg))
    _, g32, _ = aten_grads(cfg, sd, x, torch.float32, loss_fn=lambda e: L.si_snr_loss(e, refs))
    e_hip, where = grad_error(got, ref)
    e_aten, _ = grad_error(g32, ref)
    print(f"{prec}: HIP {e_hip:.2e} (worst: {where}), fp32 ATen {e_aten:.2e}, ceiling {CEILING:.0e}")
    assert e_hip <= CEILING


def test_two_backward_runs_same_bits(lib):
    for case in (CASES[0], CASES[3]):
        cfg = dict(BASE, **case)
        sd = tasnet_ref.make_state(cfg, seed=9)
        st = Step(lib, sd, cfg, _x(3, 141, seed=2), "f32")
        d_out = np.random.default_rng(4).standard_normal(st.out.shape).astype(np.float32)
        a, b = st.backward_flat(d_out), st.backward_flat(d_out)
        assert np.isfinite(a).all() and np.array_equal(a, b)


def test_refusals_write_nothing(lib):
    ok = dict(BASE, norm="gln", activate="relu", causal=False)
    sd = tasnet_ref.make_state(ok, seed=1)
    st = Step(lib, sd, ok, _x(), "f32")
    dll, cf, n, S = lib.dll, st.cf, st.n, st.S
    wsb, bwsb = lib.tasnet_workspace_bytes(cf, n, S), lib.tasnet_backward_workspace_bytes(cf, n, S)
    ws, bws = tasnet_emu.aligned(wsb), tasnet_emu.aligned(bwsb)
    out = np.full_like(st.out, 7.0)
    saved = tasnet_emu.aligned(st.saved_bytes)
    g = np.full(st.nparam, 7.0, dtype=np.float32)
    d_out = np.ones_like(st.out)

    def fwd(cfg_, saved_bytes, ws_bytes):
        return dll.onssen_tasnet_train_forward_f32(cfg_, st.image.ctypes.data, st.x.ctypes.data, n, S, S, out.ctypes.data,
                                                   saved.ctypes.data, saved_bytes, ws.ctypes.data, ws_bytes, None)

    def bwd(cfg_, saved_bytes, ws_bytes):
        return dll.onssen_tasnet_backward_f32(cfg_, st.image.ctypes.data, st.x.ctypes.data, n, S, S, st.saved.ctypes.data,
                                              saved_bytes, d_out.ctypes.data, g.ctypes.data, bws.ctypes.data, ws_bytes, None)

    assert fwd(cf, st.saved_bytes - 1, wsb) == -2 and fwd(cf, st.saved_bytes, wsb - 1) == -2
    assert bwd(cf, st.saved_bytes - 1, bwsb) == -2 and bwd(cf, st.saved_bytes, bwsb - 1) == -2
    bad = [dict(norm="bn"), dict(L=5), dict(L=66), dict(P=4), dict(N=1025), dict(num_spks=9)]
    for b in bad:
        c = tasnet_emu.lib_cfg(lib, dict(ok, **b), "f32")
        assert dll.onssen_tasnet_saved_bytes(c, n, S) == 0 and dll.onssen_tasnet_backward_workspace_bytes(c, n, S) == 0
        assert fwd(c, st.saved_bytes, wsb) == -1 and bwd(c, st.saved_bytes, bwsb) == -1
    assert (out == 7.0).all() and (g == 7.0).all() and not saved.any() and not ws.any() and not bws.any()
