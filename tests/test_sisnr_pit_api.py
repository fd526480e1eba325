"""The SI-SNR PIT loss, the parts that need no GPU: the ``tasnet_loss`` option, ``sisnr_pit_limits``, CPU tensors staying on
the PyTorch ops under ``tasnet_loss = "hip"`` with today's numbers, and what ``sisnr_pit`` refuses."""
import numpy as np
import pytest
import torch

from onssen_amd import loss as L
from onssen_amd import options


def _pair(k=2, N=3, S=40, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    refs = [torch.randn(N, S, generator=g).to(dtype) for _ in range(k)]
    ests = [(r + 0.3 * torch.randn(N, S, generator=g).to(dtype)) for r in refs]
    return ests, refs


class _FakeDevice(torch.Tensor):
    """A CPU tensor that says it lives on a device: what the limits look at, without a GPU."""
    is_cuda = True


def _fake(ts):
    return [t.as_subclass(_FakeDevice) for t in ts]


def test_option_is_in_the_table_and_validated(monkeypatch):
    env, default, conv, doc = options.TABLE["tasnet_loss"]
    assert (env, default) == ("ONSSEN_TASNET_LOSS", "aten")
    assert conv("HIP") == "hip" and conv("aten") == "aten"
    with pytest.raises(ValueError):
        options.configure(tasnet_loss="triton")
    monkeypatch.delenv("ONSSEN_TASNET_LOSS", raising=False)
    old = options.configure(tasnet_loss="hip")
    try:
        assert options.get("tasnet_loss") == "hip"
        monkeypatch.setenv("ONSSEN_TASNET_LOSS", "aten")          # a set environment variable wins
        assert options.get("tasnet_loss") == "aten"
    finally:
        options.configure(**old)


def test_limits_give_their_reasons():
    ests, refs = _pair()
    assert any("CPU" in w for w in L.sisnr_pit_limits(ests, refs))
    assert L.sisnr_pit_limits(_fake(ests), _fake(refs)) == []
    e64, r64 = _pair(dtype=torch.float64)
    assert any("float64" in w for w in L.sisnr_pit_limits(_fake(e64), _fake(r64)))
    rg = [r.clone().requires_grad_(True) for r in refs]
    assert any("reference requires a gradient" in w for w in L.sisnr_pit_limits(_fake(ests), _fake(rg)))
    with torch.no_grad():
        assert L.sisnr_pit_limits(_fake(ests), _fake(rg)) == []
    e5, r5 = _pair(k=5)
    assert any("k = 5 > 4" in w for w in L.sisnr_pit_limits(_fake(e5), _fake(r5)))
    with torch.autograd.detect_anomaly(check_nan=False):
        assert any("anomaly" in w for w in L.sisnr_pit_limits(_fake(ests), _fake(refs)))
    assert any("(N, S)" in w for w in L.sisnr_pit_limits(_fake([e[0] for e in ests]), _fake([r[0] for r in refs])))


def test_cpu_tensors_under_the_hip_option_are_todays_loss(monkeypatch):
    ests, refs = _pair(seed=3)
    out = {}
    for opt in ("aten", "hip"):
        monkeypatch.setenv("ONSSEN_TASNET_LOSS", opt)
        xs = [e.clone().requires_grad_(True) for e in ests]
        loss = L.si_snr_loss(xs, refs)
        loss.backward()
        assert L.last_si_snr_path == "aten"
        out[opt] = (loss.detach().numpy().copy(), np.stack([x.grad.numpy() for x in xs]))
    assert np.array_equal(out["aten"][0], out["hip"][0]) and np.array_equal(out["aten"][1], out["hip"][1])
    # ... which is the reference's formula: the per-row sisnr of the better of the two assignments
    a = (L.sisnr(ests[0], refs[0]) + L.sisnr(ests[1], refs[1])) / 2
    b = (L.sisnr(ests[0], refs[1]) + L.sisnr(ests[1], refs[0])) / 2
    assert np.array_equal(out["hip"][0], (-torch.maximum(a, b).sum() / 3).numpy())


def test_sisnr_pit_refuses_what_the_kernels_cannot_take():
    ests, refs = _pair()
    with pytest.raises(RuntimeError, match="CPU tensors"):
        L.sisnr_pit(ests, refs)
    e5, r5 = _pair(k=5)
    with pytest.raises(RuntimeError, match="k = 5 > 4"):
        L.sisnr_pit(_fake(e5), _fake(r5))
    with pytest.raises(RuntimeError, match=r"sisnr: shapes differ, \(3, 40\) vs \(3, 39\)"):
        L.sisnr_pit(_fake(ests), _fake([refs[0], refs[1][:, :-1]]))
    with pytest.raises(ValueError, match="2 estimates for 1 references"):
        L.sisnr_pit(_fake(ests), _fake(refs[:1]))


def test_lengths_validation():
    dev = torch.device("cpu")
    assert L._pit_lengths(None, 3, 40, dev) is None
    got = L._pit_lengths([40, 1, 7], 3, 40, dev)
    assert got.dtype == torch.int32 and got.tolist() == [40, 1, 7]
    assert L._pit_lengths(torch.tensor([5, 6, 7]), 3, 40, dev).tolist() == [5, 6, 7]
    with pytest.raises(ValueError, match="2 lengths for a batch of 3 rows"):
        L._pit_lengths([40, 40], 3, 40, dev)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 41 lies outside \[1, 40\]"):
        L._pit_lengths([40, 41, 40], 3, 40, dev)
    with pytest.raises(ValueError, match=r"lengths\[0\] = 0 lies outside"):
        L._pit_lengths([0, 4, 40], 3, 40, dev)
    with pytest.raises(TypeError):
        L._pit_lengths([40.5, 4, 40], 3, 40, dev)
    with pytest.raises(TypeError):
        L._pit_lengths(torch.tensor([1.0, 2.0, 3.0]), 3, 40, dev)
    # through the public call: the lengths are looked at after the limits, so on a device-less machine the limits speak first
    ests, refs = _pair()
    with pytest.raises(RuntimeError, match="CPU tensors"):
        L.sisnr_pit(ests, refs, lengths=[40, 40])
