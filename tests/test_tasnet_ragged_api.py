"""ConvTasNet.forward(..., lengths=) and separation.separate_tasnet on the host: what is refused, and with which words, before
any library call; the batching arithmetic of separate_tasnet on a stub model."""
import inspect

import pytest
import torch

from onssen_amd import _abi, nn as onn
from onssen_amd.separation import separate_tasnet

CFG = dict(N=8, L=4, B=4, H=8, P=3, X=1, R=1)


def _model():
    return onn.ConvTasNet(**CFG).eval()


def test_signature_keeps_the_default():
    sig = inspect.signature(onn.ConvTasNet.forward)
    assert list(sig.parameters) == ["self", "input", "lengths"] and sig.parameters["lengths"].default is None
    assert onn.ConvTasNet.RAGGED_MAX == _abi.TASNET_RAGGED_MAX == 64


def test_lengths_none_is_the_old_call(monkeypatch):
    """Without lengths the forward dispatches exactly as before: an eval forward of a CPU tensor still names the device."""
    monkeypatch.delenv("ONSSEN_CPU_AUTOGRAD", raising=False)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):
        _model()([torch.zeros(2, 40)])
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):
        _model()([torch.zeros(2, 40)], lengths=None)


@pytest.mark.parametrize("lengths, exc, words", [
    ([40, 30, 20], ValueError, "3 lengths for a batch of 2 rows"),
    ([40, 3], ValueError, r"lengths\[1\] = 3 samples is shorter than one encoder frame \(L = 4\)"),
    ([41, 30], ValueError, r"lengths\[0\] = 41 exceeds the 40 samples"),
    ([40, 30.5], TypeError, "must be integers"),
    ([40, True], TypeError, "must be integers"),
    (torch.tensor([40.0, 30.0]), TypeError, "integer tensor"),
])
def test_lengths_validation(lengths, exc, words):
    with torch.no_grad(), pytest.raises(exc, match=words):
        _model()([torch.zeros(2, 40)], lengths=lengths)


def test_more_utterances_than_the_abi_takes():
    with torch.no_grad(), pytest.raises(ValueError, match="at most 64 utterances, got 65"):
        _model()([torch.zeros(65, 40)], lengths=[40] * 65)


def test_valid_host_lengths_reach_the_device_check():
    """A list, a tuple and a CPU integer tensor pass the validation (the next refusal is the CPU input itself)."""
    for lengths in ([40, 30], (40, 30), torch.tensor([40, 30]), torch.tensor([40, 30], dtype=torch.int32)):
        with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm device"):
            _model()([torch.zeros(2, 40)], lengths=lengths)


def test_device_lengths_say_why():
    class OnDevice(torch.Tensor):                 # a tensor that reports a device, without needing one
        is_cuda = True
    t = torch.tensor([40, 30]).as_subclass(OnDevice)
    with torch.no_grad(), pytest.raises(TypeError, match="synchronisation"):
        _model()([torch.zeros(2, 40)], lengths=t)


def test_train_mode_and_autograd_are_refused():
    m = _model()
    with pytest.raises(RuntimeError, match="inference call"):       # eval mode, but the parameters want gradients
        m([torch.zeros(2, 40)], lengths=[40, 30])
    with torch.no_grad(), pytest.raises(RuntimeError, match="inference call"):
        m.train()([torch.zeros(2, 40)], lengths=[40, 30])
    m.eval()
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="inference call"):       # an input that wants a gradient
        m([torch.zeros(2, 40, requires_grad=True)], lengths=[40, 30])


class _Stub:
    """Stands in for ConvTasNet: records the calls, returns speaker s of row b as (s + 1) * x[b] over [0, S_out_b), zero after."""
    RAGGED_MAX, L, num_spks = 64, 4, 2

    def __init__(self):
        self.calls = []

    def __call__(self, input, lengths=None):
        x, = input
        self.calls.append((tuple(x.shape), list(lengths)))
        hop = self.L // 2
        so = [((v - self.L) // hop) * hop + self.L for v in lengths]
        out = [torch.zeros(x.shape[0], max(so)) for _ in range(self.num_spks)]
        for s in range(self.num_spks):
            for b, n in enumerate(so):
                out[s][b, :n] = (s + 1) * x[b, :n]
        return out


def test_separate_tasnet_batches_and_cuts():
    lens = [10 + 3 * (k % 17) for k in range(70)]                   # odd and even: some last samples fill no frame
    waves = [torch.arange(1, n + 1, dtype=torch.float32) + 100 * k for k, n in enumerate(lens)]
    m = _Stub()
    out = separate_tasnet(m, waves)
    assert [c[1] for c in m.calls] == [lens[:64], lens[64:]]
    assert [c[0] for c in m.calls] == [(64, max(lens[:64])), (6, max(lens[64:]))]
    assert len(out) == 70
    for k, (w, o) in enumerate(zip(waves, out)):
        so = ((lens[k] - 4) // 2) * 2 + 4
        assert so == min(lens[k], so) and o.shape == (2, so)
        assert torch.equal(o[0], w[:so]) and torch.equal(o[1], 2 * w[:so])
    assert separate_tasnet(_Stub(), []) == []


def test_separate_tasnet_refusals():
    with pytest.raises(ValueError, match="1-D"):
        separate_tasnet(_Stub(), [torch.zeros(1, 10)])
