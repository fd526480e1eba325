"""separation.separate_tasnet_long and tasnet_long_geometry on the host: the window arithmetic against a brute-force count, and what
is refused, with which words, before any library call."""
import pytest
import torch

from onssen_amd.nn.tasnet import ConvTasNet
from onssen_amd.separation import separate_tasnet_long, tasnet_long_geometry
from tests import tasnet_long_ref as R

SMALL = dict(N=20, L=4, B=12, H=24, P=3, X=2, R=1)


@pytest.mark.parametrize("L, W, step", [(4, 204, 120), (4, 40, 24), (4, 8, 4), (16, 80, 40), (16, 64, 48), (2, 5, 3)])
def test_window_count_and_last_window_against_brute_force(L, W, step):
    hop, O = L // 2, W - step
    for S in range(L, 6 * W + 3):
        S_out, K, v = tasnet_long_geometry(L, S, W, step)
        assert (S_out, K, v) == R.geometry(L, S, W, step), S
        assert S_out == (S - L) // hop * hop + L <= S
        if S_out <= W:
            assert (K, v) == (1, S_out)
        else:
            assert K >= 2 and O < v <= W and (K - 1) * step + v == S_out
            assert (v - L) % hop == 0 and v >= L              # the last window is whole frames: its forward returns v samples
            covered = [0] * S_out                             # every sample is covered once or twice, pairs overlap in exactly O
            for k in range(K):
                for t in range(k * step, min(k * step + W, S_out)):
                    covered[t] += 1
            assert set(covered) <= {1, 2} and sum(c == 2 for c in covered) == (K - 1) * O


def test_geometry_messages_name_the_requirement():
    assert tasnet_long_geometry(4, 1003, 204, 120) == (1002, 8, 162)
    with pytest.raises(ValueError, match="step = 121 must be a positive multiple of hop"):
        tasnet_long_geometry(4, 1003, 204, 121)
    with pytest.raises(ValueError, match="step = 0 must be a positive multiple of hop"):
        tasnet_long_geometry(4, 1003, 204, 0)
    with pytest.raises(ValueError, match="window = 205 must be L = 4 plus a multiple of hop"):
        tasnet_long_geometry(4, 1003, 205, 120)
    with pytest.raises(ValueError, match=r"overlap = window - step = 2 must lie in \[L, window / 2\]"):
        tasnet_long_geometry(4, 1003, 204, 202)               # shorter than one frame
    with pytest.raises(ValueError, match=r"overlap = window - step = 104 must lie in \[L, window / 2\] = \[4, 102\]"):
        tasnet_long_geometry(4, 1003, 204, 100)               # three windows would cover a sample
    with pytest.raises(RuntimeError, match="shorter than one encoder frame"):
        tasnet_long_geometry(4, 3, 204, 120)


def test_refusals_come_before_any_library_call():
    model = ConvTasNet(**SMALL, norm="gln").eval()
    wav = torch.zeros(1003)
    # geometry, through the entry point itself (the default step is window // 2 rounded down to a multiple of hop)
    with pytest.raises(ValueError, match="step = 121"):
        separate_tasnet_long(model, wav, 204, 121)
    with pytest.raises(ValueError, match="window = 205"):
        separate_tasnet_long(model, wav, 205)
    with pytest.raises(ValueError, match="overlap = window - step = 104"):
        separate_tasnet_long(model, wav, 204, 100)
    with pytest.raises(ValueError, match="1-D"):
        separate_tasnet_long(model, torch.zeros(2, 1003), 204)
    with pytest.raises(ValueError, match="batch"):
        separate_tasnet_long(model, wav, 204, batch=0)
    with pytest.raises(ValueError, match="num_spks = 5 > 4"):
        separate_tasnet_long(ConvTasNet(**SMALL, num_spks=5).eval(), wav, 204)
    with pytest.raises(RuntimeError, match="cannot run this configuration"):
        separate_tasnet_long(ConvTasNet(**dict(SMALL, P=4)).eval(), wav, 204)
    # a CPU tensor: long and short signals alike
    with pytest.raises(RuntimeError, match="ROCm device"):
        separate_tasnet_long(model, wav, 204, 120)
    with pytest.raises(RuntimeError, match="ROCm device"):
        separate_tasnet_long(model, wav[:100], 204, 120)
    # train mode, and autograd through the input: the wording of forward(..., lengths=)
    model.train()
    with pytest.raises(RuntimeError, match="is an inference call: it needs eval mode and no autograd"):
        separate_tasnet_long(model, wav, 204, 120)
    model.eval()
    with pytest.raises(RuntimeError, match="ROCm device"):    # the call itself runs without autograd, as separate_tasnet does
        separate_tasnet_long(model, wav.clone().requires_grad_(), 204, 120)


def test_default_step():
    """window // 2 rounded down to a multiple of hop.  204 // 2 = 102 is one (overlap 102 = window / 2: accepted); 210 // 2 = 105
    is rounded down to 104, which leaves an overlap of 106 > 105: a window of an odd number of hops needs an explicit step."""
    model = ConvTasNet(**SMALL).eval()
    with pytest.raises(RuntimeError, match="ROCm device"):
        separate_tasnet_long(model, torch.zeros(1003), 204)
    with pytest.raises(ValueError, match="overlap = window - step = 106"):
        separate_tasnet_long(model, torch.zeros(1003), 210)
    with pytest.raises(RuntimeError, match="ROCm device"):
        separate_tasnet_long(model, torch.zeros(1003), 210, 106)


class _Stub(torch.nn.Module):
    """Stands in for ConvTasNet on the host: "separates" a signal whose two sources live on the even and on the odd samples,
    and, like a real model, hands them out in an order that depends on the window."""
    L, num_spks = 4, 2

    def __init__(self):
        super().__init__()
        self.calls = []

    def _require_hip_forward(self):
        pass

    def _hip_forward_rows(self, x):
        n, S = x.shape
        S_out = (S - self.L) // 2 * 2 + self.L
        self.calls.append((n, S))
        even = x[:, :S_out].clone()
        even[:, 1::2] = 0
        odd = x[:, :S_out] - even
        swap = (x[:, 0].abs() * 1000).long() % 2 == 1
        return torch.stack([torch.where(swap[:, None], odd, even), torch.where(swap[:, None], even, odd)])


@pytest.mark.parametrize("S, batch, calls", [(1003, 4, [(4, 204), (3, 204), (1, 162)]), (1003, 16, [(7, 204), (1, 162)]),
                                             (445, 4, [(3, 204)]), (445, 2, [(2, 204), (1, 204)]), (150, 4, [(1, 150)])])
def test_the_flow_on_a_stub_model_and_the_emulated_kernels(S, batch, calls, monkeypatch):
    """The Python side end to end on host memory: gather, forwards of ``batch`` full windows, the last window's own forward,
    placement into the (C, K, W) buffer, stitch."""
    import onssen_amd.hip
    import onssen_amd.nn._core as core
    from tests.emu_build import load_emu
    lib = load_emu()
    monkeypatch.setattr(onssen_amd.hip, "get_lib", lambda: lib)
    monkeypatch.setattr(core, "_stream", lambda: None)
    monkeypatch.setattr(core, "require_device", lambda x, who: None)
    m = _Stub().eval()
    g = torch.Generator().manual_seed(S)
    wav = torch.randn(S, generator=g)
    out, est, perm = separate_tasnet_long(m, wav, 204, 120, batch=batch, return_windows=True)
    assert m.calls == calls
    S_out, K, v_last = tasnet_long_geometry(4, S, 204, 120)
    assert out.shape == (2, S_out) and perm.shape == (K, 2) and est.shape[:2] == (2, K)
    first = int((wav[0].abs() * 1000).long() % 2)             # window 0 decides which source is output channel 0
    src = torch.zeros(2, S_out)
    src[first, 0::2] = wav[:S_out][0::2]
    src[1 - first, 1::2] = wav[:S_out][1::2]
    if K == 1:
        assert torch.equal(out, src) and perm.tolist() == [[0, 1]]
        return
    swaps = [int((wav[k * 120].abs() * 1000).long() % 2) for k in range(K)]
    assert perm.tolist() == [[0, 1] if s == first else [1, 0] for s in swaps] and len(set(swaps)) == 2
    ref = R.stitch(est.numpy(), 120, v_last)
    assert all(v >= R.MARGIN for v in ref["margins"])
    R.check_stitched(out.numpy(), ref)
    single = torch.from_numpy(ref["bound"] == 0)
    assert torch.equal(out[single], src[single]) and torch.allclose(out, src, rtol=16 * R.EPS, atol=0)
    assert torch.count_nonzero(est[:, K - 1, v_last:]) == 0
