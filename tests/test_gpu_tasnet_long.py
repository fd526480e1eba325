"""Long-form ConvTasNet separation on the device (separation.separate_tasnet_long; csrc/tasnet_stitch.inc): a signal of 1003
samples through windows of 204, 120 apart, 4 per forward (8 windows: forwards of 4 and 3 full windows and one of the last window's
162 samples).  The NumPy fp64 restatement of the geometry, the permutation search and the cross-fade (tests/tasnet_long_ref.py),
applied to the window estimates the call returns, reproduces ``perm`` exactly and the output within 8 * 2^-24 (|a| + |b|) on the
overlaps and bit for bit elsewhere; every window estimate is, within the forward's 1e-5 contract, the forward of that window
alone.  S_out = 1002 is no multiple of 4 (scalar stitch rows); 1005 samples give 1004 (float4 rows), 445 samples three full
windows in one forward."""
import numpy as np
import pytest
import torch

from onssen_amd.separation import separate_tasnet_long, tasnet_long_geometry
from tests import tasnet_long_ref as R
from tests import tasnet_ref
from tests.test_gpu_tasnet import _errors, _model

pytestmark = pytest.mark.gpu

SMALL = dict(N=20, L=4, B=12, H=24, P=3, X=2, R=1, num_spks=2, activate="relu")
MODELS = {"gln": dict(norm="gln", causal=False), "cln-causal": dict(norm="cln", causal=True)}
S, WINDOW, STEP, BATCH = 1003, 204, 120, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


_MODELS = {}


def _get(name, dev):
    if name not in _MODELS:
        cfg = dict(SMALL, **MODELS[name])
        _MODELS[name] = _model(cfg, tasnet_ref.make_state(cfg, seed=5), dev)
    return _MODELS[name]


def _signal(samples, dev, seed=0):
    return torch.from_numpy((0.5 * np.random.default_rng(seed).standard_normal(samples)).astype(np.float32)).to(dev)


def _check(m, x, window, step, batch):
    S_out, K, v_last = tasnet_long_geometry(m.L, x.shape[0], window, step)
    with torch.no_grad():
        out, est, perm = separate_tasnet_long(m, x, window, step, batch=batch, return_windows=True)
        plain = m([x])
        assert out.shape == (m.num_spks, S_out) and plain[0].shape == (S_out,)
        assert est.shape == (m.num_spks, K, window) and perm.shape == (K, m.num_spks) and perm.dtype == torch.int32
        assert torch.isfinite(out).all() and torch.isfinite(est).all()
        # every window estimate is the forward of that window alone (the last one: of its v_last samples), zeros after it
        for k in range(K):
            one = torch.stack(list(m([x[k * step:k * step + window]])))
            v = v_last if k == K - 1 else window
            assert one.shape == (m.num_spks, v)
            amax, rel = _errors(est[:, k, :v].cpu().numpy(), one.cpu().numpy())
            print(f"window {k}: max |err| {amax:.2e}, rel L2 {rel:.2e} against its one-at-a-time forward")
            assert rel <= 1e-5 and amax <= 2e-5 * max(1.0, float(one.abs().max()))
        assert torch.count_nonzero(est[:, K - 1, v_last:]) == 0
    ref = R.stitch(est.cpu().numpy(), step, v_last)
    print(f"K = {K}, v_last = {v_last}, margins {['%.3g' % v for v in ref['margins']]}, perm {ref['perm'].tolist()}")
    assert all(v >= R.MARGIN for v in ref["margins"]), ref["margins"]
    assert np.array_equal(perm.cpu().numpy(), ref["perm"])
    R.check_stitched(out.cpu().numpy(), ref)
    return out, est, perm


@pytest.mark.parametrize("name", sorted(MODELS))
def test_windows_perm_and_output_against_the_restatement(name, dev):
    assert tasnet_long_geometry(4, S, WINDOW, STEP) == (1002, 8, 162)
    _check(_get(name, dev), _signal(S, dev), WINDOW, STEP, BATCH)


@pytest.mark.parametrize("samples, geo", [(1005, (1004, 8, 164)), (445, (444, 3, 204))])
def test_float4_rows_and_a_full_last_window(samples, geo, dev):
    assert tasnet_long_geometry(4, samples, WINDOW, STEP) == geo and geo[0] % 4 == 0
    _check(_get("gln", dev), _signal(samples, dev, seed=1), WINDOW, STEP, BATCH)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_a_signal_inside_one_window_is_the_plain_forward(name, dev):
    m = _get(name, dev)
    for samples in (WINDOW, WINDOW + 1, 57):
        x = _signal(samples, dev, seed=2)
        with torch.no_grad():
            plain = torch.stack(list(m([x])))
            out, est, perm = separate_tasnet_long(m, x, WINDOW, STEP, batch=BATCH, return_windows=True)
            assert torch.equal(out, plain) and torch.equal(separate_tasnet_long(m, x, WINDOW, STEP), plain)
            assert est.shape == (2, 1, plain.shape[1]) and perm.tolist() == [[0, 1]]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_captured_call_replays_to_the_same_bits(name, dev):
    m = _get(name, dev)
    x = _signal(S, dev, seed=3)
    static = torch.zeros_like(x)
    with torch.no_grad():
        eager = separate_tasnet_long(m, x, WINDOW, STEP, batch=BATCH)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm up off the default stream: workspaces and the packed image exist
            separate_tasnet_long(m, static, WINDOW, STEP, batch=BATCH)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out, est, perm = separate_tasnet_long(m, static, WINDOW, STEP, batch=BATCH, return_windows=True)
        static.copy_(x)
        g.replay()
        first = out.clone()
        g.replay()
        assert torch.equal(first, eager) and torch.equal(out, eager)
        assert perm[0].tolist() == [0, 1]
