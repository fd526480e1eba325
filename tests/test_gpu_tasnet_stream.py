"""Streaming ConvTasNet on the device: ``model.stream(n)`` fed in chunks and flushed against ``model([x])`` of the whole signal,
bit for bit -- small configurations under every precision, the recipe's widths with chunks below and above its deepest history
(256 frames), a captured push replayed on a refilled static input, and the reset of one slot among three."""
import numpy as np
import pytest
import torch

from onssen_amd.separation import separate_tasnet_stream
from tests import tasnet_ref
from tests.test_emu_tasnet_stream import CASES, SBASE, SCHEDULE
from tests.test_gpu_tasnet import _model

pytestmark = pytest.mark.gpu

RECIPE = dict(N=512, L=16, B=128, H=512, P=3, X=8, R=1, norm="cln", activate="sigmoid", causal=True, num_spks=2)
RECIPE_SCHEDULE = [40, 8, 1, 300, 8, 8, 255, 20]            # hops; the deepest history is 2 * 2^7 = 256 frames


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _signal(n, samples, dev, seed=0):
    return torch.from_numpy((0.5 * np.random.default_rng(seed).standard_normal((n, samples))).astype(np.float32)).to(dev)


def _offline(m, x):
    with torch.no_grad():
        return torch.stack([o.reshape(x.shape[0], -1) for o in m([x])])          # (spk, n, S)


def _manual(m, x, schedule):
    """Push by push -> (spk, n, S + hop): the step outputs (delay included) followed by the flush."""
    hop, at, outs = m.L // 2, 0, []
    with torch.no_grad():
        st = m.stream(x.shape[0])
        for F in schedule:
            outs.append(torch.stack(st.push(x[:, at:at + F * hop])))
            at += F * hop
        outs.append(torch.stack(st.flush()))
    assert at == x.shape[1]
    return torch.cat(outs, dim=-1)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_small_configurations(case, prec, dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    cfg = dict(SBASE, **case)
    m = _model(cfg, tasnet_ref.make_state(cfg, seed=5), dev)
    hop = cfg["L"] // 2
    x = _signal(3, sum(SCHEDULE) * hop, dev)
    ref = _offline(m, x)
    assert torch.isfinite(ref).all() and ref.shape == (cfg["num_spks"], 3, x.shape[1])
    for chunk in (7, 1000):
        est = separate_tasnet_stream(m, x, chunk)
        assert len(est) == cfg["num_spks"]
        for s, e in enumerate(est):
            assert torch.equal(e, ref[s]), f"separate_tasnet_stream(chunk={chunk}), speaker {s}"
    # the schedule, then the whole run again as 129 steps of one hop and as one step of 129 hops (the emulation runs the
    # one-hop steps for one configuration only: tests/test_emu_tasnet_stream.py says why)
    for schedule in (SCHEDULE, [1] * sum(SCHEDULE), [sum(SCHEDULE)]):
        got = _manual(m, x, schedule)
        assert torch.count_nonzero(got[..., :hop]) == 0 and torch.isfinite(got).all(), f"{len(schedule)} steps"
        assert torch.equal(got[..., hop:], ref), f"{len(schedule)} steps"
    # samples beyond the last whole hop are dropped, as the forward drops them; 1-D in, 1-D out
    with torch.no_grad():
        one = m([x[0, :101]])
    for a, b in zip(separate_tasnet_stream(m, x[0, :101], 16), one):
        assert a.shape == b.shape == (100,) and torch.equal(a, b)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_recipe_widths(prec, dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    m = _model(RECIPE, tasnet_ref.make_state(RECIPE, seed=7), dev)
    hop = RECIPE["L"] // 2
    x = _signal(2, sum(RECIPE_SCHEDULE) * hop, dev, seed=3)
    assert x.shape[1] == 5120
    ref = _offline(m, x)
    got = _manual(m, x, RECIPE_SCHEDULE)
    assert torch.isfinite(got).all() and torch.count_nonzero(got[..., :hop]) == 0
    assert torch.equal(got[..., hop:], ref)


def test_graph_replay_advances_the_stream(dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", "f32")
    cfg = dict(SBASE, **CASES[0])
    m = _model(cfg, tasnet_ref.make_state(cfg, seed=5), dev)
    hop, F, steps = cfg["L"] // 2, 8, 20
    x = _signal(3, steps * F * hop, dev, seed=9)
    ref = _offline(m, x)
    eager = _manual(m, x, [F] * steps)
    with torch.no_grad():
        st = m.stream(3)
        static = torch.zeros(3, F * hop, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm up off the default stream, then start over
            st.push(static)
            st.reset()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = torch.stack(st.push(static))
        st.reset()                                          # capture launches nothing; this is for the reader
        outs = []
        for k in range(steps):
            static.copy_(x[:, k * F * hop:(k + 1) * F * hop])
            g.replay()
            outs.append(out.clone())
        outs.append(torch.stack(st.flush()))
    got = torch.cat(outs, dim=-1)
    assert torch.equal(got, eager)
    assert torch.count_nonzero(got[..., :hop]) == 0 and torch.equal(got[..., hop:], ref)


def test_reset_of_one_slot(dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", "f32")
    cfg = dict(SBASE, **CASES[0])
    m = _model(cfg, tasnet_ref.make_state(cfg, seed=5), dev)
    hop = cfg["L"] // 2
    x = _signal(3, sum(SCHEDULE) * hop, dev, seed=1)
    y = _signal(1, (sum(SCHEDULE) - 21) * hop, dev, seed=2)
    undisturbed = _manual(m, x, SCHEDULE)
    mixed = x.clone()
    mixed[1, 21 * hop:] = y[0]
    outs, at = [], 0
    with torch.no_grad():
        st = m.stream(3)
        for i, F in enumerate(SCHEDULE):
            if i == 4:
                assert at == 21 * hop
                st.reset([1])
            outs.append(torch.stack(st.push(mixed[:, at:at + F * hop])))
            at += F * hop
        outs.append(torch.stack(st.flush()))
    got = torch.cat(outs, dim=-1)
    for b in (0, 2):
        assert torch.equal(got[:, b], undisturbed[:, b])
    assert torch.equal(got[:, 1, :21 * hop], undisturbed[:, 1, :21 * hop])
    assert torch.count_nonzero(got[:, 1, 21 * hop:22 * hop]) == 0
    assert torch.equal(got[:, 1, 22 * hop:], _offline(m, y)[:, 0])
