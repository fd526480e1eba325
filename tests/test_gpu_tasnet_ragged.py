"""ConvTasNet over ragged batches on the device: ``forward([x], lengths=)`` against a loop of one-utterance forwards, bit for
bit (fixture configurations, the recipe shape, under graph replay), against tests/tasnet_ref.py inside the bounds of
tests/test_gpu_tasnet.py, and through ``tester_tasnet.eval(batch=K)`` and ``separation.separate_tasnet``.  The padding of
every input row is NaN: a kernel that read beyond an utterance's own samples would show it."""
import os

import numpy as np
import pytest
import torch

from tests import tasnet_ref
from tests.test_gpu_tasnet import FIXTURES, _errors, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _padded(waves, dev, extra=5):
    """(n, S_max + extra) on the device, NaN beyond each row's own samples."""
    x = np.full((len(waves), max(len(w) for w in waves) + extra), np.nan, dtype=np.float32)
    for b, w in enumerate(waves):
        x[b, :len(w)] = w
    return torch.from_numpy(x).to(dev)


def _loop(m, waves, dev):
    """The one-utterance forward of every waveform: list of (num_spks, S_out_b) tensors."""
    out = []
    with torch.no_grad():
        for w in waves:
            out.append(torch.stack([o.reshape(-1) for o in m([torch.from_numpy(w).to(dev)])]))
    return out


def _check_rows(est, alone, what):
    """est: num_spks tensors (n, S_out_max); alone[b] (num_spks, S_out_b): equal bits in [0, S_out_b), zeros after."""
    est = torch.stack(list(est))                                   # (spk, n, S_out_max)
    assert est.shape[2] == max(a.shape[1] for a in alone)
    for b, a in enumerate(alone):
        so = a.shape[1]
        assert torch.isfinite(est[:, b, :so]).all(), f"{what}: utterance {b}"
        assert torch.equal(est[:, b, :so], a), f"{what}: utterance {b} differs from its one-utterance forward"
        assert torch.count_nonzero(est[:, b, so:]) == 0 and not torch.isnan(est[:, b, so:]).any(), f"{what}: utterance {b} tail"


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[10:-4])
def test_fixture_configurations(path, prec, dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(path)
    m = _model(cfg, sd, dev)
    rng = np.random.default_rng(21)
    L = cfg["L"]
    lens = [L, 150, 97, 263, 2 * 64 * (L // 2) + L + 1]              # one frame ... 129 frames and a sample that fills none
    waves = [(0.5 * rng.standard_normal(s)).astype(np.float32) for s in lens]
    with torch.no_grad():
        est = m([_padded(waves, dev)], lengths=lens)
    assert len(est) == cfg["num_spks"] and all(e.dim() == 2 and e.shape[0] == len(lens) for e in est)
    _check_rows(est, _loop(m, waves, dev), f"{os.path.basename(path)} {prec}")


_RECIPE = {}
RECIPE_LENS = [16000, 37152, 23999, 8016]


def _recipe():
    if not _RECIPE:
        sd = tasnet_ref.make_state(tasnet_ref.RECIPE, seed=11)
        rng = np.random.default_rng(13)
        waves = [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in RECIPE_LENS]
        _RECIPE["case"] = (sd, waves, [np.stack(tasnet_ref.forward(sd, w, tasnet_ref.RECIPE)) for w in waves])
    return _RECIPE["case"]


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_recipe_shape(prec, dev, monkeypatch):
    monkeypatch.setenv("ONSSEN_PRECISION", prec)
    sd, waves, refs = _recipe()
    m = _model(tasnet_ref.RECIPE, sd, dev)
    with torch.no_grad():
        est = m([_padded(waves, dev)], lengths=RECIPE_LENS)
    _check_rows(est, _loop(m, waves, dev), f"recipe {prec}")
    est = torch.stack(list(est)).cpu().numpy()
    for b, ref in enumerate(refs):
        amax, rel = _errors(est[:, b, :ref.shape[1]], ref)
        print(f"recipe ragged {prec} utterance {b} ({RECIPE_LENS[b]} samples): max |err| {amax:.2e} "
              f"(max |ref| {np.abs(ref).max():.3f}), worst rel L2 {rel:.2e}")
        assert rel <= 1e-5 and amax <= 2e-5 * max(1.0, float(np.abs(ref).max()))


def test_graph_replay_same_bits(dev):
    cfg, sd, _, _, _ = tasnet_ref.load_fixture([f for f in FIXTURES if f.endswith("g8_tasnet_gln_relu.npz")][0])
    m = _model(cfg, sd, dev)
    rng = np.random.default_rng(5)
    lens = [900, 260, 1337, 64]
    waves = [(0.5 * rng.standard_normal(s)).astype(np.float32) for s in lens]
    xd = _padded(waves, dev)
    with torch.no_grad():
        eager = torch.stack(list(m([xd], lengths=lens))).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        m([xd], lengths=lens)                                       # warm: the image exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = m([xd], lengths=lens)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(list(out)), eager)


def _collect(t, **kw):
    """eval(**kw) with every utterance's SI-SDR collected from ``_one``: ({key of the mixture: sdr}, mean)."""
    got, orig = {}, t._one

    def one(input, label, ragged):
        sdr = orig(input, label, ragged)
        mix, = input
        lens = [mix.shape[1]] * mix.shape[0] if ragged is None else ragged[0]
        for b in range(mix.shape[0]):
            got[(int(lens[b]), mix[b, :16].cpu().numpy().tobytes())] = sdr.reshape(-1)[b:b + 1].clone()
        return sdr
    t._one = one
    try:
        mean = t.eval(**kw)
    finally:
        del t._one
    torch.cuda.synchronize()
    return {k: float(v.cpu()[0]) for k, v in got.items()}, mean


def test_tester_batched_equals_the_loop(dev):
    from onssen_amd.data import time_domain, wsj0_2mix_dataloader
    from onssen_amd.evaluate import tester_tasnet
    from onssen_amd.synthetic import synth_mixture
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(FIXTURES[0])
    m = _model(cfg, sd, dev)
    fo = {"data_path": "synthetic", "batch_size": 1, "sampling_rate": 8000, "chunk_size": 400, "n_utterances": 3,
          "min_samples": 300, "max_samples": 500}
    spread = [time_domain.eval_item(*synth_mixture(900 + k, n, 8000, return_sources=True), dev)
              for k, n in enumerate([300, 1200, 517, 700, 1013, 350, 840])]
    for name, loader in (("synthetic tt loader", wsj0_2mix_dataloader("conv-tasnet", fo, "tt", dev)), ("list of items", spread)):
        t = tester_tasnet({"model": m, "test_loader": loader, "device": dev})
        one, mean1 = _collect(t)
        many, meank = _collect(t, batch=3, bucket=2)
        assert len(one) == len(list(loader)) and set(one) == set(many), name
        print(f"{name}: {len(one)} utterances, mean SI-SDR {mean1:.6f} dB (batch 1), {meank:.6f} dB (batch 3, bucket 2)")
        for k in one:
            assert np.float32(one[k]).tobytes() == np.float32(many[k]).tobytes(), f"{name}: utterance of {k[0]} samples"
        assert abs(mean1 - meank) <= 1e-9


def test_separate_tasnet_more_than_one_abi_batch(dev):
    from onssen_amd.separation import separate_tasnet
    cfg, sd, _, _, _ = tasnet_ref.load_fixture([f for f in FIXTURES if f.endswith("g8_tasnet_gln_relu.npz")][0])
    m = _model(cfg, sd, dev)
    rng = np.random.default_rng(17)
    lens = [int(v) for v in rng.integers(cfg["L"], 400, 70)]
    waves = [(0.5 * rng.standard_normal(s)).astype(np.float32) for s in lens]
    out = separate_tasnet(m, [torch.from_numpy(w).to(dev) for w in waves])
    alone = _loop(m, waves, dev)
    assert len(out) == 70
    for k in range(70):
        assert out[k].shape == alone[k].shape and torch.equal(out[k], alone[k]), f"waveform {k} ({lens[k]} samples)"
