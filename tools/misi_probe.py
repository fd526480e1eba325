#!/usr/bin/env python
"""Timings of the MISI half-step:  python tools/misi_probe.py [OUT.json]

  misi_phase        one fused launch (csrc/misi.inc) at B = 32, n = 25 536, STFT 256 / 64, for C = 2 and C = 4
  composed          the same half-step from what the package offered before the kernel: the ATen residual and add, stft_logmag(
                    return_stft=True) on (C B, n), an ATen normalisation of (C B, T, F, 2)
  separate_chimera  one call with misi_iters = 0, 1, 3 (hidden 600, 4 layers): the added cost per MISI iteration

The two half-steps are captured in a hipGraph each (20 calls per graph), warmed up, and a replay is timed with device events; the
legs alternate in one process, nine rounds each, median / min / max in microseconds per call.  The separator is timed eagerly
(device events around 10 calls, nine rounds).  Needs a ROCm device."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from onssen_amd.features import misi_phase, stft_logmag

assert torch.cuda.is_available(), "misi_probe: needs a ROCm device"
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, N_FFT, HOP, n = 32, 256, 64, 25536
CALLS, ROUNDS = 20, 9
ONE = torch.tensor([1.0, 0.0], device=dev)


def composed(mix, est):
    """(C, B, T, F, 2) unit phases through public calls: two reductions / element-wise passes over the waveforms, the STFT (which
    also writes a log-magnitude nobody reads, and rounds the spectrum to complex64), then hypot, compare, divide, select."""
    C = est.shape[1]
    d = (mix - est.sum(1)) / C
    u = torch.add(est.transpose(0, 1), d[None], out=torch.empty(C, *mix.shape, device=mix.device))      # speaker-major, one pass
    _, ri = stft_logmag(u.view(C * est.shape[0], -1), N_FFT, HOP, return_stft=True)
    h = torch.hypot(ri[..., 0], ri[..., 1]).unsqueeze(-1)
    return torch.where(h > 0, ri / h, ONE).view(C, est.shape[0], *ri.shape[1:])


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            keep = fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g, keep


def replay_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3


def eager_us(fn, calls=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def stats(v):
    return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))


res = {"shape": dict(B=B, n=n, n_fft=N_FFT, hop=HOP), "calls_per_graph": CALLS, "rounds": ROUNDS}
with torch.no_grad():
    for C in (2, 4):
        mix = 0.3 * torch.randn(B, n, device=dev)
        est = 0.2 * torch.randn(B, C, n, device=dev)
        fused_g, fused_out = graph_of(lambda: misi_phase(mix, est, N_FFT, HOP))
        comp_g, comp_out = graph_of(lambda: composed(mix, est))
        diff = (fused_out - comp_out).abs()
        res[f"C{C}_max_abs_difference"] = float(diff.max())           # (the composition rounds the spectrum to complex64 first)
        res[f"C{C}_share_of_bins_within_1e-4"] = float((diff <= 1e-4).float().mean())
        f, c = [], []
        for _ in range(ROUNDS):                                        # alternate the legs: other work shares the machine
            f.append(replay_us(fused_g))
            c.append(replay_us(comp_g))
        res[f"C{C}_misi_phase"], res[f"C{C}_composed"] = stats(f), stats(c)
        del fused_g, comp_g

    from onssen_amd import nn as onn
    from onssen_amd.separation import separate_chimera
    from onssen_amd.synthetic import make_state_dict, synth_batch
    sd = make_state_dict("chimera", 129, 600, 4, 20, 2, seed=1)
    model = onn.chimera(129, 600, 4, 20)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(dev).eval()
    wav = torch.from_numpy(synth_batch(1, B, n)).to(dev)
    legs = {K: (lambda K=K: separate_chimera(model, wav, misi_iters=K)) for K in (0, 1, 3)}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = {K: [] for K in legs}
    for _ in range(ROUNDS):
        for K, fn in legs.items():
            rows[K].append(eager_us(fn))
    for K, v in rows.items():
        res[f"separate_chimera_misi_iters_{K}"] = stats(v)
    res["added_us_per_iteration"] = round((statistics.median(rows[3]) - statistics.median(rows[0])) / 3, 2)

print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
