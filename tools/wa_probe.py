#!/usr/bin/env python
"""Timings of waveform-approximation training's two new launches:  python tools/wa_probe.py [OUT.json]

  istft_backward   onssen_istft_backward_f32 (csrc/istft_bwd.inc), mask mode, against the forward mask_istft launch it is the
                   adjoint of, at B = 32, n = 25 536 (T = 400), STFT 256 / 64, C = 2
  wa_pit           loss.wa_pit forward + backward (csrc/loss_wa.inc) against the ATen composition of the same objective with
                   autograd: (est[:, :, None] - ref[:, None]).abs().sum(-1), the permutation scan, the minimum

The protocol is tools/misi_probe.py's: every leg is captured in a hipGraph (20 calls per graph), warmed up, and a replay is timed
with device events; the legs of a pair alternate in one process, nine rounds each, median / min / max in microseconds per call.
Needs a ROCm device."""
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from onssen_amd.features import mask_istft
from onssen_amd.hip import get_lib
from onssen_amd.loss import wa_pit

assert torch.cuda.is_available(), "wa_probe: needs a ROCm device"
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, N_FFT, HOP, n, C = 32, 256, 64, 25536, 2
T, F = 1 + n // HOP, N_FFT // 2 + 1
CALLS, ROUNDS = 20, 9


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


def stats(v):
    return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))


def alternate(ga, gb):
    a, b = [], []
    for _ in range(ROUNDS):                                        # alternate the legs: other work shares the machine
        a.append(replay_us(ga))
        b.append(replay_us(gb))
    return stats(a), stats(b)


def istft_backward(ri, gy):
    g_op = torch.empty(B, T, F, C, device=dev)
    get_lib().istft_backward(ri.data_ptr(), None, 0, 0, 0, 0, None, 0, 0, B, C, T, N_FFT, HOP, n, gy.data_ptr(), g_op.data_ptr(), None,
                             torch.cuda.current_stream().cuda_stream)
    return g_op


def aten_wa(est, ref):
    """(V (B,), d sum(V) / d est) on PyTorch ops: the C^2 distances by broadcasting, the scan over itertools.permutations."""
    D = (est[:, :, None] - ref[:, None]).abs().sum(-1)
    totals = torch.stack([sum(D[:, i, p[i]] for i in range(C)) for p in itertools.permutations(range(C))], 1)
    V = totals.min(dim=1).values / (C * n)
    return V, torch.autograd.grad(V.sum(), est)[0]


def hip_wa(est, ref):
    V = wa_pit(est, ref)
    return V, torch.autograd.grad(V.sum(), est)[0]


res = {"shape": dict(B=B, n=n, T=T, n_fft=N_FFT, hop=HOP, C=C), "calls_per_graph": CALLS, "rounds": ROUNDS}
ri = torch.randn(B, T, F, 2, device=dev)
masks = torch.rand(B, T, F, C, device=dev)
gy = torch.randn(B, C, n, device=dev)
with torch.no_grad():
    fwd_g, _ = graph_of(lambda: mask_istft(ri, masks, HOP, n))
    bwd_g, _ = graph_of(lambda: istft_backward(ri, gy))
    res["mask_istft_forward"], res["istft_backward"] = alternate(fwd_g, bwd_g)
    del fwd_g, bwd_g

ref = 0.3 * torch.randn(B, C, n, device=dev)
est = (ref.flip(1) + 0.1 * torch.randn(B, C, n, device=dev)).requires_grad_(True)
hip_g, (hv, hg) = graph_of(lambda: hip_wa(est, ref))
aten_g, (av, ag) = graph_of(lambda: aten_wa(est, ref))
res["wa_value_max_relative_difference"] = float(((hv - av).abs() / av.abs()).max())
res["wa_gradient_max_abs_difference"] = float((hg - ag).abs().max())
res["wa_pit_forward_backward"], res["aten_forward_backward"] = alternate(hip_g, aten_g)

print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
