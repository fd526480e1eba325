#!/usr/bin/env python
"""Timings of the enhancement route and its kernels.  Modes:
  events [OUT.json]  device-event times, 16 utterances x 400 frames at 512 / 128, of ``separate_enhance`` against the route without
                     the magnitude mode of the inverse transform (the same forward, PyTorch ops forming clean / |X|, then
                     ``mask_istft``), alternating; median, min, max per leg -- and the largest difference of the two results
  trace              30 calls each of the label kernel, the two loss kernels (both modes) and ``mag_istft`` at the same shape, to be
                     run under `rocprofv3 --kernel-trace --stats` in a run of its own
Bytes per bin (what the kernels must move): labels 16 in + 12 out; loss MSA 8 / PSA 16; gradient MSA 12 / PSA 20.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from onssen_amd import loss as L, options
from onssen_amd.features import enhance_labels, mag_istft, mask_istft, stft_logmag
from onssen_amd.nn.enhancement import enhance
from onssen_amd.separation import separate_enhance

mode = sys.argv[1]
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, T, NFFT, HOP = 16, 400, 512, 128
F, n = NFFT // 2 + 1, HOP * (T - 1)


def timed(fn, reps, rounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return out          # us per call, one figure per round


if mode == "events":
    model = enhance(F, 300, 3).to(dev).eval()
    wav = 0.1 * torch.randn(B, n, device=dev)

    @torch.no_grad()
    def mask_route():
        logmag, ri = stft_logmag(wav, NFFT, HOP)
        mag = torch.hypot(ri[..., 0], ri[..., 1])
        clean, = model([logmag, mag])
        mask = clean / mag.clamp_min(1e-30)
        return mask_istft(ri, mask.unsqueeze(-1), HOP, n)[:, 0]

    new, old = separate_enhance(model, wav, NFFT, HOP), mask_route()
    torch.cuda.synchronize()
    res = dict(shape=[B, T, F], max_abs_difference=float((new - old).abs().max()), max_abs=float(new.abs().max()))
    rows = {"separate_enhance": [], "mask_route": []}
    for _ in range(3):                      # alternate the routes: other work shares the box
        rows["separate_enhance"] += timed(lambda: separate_enhance(model, wav, NFFT, HOP), 20, 3)
        rows["mask_route"] += timed(mask_route, 20, 3)
    for k, v in rows.items():
        res[k] = dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v))
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 2:
        json.dump(res, open(sys.argv[2], "w"), indent=1)
else:
    ri_n, ri_c = torch.randn(B, T, F, 2, device=dev), torch.randn(B, T, F, 2, device=dev)
    mn, mc, cd = enhance_labels(ri_n, ri_c)
    est = torch.rand(B, T, F, device=dev)
    options.configure(loss="1")
    for _ in range(30):
        enhance_labels(ri_n, ri_c)
        e = est.clone().requires_grad_(True)
        L.loss_mask_msa([e], [mc, cd]).backward()
        e = est.clone().requires_grad_(True)
        L.loss_mask_psa([e], [mn, mc, cd]).sum().backward()
        mag_istft(ri_n, mn, HOP, n)
    torch.cuda.synchronize()
    print("trace done: bins", B * T * F)
