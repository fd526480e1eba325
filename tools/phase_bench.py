#!/usr/bin/env python
"""Timings of the phase network's loss and reconstruction.  Modes:
  events [OUT.json]  device-event times of loss_phase forward + backward (HIP route against PyTorch-ops route, alternating) and of
                     phase_istft / mask_istft calls; median, min, max per leg (default OUT: profiles/phase_events.json)
  trace              30 calls of each, to be run under `rocprofv3 --kernel-trace --stats` in a run of its own
  trace-parent PATH  mask_istft only, through the library at PATH (a build of the parent commit), for the same kind of run
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

mode = sys.argv[1]
dev = torch.device("cuda:0")
torch.manual_seed(0)
ISTFT = {"b32_t400_f129": (32, 256, 64, 25536), "cfg5_b32_t126_f257": (32, 512, 128, 16000)}


def istft_inputs(B, nfft, hop, n):
    T, F = 1 + n // hop, nfft // 2 + 1
    ri = torch.randn(B, T, F, 2, device=dev)
    masks = torch.rand(B, T, F, 2, device=dev)
    ph = torch.nn.functional.normalize(torch.randn(2, B, T, F, 2, device=dev), dim=-1)
    return ri, masks, ph, T, F


def timed(fn, reps=50, rounds=7):
    for _ in range(5):
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


if mode == "trace-parent":
    import ctypes as C
    dll = C.CDLL(sys.argv[2])
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    dll.onssen_mask_istft_f32.argtypes = [vp, vp, i64, i64, i64, i64, i, i, i, i, i, i, vp, vp]
    for name, (B, nfft, hop, n) in ISTFT.items():
        ri, masks, ph, T, F = istft_inputs(B, nfft, hop, n)
        out = torch.empty(B, 2, n, device=dev)
        for _ in range(30):
            rc = dll.onssen_mask_istft_f32(ri.data_ptr(), masks.data_ptr(), masks.stride(0), masks.stride(3), masks.stride(1),
                                           masks.stride(2), B, 2, T, nfft, hop, n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
        torch.cuda.synchronize()
    print("trace-parent done")
    sys.exit(0)

from onssen_amd import loss as L, options
from onssen_amd.features import mask_istft, phase_istft

# cfg5 training shape: 32 chunks of 1 s at 16 kHz, STFT 512 / 128 -> (32, 126, 257)
B, T, F, D = 32, 126, 257, 20
emb = torch.nn.functional.normalize(torch.randn(B, T, F, D, device=dev), dim=-1)
one_hot = torch.nn.functional.one_hot(torch.randint(0, 3, (B, T, F), device=dev), 3)[..., :2].float()
x = torch.rand(B, T, F, device=dev) + 0.05
s1, s2 = x * torch.rand_like(x), x * torch.rand_like(x)
q1, q2 = torch.randn(B, T, F, 2, device=dev), torch.randn(B, T, F, 2, device=dev)
leaf = torch.rand(B, T, F, 2, device=dev).requires_grad_(True)
pA = torch.nn.functional.normalize(torch.randn(B, T, F, 2, device=dev), dim=-1).requires_grad_(True)
pB = torch.nn.functional.normalize(torch.randn(B, T, F, 2, device=dev), dim=-1).requires_grad_(True)
label = [one_hot, x, s1, s2, q1, q2]


def terms_step(route):
    """forward + backward of the mask and phase terms alone (the embedding term is loss_dc on either route)"""
    buf = leaf * 1.0
    mA, mB = buf[..., 0], buf[..., 1]
    if route == "hip":
        lm, lp = L._phase_terms_hip(mA, mB, pA, pB, *label[1:], True)
    else:
        lm, lp = L._phase_terms(mA, mB, pA, pB, *label[1:])
    torch.autograd.grad((lm + lp).sum(), [leaf, pA, pB])


def loss_step(route):
    options.configure(loss="1" if route == "hip" else "torch")
    e = emb.detach().requires_grad_(True)
    buf = leaf * 1.0
    got = L.loss_phase([e, buf[..., 0], buf[..., 1], pA, pB], label)
    torch.autograd.grad(got.mean(), [e, leaf, pA, pB])


if mode == "events":
    res = {}
    rows = {k: [] for k in ("terms_hip", "terms_aten", "loss_hip", "loss_aten")}
    for _ in range(3):                      # alternate the routes: other work shares the box
        rows["terms_hip"] += timed(lambda: terms_step("hip"), 20, 3)
        rows["terms_aten"] += timed(lambda: terms_step("aten"), 20, 3)
        rows["loss_hip"] += timed(lambda: loss_step("hip"), 20, 3)
        rows["loss_aten"] += timed(lambda: loss_step("aten"), 20, 3)
    options.configure(loss=None)
    for k, v in rows.items():
        res[k] = dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v))
    for name, (Bi, nfft, hop, n) in ISTFT.items():
        ri, masks, ph, Ti, Fi = istft_inputs(Bi, nfft, hop, n)
        a, b = [], []
        for _ in range(3):
            a += timed(lambda: phase_istft(ri, masks, ph, hop, n), 50, 3)
            b += timed(lambda: mask_istft(ri, masks, hop, n), 50, 3)
        res["phase_istft_" + name] = dict(median_us=statistics.median(a), min_us=min(a), max_us=max(a))
        res["mask_istft_" + name] = dict(median_us=statistics.median(b), min_us=min(b), max_us=max(b))
    res["bins"] = B * T * F
    print(json.dumps(res, indent=1))
    json.dump(res, open(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "phase_events.json"), "w"), indent=1)
else:
    for _ in range(30):
        terms_step("hip")
    for name, (Bi, nfft, hop, n) in ISTFT.items():
        ri, masks, ph, Ti, Fi = istft_inputs(Bi, nfft, hop, n)
        for _ in range(30):
            phase_istft(ri, masks, ph, hop, n)
            mask_istft(ri, masks, hop, n)
    torch.cuda.synchronize()
    print("trace done")
