#!/usr/bin/env python
"""Timings of unfolded-MISI training:  python tools/misi_train_probe.py [OUT.json]

  misi_phase_backward   onssen_misi_phase_backward_f32 (csrc/misi_bwd.inc: two launches) at B = 32, n = 25 536, STFT 256 / 64,
                        for C = 2 and C = 4, with the bytes it has to move and the bandwidth that makes
  misi_phase            the forward launch (csrc/misi.inc), for scale
  loss_wa_misi K        one forward + backward of ``loss.loss_wa_misi`` at K = 1 and K = 3 unfolded iterations
  aten                  the half-step composed of ATen operators with autograd, forward + backward: residual, ``torch.stft``
                        (centred, reflect padding, periodic Hann), Z / |Z| with the (1, 0) fallback

Every leg is captured in a hipGraph (20 calls per graph; 5 for the loss legs), warmed up, and a replay is timed with device events;
the legs alternate in one process, nine rounds each, median / min / max in microseconds per call.  Needs a ROCm device."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from onssen_amd.features import misi_phase, stft_logmag
from onssen_amd.hip import get_lib
from onssen_amd.loss import loss_wa_misi

assert torch.cuda.is_available(), "misi_train_probe: needs a ROCm device"
dev = torch.device("cuda:0")
torch.manual_seed(0)
B, N_FFT, HOP, n = 32, 256, 64, 25536
T, F = 1 + n // HOP, N_FFT // 2 + 1
CALLS, LOSS_CALLS, ROUNDS = 20, 5, 9
WINDOW = torch.hann_window(N_FFT, periodic=True, device=dev)


def aten_half_step(mix, est):
    """(B, C, T, F, 2) unit phases from ATen operators, differentiable with respect to ``est``."""
    C = est.shape[1]
    u = est + ((mix - est.sum(1)) / C)[:, None]
    Z = torch.stft(u.reshape(B * C, n), N_FFT, HOP, window=WINDOW, center=True, pad_mode="reflect", return_complex=True)
    Z = torch.view_as_real(Z.transpose(1, 2))                      # (B C, T, F, 2)
    nz = (Z[..., 0] != 0) | (Z[..., 1] != 0)
    h = torch.sqrt(torch.where(nz, Z[..., 0] ** 2 + Z[..., 1] ** 2, torch.ones_like(Z[..., 0])))
    p = torch.stack([torch.where(nz, Z[..., 0] / h, torch.ones_like(h)), torch.where(nz, Z[..., 1] / h, torch.zeros_like(h))], -1)
    return p.view(B, C, T, F, 2)


def graph_of(fn, calls):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def stats(v):
    return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))


lib = get_lib()
res = {"shape": dict(B=B, n=n, n_fft=N_FFT, hop=HOP, T=T), "calls_per_graph": CALLS, "loss_calls_per_graph": LOSS_CALLS, "rounds": ROUNDS}
for C in (2, 4):
    mix = 0.3 * torch.randn(B, n, device=dev)
    est = 0.2 * torch.randn(B, C, n, device=dev)
    g_p = torch.randn(C, B, T, F, 2, device=dev)
    nbytes = lib.misi_phase_backward_workspace_bytes(B, C, n, N_FFT, HOP)
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    g_est = torch.empty(B, C, n, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def backward_entry():
        lib.misi_phase_backward(mix.data_ptr(), n, est.data_ptr(), C * n, n, B, C, n, N_FFT, HOP, g_p.data_ptr(), g_est.data_ptr(),
                                ws.data_ptr(), nbytes, stream())

    def forward_entry():
        with torch.no_grad():
            misi_phase(mix, est, N_FFT, HOP)

    est_leaf = est.clone().requires_grad_(True)
    g_p_aten = g_p.permute(1, 0, 2, 3, 4).contiguous()

    # (torch.autograd.grad, as tools/wa_probe.py: no gradient is accumulated into a leaf, so no node of an earlier call, made on
    # another stream, takes part in a capture)
    def aten():
        return torch.autograd.grad(aten_half_step(mix, est_leaf), est_leaf, g_p_aten)[0]

    # the fused backward against the ATen composition's gradient (float32 autograd through a complex64 transform)
    backward_entry()
    g_aten = aten()
    torch.cuda.synchronize()
    res[f"C{C}_max_abs_difference_to_aten"] = float((g_est - g_aten).abs().max())
    res[f"C{C}_max_abs_gradient"] = float(g_est.abs().max())
    del g_aten

    with torch.no_grad():
        _, ri = stft_logmag(mix, N_FFT, HOP)
    masks = torch.rand(B, T, F, C, device=dev).requires_grad_(True)
    src = 0.2 * torch.randn(B, C, HOP * (T - 1), device=dev)
    kind = "chimera" if C == 2 else "upit"
    emb = [torch.zeros(1, device=dev)] if C == 2 else []

    def loss_leg(K):
        def run():                                                     # the views of the masks are made per call, inside the capture
            loss = loss_wa_misi(emb + [masks[..., c] for c in range(C)], [ri, src], K, hop_size=HOP, kind=kind)
            return torch.autograd.grad(loss, masks)[0]
        return run

    legs = {"misi_phase_backward": (graph_of(backward_entry, CALLS), CALLS), "misi_phase": (graph_of(forward_entry, CALLS), CALLS),
            "aten_half_step_fwd_bwd": (graph_of(aten, CALLS), CALLS),
            "loss_wa_misi_K1_fwd_bwd": (graph_of(loss_leg(1), LOSS_CALLS), LOSS_CALLS),
            "loss_wa_misi_K3_fwd_bwd": (graph_of(loss_leg(3), LOSS_CALLS), LOSS_CALLS)}
    rows = {k: [] for k in legs}
    for _ in range(ROUNDS):                                            # alternate the legs: other work shares the machine
        for k, (g, calls) in legs.items():
            rows[k].append(replay_us(g, calls))
    for k, v in rows.items():
        res[f"C{C}_{k}"] = stats(v)
    # what the backward has to move once: mix, est and g_p in, the fp64 frames out and in again, g_est out
    moved = 4 * (B * n + C * B * n + C * B * T * F * 2 + C * B * n) + 2 * nbytes
    res[f"C{C}_misi_phase_backward_bytes"] = moved
    res[f"C{C}_misi_phase_backward_GBps"] = round(moved / (statistics.median(rows["misi_phase_backward"]) * 1e-6) / 1e9, 1)
    del legs

print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
