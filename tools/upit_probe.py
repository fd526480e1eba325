#!/usr/bin/env python
"""GPU box: the uPIT loss and separate_upit, timed as tools/dc_k_probe.py times its variants (device events, after warm-up, the
variants alternating inside one process, windows of >= 0.5 s, median and range over the rounds).

  1. value + gradient of loss_upit_psa on the HIP kernels against the PyTorch-ops route of the same function, at 16 x 400 x 129
     for S = 2 and 3 (the masks a leaf in the network's interleaved layout);
  2. the two kernels by themselves (the library entries, no autograd) and the bytes the algorithm needs per call over that time:
     forward (1 + 3 S) 4 bytes per bin, backward (1 + 3 S + S) 4 (the maps again, plus the S gradients written);
  3. separate_upit on 16 utterances of 25 536 samples (400 frames), uPIT_LSTM(129, 129, 600, 4 layers, S)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onssen_amd import loss as L
from onssen_amd.hip import get_lib
from onssen_amd.nn import uPIT_LSTM
from onssen_amd.separation import separate_upit
from onssen_amd.synthetic import synth_batch

dev = torch.device("cuda:0")
lib = get_lib()
B, T, F = (int(os.environ.get(k, v)) for k, v in (("B", 16), ("T", 400), ("F", 129)))
ROUNDS, WINDOW = 5, 0.5
TF = T * F
stream = lambda: torch.cuda.current_stream().cuda_stream


def window(fn):
    """ms per call over a window of at least WINDOW seconds."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    reps = max(3, int(np.ceil(WINDOW * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


variants = []
for S in (2, 3):
    g = torch.Generator(device=dev).manual_seed(S)
    x = torch.rand(B, T, F, device=dev, generator=g) + 1e-3
    src = torch.rand(S, B, T, F, device=dev, generator=g) * x
    cos = torch.rand(S, B, T, F, device=dev, generator=g) * 2 - 1
    leaf = torch.rand(B, T, F, S, device=dev, generator=g).requires_grad_(True)
    label = [x] + list(src) + list(cos)

    def step(how, leaf=leaf, label=label, S=S):
        os.environ["ONSSEN_LOSS_HIP"] = how
        leaf.grad = None
        L.loss_upit_psa([leaf[..., k] for k in range(S)], label).mean().backward()
        assert L.last_upit_path == ("grad" if how == "1" else "aten")

    out, perm = torch.empty(B, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.loss_upit_workspace_bytes(B, S), dtype=torch.uint8, device=dev)
    gb, d = torch.ones(B, device=dev), torch.empty(B, T, F, S, device=dev)
    maps = (leaf.data_ptr(), TF * S, S, 1, x.data_ptr(), src.data_ptr(), B * TF, cos.data_ptr(), B * TF, None, F, B, TF, S)
    variants += [(f"S={S} value+grad, HIP kernels", lambda step=step: step("1")),
                 (f"S={S} value+grad, PyTorch ops", lambda step=step: step("0")),
                 (f"S={S} forward kernels alone", lambda maps=maps, out=out, perm=perm, ws=ws: lib.loss_upit(
                     *maps, out.data_ptr(), perm.data_ptr(), None, ws.data_ptr(), ws.numel(), stream())),
                 (f"S={S} backward kernel alone", lambda maps=maps, gb=gb, perm=perm, d=d, S=S: lib.loss_upit_grad(
                     *maps, gb.data_ptr(), perm.data_ptr(), d.data_ptr(), TF * S, S, 1, stream()))]

    torch.manual_seed(S)
    model = uPIT_LSTM(F, F, 600, num_layers=4, num_speaker=S).to(dev).eval()
    wav = torch.from_numpy(synth_batch(7, B)).to(dev)
    variants.append((f"S={S} separate_upit, {B} utterances", lambda model=model, wav=wav: separate_upit(model, wav)))

for _, fn in variants:                                   # warm-up: allocations, code objects, packed weights
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name, _ in variants}
for r in range(ROUNDS):                                  # the variants alternate: drift hits all of them alike
    for name, fn in variants:
        times[name].append(window(fn))
print(f"workload: B={B} T={T} F={F}; {ROUNDS} rounds of >= {WINDOW} s per variant")
for name, _ in variants:
    t = np.array(times[name])
    line = f"  {name:36s} median {np.median(t) * 1e3:9.1f} us  (min {t.min() * 1e3:.1f}, max {t.max() * 1e3:.1f})"
    S = int(name[2])
    if "forward kernels" in name:
        nbytes = B * TF * (1 + 3 * S) * 4
        line += f"   {nbytes / 1e6:.1f} MB needed -> {nbytes / (np.median(t) * 1e-3) / 1e12:.2f} TB/s"
    if "backward kernel" in name:
        nbytes = B * TF * (1 + 4 * S) * 4
        line += f"   {nbytes / 1e6:.1f} MB needed -> {nbytes / (np.median(t) * 1e-3) / 1e12:.2f} TB/s"
    print(line)
