#!/usr/bin/env python
"""GPU box: the split-bf16 (x3) route for ONE Conv-TasNet weight gradient at the recipe shape (3 x 3 999 rows): dW [I][J] =
dY^T X from row-major x3 images (onssen_x3_image_f32 of both operands + onssen_linear_x3t), its time (images and GEMM apart)
and its error against fp64, for the two block shapes (conv1x1: 512 x 128, Sc_conv: 128 x 512).  The exact-fp32 kernel the
backward uses (tas_wgrad_kernel + merge) is timed by the kernel trace of a training step (tools/tasnet_bench.py
--train-profile); its error against fp64 is printed here from a torch fp32 contraction with fp32 accumulation of the same
operands as the yardstick of what fp32 products give.  One JSON line per shape."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onssen_amd.hip import get_lib          # noqa: E402

lib = get_lib()
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
zero = torch.zeros(64, device=dev)


def rows_img(m):
    o = torch.empty(m.shape[0], (m.shape[1] + 31) // 32, 2, 32, device=dev, dtype=torch.int16)
    lib.x3_image(m.data_ptr(), m.shape[1], 0, 1, m.shape[0], m.shape[1], o.data_ptr(), st)
    return o


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 1)


M = 3 * 3999
torch.manual_seed(0)
for name, I, J in (("conv1x1", 512, 128), ("Sc_conv", 128, 512)):
    dY, X = torch.randn(M, I, device=dev), torch.randn(M, J, device=dev)
    ref = dY.double().t() @ X.double()
    out = torch.empty(I, J, device=dev)
    a_img, w_img = rows_img(dY), rows_img(X)
    gemm = lambda: lib.linear_x3t(a_img.data_ptr(), w_img.data_ptr(), M, I, J, zero.data_ptr(), out.data_ptr(), J, st)   # noqa: E731
    gemm()
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    rec = {"shape": name, "rows": M, "I": I, "J": J,
           "x3_err": float((out.double() - ref).abs().max()) / scale,
           "fp32_err": float(((dY.t() @ X).double() - ref).abs().max()) / scale,
           "x3_images_us": timed(lambda: (rows_img(dY), rows_img(X))), "x3_gemm_us": timed(gemm)}
    print(json.dumps(rec), flush=True)
