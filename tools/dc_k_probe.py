#!/usr/bin/env python
"""GPU box: the deep-clustering back end for 3 and 4 speakers (onssen_dc_cluster_k_f32) next to the two-speaker
launch-per-iteration form and the host (sklearn) route, on 16 utterances x 600 frames x 129 bins x D = 20 of planted clusters.

Per variant: time per dc_masks call (device events, after warm-up, windows of >= 0.5 s, the variants alternating inside one
process, median and spread over the rounds), the Lloyd iterations run, the bytes one iteration streams (B T F (D + 1) 4), and
the time of ONE iteration = (time at iters = 2 - time at iters = 0) / 2 -- with tol = 0 both iterations do full work on these
inputs (the fixed point is found at the end of the second or third)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from onssen_amd.hip import get_lib
from onssen_amd.separation import _host_label_masks, dc_masks
from tests.dc_kmeans_ref import planted

dev = torch.device("cuda:0")
lib = get_lib()
B, T, F, D = (int(os.environ.get(k, v)) for k, v in (("B", 16), ("T", 600), ("F", 129), ("D", 20)))
ROUNDS, WINDOW = 5, 0.5
stream_bytes = B * T * F * (D + 1) * 4

data = {}
for K in (2, 3, 4):
    emb, feat, _ = planted(K, B, T, F, D, K)
    data[K] = (torch.from_numpy(emb).to(dev), torch.from_numpy(feat).to(dev))


def iterations(K):
    """Lloyd iterations per utterance of the K-form at the defaults (iters = 20, tol = 1e-4), read from its workspace."""
    e, f = data[K]
    nb = int(lib.dll.onssen_dc_cluster_k_workspace_bytes(B, T, F, D, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    m = torch.empty(B, T, F, K, device=dev)
    lib.dc_cluster_k(e.data_ptr(), f.data_ptr(), B, T, F, D, K, 40.0, 20, m.data_ptr(), ws.data_ptr(), nb,
                     torch.cuda.current_stream().cuda_stream, tol=1e-4)
    torch.cuda.synchronize()
    info = ws[:16 * B].view(torch.int32).view(B, 4).cpu().numpy()
    return sorted(set(info[:, 0].tolist())), int(info[:, 1].sum())


def call(K, iters, tol):
    os.environ["ONSSEN_DC_PERSISTENT"] = "0"          # K = 2: the existing launch-per-iteration form (K > 2 has no other)
    return dc_masks(*data[K], iters=iters, tol=tol, num_speaker=K)


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


variants = [(f"K={K} {name}", (lambda K=K, it=it, tol=tol: call(K, it, tol)))
            for K in (3, 4, 2) for name, it, tol in (("default (iters=20, tol=1e-4)", 20, 1e-4), ("iters=0", 0, 0.0), ("iters=2 tol=0", 2, 0.0))]
with torch.no_grad():
    for _, fn in variants:                               # warm-up: allocations, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for r in range(ROUNDS):                              # the variants alternate: drift hits all of them alike
        for name, fn in variants:
            times[name].append(window(fn))
    print(f"workload: B={B} T={T} F={F} D={D}; one iteration streams {stream_bytes / 1e6:.1f} MB; {ROUNDS} rounds of >= {WINDOW} s per variant")
    med = {}
    for name, _ in variants:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        print(f"  {name:36s} median {np.median(t) * 1e3:8.1f} us  (min {t.min() * 1e3:.1f}, max {t.max() * 1e3:.1f})")
    for K in (3, 4, 2):
        per = (med[f"K={K} iters=2 tol=0"] - med[f"K={K} iters=0"]) / 2
        spread = max(np.ptp(times[f"K={K} iters=2 tol=0"]), np.ptp(times[f"K={K} iters=0"])) / 2
        its, conv = iterations(K)
        print(f"  K={K}: one iteration {per * 1e3:.1f} us (+- {spread * 1e3:.1f}) = {stream_bytes / per / 1e9:.2f} TB/s of the streamed bytes; "
              f"iterations run at the defaults (K-form): {its}, converged {conv}/{B}"
              + (" [the 2-means form does not record its count; same rule]" if K == 2 else ""))
    # the host route at K = 3 (separate_dc(host_kmeans=True) after the network): embedding to the host, sklearn per utterance, masks back
    from sklearn.cluster import KMeans
    e, f = data[3]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    masks = torch.zeros(B, T, F, 3, device=dev)
    n_it = []
    for b in range(B):
        act = f[b] >= (f[b].max() - 40.0 / 20.0)
        km = KMeans(n_clusters=3, random_state=0, n_init=10).fit(e[b][act].cpu().numpy())
        n_it.append(int(km.n_iter_))
        masks[b][act] = _host_label_masks(km.labels_, 3, dev)
    torch.cuda.synchronize()
    host = time.perf_counter() - t0
    print(f"  host_kmeans (sklearn, n_init=10) K=3: {host * 1e3:.0f} ms per call (one call, wall clock), iterations of the best run {sorted(set(n_it))}; "
          f"device K=3 default is {host / (med['K=3 default (iters=20, tol=1e-4)'] * 1e-3):.0f} x faster")
