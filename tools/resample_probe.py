#!/usr/bin/env python
"""GPU box: the polyphase resampler (csrc/resample.inc) by itself and inside the Edinburgh loader.

1. Kernel: 32 rows x 10 s, 48 -> 16 kHz and 44.1 -> 16 kHz, with and without ``sub``.  Warm-up, then groups of back-to-back
   launches between two HIP events; the figure is the median over the groups of (group time / launches).  Achieved bytes/s on
   the algorithmic bytes 4 (n_in (1 or 2) + n_out) per row, against the 6.29 TB/s a float4 copy reaches on this part.
2. Loader: ``EdinburghTtsFiles`` batches per second on a generated 48 kHz tree (batch 16, frame_length 400, window 1024, hop 256),
   against the same batches built the way the loaders did it before: ``read_wav`` + ``scipy.signal.resample_poly`` per file on
   the host (a pool of ``--cpus`` threads), then the same transfer, ragged STFT, crop and label launches.

    python tools/resample_probe.py [--utterances 64 --epochs 3 --cpus 16]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_COPY_TBPS = 6.29


def kernel_times(dev, rows=32, seconds=10, groups=30, per_group=10):
    from onssen_amd.features import _RESAMPLE_WS, resample
    from onssen_amd.hip import get_lib
    lib, out = get_lib(), {}
    stream = torch.cuda.current_stream().cuda_stream
    for rate in (48000, 44100):
        n = rate * seconds
        x = torch.rand(rows, n, device=dev) * 2 - 1
        s = torch.rand(rows, n, device=dev) * 2 - 1
        y, _ = resample(x, rate, 16000)                      # builds the tap image; y is reused as the output buffer
        up, down, _, n_out = lib.resample_geometry(rate, 16000, n)
        ws = _RESAMPLE_WS[(x.device, up, down)]
        lo = torch.empty(rows, dtype=torch.int32, device=dev)
        for sub in (None, s):
            launch = lambda: lib.resample(x.data_ptr(), sub.data_ptr() if sub is not None else None, n, None, rows, n, up, down,
                                          y.data_ptr(), n_out, lo.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream)
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            us = []
            for _ in range(groups):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per_group):
                    launch()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / per_group)
            med = float(np.median(us))
            nbytes = 4 * rows * (n * (2 if sub is not None else 1) + n_out)
            out[f"{rate}->16000{' sub' if sub is not None else ''}"] = {
                "us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "MB": round(nbytes / 1e6, 1),
                "TB_per_s": round(nbytes / med / 1e6, 3), "share_of_copy_rate": round(nbytes / med / 1e6 / HBM_COPY_TBPS, 3),
                "taps_per_output": 2 * (10 * max(up, down)) // up + 1}
    return out


def loader_rates(dev, utterances, epochs, cpus):
    from onssen_amd.data import EdinburghTtsFiles, read_wav, write_wav
    from onssen_amd.data.edinburgh_tts import CLEAN_DIR, NOISY_DIR, _layout
    from onssen_amd.data.wsj0_2mix import _Slot
    from onssen_amd.features import stft_logmag
    from onssen_amd.synthetic import synth_voice
    from scipy.signal import resample_poly
    root = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        for d in (NOISY_DIR, CLEAN_DIR):
            os.makedirs(os.path.join(root, d))
        rng = np.random.default_rng(0)
        base = [synth_voice(900 + i, 48000 * 6, 48000) for i in range(8)]
        names, secs = [], 0.0
        for i in range(utterances):
            n = int(rng.integers(3 * 48000, 6 * 48000))
            clean = 0.5 * base[i % 8][:n] / np.abs(base[i % 8]).max()
            write_wav(os.path.join(root, CLEAN_DIR, f"u{i:04d}.wav"), clean, 48000)
            write_wav(os.path.join(root, NOISY_DIR, f"u{i:04d}.wav"), clean + 0.05 * rng.standard_normal(n), 48000)
            names.append(f"u{i:04d}.wav")
            secs += n / 48000.0
        with open(os.path.join(root, "train"), "w") as f:
            f.write("\n".join(names) + "\n")
        fo = dict(batch_size=16, frame_length=400, sampling_rate=16000, window_size=1024, hop_size=256, db_threshold=40, data_path=root)
        out = {"corpus": f"{utterances} pairs, {secs:.0f} s of audio each side, 16-bit PCM at 48 kHz on tmpfs", "batch": "16 x 400 frames"}
        dl = EdinburghTtsFiles("chimera++", fo, "train", device=dev, seed=0)

        def rate_of(batches):
            for _ in batches():                              # first pass: header cache, pinned buffers, kernels warm
                pass
            torch.cuda.synchronize()
            t0, nb = time.perf_counter(), 0
            for _ in range(epochs):
                for _ in batches():
                    nb += 1
            torch.cuda.synchronize()
            return nb / (time.perf_counter() - t0)
        out["device_route_batches_per_s"] = rate_of(lambda: iter(dl))

        t0, nb = time.perf_counter(), 0                      # its host side alone: header cache + batch reads, no device work
        for _ in range(epochs):
            for _ in dl.host_batches():
                nb += 1
        out["device_route_host_side_batches_per_s"] = nb / (time.perf_counter() - t0)
        items = list(dl.host_batches(ring=[_Slot(True) for _ in range(len(dl))]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()                             # its device side alone, on batches that are already in pinned memory
        for _ in range(epochs):
            for it in items:
                logmag, ri = dl._device_batch(it)
                _layout("chimera++", logmag[:, 0].contiguous(), *(ri[:, i].contiguous() for i in range(3)), 40.0)
        torch.cuda.synchronize()
        out["device_route_device_side_batches_per_s"] = epochs * len(items) / (time.perf_counter() - t0)

        pool = ThreadPoolExecutor(cpus)

        def host_triple(fn):
            (noisy, _), (clean, _) = read_wav(fn), read_wav(dl._sources(fn)[1])
            n = min(len(noisy), len(clean))
            return [resample_poly(v, 1, 3).astype(np.float32) for v in (noisy[:n], clean[:n], noisy[:n] - clean[:n])]

        def host_batches():
            L, hop = fo["frame_length"], fo["hop_size"]
            for i0 in range(0, len(dl.file_list), 16):
                trips = list(pool.map(host_triple, dl.file_list[i0:i0 + 16]))
                n = np.array([len(t[0]) for t in trips])
                host = np.zeros((len(trips), 3, n.max()), np.float32)
                for b, t in enumerate(trips):
                    host[b, :, :n[b]] = np.stack(t)
                wav = torch.from_numpy(host).to(dev)
                logmag, ri = stft_logmag(wav.view(-1, wav.shape[-1]), 1024, hop, lengths=np.repeat(n, 3))
                T, F = logmag.shape[1], logmag.shape[2]
                idx = torch.from_numpy(np.arange(L)[None, :] % (1 + n // hop)[:, None]).to(dev)
                rows, trip = torch.arange(len(trips), device=dev)[:, None, None], torch.arange(3, device=dev)[None, :, None]
                logmag = logmag.view(-1, 3, T, F)[rows, trip, idx[:, None, :]]
                ri = ri.view(-1, 3, T, F, 2)[rows, trip, idx[:, None, :]]
                yield _layout("chimera++", logmag[:, 0].contiguous(), *(ri[:, i].contiguous() for i in range(3)), 40.0)
        out["host_scipy_route_batches_per_s"] = rate_of(host_batches)
        out["host_scipy_route_threads"] = cpus
        out["ratio_device_over_host"] = out["device_route_batches_per_s"] / out["host_scipy_route_batches_per_s"]
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--cpus", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_probe: needs a ROCm device (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    print(json.dumps({"kernel": kernel_times(dev), "loader": loader_rates(dev, args.utterances, args.epochs, args.cpus)}))


if __name__ == "__main__":
    main()
