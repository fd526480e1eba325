#!/usr/bin/env python
"""Timing of the ConvTasNet forward on one GPU: the HIP forward (graph replay, warmed up, median of >= 20 device-event timed
replays) against the same module's ATen forward with the same weights, for each precision, at the recipe shape (3 x 32 000)
and a throughput shape (32 x 32 000).  One JSON line per shape: ms per forward, x real time, the ATen / HIP ratio, the
algorithmic GFLOP and bytes, and the max error of the timed step against tests/tasnet_ref.py (the recipe shape; the throughput
shape is checked on its first 2 utterances).  Usage: python tools/tasnet_bench.py [--reps 20] [--out FILE]

--train: the training leg.  One step = forward + si_snr_loss + backward + clip + Adam through dist.train_step, at 3 x 32 000
(recipe) and 16 x 32 000, ``tasnet_train`` hip against aten in the same process on the same card, interleaved step by step,
warmed up, median and min-max of --reps device-event timed steps each, plus forward-only (network + loss) and backward-only
splits.  One JSON line per shape (default --out with --train: profiles/tasnet_train_bench.jsonl).
--train-profile N: N HIP training steps at the recipe shape and nothing else -- the run to put under
``rocprofv3 --kernel-trace --stats`` (a run of its own: profiling perturbs the timing).  --loss-route aten|hip picks the
route of ``loss.si_snr_loss`` (option ``tasnet_loss``) for that run.
--train-loss: the loss route as a leg of the training step.  The network on HIP (``tasnet_train`` hip) in both legs,
``tasnet_loss`` aten against hip, same protocol and columns as --train (interleaved step by step in one process, --warmup then
--reps device-event timed steps, median and min-max; step, forward + loss, backward), at 3 x 32 000 and 16 x 32 000.  The aten
leg is the default route and the yardstick.  One JSON line per shape, APPENDED to profiles/tasnet_train_bench.jsonl.

--ragged K[,K...]: whole-utterance evaluation.  64 utterances with seeded lengths uniform in 2 s .. 10 s at 8 kHz, recipe model,
one pass = the eager forwards of all 64: (a) one utterance per forward (the batch-1 loop), (b) ``forward(..., lengths=)`` with K
utterances per forward, for every K given (at most ConvTasNet.RAGGED_MAX) and every read-ahead factor of --buckets (G = 1: the
utterances as they come; G > 1: G K read ahead and sorted by length, as tester.eval does).  The batches are collated before the
clock starts; the legs are interleaved pass by pass in one process, warmed up, --reps device-event timed passes each.  One JSON
line per leg: ms per utterance, median / min / max (default --out: profiles/tasnet_ragged_bench.jsonl).  The first pass also
checks every ragged leg's estimates against the batch-1 leg's, bit for bit.
--ragged-profile K: 3 passes of the K-per-forward leg and nothing else (the run for ``rocprofv3 --kernel-trace --stats``).

--stream: streaming inference (``ConvTasNet.stream``).  The recipe with causal=True, norm="cln"; n in {1, 16, 64} streams x
F in {1, 8, 40} hops per step.  Legs, interleaved pass by pass in one process, --warmup passes then --reps device-event timed
ones, median (min - max): the eager ``push``, the graph-replayed ``push``, and the only thing a causal model could do before
there was a stream -- the (graph-replayed) offline forward over a window of receptive field + F frames per stream, of which the
last F are kept.  One JSON line per (n, F), then one line per n with the smallest measured F whose median graph-replayed step
stays under the chunk's own duration F hop / 8000 s (default --out: profiles/tasnet_stream_bench.jsonl).  Before timing, the
first pushes are checked bit for bit against the offline forward.

--long: long-form separation (``separation.separate_tasnet_long``).  The recipe model (gLN, non-causal); 60 s and 600 s of 8 kHz
audio, window = 32 000, step = 16 000, --long-batch windows per forward.  Legs, interleaved pass by pass in one process, --warmup
passes then --reps device-event timed ones, median (min - max): (a) ``separate_tasnet_long``; (b) the only thing there was before,
one whole-signal ``forward([x])`` (if it runs out of memory, the line says so instead); and, on buffers of the same call, the gather
launch alone and the stitch call alone (similarity + permutation + stitch launches), whose sum over (a) is the stitching share.
One JSON line per duration with ms per second of audio (default --out: profiles/tasnet_long_bench.jsonl).
--long-profile SECONDS: 3 calls of ``separate_tasnet_long`` on SECONDS of audio and nothing else (the run for
``rocprofv3 --kernel-trace --stats``, which splits the share by kernel)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from onssen_amd import nn as onn          # noqa: E402
from tests import tasnet_ref             # noqa: E402


def gflop_bytes(c, n, S):
    """Algorithmic work of one forward (2 flop per multiply-add) and the fp32 bytes its unfused stages move."""
    T = (S - c["L"]) // (c["L"] // 2) + 1
    N, B, H, P, blocks, spk, L = c["N"], c["B"], c["H"], c["P"], c["R"] * c["X"], c["num_spks"], c["L"]
    per_frame = N * L + N * B + blocks * (B * H + H * P + H * B) + B * spk * N + spk * N * L
    rows = n * T
    byts = 4 * rows * (2 * N + B + blocks * (B + 4 * H + 3 * B) + spk * N * 2 + spk * N) + 4 * n * S
    return 2.0 * per_frame * rows / 1e9, float(byts)


def time_graph(fn, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    for _ in range(3):
        g.replay()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def time_eager(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def _stats(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3), "max_ms": round(float(np.max(ts)), 3)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def train_leg(a):
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    dev = torch.device("cuda:0")
    c = dict(tasnet_ref.RECIPE, activate="sigmoid")          # the shipped recipe's activation
    sd = tasnet_ref.make_state(c, seed=11)
    paths = ("hip", "aten")

    def fresh():
        m = onn.ConvTasNet(**c)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).train()
        return m, build_optimizer(m.parameters(), {"name": "adam", "lr": 1e-3})

    if a.train_profile:
        os.environ["ONSSEN_TASNET_TRAIN"] = "hip"
        os.environ["ONSSEN_TASNET_LOSS"] = a.loss_route
        n, S = 3, 32000
        rng = np.random.default_rng(5)
        xd = torch.from_numpy((0.1 * rng.standard_normal((n, S))).astype(np.float32)).to(dev)
        refs = [torch.from_numpy((0.1 * rng.standard_normal((n, S))).astype(np.float32)).to(dev) for _ in range(c["num_spks"])]
        m, opt = fresh()
        for _ in range(a.train_profile):
            dist.train_step(m, opt, L.si_snr_loss, [xd], refs)
        torch.cuda.synchronize()
        return
    lines = []
    for shp in a.shapes.split(","):
        n, S = (int(v) for v in shp.split("x"))
        rng = np.random.default_rng(5)
        xd = torch.from_numpy((0.1 * rng.standard_normal((n, S))).astype(np.float32)).to(dev)
        refs = [torch.from_numpy((0.1 * rng.standard_normal((n, S))).astype(np.float32)).to(dev) for _ in range(c["num_spks"])]
        pair = {p: fresh() for p in paths}
        step, fwd, bwd, loss0 = {p: [] for p in paths}, {p: [] for p in paths}, {p: [] for p in paths}, {}
        for it in range(a.warmup + a.reps):                   # interleaved: hip, aten, hip, aten, ...
            for p in paths:
                os.environ["ONSSEN_TASNET_TRAIN"] = p
                m, opt = pair[p]
                ms, val = _timed(lambda: dist.train_step(m, opt, L.si_snr_loss, [xd], refs))
                assert m.last_train_path == p
                loss0.setdefault(p, val)
                if it >= a.warmup:
                    step[p].append(ms)
        for it in range(a.warmup + a.reps):                   # the splits, on the weights the steps left
            for p in paths:
                os.environ["ONSSEN_TASNET_TRAIN"] = p
                m, opt = pair[p]
                m.zero_grad(set_to_none=True)
                ms_f, loss = _timed(lambda: L.si_snr_loss(m([xd]), refs))
                ms_b, _ = _timed(loss.backward)
                del loss
                if it >= a.warmup:
                    fwd[p].append(ms_f)
                    bwd[p].append(ms_b)
        os.environ.pop("ONSSEN_TASNET_TRAIN", None)
        rec = {"shape": [n, S], "reps": a.reps, "warmup": a.warmup, "audio_s": n * S / 8000.0}
        for p in paths:
            rec[p] = {"step": _stats(step[p]), "forward_and_loss": _stats(fwd[p]), "backward": _stats(bwd[p]), "first_loss": loss0[p]}
        rec["aten_over_hip_step"] = round(rec["aten"]["step"]["median_ms"] / rec["hip"]["step"]["median_ms"], 2)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del pair
        torch.cuda.empty_cache()
    out = a.out or os.path.join(ROOT, "profiles", "tasnet_train_bench.jsonl")
    with open(out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


def train_loss_leg(a):
    """The loss route (option ``tasnet_loss``) as a leg of the HIP training step: see the module docstring."""
    from onssen_amd import dist, loss as L
    from onssen_amd.utils import build_optimizer
    dev = torch.device("cuda:0")
    c = dict(tasnet_ref.RECIPE, activate="sigmoid")
    sd = tasnet_ref.make_state(c, seed=11)
    routes = ("aten", "hip")
    os.environ["ONSSEN_TASNET_TRAIN"] = "hip"

    def fresh():
        m = onn.ConvTasNet(**c)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m = m.to(dev).train()
        return m, build_optimizer(m.parameters(), {"name": "adam", "lr": 1e-3})

    lines = []
    for shp in a.shapes.split(","):
        n, S = (int(v) for v in shp.split("x"))
        rng = np.random.default_rng(5)
        src = (0.1 * rng.standard_normal((c["num_spks"], n, S))).astype(np.float32)      # a training batch: mixture = sum of sources
        xd = torch.from_numpy(src.sum(axis=0)).to(dev)
        refs = [torch.from_numpy(r).to(dev) for r in src]
        pair = {r: fresh() for r in routes}
        step, fwd, bwd, loss0 = {r: [] for r in routes}, {r: [] for r in routes}, {r: [] for r in routes}, {}
        for it in range(a.warmup + a.reps):                   # interleaved: aten, hip, aten, hip, ...
            for r in routes:
                os.environ["ONSSEN_TASNET_LOSS"] = r
                m, opt = pair[r]
                ms, val = _timed(lambda: dist.train_step(m, opt, L.si_snr_loss, [xd], refs))
                assert m.last_train_path == "hip" and L.last_si_snr_path == r
                loss0.setdefault(r, val)
                if it >= a.warmup:
                    step[r].append(ms)
        for it in range(a.warmup + a.reps):                   # the splits, on the weights the steps left
            for r in routes:
                os.environ["ONSSEN_TASNET_LOSS"] = r
                m, opt = pair[r]
                m.zero_grad(set_to_none=True)
                ms_f, loss = _timed(lambda: L.si_snr_loss(m([xd]), refs))
                ms_b, _ = _timed(loss.backward)
                del loss
                if it >= a.warmup:
                    fwd[r].append(ms_f)
                    bwd[r].append(ms_b)
        rec = {"leg": "loss_route", "shape": [n, S], "reps": a.reps, "warmup": a.warmup, "audio_s": n * S / 8000.0}
        for r in routes:
            rec["loss_" + r] = {"step": _stats(step[r]), "forward_and_loss": _stats(fwd[r]), "backward": _stats(bwd[r]),
                                "first_loss": loss0[r]}
        at, hp = rec["loss_aten"]["step"], rec["loss_hip"]["step"]
        rec["aten_over_hip_step"] = round(at["median_ms"] / hp["median_ms"], 3)
        # is the difference of the medians outside the spread of both legs?
        rec["outside_both_spreads"] = bool(hp["max_ms"] < at["min_ms"] or at["max_ms"] < hp["min_ms"])
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del pair
        torch.cuda.empty_cache()
    for k in ("ONSSEN_TASNET_TRAIN", "ONSSEN_TASNET_LOSS"):
        os.environ.pop(k, None)
    out = a.out or os.path.join(ROOT, "profiles", "tasnet_train_bench.jsonl")
    with open(out, "a") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


def ragged_lengths(count=64, seed=7, lo=16000, hi=80000):
    return [int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, count)]


def ragged_batches(waves, K, G):
    """Lists of indices, K per forward; G > 1: G K read ahead, longest first (tester._forwards)."""
    out = []
    for at in range(0, len(waves), K * G):
        idx = list(range(at, min(at + K * G, len(waves))))
        if G > 1:
            idx.sort(key=lambda i: -waves[i].shape[0])
        out += [idx[j:j + K] for j in range(0, len(idx), K)]
    return out


def ragged_leg(a):
    from torch.nn.utils.rnn import pad_sequence
    dev = torch.device("cuda:0")
    c = tasnet_ref.RECIPE
    sd = tasnet_ref.make_state(c, seed=11)
    m = onn.ConvTasNet(**c)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    lens = ragged_lengths()
    rng = np.random.default_rng(8)
    waves = [torch.from_numpy((0.1 * rng.standard_normal(s)).astype(np.float32)).to(dev) for s in lens]

    def leg_ragged(K, G):
        plan = [(pad_sequence([waves[i] for i in idx], batch_first=True), [lens[i] for i in idx], idx)
                for idx in ragged_batches(waves, K, G)]

        def run(keep=None):
            for x, ln, idx in plan:
                est = m([x], lengths=ln)
                if keep is not None:
                    for b, i in enumerate(idx):
                        keep[i] = torch.stack([e[b] for e in est])
        return run

    def leg_one(keep=None):
        for i, w in enumerate(waves):
            est = m([w])
            if keep is not None:
                keep[i] = torch.stack(list(est))

    if a.ragged_profile:
        run = leg_ragged(a.ragged_profile, 1)
        with torch.no_grad():
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        return
    Ks = [int(v) for v in a.ragged.split(",")]
    Gs = [int(v) for v in a.buckets.split(",")]
    legs = {"batch1": leg_one}
    for K in Ks:
        for G in Gs:
            legs[f"ragged_K{K}_G{G}"] = leg_ragged(K, G)
    ts = {name: [] for name in legs}
    with torch.no_grad():
        base = {}
        leg_one(base)
        for name, run in legs.items():                       # same bits as the batch-1 loop, checked before anything is timed
            if name == "batch1":
                continue
            got = {}
            run(got)
            for i, e in base.items():
                assert torch.equal(got[i][:, :e.shape[1]], e), f"{name}: utterance {i} differs from its one-utterance forward"
        del base, got
        for it in range(a.warmup + a.reps):                   # interleaved: every leg once per round
            for name, run in legs.items():
                ms, _ = _timed(run)
                if it >= a.warmup:
                    ts[name].append(ms / len(waves))
    lines = []
    for name in legs:
        rec = {"leg": name, "utterances": len(waves), "audio_s": sum(lens) / 8000.0, "reps": a.reps, "warmup": a.warmup,
               "precision": os.environ.get("ONSSEN_PRECISION", "bf16x3"), "ms_per_utterance": _stats(ts[name])}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    out = a.out or os.path.join(ROOT, "profiles", "tasnet_ragged_bench.jsonl")
    with open(out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


def _graph(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def stream_leg(a):
    dev = torch.device("cuda:0")
    c = dict(tasnet_ref.RECIPE, causal=True, norm="cln")
    sd = tasnet_ref.make_state(c, seed=11)
    m = onn.ConvTasNet(**c)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    hop, rate = c["L"] // 2, 8000.0
    field = 1 + c["R"] * (c["P"] - 1) * (2 ** c["X"] - 1)          # frames one output frame depends on
    lines, keeps_up = [], {}
    with torch.no_grad():
        x = torch.from_numpy((0.1 * np.random.default_rng(5).standard_normal((2, 400 * hop))).astype(np.float32)).to(dev)
        st = m.stream(2)
        got = torch.cat([torch.stack(st.push(x[:, i * 40 * hop:(i + 1) * 40 * hop])) for i in range(10)] + [torch.stack(st.flush())], -1)
        assert torch.equal(got[..., hop:], torch.stack(list(m([x])))), "the stream differs from the offline forward"
        for n in (1, 16, 64):
            for F in (1, 8, 40):
                chunk = torch.from_numpy((0.1 * np.random.default_rng(n + F).standard_normal((n, F * hop))).astype(np.float32)).to(dev)
                window = torch.from_numpy((0.1 * np.random.default_rng(F).standard_normal((n, (field + F - 1) * hop + c["L"])))
                                          .astype(np.float32)).to(dev)
                eager, graphed = m.stream(n), m.stream(n)
                eager.reset()
                graphed.reset()
                g_step, _ = _graph(lambda: graphed.push(chunk))
                g_base, _ = _graph(lambda: m([window]))
                legs = {"stream_eager": lambda: eager.push(chunk), "stream_graph": g_step.replay, "window_forward_graph": g_base.replay}
                ts = {k: [] for k in legs}
                for it in range(a.warmup + a.reps):
                    for k, fn in legs.items():
                        ms, _ = _timed(fn)
                        if it >= a.warmup:
                            ts[k].append(ms)
                rec = {"n": n, "F": F, "chunk_ms": round(1e3 * F * hop / rate, 3), "window_frames": field + F, "reps": a.reps,
                       "warmup": a.warmup, "precision": os.environ.get("ONSSEN_PRECISION", "bf16x3")}
                rec.update({k: _stats(v) for k, v in ts.items()})
                rec["window_over_stream"] = round(rec["window_forward_graph"]["median_ms"] / rec["stream_graph"]["median_ms"], 2)
                rec["ranges_apart"] = rec["stream_graph"]["max_ms"] < rec["window_forward_graph"]["min_ms"]
                rec["real_time"] = rec["stream_graph"]["median_ms"] < rec["chunk_ms"]
                if rec["real_time"]:
                    keeps_up.setdefault(n, F)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del g_step, g_base, eager, graphed
                torch.cuda.empty_cache()
    for n in (1, 16, 64):
        rec = {"n": n, "smallest_measured_F_in_real_time": keeps_up.get(n)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    out = a.out or os.path.join(ROOT, "profiles", "tasnet_stream_bench.jsonl")
    with open(out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


def long_leg(a):
    from onssen_amd.hip import get_lib
    from onssen_amd.separation import separate_tasnet_long, tasnet_long_geometry
    dev = torch.device("cuda:0")
    c = tasnet_ref.RECIPE
    sd = tasnet_ref.make_state(c, seed=11)
    m = onn.ConvTasNet(**c)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    rate, W, step, spk = 8000, 32000, 16000, c["num_spks"]
    lib = get_lib()

    def signal(seconds):
        return torch.from_numpy((0.1 * np.random.default_rng(seconds).standard_normal(seconds * rate)).astype(np.float32)).to(dev)

    if a.long_profile:
        x = signal(a.long_profile)
        with torch.no_grad():
            for _ in range(3):
                separate_tasnet_long(m, x, W, step, batch=a.long_batch)
        torch.cuda.synchronize()
        return
    lines = []
    with torch.no_grad():
        for seconds in (60, 600):
            x = signal(seconds)
            S_out, K, v_last = tasnet_long_geometry(c["L"], x.shape[0], W, step)
            out, est, perm = separate_tasnet_long(m, x, W, step, batch=a.long_batch, return_windows=True)
            assert out.shape == (spk, S_out) and bool(torch.isfinite(out).all())
            assert bool((perm.sort(dim=1).values == torch.arange(spk, device=dev, dtype=torch.int32)).all())
            win = torch.empty(K, W, device=dev)
            nb = lib.tasnet_stitch_workspace_bytes(spk, K, W, step, v_last)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            st = torch.cuda.current_stream().cuda_stream
            legs = {"long": lambda: separate_tasnet_long(m, x, W, step, batch=a.long_batch),
                    "whole_forward": lambda: m([x]),
                    "gather": lambda: lib.tasnet_windows(x.data_ptr(), S_out, K, W, step, win.data_ptr(), st),
                    "stitch": lambda: lib.tasnet_stitch(est.data_ptr(), spk, K, W, step, v_last, out.data_ptr(), perm.data_ptr(),
                                                        ws.data_ptr(), nb, st)}
            rec = {"audio_s": seconds, "window": W, "step": step, "windows": K, "batch": a.long_batch, "reps": a.reps,
                   "warmup": a.warmup, "precision": os.environ.get("ONSSEN_PRECISION", "bf16x3")}
            try:
                legs["whole_forward"]()
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError as e:
                rec["whole_forward"] = "out of memory: " + str(e).splitlines()[0]
                del legs["whole_forward"]
                torch.cuda.empty_cache()
            ts = {k: [] for k in legs}
            for it in range(a.warmup + a.reps):
                for k, fn in legs.items():
                    ms, _ = _timed(fn)
                    if it >= a.warmup:
                        ts[k].append(ms)
            for k, v in ts.items():
                rec[k] = _stats(v)
                rec[k]["ms_per_audio_s"] = round(rec[k]["median_ms"] / seconds, 4)
            rec["stitching_share"] = round((rec["gather"]["median_ms"] + rec["stitch"]["median_ms"]) / rec["long"]["median_ms"], 5)
            if "whole_forward" in ts:
                rec["long_over_whole"] = round(rec["long"]["median_ms"] / rec["whole_forward"]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del x, out, est, perm, win, ws, legs
            m._ws.cache.clear()
            torch.cuda.empty_cache()
    out_path = a.out or os.path.join(ROOT, "profiles", "tasnet_long_bench.jsonl")
    with open(out_path, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--long-batch", type=int, default=16)
    ap.add_argument("--long-profile", type=int, default=0, metavar="SECONDS")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--ragged", default=None, metavar="K[,K...]")
    ap.add_argument("--buckets", default="1,4")
    ap.add_argument("--ragged-profile", type=int, default=0, metavar="K")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--train-profile", type=int, default=0)
    ap.add_argument("--train-loss", action="store_true")
    ap.add_argument("--loss-route", default="aten", choices=("aten", "hip"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None)
    a = ap.parse_args()
    if a.long or a.long_profile:
        return long_leg(a)
    if a.stream:
        return stream_leg(a)
    if a.ragged or a.ragged_profile:
        return ragged_leg(a)
    if a.train_loss:
        a.shapes = a.shapes or "3x32000,16x32000"
        return train_loss_leg(a)
    if a.train or a.train_profile:
        a.shapes = a.shapes or "3x32000,16x32000"
        return train_leg(a)
    a.shapes = a.shapes or "3x32000,32x32000"
    dev = torch.device("cuda:0")
    c = tasnet_ref.RECIPE
    sd = tasnet_ref.make_state(c, seed=11)
    m = onn.ConvTasNet(**c)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    lines = []
    for shp in a.shapes.split(","):
        n, S = (int(v) for v in shp.split("x"))
        x = (0.1 * np.random.default_rng(5).standard_normal((n, S))).astype(np.float32)
        xd = torch.from_numpy(x).to(dev)
        ref = np.stack(tasnet_ref.forward(sd, x[:min(n, 3)], c))
        gf, byts = gflop_bytes(c, n, S)
        rec = {"shape": [n, S], "gflop": round(gf, 2), "bytes_unfused": byts, "audio_s": n * S / 8000.0}
        with torch.no_grad():
            ms_aten, out_aten = time_eager(lambda: m._autograd_forward(xd), max(5, a.reps // 4))
            oa = np.stack([o.cpu().numpy() for o in out_aten])[:, :min(n, 3)]
            rec["aten_ms"] = round(ms_aten, 3)
            rec["aten_err"] = float(np.abs(oa - ref).max())
            for prec in ("f32", "bf16x3", "bf16"):
                os.environ["ONSSEN_PRECISION"] = prec
                ms, out = time_graph(lambda: m([xd]), a.reps)
                o = np.stack([t.cpu().numpy() for t in out])[:, :min(n, 3)]
                rec[prec] = {"ms": round(ms, 3), "x_realtime": round(rec["audio_s"] / (ms / 1e3), 1),
                             "aten_over_hip": round(ms_aten / ms, 2), "tflops": round(gf / ms, 2),
                             "max_err": float(np.abs(o - ref).max())}
        os.environ.pop("ONSSEN_PRECISION", None)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
