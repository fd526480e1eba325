#!/usr/bin/env python
"""Same-box A/B of the pipelined deep-clustering step with the target map built inside the pair launch (DCPipeline(aux_map=True),
onssen_blstm_pipe2_map_forward_f32) against the three kmeans2_* launches in front of it (aux_map=False, the sequence before).

One process, one GPU, the headline workload of bench.py (dc_l2, 32 rows).  After 0.3 s of pre-heat: ROUNDS rounds of REPS hipGraph
replays of one form, then REPS of the other, device events around each block -> ms per step per round.  Then the pair launch ALONE
(ONSSEN_BLSTM_G_READY), old entry against new, eager: what the aux workgroups cost beside the recurrence.

  python tools/pipe2_aux_ab.py [--rounds 7] [--reps 200] [--out FILE]      (prints the table; --out also writes it)"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from onssen_amd import _abi
    from onssen_amd.nn._core import _XcdPolicy, _XcdStatus
    from onssen_amd.separation import DCPipeline
    dev = torch.device("cuda", 0)
    wl = bench.build_workload("dc_l2", 32, dev)
    model, wav, hop, n, nfft = wl["model"], wl["wav"], wl["HOP"], wl["N"], wl["NFFT"]
    B = wav.shape[0]
    pipes = {"old": DCPipeline(model, B, n, nfft, hop, graph=True, aux_map=False), "new": DCPipeline(model, B, n, nfft, hop, graph=True, aux_map=True)}
    with torch.no_grad():
        for p in pipes.values():
            for _ in range(3):
                p.push(wav, check=False)
            p.replay()
    torch.cuda.synchronize()
    # both forms on the same input: the same maps, masks and waveforms; of the headers and int words, which columns differ (the Lloyd
    # kernel's placement words [67], [68] and its flag in [66] depend on where the dispatcher put its parts, nothing else may)
    o, w = pipes["old"], pipes["new"]
    stride, nmap = 1 + 2 * o.D + 64 * 2 * (o.D + 1) + 1, 4 * B * o.T * o.F
    iw_off = -(-B * stride * 4 // 256) * 256
    same = all(torch.equal(o.cws[q][o.dest_off:o.dest_off + nmap], w.cws[q][w.dest_off:w.dest_off + nmap]) for q in (0, 1))
    same = same and torch.equal(o.masks, w.masks) and all(torch.equal(o.out[q], w.out[q]) for q in (0, 1))
    cols = lambda a, b, lo, n, width: sorted(set(((a[lo:lo + n].view(torch.int32) != b[lo:lo + n].view(torch.int32)).nonzero().flatten() % width).tolist()))
    hdr = [cols(o.cws[q], w.cws[q], 0, 4 * B * stride, stride) for q in (0, 1)]
    iwd = [cols(o.cws[q], w.cws[q], iw_off, 4 * B * 72, 72) for q in (0, 1)]
    lines = [f"# maps, masks and waveforms of the two forms equal: {same}; differing header columns {hdr}, int-word columns {iwd}",f"# pipelined step, dc_l2 {B} x {pipes['new'].T} frames, hipGraph replays, {args.reps} per block, ms per step",
             "round  old(3 launches in front)  new(aux workgroups)"]
    t0 = time.time()
    while time.time() - t0 < 0.3:
        for p in pipes.values():
            timed(p.replay, 20)
    step = {"old": [], "new": []}
    for r in range(args.rounds):
        for k in ("old", "new"):
            step[k].append(timed(pipes[k].replay, args.reps))
        lines.append(f"{r:5d}  {step['old'][-1]:.4f}  {step['new'][-1]:.4f}")
    lines.append(f"range  old {min(step['old']):.4f}-{max(step['old']):.4f}  new {min(step['new']):.4f}-{max(step['new']):.4f}  "
                 f"every new round below every old round: {max(step['new']) < min(step['old'])}")

    # the pair launch by itself on the projections the steps above left: old entry / new entry (which still builds the map)
    pipe = pipes["new"]
    lib, T, F, pk = pipe.lib, pipe.T, pipe.F, model._packed.get(pipe.ug)
    weights = [t.data_ptr() for t in pk.wih_img], [t.data_ptr() for t in pk.whh_x3], [t.data_ptr() for t in pk.bias]
    st = torch.cuda.current_stream().cuda_stream
    flags = pipe.flags | _abi.BLSTM_G_READY
    pair = {"old": lambda: lib.blstm_pipe2_forward(pipe.logmag[0].data_ptr(), T * F, F, B, T, F, pipe.H, pipe.ug, *weights, pipe.ws.data_ptr(), pipe.wnb,
                                                   flags, st),
            "new": lambda: lib.blstm_pipe2_map_forward(pipe.logmag[0].data_ptr(), T * F, F, B, T, F, pipe.H, pipe.ug, *weights, pipe.ws.data_ptr(),
                                                       pipe.wnb, flags, pipe.db, pipe.D, pipe.cws[0].data_ptr(), pipe.cnb, st)}
    lines += ["# pair launch alone (ONSSEN_BLSTM_G_READY), eager, 50 per block, ms per launch", "round  old entry  new entry (+ map)"]
    alone = {"old": [], "new": []}
    for k in pair:
        timed(pair[k], 10)
    for r in range(args.rounds):
        for k in ("old", "new"):
            alone[k].append(timed(pair[k], 50))
        lines.append(f"{r:5d}  {alone['old'][-1]:.4f}  {alone['new'][-1]:.4f}")
    med = lambda v: sorted(v)[len(v) // 2]
    lines.append(f"range  old {min(alone['old']):.4f}-{max(alone['old']):.4f}  new {min(alone['new']):.4f}-{max(alone['new']):.4f}  "
                 f"median difference new - old: {1e3 * (med(alone['new']) - med(alone['old'])):+.1f} us")
    _XcdStatus.poll(wait=True)
    lines.append(f"aborted launches: {_XcdPolicy.aborts}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
