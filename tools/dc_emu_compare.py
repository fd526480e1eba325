#!/usr/bin/env python
"""The deep-clustering 2-means host code of TWO builds of the emulation library (tests/emu_build.py) on the same seeded calls:
  python tools/dc_emu_compare.py A/libonssen_emu.so B/libonssen_emu.so
One line per call: its return code and the sha256 of what it wrote (masks and the whole workspace, whose header is zeroed and
whose rest is prefilled with 0xA5), of library A and of library B.  Then the four size / offset queries over a sweep of shapes.
Exit status 1 if any line differs.  Used to show that a change of the host side (csrc/dc_run.inc) launches what it launched.

The emulation runs every work-item as an OS thread, and the workgroups of a persistent launch meet only when every workgroup of
the call is a forked process of its own (ONSSEN_EMU_FORK=1): 64 B processes of 256 threads at once, which a host with the usual
32 768 process ids holds up to B = 2.  With the workgroups one after another a Lloyd launch gives up its waits, and what it leaves
then depends on the threads' timing.  So at B = 3 (and B = 33) the calls that complete without a Lloyd launch are compared --
the launch-per-iteration form, the persistent form's compaction with iters = 0, the target map -- and every call with a Lloyd
launch at B = 2 with forked workgroups.  (Two Lloyd launches, B > 32, run on the device only: tools/dc_stream_digests.py.)"""
import ctypes as C
import hashlib
import mmap
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from onssen_amd import _abi          # noqa: E402

PER_IT = _abi.DC_CLUSTER_LAUNCH_PER_ITERATION


def shm(nbytes):
    """'Device' bytes in MAP_SHARED memory (page aligned): visible to the forked workgroups."""
    return np.frombuffer(mmap.mmap(-1, max(int(nbytes), 4096)), dtype=np.uint8, count=int(nbytes))


def f32(a):
    buf = shm(a.size * 4).view(np.float32).reshape(a.shape)
    buf[...] = a
    return buf


def P(a):
    return a.ctypes.data if a is not None else None


def inputs(seed, B, T, F, D):
    rng = np.random.default_rng(seed)
    cents = rng.standard_normal((B, 2, D))
    lab = rng.integers(0, 2, (B, T, F))
    e = np.take_along_axis(cents[:, None, None], lab[..., None, None], axis=3)[..., 0, :] + 0.3 * rng.standard_normal((B, T, F, D))
    e /= np.linalg.norm(e, axis=-1, keepdims=True)
    return f32(e.astype(np.float32)), f32(rng.uniform(-3.0, 1.0, (B, T, F)).astype(np.float32))


def workspace(lib, B, T, F, D, compact):
    nb = (lib.dll.onssen_dc_compact_workspace_bytes if compact else lib.dll.onssen_dc_cluster_workspace_bytes)(B, T, F, D)
    head = lib.dc_compact_layout(B, T, F, D)[1]
    ws = shm(nb)
    ws[:head], ws[head:] = 0, 0xA5
    return ws, nb


def digest(rc, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return f"rc {rc} {h.hexdigest()[:32]}"


def cluster(lib, seed, B, T, F, D, iters, tol, flags, frames=None):
    emb, feat = inputs(seed, B, T, F, D)
    ws, nb = workspace(lib, B, T, F, D, False)
    masks = f32(np.full((B, T, F, 2), np.nan, np.float32))
    if frames is None:
        rc = lib.dll.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, D, 40.0, iters, tol, P(masks), P(ws), nb, flags, None)
    else:
        fr = np.asarray(frames, np.int32)
        rc = lib.dll.onssen_dc_cluster_ragged_f32(P(emb), P(feat), B, T, P(fr), F, D, 40.0, iters, tol, P(masks), P(ws), nb, flags, None)
    return digest(rc, masks.view(np.uint32), ws)


def index(lib, seed, B, T, F, D, frames=None):
    _, feat = inputs(seed, B, T, F, D)
    ws, nb = workspace(lib, B, T, F, D, True)
    fr = None if frames is None else np.asarray(frames, np.int32)
    return digest(lib.dll.onssen_dc_index_f32(P(feat), B, T, P(fr), F, D, 40.0, P(ws), nb, None), ws), ws, nb


def compact(lib, seed, B, T, F, D, iters, tol, frames=None):
    """index -> the compacted array filled with seeded unit rows (every slot: the head GEMM fills the active ones) -> cluster."""
    d1, ws, nb = index(lib, seed, B, T, F, D, frames)
    _, comp_off, _ = lib.dc_compact_layout(B, T, F, D)
    rows = np.random.default_rng(seed + 1).standard_normal((B, T * F, D)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=-1, keepdims=True)
    ws[comp_off:comp_off + rows.nbytes] = rows.view(np.uint8).reshape(-1)
    masks = f32(np.full((B, T, F, 2), np.nan, np.float32))
    rc2 = lib.dll.onssen_dc_cluster_compact_f32(B, T, F, D, iters, tol, P(masks), P(ws), nb, 0, None)
    return d1 + " | " + digest(rc2, masks.view(np.uint32), ws)


def refusals(lib):
    B, T, F, D = 3, 5, 9, 8
    emb, feat = inputs(1, B, T, F, D)
    masks = f32(np.zeros((B, T, F, 2), np.float32))
    fr = np.full(B, T, np.int32)
    ws, nb = workspace(lib, B, T, F, D, True)
    nbc = lib.dll.onssen_dc_cluster_workspace_bytes(B, T, F, D)
    d = lib.dll
    yield "cluster null emb", d.onssen_dc_cluster_f32(None, P(feat), B, T, F, D, 40.0, 3, 1e-4, P(masks), P(ws), nbc, 0, None)
    yield "cluster null ws", d.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, D, 40.0, 3, 1e-4, P(masks), None, nbc, 0, None)
    yield "cluster D=33", d.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, 33, 40.0, 3, 1e-4, P(masks), P(ws), nb, 0, None)
    yield "cluster tol<0", d.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, D, 40.0, 3, -1.0, P(masks), P(ws), nbc, 0, None)
    yield "cluster short ws", d.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, D, 40.0, 3, 1e-4, P(masks), P(ws), nbc - 1, 0, None)
    yield "cluster misaligned ws", d.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, D, 40.0, 3, 1e-4, P(masks), P(ws) + 16, nbc, 0, None)
    yield "cluster misaligned emb", d.onssen_dc_cluster_f32(P(emb) + 4, P(feat), B, T, F, D, 40.0, 3, 1e-4, P(masks), P(ws), nbc, 0, None)
    yield "cluster short AND misaligned", d.onssen_dc_cluster_f32(P(emb), P(feat), B, T, F, D, 40.0, 3, 1e-4, P(masks), P(ws) + 16, 8, 0, None)
    yield "ragged null frames", d.onssen_dc_cluster_ragged_f32(P(emb), P(feat), B, T, None, F, D, 40.0, 3, 1e-4, P(masks), P(ws), nbc, 0, None)
    yield "ragged short ws", d.onssen_dc_cluster_ragged_f32(P(emb), P(feat), B, T, P(fr), F, D, 40.0, 3, 1e-4, P(masks), P(ws), 8, PER_IT, None)
    yield "index null feature", d.onssen_dc_index_f32(None, B, T, None, F, D, 40.0, P(ws), nb, None)
    yield "index D=33", d.onssen_dc_index_f32(P(feat), B, T, None, F, 33, 40.0, P(ws), nb, None)
    yield "index short ws (the clustering's size)", d.onssen_dc_index_f32(P(feat), B, T, None, F, D, 40.0, P(ws), nbc, None)
    yield "index misaligned ws", d.onssen_dc_index_f32(P(feat), B, T, None, F, D, 40.0, P(ws) + 64, nb, None)
    yield "compact null masks", d.onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4, None, P(ws), nb, 0, None)
    yield "compact D=33", d.onssen_dc_cluster_compact_f32(B, T, F, 33, 3, 1e-4, P(masks), P(ws), nb, 0, None)
    yield "compact per-iteration flag", d.onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4, P(masks), P(ws), nb, PER_IT, None)
    yield "compact per-iteration flag AND short ws", d.onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4, P(masks), P(ws), 8, PER_IT, None)
    yield "compact short ws", d.onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4, P(masks), P(ws), nb - 1, 0, None)
    yield "compact misaligned ws", d.onssen_dc_cluster_compact_f32(B, T, F, D, 3, 1e-4, P(masks), P(ws) + 128, nb, 0, None)
    yield "compact iters<0", d.onssen_dc_cluster_compact_f32(B, T, F, D, -1, 1e-4, P(masks), P(ws), nb, 0, None)


def calls(lib):
    """(name, digest) of every call, in a fixed order."""
    B, T, F = 3, 5, 9
    ragged = [5, 1, 3]                               # one row of ONE frame
    os.environ["ONSSEN_EMU_FORK"] = "0"              # workgroups one after another: calls without a Lloyd launch
    for D in (20, 8, 7):
        yield f"dc_index B={B} T={T} F={F} D={D}", index(lib, D, B, T, F, D)[0]
        yield f"dc_index ragged B={B} T={T} F={F} D={D}", index(lib, D, B, T, F, D, ragged)[0]
        for tol in (0.0, 1e-4):
            tag = f"B={B} T={T} F={F} D={D} tol={tol:g}"
            yield f"dc_cluster persistent iters=0 {tag}", cluster(lib, D, B, T, F, D, 0, tol, 0)
            yield f"dc_cluster_ragged persistent iters=0 {tag}", cluster(lib, D, B, T, F, D, 0, tol, 0, ragged)
            for iters in (0, 3):
                yield f"dc_cluster per-iteration iters={iters} {tag}", cluster(lib, D, B, T, F, D, iters, tol, PER_IT)
                yield f"dc_cluster_ragged per-iteration iters={iters} {tag}", cluster(lib, D, B, T, F, D, iters, tol, PER_IT, ragged)
    # more utterances than one Lloyd launch takes (32 under the mock's 256 CUs): with iters = 0 the persistent form launches none
    yield "dc_cluster persistent iters=0 B=33 T=2 F=9 D=20", cluster(lib, 5, 33, 2, 9, 20, 0, 1e-4, 0)
    os.environ["ONSSEN_EMU_FORK"] = "1"              # forked workgroups over shared memory: the persistent launches complete
    lib.dll.onssen_xcd_spin_limit(40000000)          # (emulated workgroups are OS processes: be patient)
    for D in (20, 8, 7):
        for iters in (0, 3):
            for tol in (0.0, 1e-4):
                tag = f"B=2 T={T} F={F} D={D} iters={iters} tol={tol:g} (forked)"
                if iters:
                    yield f"dc_cluster persistent {tag}", cluster(lib, D, 2, T, F, D, iters, tol, 0)
                    yield f"dc_cluster_ragged persistent {tag}", cluster(lib, D, 2, T, F, D, iters, tol, 0, [1, 5])
                yield f"dc_index + dc_cluster_compact {tag}", compact(lib, D, 2, T, F, D, iters, tol)
                yield f"dc_index + dc_cluster_compact ragged {tag}", compact(lib, D, 2, T, F, D, iters, tol, [1, 5])
    os.environ["ONSSEN_EMU_FORK"] = "0"
    for name, rc in refusals(lib):
        yield "refusal: " + name, f"rc {rc}"


def queries(lib):
    """Every value of the four size / offset queries over B, D in 0 .. 34 (and -1) and a few T, F -> (count, sha256)."""
    h, n = hashlib.sha256(), 0
    for B in range(-1, 35):
        for D in range(-1, 35):
            vals = [lib.dll.onssen_dc_cluster_status_offset(B, D)]
            for T, F in ((0, 9), (5, 0), (1, 1), (5, 9), (100, 129), (2000, 129)):
                co, do = C.c_size_t(0xdead), C.c_size_t(0xbeef)
                vals += [lib.dll.onssen_dc_cluster_workspace_bytes(B, T, F, D), lib.dll.onssen_dc_compact_workspace_bytes(B, T, F, D),
                         lib.dll.onssen_dc_compact_layout(B, T, F, D, C.byref(co), C.byref(do)), co.value, do.value,
                         lib.dll.onssen_dc_compact_layout(B, T, F, D, None, None)]
            h.update(repr(vals).encode())
            n += len(vals)
    return n, h.hexdigest()[:32]


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = _abi.Lib(sys.argv[1]), _abi.Lib(sys.argv[2])
    bad = total = 0
    for (name, da), (_, db) in zip(calls(a), calls(b)):
        total += 1
        bad += da != db
        print(f"{'same' if da == db else 'DIFF'}  {name}: {da}" + ("" if da == db else f"  !=  {db}"), flush=True)
    (n, qa), (_, qb) = queries(a), queries(b)
    bad += qa != qb
    print(f"{'same' if qa == qb else 'DIFF'}  {n} query values: {qa}" + ("" if qa == qb else f"  !=  {qb}"))
    print(f"{total} calls and {n} query values compared, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
