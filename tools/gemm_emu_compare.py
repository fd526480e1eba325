#!/usr/bin/env python
"""The GEMM host code of TWO builds of the emulation library (tests/emu_build.py) on the same seeded calls:
  python tools/gemm_emu_compare.py A/libonssen_emu.so B/libonssen_emu.so [--quick]
One line per call: its return code and the sha256 of everything the call may write (outputs prefilled with NaN, images with
0xA5 bytes, so that a tile nobody wrote or a store past the matrix shows), of library A and of library B.  Then every refusal of
every entry (tools.gemm_emu_compare.refusals: tests/test_emu_gemm_refusals.py holds their codes).  Exit status 1 if any line
differs.  Used to show that a change of the host side (csrc/gemm_run.inc) launches what it launched: every entry, every epilogue,
both term counts, vector and scalar loads / stores, the four environment switches crossed, and both sides of the pair / compact
entries' half-height switch (257 half-height tiles: minutes on the emulation, left out with --quick).

GEMM workgroups do not meet, so they run one after another (no forked workgroups)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from onssen_amd import _abi          # noqa: E402

BIAS, L2N, SIG, RELU, BF16 = _abi.EPI_BIAS, _abi.EPI_L2NORM, _abi.EPI_SIGMOID, _abi.EPI_RELU, _abi.EPI_BF16
SWITCHES = ("ONSSEN_X3Q", "ONSSEN_X3Q_BM", "ONSSEN_X3R", "ONSSEN_X3Q_SMALL")


def P(a):
    return a.ctypes.data if a is not None else None


def env(q=None, bm=None, r=None, small=None):
    """Set (or unset: None) the four switches; the library reads them on every call."""
    for k, v in zip(SWITCHES, (q, bm, r, small)):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)


def rand(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def nans(*shape, offset=0):
    """A NaN-filled float32 array whose data starts `offset` floats past a 16-byte boundary."""
    raw = np.full(int(np.prod(shape)) + 8, np.nan, np.float32)
    o = (-raw.ctypes.data % 16) // 4 + offset
    return raw[o:o + int(np.prod(shape))].reshape(shape)


def image(rows, K):
    return np.full((rows, (K + 31) // 32, 2, 32), 0xA5A5, np.uint16)


def digest(rc, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).view(np.uint8).tobytes())
    return f"rc {rc} {h.hexdigest()[:32]}"


class Operands:
    """Seeded A (Bb, Tt, K) read time-major (m = t*Bb + b), W (N, K), bias, and their x3 images made by the library under test."""
    def __init__(self, lib, Bb, Tt, K, N, seed):
        self.Bb, self.Tt, self.K, self.N, self.M = Bb, Tt, K, N, Bb * Tt
        self.x, self.W, self.bias = rand(seed, Bb, Tt, K), rand(seed + 1, N, K), rand(seed + 2, N)
        self.a_img, self.w_img = image(self.M, K), image(N, K)
        self.rc = (lib.dll.onssen_x3_image_f32(P(self.x), K, Tt * K, Bb, self.M, K, P(self.a_img), None),
                   lib.dll.onssen_x3_image_f32(P(self.W), K, 0, 1, N, K, P(self.w_img), None))

    def out(self, pad=0, offset=0):
        return nans(self.Bb, self.Tt, self.N + pad, offset=offset)


def fp32_forms(lib):
    d = lib.dll
    Bb, Tt = 3, 47
    for K, ld in ((37, 64), (40, 64)):                       # odd K: scalar A loads; K % 4 == 0: vector loads
        for N, bn in ((100, "linear_f32"), (180, "linear_bf16x3")):
            x, W, bias = rand(K, Bb, Tt, K), np.zeros((N, ld), np.float32), rand(K + 2, N)
            W[:, :K] = rand(K + 1, N, K)
            planes = np.full((2, N, ld), 0xA5A5, np.uint16)
            if bn == "linear_bf16x3":
                yield f"linear_pack_bf16x3 N={N} K={K} ld={ld}", digest(d.onssen_linear_pack_bf16x3(P(W), N, K, ld, ld, P(planes), None), planes)
            for mode, group, with_res in ((BIAS, 0, 0), (L2N, 20, 0), (SIG, 0, 0), (L2N, 2, 1), (RELU, 0, 0), (RELU, 0, 1)):
                for pad, off in ((0, 0), (3, 1)):            # dense aligned C rows (vector stores) / odd strides, misaligned C
                    out = nans(Bb, Tt, N + pad, offset=off)
                    res = rand(K + 3, Bb, Tt, N + pad) if with_res else None       # (laid out like C)
                    if bn == "linear_f32":
                        rc = d.onssen_linear_f32(P(x), K, Tt * K, Bb, Tt * Bb, K, P(W), ld, P(bias), N, mode, group, 1e-12, P(res), P(out),
                                                 N + pad, Tt * (N + pad), None)
                    else:
                        rc = d.onssen_linear_bf16x3(P(x), K, Tt * K, Bb, Tt * Bb, K, P(planes), ld, P(bias), N, mode, group, 1e-12, P(res),
                                                    P(out), N + pad, Tt * (N + pad), None)
                    yield f"{bn} mode={mode} group={group} resid={res is not None} K={K} c_pad={pad}", digest(rc, out)


def images(lib):
    d = lib.dll
    for K, M, shift in ((70, 150, 0), (64, 64, -3), (33, 97, 7)):
        ld = M + 3
        src = rand(K + M, K, ld)
        KB = (K + 31) // 32
        rows, t = image(K, M), image(M, K)
        yield f"x3_image rows={K} K={M} ld={ld}", digest(d.onssen_x3_image_f32(P(src), ld, 0, 1, K, M, P(rows), None), rows)
        yield f"x3_image_t M={M} K={K} shift={shift}", digest(d.onssen_x3_image_t_f32(P(src), ld, M, K, shift, P(t), None), t)
        rows, t = image(K, M), image(M, K)
        yield f"x3_image_both M={M} K={K}", digest(d.onssen_x3_image_both_f32(P(src), ld, M, K, P(rows), P(t), None), rows, t)
        rows, t, part = image(K, M), image(M, K), nans(KB, M)
        yield f"x3_image_both_colsum M={M} K={K}", digest(d.onssen_x3_image_both_colsum_f32(P(src), ld, M, K, P(rows), P(t), P(part), None), rows, t, part)
    x = rand(5, 3, 47, 37)                                   # strided rows: (B, T, K) read time-major
    img = image(141, 37)
    yield "x3_image time-major rows", digest(d.onssen_x3_image_f32(P(x), 37, 47 * 37, 3, 141, 37, P(img), None), img)


def x3p(lib):
    d = lib.dll
    ops = {K: Operands(lib, 3, 91, K, 440, 8 + K) for K in (37, 64)}        # M = 273, N = 440: ragged in every tile shape
    def call(o, mode, group, pad=4, off=0):
        out = o.out(pad, off)
        return digest(d.onssen_linear_x3p(P(o.a_img), o.M, o.K, P(o.w_img), P(o.bias), o.N, mode, group, 1e-12, P(out), o.Bb, o.N + pad,
                                          o.Tt * (o.N + pad), None), out)
    for K, o in ops.items():
        yield f"operand images K={K}", digest(o.rc, o.a_img, o.w_img)
    for q in (None, 0, 256, 320):
        for bm in (None, 128, 256):
            for mode, group, K in ((BIAS, 0, 37), (L2N, 20, 64), (SIG, 0, 37), (L2N, 40, 37)):
                for bf in (0, BF16):
                    env(q, bm)
                    yield f"linear_x3p X3Q={q} X3Q_BM={bm} mode={mode | bf:#x} group={group} K={K}", call(ops[K], mode | bf, group)
    for q, bm in ((None, None), (256, 128), (320, 128), (256, 256), (0, None)):
        for r in (None, 1, 0):
            for bf in (0, BF16):
                for mode, group in ((BIAS, 0), (SIG, 0)):    # (ONSSEN_X3R is for the bias mode only)
                    env(q, bm, r)
                    yield f"linear_x3p X3Q={q} X3Q_BM={bm} X3R={r} mode={mode | bf:#x}", call(ops[37], mode | bf, group)
    for r in (None, 1):
        for mode, group, K in ((BIAS | BF16, 0, 37), (BIAS, 0, 64), (SIG, 0, 37), (L2N, 20, 64)):
            env(None, None, r, 8)                            # KB = 2 <= 8: 128 x 128 tiles in the bias mode (unless ONSSEN_X3R=1)
            yield f"linear_x3p X3Q_SMALL=8 X3R={r} mode={mode:#x} K={K}", call(ops[K], mode, group)
    env(None, None, None, 1)                                 # below the call's KB: not taken
    yield "linear_x3p X3Q_SMALL=1 mode=0 K=37", call(ops[37], BIAS, 0)
    for q in (None, 0):
        for mode, group in ((BIAS, 0), (L2N, 20), (SIG, 0)):
            env(q)                                           # dense, aligned C: vector stores; then a misaligned C
            yield f"linear_x3p X3Q={q} mode={mode} dense C", call(ops[64], mode, group, 0, 0)
            yield f"linear_x3p X3Q={q} mode={mode} misaligned C", call(ops[64], mode, group, 0, 1)
    env()


def heads(lib, quick):
    d = lib.dll
    for M, bm, q in ((273, 256, None), (150, 128, None), (150, None, 0)):    # (ONSSEN_X3Q is ignored: no round-1 form)
        o = Operands(lib, 1, M, 75, 440, 21)
        e, inv = nans(M, 440), nans(M, 22)
        env(q, bm)
        yield f"linear_x3p_norms M={M} X3Q={q} X3Q_BM={bm}", digest(d.onssen_linear_x3p_norms(P(o.a_img), M, 75, P(o.w_img), P(o.bias), 440, 20, 1e-12,
                                                                                        P(e), P(inv), None), e, inv)
    R, Tt = 3, 47
    for group, N, bm, q, bf in ((2, 514, 256, None, 0), (2, 38, 128, 0, 1), (20, 440, 256, 0, 0), (20, 440, None, None, 1), (40, 440, 128, None, 0)):
        o = Operands(lib, 2 * R, Tt, 75, N, 9)
        resid, out = rand(99, R, Tt, N), o.out()
        env(q, bm)
        yield (f"linear_x3p_resid group={group} N={N} X3Q={q} X3Q_BM={bm} bf16={bf}",
               digest(d.onssen_linear_x3p_resid(P(o.a_img), o.M, 75, P(o.w_img), P(o.bias), N, group, 1e-12, P(resid), R, P(out), 2 * R, N, Tt * N, bf, None), out))
    env(0, 256, 1, 8)                                        # pair and compact: no switch applies
    group = 20
    shapes = [(2, 30, 75, 286), (2, 150, 75, 286), (3, 91, 33, 440)]
    if not quick:                                            # 252 half-height tiles: one round, 128 rows; 261: two rounds, 256 rows
        shapes += [(1, 3584, 32, 2580), (1, 3585, 32, 2580)]
    for Bb, Tt, K, N in shapes:
        o = Operands(lib, Bb, Tt, K, N, 10)
        F, Na = N // group, (N - 21) // group * group           # the split inside the last tile, a multiple of the group
        for bf in (0, 1):
            for off in (0, 1):
                out_a, out_b = nans(Bb, Tt, Na, offset=off), nans(Bb, Tt, N - Na)
                rc = d.onssen_linear_x3p_pair(P(o.a_img), o.M, K, P(o.w_img), P(o.bias), N, Na, group, 1e-12, P(out_a), Bb, Na, Tt * Na,
                                              P(out_b), N - Na, Tt * (N - Na), bf, None)
                yield f"linear_x3p_pair M={o.M} N={N} n_split={Na} K={K} bf16={bf} c_off={off}", digest(rc, out_a, out_b)
        if N % group:
            continue
        per = Tt * F                                         # compacted rows per utterance: every third bin dropped
        keep = np.arange(per) % 3 != 0
        dest = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)[None].repeat(Bb, 0).copy()
        for bf in (0, 1):
            comp = nans(Bb, per, group)
            rc = d.onssen_linear_x3p_compact(P(o.a_img), o.M, K, P(o.w_img), P(o.bias), N, group, 1e-12, P(dest), per, F, P(comp), Bb, per * group, bf, None)
            yield f"linear_x3p_compact M={o.M} N={N} K={K} bf16={bf}", digest(rc, comp)
    env()


def gradients(lib):
    d = lib.dll
    H, Kx, TB = 12, 40, 70
    NP, N1, KB = 4 * H, Kx + H, (TB + 31) // 32
    def img(m):
        o = image(m.shape[0], m.shape[1])
        assert d.onssen_x3_image_f32(P(m), m.shape[1], 0, 1, m.shape[0], m.shape[1], P(o), None) == 0
        return o
    dP, hf, hr, x = rand(31, 2, NP, TB), rand(32, H, TB), rand(33, H, TB), rand(34, Kx, TB)
    a = np.stack([img(dP[0]), img(dP[1])])
    w, w1, bias = np.stack([img(np.concatenate([x, hf])), img(np.concatenate([x, hr]))]), img(np.concatenate([hf, x, hr])), rand(35, N1)
    for ldc in (N1, N1 + 3):
        out = nans(2, NP, ldc)
        yield f"linear_x3p_batched ldc={ldc}", digest(d.onssen_linear_x3p_batched(P(a), NP * KB * 64, NP, TB, P(w), N1 * KB * 64, P(bias), N1, P(out),
                                                                              NP * ldc, ldc, 2, None), out)
    ih, hh = nans(2, 4 * H, Kx), nans(2, 4 * H, H)
    yield "linear_x3p_batched_split", digest(d.onssen_linear_x3p_batched_split(P(a), NP * KB * 64, NP, TB, P(w), N1 * KB * 64, P(bias), N1, 4, P(ih), 4 * H * Kx,
                                                                               Kx, H * Kx, Kx, P(hh), 4 * H * H, H, H * H, 2, None), ih, hh)
    ih, hh = nans(2, 4 * H, Kx), nans(2, 4 * H, H)
    yield "linear_x3p_batched_split_alt", digest(d.onssen_linear_x3p_batched_split_alt(P(a), NP * KB * 64, NP, TB, P(w1), H * KB * 64, P(bias), N1, 4, P(hh),
                                                                                       4 * H * H, H, H * H, H, P(ih), 4 * H * Kx, Kx, H * Kx, Kx, 2, None), ih, hh)
    for H, Kx, T, B in ((16, 40, 9, 5), (16, 13, 7, 3)):
        NP, K = 4 * H, T * B
        dp_img, y_img, x_img, zero = img(rand(H, K, 2 * NP)), img(rand(H + 1, K, 2 * H)), img(rand(H + 2, K, Kx)), np.zeros(64, np.float32)
        ih, hh = nans(2, 4 * H, Kx), nans(2, 4 * H, H)
        yield f"lstm_wgrad_images H={H} Kx={Kx} T={T} B={B}", digest(d.onssen_lstm_wgrad_images_f32(
            P(dp_img), P(y_img), P(x_img), K, B, NP, H, Kx, P(zero), 4, P(ih), 4 * H * Kx, Kx, H * Kx, P(hh), 4 * H * H, H, H * H, None), ih, hh)
    for K, M, N in ((70, 44, 40), (45, 300, 170)):
        a_r, w_r, got, zero = img(rand(K, K, M)), img(rand(K + 1, K, N)), nans(M, N + 3), np.zeros(64, np.float32)
        yield f"linear_x3t K={K} M={M} N={N}", digest(d.onssen_linear_x3t(P(a_r), P(w_r), K, M, N, P(zero), P(got), N + 3, None), got)


def refusals(lib):
    """(name, return code) of every refusal of every GEMM entry: nothing is launched, nothing is written."""
    d = lib.dll
    env()
    M, K, N, ld, R = 12, 40, 40, 64, 3
    A, W, bias, C, C2 = rand(1, M, K), rand(2, N, ld), rand(3, N), nans(M, N), nans(M, N)
    planes, a_img, w_img, zero = np.zeros((2, N, ld), np.uint16), image(M, K), image(N, K), np.zeros(64, np.float32)
    dest = np.zeros((R, 8), np.int32)
    big_K = 32 * 65537                                       # KB = 65537: 256 * KB * 128 passes 2^31
    def f32(A_=A, W_=W, ldw=ld, mode=BIAS, group=0, resid=None, M_=M):
        return d.onssen_linear_f32(P(A_), K, 0, 1, M_, K, P(W_), ldw, P(bias), N, mode, group, 1e-12, P(resid), P(C), N, 0, None)
    yield "linear_f32 null A", f32(A_=None)
    yield "linear_f32 M=0", f32(M_=0)
    yield "linear_f32 ldw < K", f32(ldw=36)
    yield "linear_f32 ldw % 4", f32(ldw=42)
    yield "linear_f32 misaligned W", d.onssen_linear_f32(P(A), K, 0, 1, M, K, P(W) + 4, ld, P(bias), N, BIAS, 0, 0.0, None, P(C), N, 0, None)
    yield "linear_f32 group 0", f32(mode=L2N, group=0)
    yield "linear_f32 group 7 (80 % group)", f32(mode=L2N, group=7)
    yield "linear_f32 group 16 (N % group)", f32(mode=L2N, group=16)
    yield "linear_f32 resid with sigmoid", f32(mode=SIG, resid=C2)
    yield "linear_f32 unknown mode", f32(mode=4)
    yield "linear_pack_bf16x3 null planes", d.onssen_linear_pack_bf16x3(P(W), N, K, ld, ld, None, None)
    yield "linear_pack_bf16x3 ld_in < K", d.onssen_linear_pack_bf16x3(P(W), N, K, 39, ld, P(planes), None)
    yield "linear_pack_bf16x3 ld_out % 32", d.onssen_linear_pack_bf16x3(P(W), N, K, ld, 48, P(planes), None)
    def x3(w=planes, ldw=ld, mode=BIAS, group=0, resid=None, woff=0):
        return d.onssen_linear_bf16x3(P(A), K, 0, 1, M, K, (P(w) + woff) if w is not None else None, ldw, P(bias), N, mode, group, 1e-12, P(resid), P(C), N, 0, None)
    yield "linear_bf16x3 null planes", x3(w=None)
    yield "linear_bf16x3 ldw < K", x3(ldw=32)
    yield "linear_bf16x3 ldw % 32", x3(ldw=48)
    yield "linear_bf16x3 misaligned planes", x3(woff=2)
    yield "linear_bf16x3 group 0", x3(mode=L2N)
    yield "linear_bf16x3 group 3 (160 % group)", x3(mode=L2N, group=3)
    yield "linear_bf16x3 group 16 (N % group)", x3(mode=L2N, group=16)
    yield "linear_bf16x3 resid without L2NORM", x3(resid=C2)
    yield "linear_bf16x3 RELU", x3(mode=RELU)
    yield "x3_image null img", d.onssen_x3_image_f32(P(A), K, 0, 1, M, K, None, None)
    yield "x3_image rows=0", d.onssen_x3_image_f32(P(A), K, 0, 1, 0, K, P(a_img), None)
    yield "x3_image misaligned img", d.onssen_x3_image_f32(P(A), K, 0, 1, M, K, P(a_img) + 2, None)
    yield "x3_image_t null src", d.onssen_x3_image_t_f32(None, K, K, M, 0, P(w_img), None)
    yield "x3_image_t ld < M", d.onssen_x3_image_t_f32(P(A), K - 1, K, M, 0, P(w_img), None)
    yield "x3_image_t misaligned img", d.onssen_x3_image_t_f32(P(A), K, K, M, 0, P(w_img) + 8, None)
    yield "x3_image_both null img_t", d.onssen_x3_image_both_f32(P(A), K, K, M, P(a_img), None, None)
    yield "x3_image_both ld < M", d.onssen_x3_image_both_f32(P(A), K - 1, K, M, P(a_img), P(w_img), None)
    yield "x3_image_both misaligned img_rows", d.onssen_x3_image_both_f32(P(A), K, K, M, P(a_img) + 2, P(w_img), None)
    yield "x3_image_both_colsum null colsum", d.onssen_x3_image_both_colsum_f32(P(A), K, K, M, P(a_img), P(w_img), None, None)
    yield "x3_image_both_colsum misaligned img_t", d.onssen_x3_image_both_colsum_f32(P(A), K, K, M, P(a_img), P(w_img) + 2, P(C), None)
    def xp(a=a_img, aoff=0, K_=K, mode=BIAS, group=0):
        return d.onssen_linear_x3p((P(a) + aoff) if a is not None else None, M, K_, P(w_img), P(bias), N, mode, group, 1e-12, P(C), 1, N, 0, None)
    yield "linear_x3p null a_img", xp(a=None)
    yield "linear_x3p misaligned a_img", xp(aoff=2)
    yield "linear_x3p KB overflow", xp(K_=big_K)
    yield "linear_x3p pairs", xp(mode=L2N, group=2)
    yield "linear_x3p pairs, bf16", xp(mode=L2N | BF16, group=2)
    yield "linear_x3p group 0", xp(mode=L2N)
    yield "linear_x3p group 10 (group % 4)", xp(mode=L2N, group=10)
    yield "linear_x3p group 8 (80 / group > 4)", xp(mode=L2N, group=8)
    yield "linear_x3p group 16 (80 % group)", xp(mode=L2N, group=16)
    yield "linear_x3p group 80 (N % group)", xp(mode=L2N, group=80)
    yield "linear_x3p RELU", xp(mode=RELU)
    yield "linear_x3p null AND misaligned", d.onssen_linear_x3p(P(a_img) + 2, M, K, P(w_img), None, N, BIAS, 0, 0.0, P(C), 1, N, 0, None)
    def norms(inv=C2, group=20, K_=K):
        return d.onssen_linear_x3p_norms(P(a_img), M, K_, P(w_img), P(bias), N, group, 1e-12, P(C), P(inv), None)
    yield "linear_x3p_norms null inv_norm", norms(inv=None)
    yield "linear_x3p_norms group 2", norms(group=2)
    yield "linear_x3p_norms group 16", norms(group=16)
    yield "linear_x3p_norms KB overflow", norms(K_=big_K)
    def resid(group=2, res=C2, mod=R, K_=K, w=w_img, woff=0):
        return d.onssen_linear_x3p_resid(P(a_img), M, K_, P(w) + woff, P(bias), N, group, 1e-12, P(res), mod, P(C), R, N, 0, 0, None)
    yield "linear_x3p_resid group 0", resid(group=0)
    yield "linear_x3p_resid group 3", resid(group=3)
    yield "linear_x3p_resid group 8", resid(group=8)
    yield "linear_x3p_resid group 16 (N % group)", resid(group=16)
    yield "linear_x3p_resid resid_mod 0", resid(mod=0)
    yield "linear_x3p_resid misaligned w_img", resid(woff=4)
    yield "linear_x3p_resid KB overflow", resid(K_=big_K)
    yield "linear_x3p_resid KB overflow, no residual", resid(K_=big_K, res=None)
    def pair(c2=C2, group=20, n_split=20, K_=K, aoff=0):
        return d.onssen_linear_x3p_pair(P(a_img) + aoff, M, K_, P(w_img), P(bias), N, n_split, group, 1e-12, P(C), 1, 20, 0, P(c2), 20, 0, 0, None)
    yield "linear_x3p_pair null C2", pair(c2=None)
    yield "linear_x3p_pair group 2", pair(group=2)
    yield "linear_x3p_pair group 8", pair(group=8)
    yield "linear_x3p_pair n_split 0", pair(n_split=0)
    yield "linear_x3p_pair n_split = N", pair(n_split=N)
    yield "linear_x3p_pair n_split % group", pair(n_split=10)
    yield "linear_x3p_pair misaligned a_img", pair(aoff=2)
    yield "linear_x3p_pair KB overflow", pair(K_=big_K)
    yield "linear_x3p_pair bad group AND misaligned", pair(group=8, aoff=2)
    def compact(dst=dest, group=20, F=2, K_=K, coff=0, bs=160):
        return d.onssen_linear_x3p_compact(P(a_img), M, K_, P(w_img), P(bias), N, group, 1e-12, P(dst), 8, F, P(C) + coff, R, bs, 0, None)
    yield "linear_x3p_compact null dest", compact(dst=None)
    yield "linear_x3p_compact F=0", compact(F=0)
    yield "linear_x3p_compact group 2", compact(group=2)
    yield "linear_x3p_compact N != F * group", compact(F=3)
    yield "linear_x3p_compact misaligned comp", compact(coff=4)
    yield "linear_x3p_compact comp_bs % 4", compact(bs=162)
    yield "linear_x3p_compact KB overflow", compact(K_=big_K)
    def batched(batch=2, a_bs=0, aoff=0, K_=K):
        return d.onssen_linear_x3p_batched(P(a_img) + aoff, a_bs, M, K_, P(w_img), 0, P(bias), N, P(C), 0, N, batch, None)
    yield "linear_x3p_batched ldc < N", d.onssen_linear_x3p_batched(P(a_img), 0, M, K, P(w_img), 0, P(bias), N, P(C), 0, N - 1, 2, None)
    yield "linear_x3p_batched batch 0", batched(batch=0)
    yield "linear_x3p_batched batch 65536", batched(batch=65536)
    yield "linear_x3p_batched a_bs % 8", batched(a_bs=4)
    yield "linear_x3p_batched misaligned a_img", batched(aoff=2)
    yield "linear_x3p_batched KB overflow", batched(K_=big_K)
    def split(c2=C2, n_split=24, w_bs=0, batch=2, odd=None):
        if odd is None:
            return d.onssen_linear_x3p_batched_split(P(a_img), 0, M, K, P(w_img), w_bs, P(bias), N, 1, P(C), 0, N, 0, n_split, P(c2), 0, N, 0, batch, None)
        return d.onssen_linear_x3p_batched_split_alt(P(a_img), 0, M, K, P(w_img), w_bs, P(bias), N, 1, P(C), 0, N, 0, n_split, P(c2), 0, N, 0, odd, batch, None)
    yield "linear_x3p_batched_split null C2", split(c2=None)
    yield "linear_x3p_batched_split n_split 0", split(n_split=0)
    yield "linear_x3p_batched_split n_split = N", split(n_split=N)
    yield "linear_x3p_batched_split w_bs % 8", split(w_bs=12)
    yield "linear_x3p_batched_split batch 65536", split(batch=65536)
    yield "linear_x3p_batched_split_alt null C2", split(c2=None, odd=8)
    yield "linear_x3p_batched_split_alt n_split_odd 0", split(odd=0)
    yield "linear_x3p_batched_split_alt n_split_odd < 0", split(odd=-1)
    yield "linear_x3p_batched_split_alt n_split_odd = N", split(odd=N)
    yield "linear_x3p_batched_split_alt n_split = N", split(n_split=N, odd=8)
    def wgrad(NP=32, Hp=8, K_=6, zero_=zero, doff=0):
        return d.onssen_lstm_wgrad_images_f32(P(a_img) + doff, P(a_img), P(w_img), K_, 2, NP, Hp, 13, P(zero_), 1, P(C), 0, 13, 0, P(C2), 0, 8, 0, None)
    yield "lstm_wgrad_images null zero16", wgrad(zero_=None)
    yield "lstm_wgrad_images NP % 32", wgrad(NP=40)
    yield "lstm_wgrad_images Hp % 8", wgrad(Hp=4)
    yield "lstm_wgrad_images image overflow", wgrad(NP=32 * 4096, K_=4096)
    yield "lstm_wgrad_images misaligned dp_img", wgrad(doff=2)
    def x3t(ldc=N, K_=6, M_=M, zoff=0):
        return d.onssen_linear_x3t(P(a_img), P(w_img), K_, M_, N, P(zero) + zoff, P(C), ldc, None)
    yield "linear_x3t ldc < N", x3t(ldc=N - 1)
    yield "linear_x3t K=0", x3t(K_=0)
    yield "linear_x3t image overflow", x3t(K_=1 << 20, M_=1 << 10)
    yield "linear_x3t misaligned zero16", x3t(zoff=4)


def calls(lib, quick):
    for part in (fp32_forms(lib), images(lib), x3p(lib), heads(lib, quick), gradients(lib)):
        yield from part
    for name, rc in refusals(lib):
        yield "refusal: " + name, f"rc {rc}"


def main():
    args = [a for a in sys.argv[1:] if a != "--quick"]
    if len(args) != 2:
        sys.exit(__doc__)
    quick = "--quick" in sys.argv
    a, b = _abi.Lib(args[0]), _abi.Lib(args[1])
    bad = total = nref = 0
    for (name, da), (_, db) in zip(calls(a, quick), calls(b, quick)):
        total += 1
        nref += name.startswith("refusal: ")
        bad += da != db
        print(f"{'same' if da == db else 'DIFF'}  {name}: {da}" + ("" if da == db else f"  !=  {db}"), flush=True)
    print(f"{total - nref} calls and {nref} refusals compared, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
