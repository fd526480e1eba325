"""The three inverse transforms (mask_istft, phase_istft, mag_istft) restated in float64 on the NumPy oracle's transforms, with
their explicit adjoints -- the reference of tests/test_emu_istft_bwd.py, tests/test_gpu_istft_bwd.py and tests/test_gpu_wa_e2e.py
-- and the inputs those tests share.

    forward :  y_c[n] = rw[n] sum_t w[i] irfft(S_c[t])[i],  i = n + N/2 - t hop        (oracle.np_oracle.istft)
               S_c = X m_c (mode 0),  m_c |X| p_c (mode 1),  m_c X / |X| (mode 2);  |X| = np.hypot in float32, as the kernel's
               hypotf; mode 2's quotients are float32 too and (1, 0) where X = 0
    adjoint :  G_c[t] = (a_f / N) rfft(w[i] rw[n] gy_c[n]),  a_f = 1 at DC / Nyquist, else 2
               mode 0: g_m = Re X Re G + Im X Im G;  mode 1: g_m = |X| (Re p Re G + Im p Im G), g_p = m |X| (Re G, Im G);
               mode 2: g_m = Re u Re G + Im u Im G -- the imaginary terms dropped at DC / Nyquist (irfft ignores them)

``self_check`` compares the adjoints with torch float64 autograd of the same restatement, on the CPU.  Every case is built once
per process and must be left unchanged."""
import functools

import numpy as np

from onssen_amd.synthetic import synth_mixture_k
from oracle import np_oracle as O

MASK, PHASE, MAG = 0, 1, 2
MODE_NAMES = {MASK: "mask", PHASE: "phase", MAG: "mag"}

SHAPES = [(256, 64, 21, 2),        # (n_fft, hop, frames, speakers): more frames than one workgroup's first round
          (256, 100, 16, 3),       # a hop that does not divide the window; odd C
          (512, 128, 9, 2),
          (1024, 256, 6, 2),
          (256, 64, 12, 4),
          (256, 256, 5, 2)]        # no overlap: wss = 0 at the frame starts, the rw = 1 branch
MAG_ONLY_SHAPE = (256, 64, 12, 1)
RAGGED_SHAPE = (256, 64, 21, 2)    # frames = [T, T - 5]


def shapes_of(mode):
    return SHAPES + [MAG_ONLY_SHAPE] if mode == MAG else SHAPES


def window_rw(n_fft, hop, T):
    """w (N,), rw (N + hop (T - 1),): the reciprocal window sum of squares of O.istft, 1 where the sum is not above tiny."""
    w = O.hann_periodic(n_fft)
    wss = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        wss[t * hop:t * hop + n_fft] += w * w
    nz = wss > np.finfo(np.float64).tiny
    return w, np.where(nz, 1.0 / np.where(nz, wss, 1.0), 1.0)


def parts(ri):
    """ri (T, F, 2) float32 -> X complex128, |X| (float32 hypot, as float64), u = X / |X| with float32 quotients (complex128)."""
    ri = np.asarray(ri, dtype=np.float32)
    h = np.hypot(ri[..., 0], ri[..., 1])                            # float32
    nz = h > 0
    safe = np.where(nz, h, np.float32(1))
    ux = np.where(nz, ri[..., 0] / safe, np.float32(1)).astype(np.float32)
    uy = np.where(nz, ri[..., 1] / safe, np.float32(0)).astype(np.float32)
    return ri[..., 0].astype(np.float64) + 1j * ri[..., 1].astype(np.float64), h.astype(np.float64), ux.astype(np.float64) + 1j * uy.astype(np.float64)


def operand(ri, m, mode, p=None):
    """One speaker's spectrum S (T, F) complex128: m (T, F) its mask / magnitude, p (T, F, 2) its phase vectors (mode 1)."""
    X, h, u = parts(ri)
    m = np.asarray(m, dtype=np.float64)
    if mode == MASK:
        return X * m
    if mode == PHASE:
        p = np.asarray(p, dtype=np.float64)
        return m * h * (p[..., 0] + 1j * p[..., 1])
    return m * u


def forward(ri, m, mode, hop, length, p=None, f32_frames=False):
    """One utterance: ri (T, F, 2), m (T, F, C), p (C, T, F, 2) -> (C, length) float64.  ``f32_frames``: the windowed frames
    are rounded to float32 before the overlap-add, as the kernel stores them."""
    T, F, C = m.shape
    n_fft = 2 * (F - 1)
    out = []
    for c in range(C):
        S = operand(ri, m[..., c], mode, None if p is None else p[c])
        if not f32_frames:
            out.append(O.istft(S, hop, length))
            continue
        w, rw = window_rw(n_fft, hop, T)
        fr = (w[None] * np.fft.irfft(S, n=n_fft, axis=1)).astype(np.float32).astype(np.float64)
        y = np.zeros(n_fft + hop * (T - 1))
        for t in range(T):
            y[t * hop:t * hop + n_fft] += fr[t]
        y = (y * rw)[n_fft // 2:]
        out.append(y[:length] if len(y) >= length else np.pad(y, (0, length - len(y))))
    return np.stack(out)


def adjoint(ri, m, mode, hop, gy, p=None):
    """One utterance: gy (C, length) the gradient at forward's result -> g_m (T, F, C), g_p (C, T, F, 2) (zeros outside mode 1),
    float64."""
    T, F, C = m.shape
    n_fft = 2 * (F - 1)
    gy = np.asarray(gy, dtype=np.float64)
    length = gy.shape[1]
    w, rw = window_rw(n_fft, hop, T)
    X, h, u = parts(ri)
    alpha = np.full(F, 2.0)
    alpha[0] = alpha[-1] = 1.0
    edge = np.zeros(F, dtype=bool)
    edge[0] = edge[-1] = True
    g_m, g_p = np.zeros((T, F, C)), np.zeros((C, T, F, 2))
    for c in range(C):
        full = np.zeros(n_fft + hop * (T - 1) + max(0, length))
        full[n_fft // 2:n_fft // 2 + length] = gy[c]
        full = full[:n_fft + hop * (T - 1)] * rw
        idx = np.arange(n_fft)[None, :] + hop * np.arange(T)[:, None]
        G = alpha[None] / n_fft * np.fft.rfft(full[idx] * w[None], axis=1)
        Gr, Gi = G.real, np.where(edge[None], 0.0, G.imag)
        if mode == MASK:
            g_m[..., c] = X.real * Gr + X.imag * Gi
        elif mode == PHASE:
            pc = np.asarray(p[c], dtype=np.float64)
            g_m[..., c] = h * (pc[..., 0] * Gr + pc[..., 1] * Gi)
            s = np.asarray(m[..., c], dtype=np.float64) * h
            g_p[c, ..., 0], g_p[c, ..., 1] = s * Gr, s * Gi
        else:
            g_m[..., c] = u.real * Gr + u.imag * Gi
    return g_m, g_p


def torch_forward(ri, m, mode, hop, length, p=None):
    """``forward`` in torch float64 on the CPU (m and p may require grad): the restatement autograd differentiates."""
    import torch
    T, F, C = m.shape
    n_fft = 2 * (F - 1)
    X, h, u = parts(ri)
    w, rw = window_rw(n_fft, hop, T)
    X, h, u, w, rw = (torch.from_numpy(np.ascontiguousarray(a)) for a in (X, h, u, w, rw))
    out = []
    for c in range(C):
        if mode == MASK:
            S = X * m[..., c]
        elif mode == PHASE:
            S = (m[..., c] * h) * torch.complex(p[c, ..., 0], p[c, ..., 1])
        else:
            S = m[..., c] * u
        fr = torch.fft.irfft(S, n=n_fft, dim=1) * w[None]
        y = torch.zeros(n_fft + hop * (T - 1) + length, dtype=torch.float64)
        for t in range(T):
            y = y + torch.nn.functional.pad(fr[t], (t * hop, hop * (T - 1 - t) + length))
        y = y[:n_fft + hop * (T - 1)] * rw
        y = torch.cat([y, torch.zeros(length, dtype=torch.float64)])
        out.append(y[n_fft // 2:n_fft // 2 + length])
    return torch.stack(out)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(n_fft, hop, T, C, B=2):
    """ri (B,T,F,2) f32 spectra of synthetic mixtures of n = hop (T - 1) samples; masks (B,T,F,C) f32 in [0, 1); mags (B,T,F,C)
    f32 = masks |X|; phases (C,B,T,F,2) f32 unit vectors; gy (B,C,n) f32: the gradient arriving at the waveforms."""
    rng = np.random.default_rng(2300 + n_fft + hop + 7 * C + T)
    n = hop * (T - 1)
    k = Case()
    mix = np.stack([synth_mixture_k(30 + b, n, num_speaker=max(C, 2))[0] for b in range(B)]).astype(np.float32)
    X = [O.stft(mix[b], n_fft, hop) for b in range(B)]
    assert X[0].shape[0] == T
    F = X[0].shape[1]
    k.ri = np.ascontiguousarray(np.stack([np.stack([x.real, x.imag], -1) for x in X]), dtype=np.float32)
    k.masks = rng.random((B, T, F, C)).astype(np.float32)
    k.mags = (k.masks * np.hypot(k.ri[..., 0], k.ri[..., 1])[..., None]).astype(np.float32)
    p = rng.standard_normal((C, B, T, F, 2))
    k.phases = np.ascontiguousarray(p / np.linalg.norm(p, axis=-1, keepdims=True), dtype=np.float32)
    k.gy = rng.standard_normal((B, C, n)).astype(np.float32)
    k.B, k.C, k.T, k.F, k.n, k.n_fft, k.hop = B, C, T, F, n, n_fft, hop
    for a in (k.ri, k.masks, k.mags, k.phases, k.gy):
        a.setflags(write=False)
    return k


def operand_of(k, mode):
    return k.mags if mode == MAG else k.masks


@functools.lru_cache(maxsize=None)
def reference(n_fft, hop, T, C, mode, ragged=False, B=2):
    """g_op (B,T,F,C), g_ph (C,B,T,F,2) float64 of the case; ``ragged``: frames = [T, T - 5, ...], lengths = hop (frames - 1)."""
    k = case(n_fft, hop, T, C, B)
    g_op, g_ph = np.zeros((B, T, k.F, C)), np.zeros((C, B, T, k.F, 2))
    frames, lengths = ragged_extents(k) if ragged else ([T] * B, [k.n] * B)
    for b in range(B):
        Tb, nb = frames[b], lengths[b]
        gm, gp = adjoint(k.ri[b, :Tb], operand_of(k, mode)[b, :Tb], mode, hop, k.gy[b, :, :nb], k.phases[:, b, :Tb])
        g_op[b, :Tb], g_ph[:, b, :Tb] = gm, gp
    return g_op, g_ph


def ragged_extents(k):
    frames = [k.T - 5 * b for b in range(k.B)]
    return frames, [k.hop * (t - 1) for t in frames]


def self_check():
    """The explicit adjoints against torch float64 autograd of the same restatement, every mode, two shapes (one with a hop that
    does not divide the window and an odd C, one without overlap).  Returns the largest relative difference."""
    import torch
    worst = 0.0
    for shape in [(256, 100, 16, 3), (256, 256, 5, 2), (512, 128, 9, 2)]:
        k = case(*shape)
        for mode in (MASK, PHASE, MAG):
            m = torch.from_numpy(operand_of(k, mode)[0].astype(np.float64)).requires_grad_(True)
            p = torch.from_numpy(k.phases[:, 0].astype(np.float64)).requires_grad_(mode == PHASE)
            y = torch_forward(k.ri[0], m, mode, k.hop, k.n, p)
            np.testing.assert_allclose(y.detach().numpy(), forward(k.ri[0], operand_of(k, mode)[0], mode, k.hop, k.n, k.phases[:, 0]),
                                       rtol=0, atol=1e-12)
            (y * torch.from_numpy(k.gy[0].astype(np.float64))).sum().backward()
            gm, gp = adjoint(k.ri[0], operand_of(k, mode)[0], mode, k.hop, k.gy[0], k.phases[:, 0])
            worst = max(worst, np.abs(m.grad.numpy() - gm).max() / np.abs(gm).max())
            if mode == PHASE:
                worst = max(worst, np.abs(p.grad.numpy() - gp).max() / np.abs(gp).max())
    return worst


# Bounds of the gradient tests: 4 x the largest max |got - ref| measured on the host-side build over all shapes, per gradient kind
# (operation order differs between the builds); per case the hard ceiling is 1e-5 max |ref|.  The absolute maxima all come from the
# shape without overlap, whose gradients are ~500 x larger than the others' (rw = 1 / w[i]^2 next to the window's zero), so an
# absolute bound alone would say nothing about the other shapes: the same 4 x margin is also asserted on the largest RELATIVE error
# max |got - ref| / max |ref| measured over all modes and shapes.  Per-shape values: DESIGN section 23.
GRAD_MEASURED_MAX = {(MASK, "g_mask"): 3.005e-05, (PHASE, "g_mask"): 2.905e-05, (PHASE, "g_phase"): 1.519e-05, (MAG, "g_mag"): 7.212e-06}
GRAD_BOUND = {key: 4 * v for key, v in GRAD_MEASURED_MAX.items()}
GRAD_MEASURED_REL = 4.78e-08       # mag (256, 64, 12, 4)
GRAD_REL_BOUND = 4 * GRAD_MEASURED_REL
