"""Inputs shared by the MISI tests (tests/test_emu_misi.py, tests/test_misi_api.py, tests/test_gpu_misi.py): synthetic
mixtures of C voices, their float32 spectra, random masks and the estimates those masks give on the mixture's phase.  Every
case is built once per process and must be left unchanged."""
import functools

import numpy as np

from onssen_amd.synthetic import synth_mixture_k
from oracle import np_oracle as O

SHAPES = [(256, 64, 768, 2),        # (n_fft, hop, samples, speakers)
          (256, 100, 1500, 3),      # a hop that does not divide the window; odd C: the last pair repeats its speaker
          (512, 128, 2048, 2),      # the 2 * 4^k plan
          (1024, 256, 4096, 2),     # 16 samples per lane
          (256, 64, 2000, 4)]
EFFECT_SHAPE = (256, 64, 4096, 2)   # the SI-SDR gain on the device


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(n_fft, hop, n, C, B=2):
    """mix (B,n) f32; src (B,C,n) f32; X: B complex64 (T,F); ri (B,T,F,2) f32; masks (B,T,F,C) f32 in [0, 1); est (B,C,n) f32:
    O.istft(X * mask_c) -- what mask_istft returns for these masks, from the oracle."""
    rng = np.random.default_rng(1000 + n_fft + hop + 7 * C + n)
    k = Case()
    sigs = [synth_mixture_k(30 + b, n, num_speaker=C) for b in range(B)]
    k.mix = np.ascontiguousarray(np.stack([s[0] for s in sigs]), dtype=np.float32)
    k.src = np.ascontiguousarray(np.stack([np.stack(s[1:]) for s in sigs]), dtype=np.float32)
    k.X = [O.stft(k.mix[b], n_fft, hop) for b in range(B)]
    T, F = k.X[0].shape
    k.ri = np.ascontiguousarray(np.stack([np.stack([x.real, x.imag], -1) for x in k.X]), dtype=np.float32)
    k.masks = rng.random((B, T, F, C)).astype(np.float32)
    k.est = np.ascontiguousarray(np.stack([np.stack([O.istft(k.X[b] * k.masks[b, ..., c], hop, n) for c in range(C)])
                                           for b in range(B)]), dtype=np.float32)
    k.B, k.C, k.T, k.F, k.n, k.n_fft, k.hop = B, C, T, F, n, n_fft, hop
    for a in (k.mix, k.src, k.ri, k.masks, k.est):
        a.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def oracle_case(n_fft, hop, n, C, B=2):
    """``case`` with ORACLE magnitudes: ratio (B,T,F,C) f32 = |stft(src_c)| / |X| (0 where X = 0), so that ratio * |X| is the true
    source magnitude, on the mixture's phase."""
    k = case(n_fft, hop, n, C, B)
    o = Case()
    o.__dict__.update(k.__dict__)
    absX = np.stack([np.abs(x) for x in k.X]).astype(np.float64)
    S = np.stack([np.stack([np.abs(O.stft(k.src[b, c], n_fft, hop)) for c in range(C)], -1) for b in range(B)]).astype(np.float64)
    o.ratio = np.where(absX[..., None] > 0, S / np.where(absX > 0, absX, 1.0)[..., None], 0.0).astype(np.float32)
    o.ratio.setflags(write=False)
    return o


def reference_spectra(k):
    """Z (B, C, T, F) complex128 of the half-step on the case's estimates (tests/misi_ref.py)."""
    from tests.misi_ref import misi_spectra
    return np.stack([misi_spectra(k.mix[b], k.est[b], k.n_fft, k.hop) for b in range(k.B)])


def check_phase(got, Z, what=""):
    """Rule (a) of the half-step's tests.  got (C,B,T,F,2) float32, Z (B,C,T,F) complex128 the float64 reference spectra.
    On bins with |Z| >= 1e-6 max|Z| every component is within 1e-6 of Z / |Z| -- one float32 rounding of an fp64 quotient is
    <= 6e-8 and the fp64 transform error relative to such a bin is <~ 3e-8 at N = 1024: about ten-fold margin; the bins left
    out are at most 1 % of the case (the reference alone leaves out <= 0.06 % on these inputs); every output, the excluded bins
    included, is finite and of unit norm within 1e-6."""
    from tests.misi_ref import unit
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what
    norm = np.hypot(got[..., 0], got[..., 1])
    Zc = np.moveaxis(Z, 1, 0)                                     # (C, B, T, F)
    keep = np.abs(Zc) >= 1e-6 * np.abs(Zc).max()
    err = np.abs(got - unit(Zc))[keep].max()
    left_out = 1.0 - keep.mean()
    print(f"{what}: max |p - ref| on kept bins {err:.3e} (bound 1e-6), left out {100 * left_out:.4f} % (cap 1 %), "
          f"max | |p| - 1 | {np.abs(norm - 1).max():.3e} (bound 1e-6)")
    assert left_out <= 0.01, (what, left_out)
    assert err <= 1e-6, (what, err)
    assert np.abs(norm - 1).max() <= 1e-6, what


# Bound of the whole iteration, rule (d): 4 x the largest max |out - ref| measured on the host-side build over the five shapes
# and K in {1, 3} (the device's hypot and contraction differ from the host's).  Measured values: tests/test_emu_misi.py.
ITER_MEASURED_MAX = 1.118e-07      # (256, 64, 2000, 4), K = 3
ITER_BOUND = 4 * ITER_MEASURED_MAX
