"""Inputs shared by the phase-aware iSTFT tests (tests/test_emu_phase_istft.py, tests/test_gpu_phase_e2e.py) and by
tools/gen_golden_mask_istft.py: real STFTs of synthetic mixtures, random masks, random unit phase vectors."""
import numpy as np

from onssen_amd.synthetic import synth_mixture
from oracle import np_oracle as O

SHAPES = [(256, 64, 768), (256, 100, 1500), (512, 128, 2048), (1024, 256, 4096)]       # (n_fft, hop, samples)


def case(n_fft, hop, n, C=2, B=2):
    """specs: B complex (T, F) spectra; ri (B,T,F,2) float32; masks (B,T,F,C); phases (C,B,T,F,2), unit vectors."""
    rng = np.random.default_rng(n_fft + hop + 7 * C)
    specs = [O.stft(synth_mixture(30 + b, n), n_fft, hop) for b in range(B)]
    T, F = specs[0].shape
    ri = np.ascontiguousarray(np.stack([np.stack([s.real, s.imag], -1) for s in specs]), dtype=np.float32)
    masks = rng.random((B, T, F, C)).astype(np.float32)
    p = rng.standard_normal((C, B, T, F, 2))
    phases = np.ascontiguousarray(p / np.linalg.norm(p, axis=-1, keepdims=True), dtype=np.float32)
    return specs, ri, masks, phases


def reference(ri, masks, phases, hop, length):
    """(B, C, length) float64: O.istft(mask |X| (p.re + i p.im)) per speaker, |X| of the float32 spectrum the kernel reads."""
    X = ri[..., 0].astype(np.float64) + 1j * ri[..., 1].astype(np.float64)
    B, C = masks.shape[0], masks.shape[3]
    return np.stack([np.stack([O.istft(masks[b, ..., c] * np.abs(X[b]) * (phases[c, b, ..., 0] + 1j * phases[c, b, ..., 1]), hop, length)
                               for c in range(C)]) for b in range(B)])


def atol(ref):
    """2e-6 is the project's iSTFT bound (tests/test_emu_kernels.py); 4 eps32 max|ref| more for the float32 hypotf and the
    product mask |X| p, which the float64 reference does not round."""
    return 2e-6 + 4 * np.finfo(np.float32).eps * np.abs(ref).max()
