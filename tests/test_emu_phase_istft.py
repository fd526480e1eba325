"""onssen_phase_istft_f32 (mask_istft_kernel with its phase flag) in the host-side build against the NumPy oracle, against
onssen_mask_istft_f32 on the mixture's own phase, and onssen_mask_istft_f32 itself against the bits it gave before the flag
existed (tests/golden/g9_mask_istft_bits.npz, tools/gen_golden_mask_istft.py)."""
import os

import numpy as np
import pytest

from tests.emu_build import load_emu
from tests.phase_istft_cases import SHAPES, atol, case, reference


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return a.ctypes.data


def phase_istft(lib, ri, masks, phases, n_fft, hop, length):
    B, T, F, C = masks.shape
    out = np.full((B, C, length), np.nan, np.float32)
    lib.phase_istft(P(ri), P(masks), T * F * C, 1, F * C, C, P(phases), B * T * F * 2, B, C, T, n_fft, hop, length, P(out), None)
    return out


@pytest.mark.parametrize("n_fft,hop,n,C", [s + (2,) for s in SHAPES] + [SHAPES[0] + (3,)])
def test_phase_istft_matches_oracle(lib, n_fft, hop, n, C):
    """Random masks and unit phases; C = 3 covers the last speaker pair with one speaker."""
    _, ri, masks, phases = case(n_fft, hop, n, C)
    out = phase_istft(lib, ri, masks, phases, n_fft, hop, n)
    ref = reference(ri, masks, phases, hop, n)
    print(f"n_fft {n_fft} hop {hop} C {C}: max |out - ref| {np.abs(out - ref).max():.3e}, bound {atol(ref):.3e}")
    assert np.isfinite(out).all() and np.abs(out - ref).max() <= atol(ref)


@pytest.mark.parametrize("n_fft,hop,n", SHAPES)
def test_mixture_phase_gives_mask_istft(lib, n_fft, hop, n):
    """phase = X / |X|: mask |X| X / |X| is the operand of mask_istft."""
    _, ri, masks, _ = case(n_fft, hop, n)
    B, T, F, C = masks.shape
    mag = np.maximum(np.hypot(ri[..., 0], ri[..., 1]), np.float32(1e-30))
    own = (ri / mag[..., None]).astype(np.float32)
    phases = np.ascontiguousarray(np.stack([own] * C))
    out = phase_istft(lib, ri, masks, phases, n_fft, hop, n)
    plain = np.full((B, C, n), np.nan, np.float32)
    lib.mask_istft(P(ri), P(masks), T * F * C, 1, F * C, C, B, C, T, n_fft, hop, n, P(plain), None)
    print(f"n_fft {n_fft} hop {hop}: max |phase_istft - mask_istft| {np.abs(out - plain).max():.3e}, bound {atol(plain):.3e}")
    assert np.abs(out - plain).max() <= atol(plain)


def test_mask_istft_keeps_its_bits(lib, golden_dir):
    """Every instantiation without the flag keeps its code path: the same bits as before the flag existed."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_golden_mask_istft", os.path.join(os.path.dirname(golden_dir), "..", "tools",
                                                                                         "gen_golden_mask_istft.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(os.path.join(golden_dir, "g9_mask_istft_bits.npz"))
    got = gen.outputs(lib)
    assert sorted(got) == sorted(want.files) and len(got) == 5
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_refusals(lib):
    _, ri, masks, phases = case(256, 64, 768)
    B, T, F, C = masks.shape
    out = np.zeros((B, C, 768), np.float32)
    args = lambda ph, p_sc: (P(ri), P(masks), T * F * C, 1, F * C, C, ph, p_sc, B, C, T, 256, 64, 768, P(out), None)
    assert lib.dll.onssen_phase_istft_f32(*args(None, 0)) != 0                       # no phase: that is onssen_mask_istft_f32
    assert lib.dll.onssen_phase_istft_f32(*args(P(phases) + 4, B * T * F * 2)) != 0    # (re, im) pairs are read as 8-byte words
    assert lib.dll.onssen_phase_istft_f32(*args(P(phases), B * T * F * 2 + 1)) != 0
