"""misi_phase_kernel (csrc/misi.inc) and the ragged phase-aware iSTFT in the host-side build: the half-step against the float64
restatement in tests/misi_ref.py, degenerate inputs, ragged batches, whole MISI iterations through the C ABI, refusals."""
import numpy as np
import pytest

from tests import misi_cases as MC
from tests import misi_ref as R
from tests.emu_build import load_emu


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return a.ctypes.data


def misi_phase(lib, mix, est, n_fft, hop, lengths=None):
    B, C, n = est.shape
    T, F = 1 + n // hop, n_fft // 2 + 1
    out = np.full((C, B, T, F, 2), np.nan, np.float32)
    lens = None if lengths is None else np.asarray(lengths, np.int32)
    lib.misi_phase(P(mix), mix.strides[0] // 4, P(est), est.strides[0] // 4, est.strides[1] // 4, B, C, n, n_fft, hop, P(out), None,
                   n_per_utt=None if lens is None else P(lens))
    return out


def phase_istft(lib, ri, masks, phases, n_fft, hop, length, frames=None, lengths=None):
    B, T, F, C = masks.shape
    out = np.full((B, C, length), np.nan, np.float32)
    fr = None if frames is None else np.asarray(frames, np.int32)
    ln = None if lengths is None else np.asarray(lengths, np.int32)
    lib.phase_istft(P(ri), P(masks), T * F * C, 1, F * C, C, P(phases), B * T * F * 2, B, C, T, n_fft, hop, length, P(out), None,
                    frames=None if fr is None else P(fr), lengths=None if ln is None else P(ln))
    return out


def mask_istft(lib, ri, masks, n_fft, hop, length):
    B, T, F, C = masks.shape
    out = np.full((B, C, length), np.nan, np.float32)
    lib.mask_istft(P(ri), P(masks), T * F * C, 1, F * C, C, B, C, T, n_fft, hop, length, P(out), None)
    return out


# ------------------------------------------------------------------------------------------------- (a) the half-step
@pytest.mark.parametrize("n_fft,hop,n,C", MC.SHAPES)
def test_misi_phase_matches_fp64_reference(lib, n_fft, hop, n, C):
    k = MC.case(n_fft, hop, n, C)
    got = misi_phase(lib, k.mix, k.est, n_fft, hop)
    MC.check_phase(got, MC.reference_spectra(k), f"n_fft {n_fft} hop {hop} n {n} C {C}")


def test_misi_phase_takes_strided_estimates_and_more_than_four_speakers(lib):
    """C = 5 takes the 8-estimate instantiation (three of its loads repeat estimate 4 and enter the sum as 0); the estimates sit
    in a larger buffer with their own batch and speaker strides."""
    k = MC.case(256, 64, 768, 2)
    rng = np.random.default_rng(5)
    big = np.full((2, 6, 800), np.nan, np.float32)
    big[:, :5, :768] = (0.2 * rng.standard_normal((2, 5, 768))).astype(np.float32)
    est = big[:, :5, :768]
    got = misi_phase(lib, k.mix, est, 256, 64)
    Z = np.stack([R.misi_spectra(k.mix[b], est[b], 256, 64) for b in range(2)])
    MC.check_phase(got, Z, "C 5, strided")


# ------------------------------------------------------------------------------------------------- (b) degenerate inputs
def test_zero_estimate_and_whole_mixture(lib):
    """est_0 = 0, est_1 = mix: no residual, so u_0 = 0 -- plane 0 is (1, 0) everywhere -- and u_1 = mix: plane 1 is the
    mixture's own phase, stft_ri / |stft_ri| of onssen_stft_logmag_f32, under rule (a) (reference: the float64 spectrum)."""
    k = MC.case(256, 64, 768, 2)
    est = np.ascontiguousarray(np.stack([np.zeros_like(k.mix), k.mix], 1))
    got = misi_phase(lib, k.mix, est, 256, 64)
    assert (got[0, ..., 0] == 1).all() and (got[0, ..., 1] == 0).all()
    B, T, F = k.B, k.T, k.F
    logmag, ri = np.zeros((B, T, F), np.float32), np.zeros((B, T, F, 2), np.float32)
    lib.stft_logmag(P(k.mix), B, k.n, k.n, 256, 64, 1e-7, P(logmag), P(ri), None)
    Zk = (ri[..., 0].astype(np.float64) + 1j * ri[..., 1].astype(np.float64))[:, None]          # (B, 1, T, F)
    MC.check_phase(got[1:], Zk, "plane 1 against onssen_stft_logmag_f32")
    # (that spectrum is rounded to complex64; the float64 spectrum is the reference proper)
    Z64 = np.stack([R.stft64(k.mix[b], 256, 64) for b in range(B)])[:, None]
    MC.check_phase(got[1:], Z64, "plane 1 against the float64 spectrum")


def test_all_zero_inputs(lib):
    mix, est = np.zeros((2, 768), np.float32), np.zeros((2, 3, 768), np.float32)
    got = misi_phase(lib, mix, est, 256, 64)
    assert (got[..., 0] == 1).all() and (got[..., 1] == 0).all()


# ------------------------------------------------------------------------------------------------- (c) ragged batches
RAG_LENGTHS = (1500, 1100, 700)


def ragged_inputs():
    n_fft, hop, n, C = 256, 100, 1500, 3
    k = MC.case(n_fft, hop, n, C, B=3)
    mix, est = k.mix.copy(), k.est.copy()
    for b, nb in enumerate(RAG_LENGTHS):          # nothing beyond a row's own length may be read
        mix[b, nb:] = np.nan
        est[b, :, nb:] = np.nan
    return k, mix, est


def test_misi_phase_ragged_rows_are_their_batch1_bytes(lib):
    k, mix, est = ragged_inputs()
    got = misi_phase(lib, mix, est, k.n_fft, k.hop, lengths=RAG_LENGTHS)
    assert np.isfinite(got).all()
    for b, nb in enumerate(RAG_LENGTHS):
        Tb = 1 + nb // k.hop
        one = misi_phase(lib, np.ascontiguousarray(mix[b:b + 1, :nb]), np.ascontiguousarray(est[b:b + 1, :, :nb]), k.n_fft, k.hop)
        assert one.shape[2] == Tb
        assert got[:, b, :Tb].tobytes() == one[:, 0].tobytes(), b
        assert (got[:, b, Tb:, :, 0] == 1).all() and (got[:, b, Tb:, :, 1] == 0).all(), b


def test_phase_istft_ragged_rows_are_their_batch1_bytes(lib):
    k, _, _ = ragged_inputs()
    rng = np.random.default_rng(11)
    p = rng.standard_normal((k.C, k.B, k.T, k.F, 2))
    phases = np.ascontiguousarray(p / np.linalg.norm(p, axis=-1, keepdims=True), dtype=np.float32)
    ri, masks = k.ri.copy(), k.masks.copy()
    frames = [1 + nb // k.hop for nb in RAG_LENGTHS]
    for b, Tb in enumerate(frames):
        ri[b, Tb:] = np.nan
        masks[b, Tb:] = np.nan
        phases[:, b, Tb:] = np.nan
    got = phase_istft(lib, ri, masks, phases, k.n_fft, k.hop, k.n, frames=frames, lengths=RAG_LENGTHS)
    for b, (Tb, nb) in enumerate(zip(frames, RAG_LENGTHS)):
        one = phase_istft(lib, np.ascontiguousarray(ri[b:b + 1, :Tb]), np.ascontiguousarray(masks[b:b + 1, :Tb]),
                          np.ascontiguousarray(phases[:, b:b + 1, :Tb]), k.n_fft, k.hop, nb)
        assert np.isfinite(one).all()
        assert got[b, :, :nb].tobytes() == one[0].tobytes(), b
        assert (got[b, :, nb:] == 0).all(), b


# ------------------------------------------------------------------------------------------------- (d) whole iterations
def run_iterations(lib, k, K):
    """K MISI iterations through the C ABI from the case's masks on the mixture's phase -> (B, C, n) float32."""
    est = mask_istft(lib, k.ri, k.masks, k.n_fft, k.hop, k.n)
    for _ in range(K):
        ph = misi_phase(lib, k.mix, est, k.n_fft, k.hop)
        est = phase_istft(lib, k.ri, k.masks, ph, k.n_fft, k.hop, k.n)
    return est


def reference_iterations(k, K):
    """The same in float64 (tests/misi_ref.py): magnitudes mask * |X| of the float32 spectrum the kernels read."""
    X = k.ri[..., 0].astype(np.float64) + 1j * k.ri[..., 1].astype(np.float64)
    out = []
    for b in range(k.B):
        mag = np.moveaxis(k.masks[b].astype(np.float64), -1, 0) * np.abs(X[b])[None]
        p0 = R.unit(X[b])
        out.append(R.misi(mag, np.stack([p0[..., 0] + 1j * p0[..., 1]] * k.C), k.mix[b], k.hop, K)[-1])
    return np.stack(out)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n_fft,hop,n,C", MC.SHAPES)
def test_whole_iterations_match_fp64_reference(lib, n_fft, hop, n, C, K):
    """K iterations (misi_phase, phase_istft, ...) against the float64 restatement.  A phase at a weak bin is ill-conditioned and
    its error passes through the next transform, so the bound is measured, not derived: the largest max |out - ref| on this
    build is MC.ITER_MEASURED_MAX (values per case below), the bound MC.ITER_BOUND is 4 x that -- the device's hypot and
    contraction differ from the host's.  Sanity ceiling: a value above 1e-4 max|ref| is a defect, not a tolerance.

    Measured on the host-side build, max |out - ref| (max |ref|):
      (256, 64, 768, 2)    K = 1: 2.709e-08 (0.524)   K = 3: 4.167e-08 (0.527)
      (256, 100, 1500, 3)  K = 1: 4.374e-08 (0.642)   K = 3: 8.452e-08 (0.623)
      (512, 128, 2048, 2)  K = 1: 4.242e-08 (0.672)   K = 3: 4.307e-08 (0.680)
      (1024, 256, 4096, 2) K = 1: 2.702e-08 (0.469)   K = 3: 3.008e-08 (0.470)
      (256, 64, 2000, 4)   K = 1: 4.439e-08 (0.539)   K = 3: 1.118e-07 (0.536)
    so MC.ITER_MEASURED_MAX = 1.118e-07 and MC.ITER_BOUND = 4.472e-07 -- about one float32 rounding of the output per iteration,
    far below the 1e-4 max|ref| ceiling.
    """
    k = MC.case(n_fft, hop, n, C)
    out, ref = run_iterations(lib, k, K), reference_iterations(k, K)
    err, top = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"n_fft {n_fft} hop {hop} n {n} C {C} K {K}: max |out - ref| {err:.3e}, max |ref| {top:.3f}, bound {MC.ITER_BOUND:.3e}")
    assert np.isfinite(out).all()
    assert err <= 1e-4 * top
    assert err <= MC.ITER_BOUND


# ------------------------------------------------------------------------------------------------- (e) refusals
E_ARG, E_ALIGN = -1, -3          # ONSSEN_E_ARG, ONSSEN_E_ALIGN (include/onssen_hip.h)


def test_misi_phase_refusals(lib):
    k = MC.case(256, 64, 768, 2)
    B, C, n = k.est.shape
    out = np.zeros((C, B, k.T, k.F, 2), np.float32)
    lens = np.full(B, n, np.int32)
    f, fr = lib.dll.onssen_misi_phase_f32, lib.dll.onssen_misi_phase_ragged_f32

    def args(mix=P(k.mix), est=P(k.est), C=C, n=n, n_fft=256, hop=64, phase=P(out)):
        return (mix, n, est, C * n, n, B, C, n, n_fft, hop, phase, None)

    def rargs(**kw):
        a = args(**kw)
        return a[:8] + (P(lens),) + a[8:]

    assert f(*args()) == 0 and fr(*rargs()) == 0
    bad = [dict(mix=None), dict(est=None), dict(phase=None), dict(C=1), dict(C=9), dict(hop=0), dict(hop=-3), dict(hop=257),
           dict(n=128), dict(n_fft=128), dict(n_fft=2048), dict(n_fft=300)]
    for kw in bad:
        assert f(*args(**kw)) == E_ARG, kw
        assert fr(*rargs(**kw)) == E_ARG, kw
    a = list(rargs())
    a[8] = None
    assert fr(*a) == E_ARG                                        # the ragged form without its lengths
    assert f(*args(phase=P(out) + 4)) == E_ALIGN and fr(*rargs(phase=P(out) + 4)) == E_ALIGN
    assert not np.isnan(out).any()


def test_phase_istft_refusals(lib):
    """The ragged form refuses what the uniform form refuses, and missing extents; the uniform form's returns are unchanged."""
    from tests.phase_istft_cases import case
    _, ri, masks, phases = case(256, 64, 768)
    B, T, F, C = masks.shape
    out = np.zeros((B, C, 768), np.float32)
    fr, ln = np.full(B, T, np.int32), np.full(B, 768, np.int32)
    uni = lambda ph, p_sc: (P(ri), P(masks), T * F * C, 1, F * C, C, ph, p_sc, B, C, T, 256, 64, 768, P(out), None)
    rag = lambda ph, p_sc, f=P(fr), l=P(ln): (P(ri), P(masks), T * F * C, 1, F * C, C, ph, p_sc, B, C, T, f, 256, 64, 768, l, P(out), None)
    u, r = lib.dll.onssen_phase_istft_f32, lib.dll.onssen_phase_istft_ragged_f32
    assert u(*uni(P(phases), B * T * F * 2)) == 0 and r(*rag(P(phases), B * T * F * 2)) == 0
    assert u(*uni(None, 0)) == E_ARG and r(*rag(None, 0)) == E_ARG
    assert u(*uni(P(phases) + 4, B * T * F * 2)) == E_ALIGN and r(*rag(P(phases) + 4, B * T * F * 2)) == E_ALIGN
    assert u(*uni(P(phases), B * T * F * 2 + 1)) == E_ALIGN and r(*rag(P(phases), B * T * F * 2 + 1)) == E_ALIGN
    assert r(*rag(P(phases), B * T * F * 2, f=None)) == E_ARG and r(*rag(P(phases), B * T * F * 2, l=None)) == E_ARG
