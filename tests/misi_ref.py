"""MISI (multiple input spectrogram inversion) restated in float64 on the NumPy oracle's transforms -- the reference of
tests/test_emu_misi.py, tests/test_misi_api.py and tests/test_gpu_misi.py.

    s_c^(0)  = istft(A_c * p_c^(0))                           A_c the estimated magnitudes, p^(0) the starting phases
    u_c      = s_c^(k) + (x - sum_j s_j^(k)) / C              the mixture's residual, spread evenly
    p_c      = Z_c / |Z_c|,  Z_c = stft(u_c);  1 where Z_c = 0
    s_c^(k+1) = istft(A_c * p_c)

``stft64`` is ``oracle.np_oracle.stft`` without its two roundings (the float32 cast of the signal, the complex64 cast of the
spectrum): the same framing, window and transform in float64.  ``oracle.np_oracle.istft`` is float64 already."""
import numpy as np

from oracle import np_oracle as O


def stft64(sig, n_fft, hop):
    """(T, F) complex128: O.stft's framing (centred, reflect padding, periodic Hann, 1 + len // hop frames) in float64."""
    y = np.pad(np.asarray(sig, dtype=np.float64), n_fft // 2, mode="reflect")
    n_frames = 1 + (len(y) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    return np.fft.rfft(y[idx] * O.hann_periodic(n_fft)[None, :], axis=1)


def misi_spectra(mix, est, n_fft, hop):
    """mix (n,), est (C, n) -> Z (C, T, F) complex128: the spectra of u_c = est_c + (mix - sum_j est_j) / C, sum in index order."""
    mix, est = np.asarray(mix, dtype=np.float64), np.asarray(est, dtype=np.float64)
    C = est.shape[0]
    total = est[0].copy()
    for j in range(1, C):
        total = total + est[j]
    d = (mix - total) / C
    return np.stack([stft64(est[c] + d, n_fft, hop) for c in range(C)])


def unit(Z):
    """Z / |Z| as (..., 2) float64, (1, 0) where Z = 0."""
    h = np.abs(Z)
    nz = h > 0
    safe = np.where(nz, h, 1.0)
    return np.stack([np.where(nz, Z.real / safe, 1.0), np.where(nz, Z.imag / safe, 0.0)], -1)


def misi_phase(mix, est, n_fft, hop):
    """(C, T, F, 2) float64 unit phase vectors of one utterance, and |Z| (C, T, F)."""
    Z = misi_spectra(mix, est, n_fft, hop)
    return unit(Z), np.abs(Z)


def misi(mag, phase0, mix, hop, iters):
    """mag (C, T, F) real magnitudes, phase0 (C, T, F) complex unit phases, mix (n,) -> [s^(0), ..., s^(iters)], each (C, n)
    float64."""
    mag = np.asarray(mag, dtype=np.float64)
    C, _, F = mag.shape
    n_fft, n = 2 * (F - 1), len(mix)
    rebuild = lambda p: np.stack([O.istft(mag[c] * p[c], hop, n) for c in range(C)])
    est = [rebuild(np.asarray(phase0, dtype=np.complex128))]
    for _ in range(iters):
        p, _ = misi_phase(mix, est[-1], n_fft, hop)
        est.append(rebuild(p[..., 0] + 1j * p[..., 1]))
    return est


def si_sdr(est, ref):
    """Scale-invariant SDR in dB of est (n,) against ref (n,), float64."""
    est, ref = np.asarray(est, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    est, ref = est - est.mean(), ref - ref.mean()
    proj = np.dot(est, ref) / np.dot(ref, ref) * ref
    return 10.0 * np.log10(np.dot(proj, proj) / np.dot(est - proj, est - proj))
