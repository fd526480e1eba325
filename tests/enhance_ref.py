"""float64 restatements for the enhancement tests (tests/test_emu_enhance.py, test_enhance_api.py, test_gpu_enhance.py): the two
losses of onssen/loss/loss_mask.py with their gradients in closed form (no autograd), the label maps of
onssen/data/daps_enhance.py:104-106, and the reconstruction ``istft(m * exp(i angle(X)))`` through the NumPy oracle.
tests/test_enhance_api.py pins the losses against float64 torch autograd of the literal upstream expressions."""
import numpy as np

from oracle import np_oracle as O

EPS32 = float(np.finfo(np.float32).eps)
# (B, TF) of the loss tests: TF no multiple of 256 or of the 32 slices; fewer bins than slices (empty slices); one bin into the
# second stride of a slice
LOSS_SHAPES = [(3, 903), (1, 5), (2, 32 * 256 + 1)]


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- losses ----------------------------------------------------------------------------------------------------------------
def msa(est, clean):
    """(per_utt (B,), total): per_utt[b] = sum_bins (est - clean)^2, total = MSELoss's mean over all bins."""
    d = f64(est) - f64(clean)
    per_utt = (d * d).reshape(d.shape[0], -1).sum(1)
    return per_utt, per_utt.sum() / d.size


def msa_grad(est, clean, g=1.0):
    """d (g * total) / d est = g * 2 / (B T F) * (est - clean)."""
    d = f64(est) - f64(clean)
    return float(g) * 2.0 / d.size * d


def psa_target(x, s, c):
    return np.minimum(f64(x), np.maximum(f64(s) * f64(c), 0.0))


def psa(mask, x, s, c):
    """per_utt (B,) = sum_bins |mask x - min(x, relu(s c))|."""
    r = f64(mask) * f64(x) - psa_target(x, s, c)
    return np.abs(r).reshape(r.shape[0], -1).sum(1)


def psa_grad(mask, x, s, c, g):
    """d (sum_b g[b] per_utt[b]) / d mask = g[b] x sign(mask x - t), sign(0) = 0."""
    r = f64(mask) * f64(x) - psa_target(x, s, c)
    gb = f64(g).reshape((-1,) + (1,) * (r.ndim - 1))
    return gb * f64(x) * np.sign(r)


def loss_case(B, TF, seed):
    """float32 maps (B, TF) of one loss call: est / mask, x = mag_noisy, s = mag_clean, c = cos_diff.  Planted in every row, as
    far as TF reaches: bin 0 has mask x - t = 0 exactly (0.5 * 2 - min(2, 1 * 1)), bin 1 a negative s c (the relu clamps the
    target to 0), bin 2 has s c > x (the min clamps it to x)."""
    rng = np.random.default_rng(seed)
    x = (np.abs(rng.standard_normal((B, TF))) + 1e-3).astype(np.float32)
    s = (x * rng.random((B, TF)) * 1.5).astype(np.float32)
    c = np.cos(rng.uniform(-np.pi, np.pi, (B, TF))).astype(np.float32)
    est = rng.random((B, TF)).astype(np.float32)
    plant = [(0.5, 2.0, 1.0, 1.0), (0.25, 1.0, 0.75, -0.5), (0.75, 0.5, 2.0, 0.875)]
    for k, (m_, x_, s_, c_) in enumerate(plant[:TF]):
        est[:, k], x[:, k], s[:, k], c[:, k] = m_, x_, s_, c_
    return dict(est=est, x=x, s=s, c=c)


# ---- labels ----------------------------------------------------------------------------------------------------------------
def labels(noisy_ri, clean_ri):
    """(|X|, |S|, cos(angle X - angle S)) in float64 from the float32 (..., 2) spectra."""
    X = f64(noisy_ri[..., 0]) + 1j * f64(noisy_ri[..., 1])
    S = f64(clean_ri[..., 0]) + 1j * f64(clean_ri[..., 1])
    return np.abs(X), np.abs(S), np.cos(np.angle(X) - np.angle(S))


def labels_case(n_bins, seed):
    """Two (n_bins, 2) float32 spectra; planted as far as n_bins reaches: bin 0 has X = 0 (angle 0, magnitude 0), bin 1 a clean
    value on the negative real axis (atan2f = pi), bin 2 both (then cos_diff = cos(-pi) = -1)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n_bins, 2)).astype(np.float32)
    b = rng.standard_normal((n_bins, 2)).astype(np.float32)
    a[0] = (0.0, 0.0)
    if n_bins > 1:
        b[1] = (-1.5, 0.0)
    if n_bins > 2:
        a[2], b[2] = (0.0, 0.0), (-0.25, 0.0)
    return a, b


# ---- magnitude reconstruction ----------------------------------------------------------------------------------------------
def mag_reference(ri, mags, hop, length, frames=None, lengths=None):
    """(B, C, length) float64: O.istft(m_c * exp(i angle(X)), hop, length) per channel, X the float32 spectrum the kernel reads
    (np.angle(0) = 0: a silent bin keeps the magnitude on the real axis).  ``frames`` / ``lengths``: row b is its first frames[b]
    frames and lengths[b] samples, zeros after them."""
    X = f64(ri[..., 0]) + 1j * f64(ri[..., 1])
    B, T, F, C = mags.shape
    out = np.zeros((B, C, length))
    for b in range(B):
        Tb = T if frames is None else int(frames[b])
        nb = length if lengths is None else int(lengths[b])
        unit = np.exp(1j * np.angle(X[b, :Tb]))
        for c in range(C):
            out[b, c, :nb] = O.istft(f64(mags[b, :Tb, :, c]) * unit, hop, nb)
    return out


def mag_atol(ref):
    """2e-6 is the project's iSTFT grade (tests/test_emu_kernels.py); 6 eps32 max|ref| more for the float32 hypotf, the two
    float32 quotients and the product with the magnitude, none of which the float64 reference rounds."""
    return 2e-6 + 6 * EPS32 * np.abs(ref).max()


def mag_case(n_fft, hop, n, C, B=2):
    """ri (B,T,F,2) float32 -- real STFTs of synthetic mixtures with some bins planted exactly 0 -- and magnitudes (B,T,F,C)."""
    from tests.phase_istft_cases import case
    _, ri, mags, _ = case(n_fft, hop, n, C, B)
    ri = ri.copy()
    ri[:, 1::3, 5::17] = 0.0           # silent bins inside the band
    ri[:, 2, 0] = 0.0                  # a silent DC bin and a silent Nyquist bin
    ri[:, 3, -1] = 0.0
    return ri, (2.0 * mags).astype(np.float32)
