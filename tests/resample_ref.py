"""Float64 reference and error bound of the polyphase resampler (shared by tests/test_emu_resample.py, tests/test_gpu_resample.py
and tests/test_gpu_edinburgh.py; not a test module).

reference   scipy.signal.resample_poly(float64(x) [- float64(sub)], up, down) -- default window: firwin(2 half + 1, 1 / M, kaiser 5)
absum[m]    sum_n |x[n]| |h[m down - n up + half]| from the definition (include/onssen_hip.h), the scale of the rounding errors
bound       |y - ref| <= 2^-24 |ref| + 1e-13 absum
            one round-to-nearest to fp32 is at most half an ulp, <= 2^-24 |ref|; an fp64 sum of at most 61 products (48 -> 16 kHz;
            56 for 44.1 -> 16 kHz) in any order stays below 61 * 2^-53 absum = 7e-15 absum on either side.  A ratio with more
            terms per output (the unstaged kernel's cases) gets 2 * terms * 2^-53 in place of 1e-13 where that is larger: the
            library's sum and SciPy's each carry `terms` roundings."""
from math import gcd

import numpy as np


def reduced(up, down):
    g = gcd(int(up), int(down))
    return int(up) // g, int(down) // g


def taps(up, down):
    """(h, half) of a ratio, by SciPy (resample_poly's own design)."""
    from scipy.signal import firwin
    up, down = reduced(up, down)
    M = max(up, down)
    if M == 1:
        return np.ones(1), 0
    half = 10 * M
    return up * firwin(2 * half + 1, 1.0 / M, window=("kaiser", 5.0)), half


def n_out(n_in, up, down):
    up, down = reduced(up, down)
    return -(-int(n_in) * up // down)


def reference(x, up, down, sub=None):
    from scipy.signal import resample_poly
    v = np.asarray(x, np.float64)
    if sub is not None:
        v = v - np.asarray(sub, np.float64)
    up, down = reduced(up, down)
    return v.copy() if up == down else resample_poly(v, up, down)


def direct(x, up, down, ms, absolute=False):
    """The definition's sum at the output indices ``ms`` in float64 (absolute: of |x| |h|, the error scale)."""
    up, down = reduced(up, down)
    h, half = taps(up, down)
    v = np.asarray(x, np.float64)
    if absolute:
        v, h = np.abs(v), np.abs(h)
    L = 2 * half // up + 1
    c = np.asarray(ms, np.int64) * down + half
    j = np.arange(L, dtype=np.int64)
    n = (c // up)[:, None] - j[None, :]
    k = (c % up)[:, None] + j[None, :] * up
    ok = (n >= 0) & (n < len(v)) & (k <= 2 * half)
    return np.where(ok, v[np.clip(n, 0, len(v) - 1)] * h[np.clip(k, 0, 2 * half)], 0.0).sum(axis=1)


def absum(x, up, down, ms, sub=None):
    v = np.asarray(x, np.float64)
    if sub is not None:
        v = v - np.asarray(sub, np.float64)
    return direct(v, up, down, ms, absolute=True)


def terms(up, down):
    up, down = reduced(up, down)
    return 2 * taps(up, down)[1] // up + 1


def ratio(y, ref, ab, up=1, down=3):
    """max over the outputs of |y - ref| / bound; a test asserts it is <= 1 (and prints it)."""
    coeff = max(1e-13, 2.0 * terms(up, down) * 2.0 ** -53)
    err = np.abs(np.asarray(y, np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + coeff * ab
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0
