"""NumPy fp64 restatement of the SI-SNR permutation-invariant training loss (onssen/loss/loss_e2e.py:45-87 as restated in
onssen_amd/loss.py: sisnr, si_snr_loss), with ragged rows, and the inputs the SI-SNR PIT tests share.

For estimates x_i and references s_j, each (N, S), eps = 1e-8, row b over its first lengths[b] samples:
  x~ = x - mean(x), s~ = s - mean(s), D = <x~, s~>, E = |s~|^2 + eps, a = D / E, t = a s~, n = |x~ - t|
  v(i, j) = 20 log10(eps + |t| / (n + eps))
  V_b = max_p (1/k) sum_i v(i, p(i)) over itertools.permutations(range(k)), the first maximum wins; loss = -sum_b V_b / N.
Gradient of v with respect to x (a norm that is exactly zero has subgradient zero, sign(0) = 0, as ATen):
  K (cT s~ - cN (x~ - a (1 + eps / E) s~)),  K = 20 / (ln 10 u), u = eps + |t| / (n + eps),
  cT = sign(a) |s~| / (E (n + eps)),  cN = |t| / ((n + eps)^2 n)
which is A x + B s + C with A = -K cN, B = K (cT + cN a (1 + eps / E)), C = -(A mean(x) + B mean(s))."""
from itertools import permutations

import numpy as np

EPS = 1e-8
SHAPES_S = (5, 63, 64, 65, 257, 511, 512, 513, 1030)      # 512 = the samples one workgroup takes (csrc/loss_sisnr.inc: CHMIN)
S_ABOVE_CHUNK_GROWTH = 64 * 512 + 5                       # beyond it a row's chunks grow instead of their number


def pair(x, s):
    """One estimate against one reference (1-D fp64) -> (v, gradient, |A x|, |B s|, |C|)."""
    mx, ms = x.mean(), s.mean()
    xt, st = x - mx, s - ms
    D, S2 = float(xt @ st), float(st @ st)
    E = S2 + EPS
    a = D / E
    t = a * st
    T, n = float(np.linalg.norm(t)), float(np.linalg.norm(xt - t))
    u = EPS + T / (n + EPS)
    v = 20.0 * np.log10(u)
    K = 20.0 / np.log(10.0) / u
    f = 1.0 + EPS / E
    cT = np.sign(a) * np.sqrt(S2) / (E * (n + EPS)) if T > 0.0 else 0.0
    cN = T / ((n + EPS) ** 2 * n) if n > 0.0 else 0.0
    g = K * (cT * st - cN * (xt - a * f * st))
    A, B = -K * cN, K * (cT + cN * a * f)
    return v, g, np.abs(A * x), np.abs(B * s), abs(A * mx + B * ms)


def reference(ests, refs, lengths=None, g_value=None, g_total=1.0):
    """ests, refs: k arrays (N, S).  -> dict(value (N,), perm (N,), loss, margin (N,): best minus second-best assignment in dB,
    grad (k, N, S): gradient of sum_b g_value[b] V_b + g_total loss with respect to the estimates, terms (k, N, S):
    |A x| + |B s| + |C| of that gradient)."""
    ests = [np.asarray(e, np.float64) for e in ests]
    refs = [np.asarray(r, np.float64) for r in refs]
    k, (N, S) = len(ests), ests[0].shape
    lengths = [S] * N if lengths is None else [int(v) for v in lengths]
    g_value = np.zeros(N) if g_value is None else np.asarray(g_value, np.float64)
    perms = list(permutations(range(k)))
    value, perm, margin = np.zeros(N), np.zeros(N, np.int64), np.full(N, np.inf)
    grad, terms = np.zeros((k, N, S)), np.zeros((k, N, S))
    for b in range(N):
        L = lengths[b]
        tab = [[pair(ests[i][b, :L], refs[j][b, :L]) for j in range(k)] for i in range(k)]
        per_perm = np.array([sum(tab[i][p[i]][0] for i in range(k)) / k for p in perms])
        perm[b] = int(np.argmax(per_perm))                   # the first maximum
        value[b] = per_perm[perm[b]]
        if len(perms) > 1:
            margin[b] = value[b] - np.sort(per_perm)[-2]
        w = (g_value[b] - g_total / N) / k
        for i in range(k):
            _, g, ax, bs, c = tab[i][perms[perm[b]][i]]
            grad[i, b, :L] = w * g
            terms[i, b, :L] = abs(w) * (ax + bs + c)
    return dict(value=value, perm=perm, loss=-value.sum() / N, margin=margin, grad=grad, terms=terms)


def planted(k, N, S, seed, noise=0.3):
    """refs = N(0, 1); est_i = the row-wise randomly permuted references + noise N(0, 1) + a DC offset of 0.05.
    -> (ests (k, N, S), refs (k, N, S)) float32"""
    rng = np.random.default_rng(seed)
    refs = rng.standard_normal((k, N, S)).astype(np.float32)
    ests = np.empty_like(refs)
    for b in range(N):
        p = rng.permutation(k)
        for i in range(k):
            ests[i, b] = refs[p[i], b] + noise * rng.standard_normal(S).astype(np.float32) + np.float32(0.05)
    return ests, refs


def planted_clear(k, N, S, seed, noise=0.3):
    """``planted`` with the first seed from ``seed`` on whose best and second-best assignments differ by at least 1 dB in every
    row (five samples of four speakers do not always separate that clearly) -> (ests, refs, reference(ests, refs))."""
    for s in range(seed, seed + 50):
        ests, refs = planted(k, N, S, s, noise)
        ref = reference(ests, refs)
        if (ref["margin"] >= 1.0).all():
            return ests, refs, ref
    raise AssertionError(f"no seed in [{seed}, {seed + 50}) separates k={k} N={N} S={S} by 1 dB")


def ulp32(x):
    """Spacing of float32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_values(got_value, got_perm, got_total, ref, tag=""):
    """Item 1 of the issue: per-row value within 2 fp32 ulps of |V_ref|, loss within 2 ulps of max_b |V_b|, permutation equal
    (after asserting the 1 dB margin of the restatement)."""
    ev = np.abs(np.asarray(got_value, np.float64) - ref["value"]) / ulp32(ref["value"])
    et = abs(float(got_total) - ref["loss"]) / float(ulp32(np.abs(ref["value"]).max()))
    print(f"{tag}: value error {ev.max():.2f} ulp, loss error {et:.2f} ulp (bound 2), worst margin {ref['margin'].min():.2f} dB, "
          f"largest value {ref['value'].max():.1f} dB")
    assert (ref["margin"] >= 1.0).all(), ref["margin"]
    assert np.array_equal(np.asarray(got_perm, np.int64), ref["perm"])
    assert ev.max() <= 2.0 and et <= 2.0


def check_grad(got, ref, tag=""):
    """Item 2 of the issue: |g - g_ref| <= 2^-23 |g_ref| + 1e-9 (|A x| + |B s| + |C|), elementwise."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref["grad"])
    bound = 2.0 ** -23 * np.abs(ref["grad"]) + 1e-9 * ref["terms"]
    live = bound > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    # the second figure: the error in units of the terms alone (what the fp64 coefficients cost)
    on_terms = float((np.maximum(err - 2.0 ** -24 * np.abs(ref["grad"]), 0.0)[live] / ref["terms"][live]).max()) if live.any() else 0.0
    print(f"{tag}: gradient error {worst:.3f} of its bound; beyond one rounding: {on_terms:.2e} of |A x| + |B s| + |C| (allowed 1e-9)")
    assert np.isfinite(got).all()
    assert (err <= bound).all()
