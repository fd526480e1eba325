"""float64 restatements for the uPIT tests (tests/test_emu_upit.py, test_upit_api.py, test_gpu_upit.py): the pair matrix of the
utterance-level permutation-invariant mask loss, the totals per assignment, the minimum with the index of its first occurrence,
and the gradient's sign.  Definitions as csrc/loss_upit.inc states them."""
from itertools import permutations
from math import factorial

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
# bins per utterance: one bin (31 empty slices, and the clipping makes ties); 3 * 129, a multiple of neither 4 nor 256; 67 * 129,
# more than 256 bins in each of the 32 slices
TFS = [1, 387, 8643]
# (S, TF, psa)
SHAPES = [(S, TF, psa) for S in (2, 3, 4) for TF in TFS for psa in (False, True)]
# beyond SHAPES: a slice longer than one pass of the workgroup (4 * 256 bins), with a tail of 1 bin in the last pass
LONG = (2, 32 * 1028 + 1, True)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def perms(S):
    return list(permutations(range(S)))


def targets(x, src, cos=None):
    """(S, B, TF) float64: mag_s_j (MSA) or min(x, relu(mag_s_j cos_j)) (PSA)."""
    if cos is None:
        return f64(src)
    return np.minimum(f64(x)[None], np.maximum(f64(src) * f64(cos), 0.0))


def pair_matrix(masks, x, src, cos=None):
    """(B, S, S): pair[b][k][j] = sum_bins |m_k x - t_j|; masks (S, B, TF), x (B, TF), src / cos (S, B, TF)."""
    t = targets(x, src, cos)
    est = f64(masks) * f64(x)[None]
    return np.abs(est[:, None] - t[None, :]).sum(-1).transpose(2, 0, 1)


def totals(pair):
    """(B, S!): total[b][p] = sum_k pair[b][k][p[k]], p in the order of itertools.permutations."""
    S = pair.shape[1]
    return np.stack([sum(pair[:, k, p[k]] for k in range(S)) for p in perms(S)], 1)


def best(pair):
    """(out (B,), perm (B,)): the minimum total and the index of its first occurrence."""
    tot = totals(pair)
    return tot.min(1), tot.argmin(1)


def grad_sign(masks, x, src, cos, perm):
    """(S, B, TF): sign(m_k x - t_{p[k]}), p = assignment number perm[b]; sign(0) = 0."""
    t = targets(x, src, cos)
    S, B = t.shape[:2]
    table = perms(S)
    out = np.empty_like(t)
    for b in range(B):
        p = table[int(perm[b])]
        for k in range(S):
            out[k, b] = np.sign(f64(masks[k, b]) * f64(x[b]) - t[p[k], b])
    return out


def pair_bound(x, src, cos=None):
    """(B, S) per target j: 1e-5 * sum_bins (x + t_j).  The residual m x - t is one fused multiply-add of |m x| <= x and t
    (after one rounding of s c for PSA): its absolute value is off by about eps32 (x + t) at worst, the sums are fp64 and the
    result is rounded to fp32 once -- a margin of two orders."""
    t = targets(x, src, cos)
    return 1e-5 * (f64(x)[None] + t).sum(-1).T


def out_bound(x, src, cos, perm):
    """(B,): the sum of the S entries' bounds along assignment number perm[b] -- every target once, whatever the assignment."""
    return pair_bound(x, src, cos).sum(1)


_CASES = {}


def loss_case(S, TF, seed, psa):
    """float32 maps of one loss call with B = S! rows: masks (S, B, TF), x (B, TF), src (S, B, TF), cos (S, B, TF) or None.
    Row b has the b-th assignment planted: m_k = clip(t_{p[k]} / x + U(-0.05, 0.05), 0, 1).  As far as TF reaches (as
    tests/enhance_ref.py: loss_case): bin 0 has a residual of exactly 0 for every mask, bin 1 a negative s c (the relu clamps
    the target to 0), bin 2 has s c > x (the min clamps it to x).  Computed once per key and shared: do not write into it."""
    key = (S, TF, seed, psa)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed)
    B = factorial(S)
    x = (np.abs(rng.standard_normal((B, TF))) + 1e-3).astype(np.float32)
    src = (x[None] * rng.random((S, B, TF)) * 1.5).astype(np.float32)
    cos = np.cos(rng.uniform(-np.pi, np.pi, (S, B, TF))).astype(np.float32) if psa else None
    plant = [(2.0, 1.0, 1.0), (1.0, 0.75, -0.5), (0.5, 2.0, 0.875)]          # (x, s, c) of bins 0, 1, 2
    for e, (x_, s_, c_) in enumerate(plant[:TF]):
        x[:, e], src[:, :, e] = x_, s_
        if psa:
            cos[:, :, e] = c_
    t = targets(x, src, cos)
    masks = np.empty((S, B, TF), np.float32)
    for b, p in enumerate(perms(S)):
        for k in range(S):
            masks[k, b] = np.clip(t[p[k], b] / f64(x[b]) + rng.uniform(-0.05, 0.05, TF), 0.0, 1.0)
    if TF > 0:
        masks[:, :, 0] = (t[0, :, 0] / f64(x[:, 0])).astype(np.float32)      # 0.5 * 2 - 1 = 0 exactly (every target of bin 0 is 1)
    for a in (x, src, masks) + ((cos,) if psa else ()):
        a.setflags(write=False)
    c = _CASES[key] = dict(masks=masks, x=x, src=src, cos=cos)
    return c


def margin(pair):
    """(B,): the second smallest total minus the smallest, per row."""
    tot = np.sort(totals(pair), 1)
    return tot[:, 1] - tot[:, 0]
