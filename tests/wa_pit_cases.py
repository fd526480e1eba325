"""Inputs and float64 reference of the waveform-approximation loss tests (tests/test_emu_wa_pit.py, tests/test_gpu_wa_pit.py):

    D[b,i,j] = sum_{n < n_b} |est_i[n] - ref_j[n]|
    V[b]     = min over permutations p of sum_i D[b,i,p(i)] / (C n_b)       lexicographic order, the first minimum wins
    d est_i[n] = gV[b] sign(est_i[n] - ref_p(i)[n]) / (C n_b)               0 at equality and at n >= n_b

Every case is built once per process and must be left unchanged."""
import functools
import itertools

import numpy as np

B = 3


class Case:
    pass


def reference(est, ref, lengths, g_value):
    """V (B,) float64, the index of the winning permutation per row, the permutations, the gradient (B,C,n) float64 and the
    relative gap between the best and the second-best permutation value per row."""
    est, ref = np.asarray(est, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nB, C, n = est.shape
    perms = list(itertools.permutations(range(C)))                  # lexicographic
    V, index, grad, gap = np.zeros(nB), [], np.zeros_like(est), np.full(nB, np.inf)
    for b in range(nB):
        nb = n if lengths is None else int(lengths[b])
        D = np.abs(est[b, :, None, :nb] - ref[b, None, :, :nb]).sum(-1)
        vals = [sum(D[i, p[i]] for i in range(C)) / (C * nb) for p in perms]
        best = 0
        for q in range(1, len(perms)):
            if vals[q] < vals[best]:
                best = q
        V[b] = vals[best]
        index.append(best)
        if len(perms) > 1:
            gap[b] = (sorted(vals)[1] - vals[best]) / vals[best]
        for i in range(C):
            grad[b, i, :nb] = float(g_value[b]) * np.sign(est[b, i, :nb] - ref[b, perms[best][i], :nb]) / (C * nb)
    return V, index, perms, grad, gap


@functools.lru_cache(maxsize=None)
def case(C, n, ragged=False, tie=False):
    """est, ref (B,C,n) float32: the estimates are the references in another order plus noise, with exact ties est == ref planted
    at every 50th sample; ``tie``: references 0 and 1 are identical, so every row has two best permutations exactly."""
    rng = np.random.default_rng(500 + 10 * C + n + (3 if ragged else 0) + (5 if tie else 0))
    k = Case()
    ref = rng.standard_normal((B, C, n)).astype(np.float32)
    if tie:
        ref[:, 1] = ref[:, 0]
    est = np.empty_like(ref)
    order = []
    for b in range(B):
        p = list(rng.permutation(C))
        order.append(p)
        for i in range(C):
            est[b, i] = ref[b, p[i]] + (0.3 * rng.standard_normal(n)).astype(np.float32)
            est[b, i, ::50] = ref[b, p[i], ::50]
    k.est, k.ref = est, ref
    k.lengths = [n, n - 77, n // 2 + 1] if ragged else None
    k.g_value = (0.5 + rng.random(B)).astype(np.float32)
    k.V, k.perm_index, perms, k.grad, gap = reference(est, ref, k.lengths, k.g_value)
    if tie:
        assert C == 2 and (gap == 0).all(), gap
        assert k.perm_index == [0] * B, k.perm_index          # the lexicographically first of the two
    else:
        assert (gap > 1e-4).all(), gap               # no case is decided by rounding
        assert [list(perms[q]) for q in k.perm_index] == [[int(v) for v in p] for p in order]
    k.planted = np.zeros((B, C, n), dtype=bool)
    k.planted[:, :, ::50] = True
    if k.lengths is not None:
        for b, nb in enumerate(k.lengths):
            k.planted[b, :, nb:] = True
    assert (k.grad[k.planted] == 0).all()
    for a in (k.est, k.ref, k.g_value):
        a.setflags(write=False)
    return k


def strided_ref(k):
    """The references as a view of a larger NaN-filled buffer: their own batch and speaker strides, rows off 16-byte boundaries."""
    def make(be):
        nB, C, n = k.ref.shape
        big = np.full((nB, C + 1, n + 5), np.nan, np.float32)
        big[:, :C, :n] = k.ref
        return be.dev(big)[:, :C, :n]
    return make
