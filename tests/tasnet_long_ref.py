"""NumPy fp64 restatement of the long-form Conv-TasNet stitching (csrc/tasnet_stitch.inc): the geometry,
the pairwise similarity, the lexicographic permutation search with its margin, the serial composition and the cross-fade.
Shared by tests/test_emu_tasnet_long.py, tests/test_tasnet_long_api.py and tests/test_gpu_tasnet_long.py."""
import itertools

import numpy as np

EPS = 2.0 ** -24
MARGIN = 1e-3            # best and second-best permutation scores differ by at least this share of the best


def geometry(L, S, W, step):
    """(S_out, K, v_last) by counting: windows are added until the plain forward's S_out samples are covered."""
    hop = L // 2
    S_out = (S - L) // hop * hop + L
    K = 1
    while (K - 1) * step + W < S_out:
        K += 1
    return S_out, K, min(W, S_out - (K - 1) * step)


def pair_choice(a, b):
    """a, b (C, O): the overlap as the older and the newer window hold it -> (pi, margin): pi[i] = the row of the newer window
    matched to row i of the older one (first maximum in lexicographic order), margin = (best - second best) / best."""
    C = a.shape[0]
    sim = (a.astype(np.float64)[:, None, :] * b.astype(np.float64)[None, :, :]).sum(-1)     # equal rows give equal entries
    scores = [(sum(sim[i, p[i]] for i in range(C)), p) for p in itertools.permutations(range(C))]
    best = max(s for s, _ in scores)
    pi = next(p for s, p in scores if s == best)
    rest = [s for s, p in scores if p != pi]
    margin = (best - max(rest)) / best if rest and best > 0 else (np.inf if not rest else 0.0)
    return list(pi), margin


def stitch(est, step, v_last):
    """est (C, K, W) -> dict(perm (K, C), out fp64 (C, S_out), bound (C, S_out): 0 where one window covers the sample and
    8 eps (|a| + |b|) on an overlap, margins: one per pair)."""
    C, K, W = est.shape
    O = W - step
    S_out = (K - 1) * step + v_last
    perm = np.zeros((K, C), np.int32)
    perm[0] = np.arange(C)
    margins = []
    for k in range(1, K):
        pi, m = pair_choice(est[:, k - 1, step:], est[:, k, :O])
        margins.append(m)
        perm[k] = [pi[perm[k - 1, c]] for c in range(C)]
    out = np.zeros((C, S_out), np.float64)
    bound = np.zeros((C, S_out), np.float64)
    w_new = (np.arange(O) + 0.5) / O
    for c in range(C):
        for k in range(K):
            v = v_last if k == K - 1 else W
            lo = O if k > 0 else 0
            row = est[perm[k, c], k].astype(np.float64)
            out[c, k * step + lo:k * step + v] = row[lo:v]
            if k > 0:
                a = est[perm[k - 1, c], k - 1, step:].astype(np.float64)
                b = row[:O]
                out[c, k * step:k * step + O] = (1.0 - w_new) * a + w_new * b
                bound[c, k * step:k * step + O] = 8 * EPS * (np.abs(a) + np.abs(b))
    return dict(perm=perm, out=out, bound=bound, margins=margins)


def check_stitched(got, ref):
    """Bit for bit where one window covers a sample, within the bound on the overlaps."""
    got64 = got.astype(np.float64)
    single = ref["bound"] == 0
    assert np.array_equal(got64[single], ref["out"][single]), "a sample that one window covers is not a copy"
    err = np.abs(got64 - ref["out"])
    worst = np.argmax(err - ref["bound"])
    assert np.all(err <= ref["bound"]), f"overlap error {err.flat[worst]:.3e} > bound {ref['bound'].flat[worst]:.3e}"
