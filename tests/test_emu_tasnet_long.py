"""Long-form Conv-TasNet stitching (onssen_tasnet_windows_f32, onssen_tasnet_stitch_f32; csrc/tasnet_stitch.inc) on the host-side
emulation build, on planted data: independent Gaussian sources cut into windows of W = 40 samples, 24 apart (overlap 16), the
rows of every window shuffled by a planted permutation.  The permutations that come back undo the planted ones relative to
window 0 and the output equals the sources -- bit for bit where one window covers a sample, within 8 * 2^-24 (|a| + |b|) on an
overlap (w_new, w_old, two products and a sum: at most four roundings of 2^-24 relative each on either term, times two; the
weights sum to 1).  What lies beyond the last window's valid samples is NaN here: it is never read."""
import itertools

import numpy as np
import pytest

from tests import tasnet_emu, tasnet_long_ref as R
from tests.emu_build import load_emu

W, STEP = 40, 24
O = W - STEP
E_ARG, E_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _f32(shape, fill=None):
    a = tasnet_emu.aligned(int(np.prod(shape)) * 4).view(np.float32).reshape(shape)
    if fill is not None:
        a[...] = fill
    return a


def _planted(C, K, v_last, seed):
    """(est (C, K, W), sources (C, S_out), planted (K, C)): row planted[k][c] of window k carries source c."""
    rng = np.random.default_rng(seed)
    S_out = (K - 1) * STEP + v_last
    src = rng.standard_normal((C, S_out)).astype(np.float32)
    planted = np.stack([rng.permutation(C) for _ in range(K)])
    est = _f32((C, K, W), np.nan)
    for k in range(K):
        v = v_last if k == K - 1 else W
        for c in range(C):
            est[planted[k, c], k, :v] = src[c, k * STEP:k * STEP + v]
    return est, src, planted


def _stitch(lib, est, v_last, step=STEP, ws_cut=0, C=None):
    Cn, K, Wn = est.shape
    C = Cn if C is None else C
    S_out = (K - 1) * step + v_last
    out = _f32((Cn, max(S_out, 1)), np.float32(-7.0))
    perm = np.full((K, Cn), -7, np.int32)
    nb = int(lib.dll.onssen_tasnet_stitch_workspace_bytes(C, K, Wn, step, v_last))
    ws = tasnet_emu.aligned(max(nb, 256))
    rc = lib.dll.onssen_tasnet_stitch_f32(est.ctypes.data, C, K, Wn, step, v_last, out.ctypes.data, perm.ctypes.data, ws.ctypes.data,
                                          max(nb - ws_cut, 0), None)
    return rc, out, perm, nb


CASES = [(C, K, v) for C in (2, 3, 4) for K in (1, 2, 5) for v in (O + 1, W)]


@pytest.mark.parametrize("C, K, v_last", CASES)
def test_planted_permutations_are_undone(lib, C, K, v_last):
    est, src, planted = _planted(C, K, v_last, seed=100 * C + 10 * K + v_last)
    ref = R.stitch(est, STEP, v_last)
    assert len(ref["margins"]) == K - 1 and all(m >= R.MARGIN for m in ref["margins"]), ref["margins"]
    rc, out, perm, nb = _stitch(lib, est, v_last)
    assert rc == 0 and nb >= max(K - 1, 1) * C * C * 8
    inv0 = np.argsort(planted[0])                           # output channel c = row c of window 0 = source inv0[c]
    want = planted[:, inv0].astype(np.int32)
    assert np.array_equal(want, ref["perm"])                # the restatement agrees with the plant ...
    assert np.array_equal(perm, want), (perm, want)         # ... and so does the library
    assert np.isfinite(out).all()
    R.check_stitched(out, ref)
    # against the sources themselves: a copy outside the overlaps, a == b == the source inside them
    single = ref["bound"] == 0
    assert np.array_equal(out[single], src[inv0][single])
    assert np.all(np.abs(out.astype(np.float64) - src[inv0]) <= 16 * R.EPS * np.abs(src[inv0]))
    # a second run gives the same bits
    rc2, out2, perm2, _ = _stitch(lib, est, v_last)
    assert rc2 == 0 and np.array_equal(out.view(np.uint32), out2.view(np.uint32)) and np.array_equal(perm, perm2)


@pytest.mark.parametrize("v_last", [O + 1, W])
def test_cross_fade_of_estimates_that_differ(lib, v_last):
    """The plant plus window-dependent noise: a != b on the overlaps, as the estimates of two forwards are."""
    est, _, planted = _planted(4, 5, v_last, seed=21)
    est += (0.2 * np.random.default_rng(22).standard_normal(est.shape)).astype(np.float32)
    ref = R.stitch(est, STEP, v_last)
    assert all(m >= R.MARGIN for m in ref["margins"]), ref["margins"]
    rc, out, perm, _ = _stitch(lib, est, v_last)
    assert rc == 0 and np.array_equal(perm, ref["perm"]) and np.array_equal(perm, planted[:, np.argsort(planted[0])])
    assert (ref["bound"] > 0).sum() == 4 * 4 * O and np.isfinite(out).all()
    R.check_stitched(out, ref)


def test_cases_cover_both_store_widths():
    """v_last = W gives an S_out that is a multiple of 4 (the float4 path), v_last = O + 1 one that is not (the scalar path)."""
    assert W % 4 == 0 and STEP % 4 == 0 and (O + 1) % 4 != 0
    assert O <= W // 2 and {v for _, _, v in CASES} == {O + 1, W}


def test_silent_overlap_gives_the_identity(lib):
    est, _, planted = _planted(3, 2, W, seed=3)
    assert not np.array_equal(planted[0], planted[1])       # the plant would have asked for another permutation
    est[:, 0, STEP:] = 0.0
    est[:, 1, :O] = 0.0
    rc, out, perm, _ = _stitch(lib, est, W)
    assert rc == 0 and np.array_equal(perm, np.tile(np.arange(3, dtype=np.int32), (2, 1)))
    assert np.array_equal(out[:, :STEP], est[:, 0, :STEP]) and np.all(out[:, STEP:W] == 0.0)
    assert np.array_equal(out[:, W:], est[:, 1, O:])


def test_first_maximum_in_lexicographic_order_wins(lib):
    """Rows 1 and 2 of the newer window are the same signal: (0, 1, 2) and (0, 2, 1) tie exactly, the first is kept."""
    rng = np.random.default_rng(11)
    est = _f32((3, 2, W), 0.0)
    est[:, 0] = rng.standard_normal((3, W))
    est[0, 1, :O] = est[0, 0, STEP:]
    est[1, 1, :O] = est[2, 1, :O] = est[1, 0, STEP:] + est[2, 0, STEP:]
    est[:, 1, O:] = rng.standard_normal((3, W - O))
    pi, _ = R.pair_choice(est[:, 0, STEP:], est[:, 1, :O])
    assert pi == [0, 1, 2]
    scores = {p: sum(float(np.dot(est[i, 0, STEP:].astype(np.float64), est[p[i], 1, :O].astype(np.float64))) for i in range(3))
              for p in itertools.permutations(range(3))}
    assert scores[(0, 1, 2)] == scores[(0, 2, 1)] == max(scores.values())
    rc, _, perm, _ = _stitch(lib, est, W)
    assert rc == 0 and perm[1].tolist() == [0, 1, 2]


@pytest.mark.parametrize("what, kw", [
    ("C > 4", dict(C=5)),
    ("C < 1", dict(C=0)),
    ("overlap above W / 2", dict(step=W // 2 - 4)),
    ("no overlap", dict(step=W)),
    ("v_last = overlap", dict(v_last=O)),
    ("v_last > W", dict(v_last=W + 1)),
])
def test_refused_geometry_writes_nothing(lib, what, kw):
    est, _, _ = _planted(4, 3, W, seed=5)
    args = dict(dict(v_last=W, step=STEP, C=None), **kw)
    rc, out, perm, nb = _stitch(lib, est, args["v_last"], step=args["step"], C=args["C"])
    assert (rc, nb) == (E_ARG, 0), what
    assert np.all(out == -7.0) and np.all(perm == -7), what


def test_short_workspace_and_null_pointers_write_nothing(lib):
    est, _, _ = _planted(4, 3, W, seed=5)
    rc, out, perm, nb = _stitch(lib, est, W, ws_cut=1)
    assert rc == E_WORKSPACE and nb > 0 and np.all(out == -7.0) and np.all(perm == -7)
    ws = tasnet_emu.aligned(nb)
    for hole in range(4):
        ptrs = [est.ctypes.data, out.ctypes.data, perm.ctypes.data, ws.ctypes.data]
        ptrs[hole] = None
        assert lib.dll.onssen_tasnet_stitch_f32(ptrs[0], 4, 3, W, STEP, W, ptrs[1], ptrs[2], ptrs[3], nb, None) == E_ARG
    assert np.all(out == -7.0) and np.all(perm == -7)
    assert _stitch(lib, est, W)[0] == 0


@pytest.mark.parametrize("S, K, Wn, step", [(100, 4, 40, 24), (99, 4, 40, 24), (97, 4, 40, 24), (101, 5, 41, 23), (40, 1, 40, 24),
                                            (30, 1, 40, 24)])
def test_windows_equal_numpy_slices(lib, S, K, Wn, step):
    """Rows against NumPy slicing, the zero-filled tail included: aligned float4 rows (W and step multiples of 4, with the
    signal ending inside, and at the end of, a float4) and the scalar path."""
    x = _f32((S,))
    x[:] = np.random.default_rng(S).standard_normal(S)
    win = _f32((K, Wn), np.nan)
    assert lib.dll.onssen_tasnet_windows_f32(x.ctypes.data, S, K, Wn, step, win.ctypes.data, None) == 0
    want = np.zeros((K, Wn), np.float32)
    for k in range(K):
        piece = x[k * step:k * step + Wn]
        want[k, :len(piece)] = piece
    assert len(x[(K - 1) * step:(K - 1) * step + Wn]) < Wn or S == Wn      # the last row has a zero-filled tail (or ends the signal)
    assert np.array_equal(win.view(np.uint32), want.view(np.uint32))


def test_windows_refusals_write_nothing(lib):
    x = _f32((100,), 1.0)
    win = _f32((6, W), np.nan)
    for S, K, Wn, step in [(100, 6, W, 24), (0, 1, W, 24), (100, 0, W, 24), (100, 2, 0, 24), (100, 2, W, 0)]:
        assert lib.dll.onssen_tasnet_windows_f32(x.ctypes.data, S, K, Wn, step, win.ctypes.data, None) == E_ARG, (S, K, Wn, step)
    assert lib.dll.onssen_tasnet_windows_f32(None, 100, 2, W, 24, win.ctypes.data, None) == E_ARG
    assert lib.dll.onssen_tasnet_windows_f32(x.ctypes.data, 100, 2, W, 24, None, None) == E_ARG
    assert np.isnan(win).all()
