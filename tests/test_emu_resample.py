"""The polyphase resampler (csrc/resample.inc) in the host-side build (tests/emu) against scipy.signal.resample_poly in float64.
Bound of every value check (tests/resample_ref.py, derived there): |y - ref| <= 2^-24 |ref| + 1e-13 absum.
Taps: |h - up firwin(2 half + 1, 1 / M, kaiser 5)| <= 1e-12 max|h| -- two double-precision evaluations of the formula differ by
3e-16; the bound leaves room for another I0 series and is five orders below the fp32 rounding of the output.
The kernel's tile is 1024 outputs (rsmp::TILE): the 20011-sample rows give 6671 / 7261 outputs, seven tiles each."""
import time

import numpy as np
import pytest

from tests import resample_ref as R
from tests.emu_build import load_emu

E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return None if a is None else a.ctypes.data


def workspace(lib, up, down):
    nb = lib.resample_workspace_bytes(up, down)
    ws = np.full(nb // 8, np.nan, np.float64)
    lib.resample_prepare(up, down, P(ws), nb, None)
    return ws


def run(lib, up, down, lengths, seed=0, with_sub=False, pad_out=7, ragged=True, ws=None):
    """One launch over rows of ``lengths`` samples.  Whatever lies beyond a row's length is NaN, y is pre-filled with NaN.
    Returns (x, sub, y, lengths_out)."""
    rng = np.random.default_rng(seed)
    B, n_in = len(lengths), max(lengths)
    stride_in = n_in + 5
    x = np.full((B, stride_in), np.nan, np.float32)
    sub = np.full((B, stride_in), np.nan, np.float32) if with_sub else None
    for b, n in enumerate(lengths):
        x[b, :n] = rng.uniform(-1, 1, n)
        if with_sub:
            sub[b, :n] = rng.uniform(-1, 1, n)
    stride_out = R.n_out(n_in, up, down) + pad_out
    y = np.full((B, stride_out), np.nan, np.float32)
    lo = np.full(B, -77, np.int32)
    li = np.asarray(lengths, np.int32)
    ws = workspace(lib, up, down) if ws is None else ws
    lib.resample(P(x), P(sub), stride_in, P(li) if ragged else None, B, n_in, up, down, P(y), stride_out, P(lo), P(ws), ws.nbytes,
                 None)
    return x, sub, y, lo


def check_rows(x, sub, y, lo, up, down, lengths, what):
    worst = 0.0
    for b, n in enumerate(lengths):
        no = R.n_out(n, up, down)
        assert lo[b] == no
        ref = R.reference(x[b, :n], up, down, None if sub is None else sub[b, :n])
        assert len(ref) == no
        ab = R.absum(x[b, :n], up, down, np.arange(no), None if sub is None else sub[b, :n])
        worst = max(worst, R.ratio(y[b, :no], ref, ab, up, down))
        assert np.all(y[b, no:] == 0.0) and not np.signbit(y[b, no:]).any()
    print(f"{what}: largest |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (2, 1), (640, 441)])
def test_taps_against_firwin(lib, up, down):
    from scipy.signal import firwin
    M = max(up, down)
    ref = up * firwin(20 * M + 1, 1.0 / M, window=("kaiser", 5.0))
    h = np.array(lib.resample_taps(up, down))
    assert h.shape == ref.shape
    worst = np.abs(h - ref).max() / np.abs(ref).max()
    print(f"taps {up}/{down}: largest |h - firwin| / max|h| = {worst:.2e}")
    assert worst <= 1e-12


CASES = [(1, 3, (1000, 1, 61, 999)), (160, 441, (2000, 5, 441)), (2, 1, (333, 1)), (320, 441, (700,)),
         (1, 3, (20011, 3000)), (160, 441, (20011,))]


@pytest.mark.parametrize("up,down,lengths", CASES)
def test_ragged_values_padding_and_lengths(lib, up, down, lengths):
    x, sub, y, lo = run(lib, up, down, lengths, seed=3)
    check_rows(x, sub, y, lo, up, down, lengths, f"{up}/{down} {lengths}")


@pytest.mark.parametrize("up,down,lengths", [(1, 3, (1000, 61, 2500)), (160, 441, (2000, 441))])
def test_subtraction_on_load(lib, up, down, lengths):
    x, sub, y, lo = run(lib, up, down, lengths, seed=5, with_sub=True)
    check_rows(x, sub, y, lo, up, down, lengths, f"sub {up}/{down} {lengths}")


def test_unstaged_kernel_for_a_long_filter(lib):
    """1/500: 10001 taps per output do not fit the staged span, so the inputs are read where they are (resample_kernel<false>)."""
    up, down, lengths = 1, 500, (30011, 700)
    x, sub, y, lo = run(lib, up, down, lengths, seed=7, with_sub=True)
    check_rows(x, sub, y, lo, up, down, lengths, "1/500")


def test_uniform_batch_without_lengths(lib):
    up, down, lengths = 160, 441, (1500, 1500)
    x, sub, y, lo = run(lib, up, down, lengths, seed=9, ragged=False)
    check_rows(x, sub, y, lo, up, down, lengths, "uniform 160/441")


@pytest.mark.parametrize("up,down,lengths", [(1, 3, (1000, 1, 61, 3100)), (160, 441, (2000, 5, 441))])
def test_rows_equal_their_batch_1_result_and_runs_repeat(lib, up, down, lengths):
    ws = workspace(lib, up, down)
    x, sub, y, lo = run(lib, up, down, lengths, seed=13, with_sub=True, ws=ws)
    x2, sub2, y2, lo2 = run(lib, up, down, lengths, seed=13, with_sub=True, ws=ws)
    assert y.tobytes() == y2.tobytes() and lo.tobytes() == lo2.tobytes()
    for b, n in enumerate(lengths):
        no = R.n_out(n, up, down)
        xb, sb = np.ascontiguousarray(x[b, :n]), np.ascontiguousarray(sub[b, :n])
        yb = np.full(no, np.nan, np.float32)
        lib.resample(P(xb), P(sb), n, None, 1, n, up, down, P(yb), no, None, P(ws), ws.nbytes, None)
        assert yb.tobytes() == y[b, :no].tobytes()


def test_equal_rates_copy(lib):
    lengths = (300, 1)
    x, sub, y, lo = run(lib, 441, 441, lengths, seed=17)
    for b, n in enumerate(lengths):
        assert lo[b] == n and y[b, :n].tobytes() == x[b, :n].tobytes() and np.all(y[b, n:] == 0.0)
    x, sub, y, lo = run(lib, 3, 3, lengths, seed=19, with_sub=True)
    for b, n in enumerate(lengths):
        want = (x[b, :n].astype(np.float64) - sub[b, :n].astype(np.float64)).astype(np.float32)
        assert y[b, :n].tobytes() == want.tobytes()


def test_refusals_leave_y_untouched(lib):
    ws = workspace(lib, 1, 3)
    x = np.zeros((2, 100), np.float32)
    y = np.full((2, 40), np.nan, np.float32)
    call = lambda up, down, stride_out, ws_bytes: lib.dll.onssen_resample_f32(P(x), None, 100, None, 2, 100, up, down, P(y), stride_out,
                                                                              None, P(ws), ws_bytes, None)
    assert call(0, 3, 40, ws.nbytes) == E_ARG                          # up < 1
    assert call(1, 0, 40, ws.nbytes) == E_ARG
    assert call(1, 2049, 40, 1 << 30) == E_ARG                         # a reduced ratio above the limit
    assert call(2053, 3, 40, 1 << 30) == E_ARG
    assert call(1, 3, 40, ws.nbytes - 8) == E_ARG                      # a short workspace
    assert call(1, 3, 33, ws.nbytes) == E_ARG                          # n_out = 34 does not fit
    assert lib.dll.onssen_resample_workspace_bytes(1, 2049) == 0 and lib.dll.onssen_resample_workspace_bytes(0, 1) == 0
    assert lib.dll.onssen_resample_prepare(1, 3, P(ws), ws.nbytes - 8, None) == E_ARG
    assert lib.dll.onssen_resample_geometry(16000, 0, 10, None, None, None, None) == E_ARG
    assert np.isnan(y).all()
    assert call(4096, 2 * 4096 * 3 // 2, 40, ws.nbytes) == 0            # 4096 / 12288 reduces to 1 / 3: accepted
    assert not np.isnan(y).any()


def test_64_bit_indexing(lib):
    """160/441 over 13 500 000 samples: 4 897 960 outputs, the last m down = 2 159 999 919 > 2^31.  Checked where 32-bit index
    arithmetic would go wrong: the first and the last 4096 outputs and the stripe in which m 441 crosses 2^31."""
    up, down, n = 160, 441, 13_500_000
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, n).astype(np.float32)
    no = R.n_out(n, up, down)
    assert no == 4_897_960 and (no - 1) * down > 2 ** 31
    y = np.full(no, np.nan, np.float32)
    ws = workspace(lib, up, down)
    t0 = time.time()
    lib.resample(P(x), None, n, None, 1, n, up, down, P(y), no, None, P(ws), ws.nbytes, None)
    print(f"emulated launch: {time.time() - t0:.1f} s")
    ref = R.reference(x, up, down)
    assert len(ref) == no and not np.isnan(y).any()
    worst = 0.0
    for lo, hi in ((0, 4096), (no - 4096, no), (4_868_000, 4_871_000)):
        ms = np.arange(lo, hi)
        worst = max(worst, R.ratio(y[lo:hi], ref[lo:hi], R.absum(x, up, down, ms), up, down))
    assert 4_868_000 * down < 2 ** 31 < 4_871_000 * down
    print(f"2^31 case: largest |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0
