"""The uPIT loss entries in the host-side build (tests/emu) against the float64 restatements (tests/upit_ref.py):
onssen_loss_upit_workspace_bytes, onssen_loss_upit_f32 and onssen_loss_upit_grad_f32.  Bounds (none of them taken from the
kernels' output, derived as tests/test_emu_enhance.py derives its own):
  pair     |pair[k][j] - ref| <= 1e-5 * sum_bins (x + t_j): the residual m_k x - t_j is one fused multiply-add of |m_k x| <= x and
           t_j (after one rounding of s c for PSA), so each |.| is off by about eps32 (x + t_j) at worst; the sums are fp64 and
           the result is rounded to fp32 once (6e-8): a margin of two orders
  out      the sum of the S entries' bounds along the winning assignment
  perm     at TF >= 387 the planted assignment wins in float64 by >= 100 of those bounds (asserted for every row), so perm[b] = b;
           at TF = 1 the clipping makes ties: perm must attain the minimum of the returned pair matrix
  d masks  exactly float32(g x) * sign: the product of two floats rounds once whether it is formed in fp32 or fp64, and the
           residual is a fused multiply-add, whose sign is the exact one (a planted residual of exactly 0 gives 0)"""
from math import factorial

import numpy as np
import pytest

from tests import upit_ref as R
from tests.emu_build import load_emu


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return None if a is None else a.ctypes.data


def aligned(n, fill, align=256):
    raw = np.full(n + align, fill, np.uint8)
    off = -raw.ctypes.data % align
    return raw[off:off + n]


def interleave(masks):
    """(S, B, TF) -> the contiguous (B, TF, S) buffer the network writes."""
    return np.ascontiguousarray(masks.transpose(1, 2, 0))


def run(lib, c, interleaved=True, frames=None, F=0, g=None, want_pair=True):
    """(out, perm, pair, d (S, B, TF)) of one value call and one gradient call; outputs prefilled with NaN / -1, the workspace
    with 0xA5 (it needs no zeroing)."""
    S, B, TF = c["masks"].shape
    if interleaved:
        m = interleave(c["masks"])
        st = (TF * S, S, 1)
    else:
        m = np.ascontiguousarray(c["masks"])
        st = (TF, 1, B * TF)
    src, cos = np.ascontiguousarray(c["src"]), None if c["cos"] is None else np.ascontiguousarray(c["cos"])
    out, perm = np.full(B, np.nan, np.float32), np.full(B, -1, np.int32)
    pair = np.full((B, S, S), np.nan, np.float32) if want_pair else None
    ws = aligned(lib.loss_upit_workspace_bytes(B, S), 0xA5)
    maps = (P(m), *st, P(c["x"]), P(src), B * TF, P(cos), B * TF, P(frames), F, B, TF, S)
    lib.loss_upit(*maps, P(out), P(perm), P(pair), P(ws), ws.nbytes, None)
    g = np.ones(B, np.float32) if g is None else g
    d = np.full(m.shape, np.nan, np.float32)
    lib.loss_upit_grad(*maps, P(g), P(perm), P(d), *st, None)
    return out, perm, pair, d.transpose(2, 0, 1) if interleaved else d


def check_against_ref(c, out, perm, pair, d, g):
    S, B, TF = c["masks"].shape
    ref_pair = R.pair_matrix(c["masks"], c["x"], c["src"], c["cos"])
    pb = R.pair_bound(c["x"], c["src"], c["cos"])                                      # (B, S): per target j
    print("pair max |out - ref| / bound", (np.abs(pair - ref_pair) / pb[:, None, :]).max())
    assert (np.abs(pair - ref_pair) <= pb[:, None, :]).all()
    ref_out, ref_perm = R.best(ref_pair)
    ob = R.out_bound(c["x"], c["src"], c["cos"], ref_perm)
    print("out |out - ref| / bound", np.abs(out - ref_out) / ob)
    assert (np.abs(out - ref_out) <= ob).all()
    if TF >= 387:
        mg = R.margin(ref_pair) / ob
        print("float64 margin of the planted assignment / bound", mg)
        assert (mg >= 100).all() and (ref_perm == np.arange(B)).all()                  # every row: none left out
        assert (perm == np.arange(B)).all()
    else:
        tot = R.totals(pair.astype(np.float64))
        assert ((perm >= 0) & (perm < factorial(S))).all()
        assert (tot[np.arange(B), perm] == tot.min(1)).all()                           # perm attains the minimum of the returned pair
    sign = R.grad_sign(c["masks"], c["x"], c["src"], c["cos"], perm)
    want = (g[None, :, None] * c["x"][None]).astype(np.float32) * sign.astype(np.float32)      # float32(g x) * sign, exactly
    np.testing.assert_array_equal(d, want)
    assert (d[:, :, 0] == 0.0).all() and (sign[:, :, 0] == 0).all()                    # the planted residual of exactly 0


@pytest.mark.parametrize("S,TF,psa", R.SHAPES + [R.LONG])
def test_value_pair_perm_and_gradient(lib, S, TF, psa):
    c = R.loss_case(S, TF, seed=100 * S + int(psa), psa=psa)
    B = factorial(S)
    g = np.random.default_rng(S).standard_normal(B).astype(np.float32)
    out, perm, pair, d = run(lib, c, g=g)
    check_against_ref(c, out, perm, pair, d, g)
    if TF != 387:              # (the host build runs a workgroup as 256 OS threads: the repeats go to one size, every S and loss)
        return
    # a second call gives the same bytes; so do the masks as S separate maps (with the optional outputs left out)
    again, apart = run(lib, c, g=g), run(lib, c, interleaved=False, g=g, want_pair=False)
    for a, b in zip((out, perm, pair, d), again):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    for a, b in zip((out, perm, d), (apart[0], apart[1], apart[3])):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("S", [2, 3, 4])
def test_identical_targets_take_the_first_assignment(lib, S):
    c = dict(R.loss_case(S, 387, seed=7, psa=True))
    c["src"] = np.repeat(c["src"][:1], S, 0)
    c["cos"] = np.repeat(c["cos"][:1], S, 0)
    out, perm, pair, _ = run(lib, c)
    assert (perm == 0).all()
    assert (pair == pair[:, :, :1]).all()                                              # every column of a row's pair matrix alike


@pytest.mark.parametrize("psa", [False, True])
def test_ragged_rows_are_their_batch_1_calls(lib, psa):
    S, T, F = 3, 5, 129
    full = R.loss_case(S, T * F, seed=31, psa=psa)
    frames = np.array([1, T - 1, T], np.int32)
    c = {k: (None if v is None else np.ascontiguousarray(v[..., :3, :] if k != "x" else v[:3])) for k, v in full.items()}
    g = np.array([0.5, -2.0, 1.25], np.float32)
    out, perm, pair, d = run(lib, c, frames=frames, F=F, g=g)
    for b in range(3):
        n = int(frames[b]) * F
        one = {k: (None if v is None else np.ascontiguousarray(v[..., b:b + 1, :n])) for k, v in c.items()}
        o1, p1, pr1, d1 = run(lib, one, g=g[b:b + 1])
        assert out[b:b + 1].tobytes() == o1.tobytes() and pair[b:b + 1].tobytes() == pr1.tobytes(), b
        assert perm[b] == p1[0], b
        assert np.ascontiguousarray(d[:, b, :n]).tobytes() == np.ascontiguousarray(d1[:, 0]).tobytes(), b
        assert (d[:, b, n:] == 0.0).all() and not np.signbit(d[:, b, n:]).any(), b
    # the last row covers everything: the call without frames gives its bytes too
    o2 = run(lib, c, g=g)[0]
    assert o2[2:].tobytes() == out[2:].tobytes()


def test_refusals(lib):
    c = R.loss_case(2, 387, seed=200, psa=False)
    S, B, TF = c["masks"].shape
    m = interleave(c["masks"])
    out, perm, g = np.zeros(B, np.float32), np.zeros(B, np.int32), np.ones(B, np.float32)
    d = np.zeros_like(m)
    ws = aligned(lib.loss_upit_workspace_bytes(B, 4), 0)
    assert lib.loss_upit_workspace_bytes(B, 2) == B * 32 * 4 * 8 and lib.loss_upit_workspace_bytes(B, 4) == B * 32 * 16 * 8
    assert lib.loss_upit_workspace_bytes(B, 1) == 0 and lib.loss_upit_workspace_bytes(B, 5) == 0
    f, gf = lib.dll.onssen_loss_upit_f32, lib.dll.onssen_loss_upit_grad_f32
    src = np.ascontiguousarray(np.concatenate([c["src"], c["src"], c["src"]]))         # room for S up to 5 + 1
    a = lambda S_, TF_=TF: (P(m), TF * S, S, 1, P(c["x"]), P(src), B * TF, None, 0, None, 0, B, TF_, S_)
    tail = (P(out), P(perm), None, P(ws), ws.nbytes, None)
    assert f(*a(2), *tail) == 0
    assert f(*a(1), *tail) == -1 and f(*a(5), *tail) == -1                             # ONSSEN_E_ARG: S outside 2 .. 4
    assert f(*a(2, 0), *tail) == -1                                                    # TF < 1
    assert f(*a(2), P(out), P(perm), None, P(ws), lib.loss_upit_workspace_bytes(B, 2) - 8, None) == -2      # ONSSEN_E_WORKSPACE
    assert f(*a(2), P(out), P(perm), None, P(ws) + 4, ws.nbytes - 4, None) == -3       # ONSSEN_E_ALIGN: fp64 partial sums
    assert f(*a(2), None, P(perm), None, P(ws), ws.nbytes, None) == -1
    assert f(*a(2)[:9], P(perm), 0, B, TF, 2, *tail) == -1                             # frames without F
    gt = (P(g), P(perm), P(d), TF * S, S, 1, None)
    assert gf(*a(2), *gt) == 0
    assert gf(*a(1), *gt) == -1 and gf(*a(5), *gt) == -1 and gf(*a(2, 0), *gt) == -1
    assert gf(*a(2), None, P(perm), P(d), TF * S, S, 1, None) == -1
    assert gf(*a(2), P(g), None, P(d), TF * S, S, 1, None) == -1


@pytest.mark.parametrize("psa", [False, True])
def test_two_speakers_agree_with_the_chimera_mask_term(lib, psa):
    c = R.loss_case(2, 387, seed=300 + int(psa), psa=psa)
    S, B, TF = c["masks"].shape
    out, perm, _, _ = run(lib, c)
    ma, mb = np.ascontiguousarray(c["masks"][0]), np.ascontiguousarray(c["masks"][1])
    s1, s2 = np.ascontiguousarray(c["src"][0]), np.ascontiguousarray(c["src"][1])
    c1, c2 = (np.ascontiguousarray(c["cos"][0]), np.ascontiguousarray(c["cos"][1])) if psa else (None, None)
    o2, p2 = np.full(B, np.nan, np.float32), np.full(B, -1, np.int32)
    ws = aligned(lib.loss_mask_workspace_bytes(B), 0xA5)
    lib.loss_mask(P(ma), P(mb), TF, 1, P(c["x"]), P(s1), P(s2), P(c1), P(c2), B, TF, P(o2), P(ws), ws.nbytes, None, perm=P(p2))
    ob = R.out_bound(c["x"], c["src"], c["cos"], perm)
    assert (np.abs(out - o2) <= 2 * ob).all()
    assert (perm == p2).all()
