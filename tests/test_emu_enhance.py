"""The enhancement entries in the host-side build (tests/emu) against the float64 restatements (tests/enhance_ref.py):
onssen_labels_enhance_f32, onssen_loss_enhance_f32 / _grad_f32 and onssen_mag_istft_f32 / _ragged_f32.  Bounds (none of them
taken from the kernels' output, derived as tests/test_emu_loss_phase.py derives its own):
  MSA value   |out - ref| <= 1e-5 * sum_bins (est - clean)^2: every bin contributes two fp32 roundings (the difference, the
              square) of a non-negative term -- at most ~3 eps32 = 3.6e-7 relative per term, and nothing cancels in a sum of
              non-negative terms -- the sums are fp64 and the result is rounded to fp32 once (6e-8): a 20-fold margin
  PSA value   |out - ref| <= 1e-5 * sum_bins 2 x: the residual mask x - t is one fused multiply-add of quantities bounded by x
              (mask <= 1, t <= x) after one rounding of s c, so each |.| is off by a few eps32 of 2 x at worst
  d mask      exactly float32(g * x) * sign: the product of two floats rounds once whether it is formed in fp32 or fp64, and
              the residual is a fused multiply-add, whose sign is the exact one (a planted residual of exactly 0 gives 0)
  d est       within 4 eps32 |g 2 scale (est - clean)|: g * 2 is exact, then three roundings (times scale, the difference,
              the product), 1.5 eps32 to first order
  mag_istft   2e-6 + 6 eps32 max|ref| (tests/enhance_ref.py: mag_atol)
  labels      bit equality with onssen_cos_difference_f32 and with hypotf of the same floats"""
import numpy as np
import pytest

from onssen_amd import _abi
from tests import enhance_ref as R
from tests.emu_build import load_emu
from tests.phase_istft_cases import SHAPES

MSA, PSA = _abi.ENHANCE_MSA, _abi.ENHANCE_PSA
LOSS_SHAPES = R.LOSS_SHAPES


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return a.ctypes.data


def aligned_bytes(n, fill, align=256):
    raw = np.full(n + align, fill, np.uint8)
    off = -raw.ctypes.data % align
    return raw[off:off + n]


def run_loss(lib, mode, c, scale, g):
    B, TF = c["est"].shape
    per_utt, total = np.full(B, np.nan, np.float32), np.full(1, np.nan, np.float32)
    ws = aligned_bytes(lib.loss_enhance_workspace_bytes(B), 0xA5)          # the workspace needs no zeroing
    maps = (P(c["est"]), P(c["x"]), P(c["s"]), P(c["c"])) if mode == PSA else (P(c["est"]), None, P(c["s"]), None)
    lib.loss_enhance(mode, *maps, B, TF, scale, P(per_utt), P(total), P(ws), ws.nbytes, None)
    d = np.full((B, TF), np.nan, np.float32)
    lib.loss_enhance_grad(mode, *maps, B, TF, scale, P(g), P(d), None)
    return per_utt, total, d


@pytest.mark.parametrize("B,TF", LOSS_SHAPES)
def test_msa_value_and_gradient(lib, B, TF):
    c = R.loss_case(B, TF, seed=11 + B)
    scale = np.float32(1.0 / (B * TF))
    g = np.array([-1.7], np.float32)
    per_utt, total, d = run_loss(lib, MSA, c, scale, g)
    ref_utt, _ = R.msa(c["est"], c["s"])
    ref_total = float(scale) * ref_utt.sum()                # the caller's scale as the kernel gets it: a float32
    bound = 1e-5 * ref_utt
    print("MSA per_utt |out - ref| / bound", np.abs(per_utt - ref_utt) / bound)
    print("MSA total   |out - ref| / bound", abs(float(total[0]) - ref_total) / (float(scale) * bound.sum()))
    assert (np.abs(per_utt - ref_utt) <= bound).all()
    assert abs(float(total[0]) - ref_total) <= float(scale) * bound.sum()
    ref_d = float(g[0]) * 2.0 * float(scale) * (R.f64(c["est"]) - R.f64(c["s"]))
    err = np.abs(d - ref_d)
    print("MSA gradient max |err| / bound", (err / np.maximum(4 * R.EPS32 * np.abs(ref_d), 1e-300)).max())
    assert np.isfinite(d).all() and (err <= 4 * R.EPS32 * np.abs(ref_d)).all()
    again = run_loss(lib, MSA, c, scale, g)
    for a, b in zip((per_utt, total, d), again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("B,TF", LOSS_SHAPES)
def test_psa_value_and_gradient(lib, B, TF):
    c = R.loss_case(B, TF, seed=23 + B)
    scale = np.float32(0.125)
    g = np.random.default_rng(B).standard_normal(B).astype(np.float32)
    per_utt, total, d = run_loss(lib, PSA, c, scale, g)
    ref_utt = R.psa(c["est"], c["x"], c["s"], c["c"])
    bound = 1e-5 * 2.0 * R.f64(c["x"]).sum(1)
    print("PSA per_utt |out - ref| / bound", np.abs(per_utt - ref_utt) / bound)
    assert (np.abs(per_utt - ref_utt) <= bound).all()
    assert abs(float(total[0]) - 0.125 * ref_utt.sum()) <= 0.125 * bound.sum()
    sign = np.sign(R.psa_grad(c["est"], c["x"], c["s"], c["c"], np.ones(B)))
    want = (g[:, None] * c["x"]).astype(np.float32) * sign.astype(np.float32)          # float32(g x) * sign, exactly
    np.testing.assert_array_equal(d, want)
    assert (d[:, 0] == 0.0).all() and (sign[:, 0] == 0).all()                          # the planted residual of exactly 0
    if TF > 2:
        assert (sign[:, 1] > 0).all() and (sign[:, 2] < 0).all()                       # target clamped to 0 by the relu, to x by the min
    again = run_loss(lib, PSA, c, scale, g)
    for a, b in zip((per_utt, total, d), again):
        assert a.tobytes() == b.tobytes()


def test_loss_refusals(lib):
    c = R.loss_case(2, 40, seed=1)
    out, tot, g = np.zeros(2, np.float32), np.zeros(1, np.float32), np.ones(2, np.float32)
    ws = aligned_bytes(lib.loss_enhance_workspace_bytes(2), 0)
    f = lib.dll.onssen_loss_enhance_f32
    ok = (MSA, P(c["est"]), None, P(c["s"]), None, 2, 40, 1.0, P(out), P(tot), P(ws), ws.nbytes, None)
    assert f(*ok) == 0
    assert f(MSA, None, *ok[2:]) == -1                                                 # ONSSEN_E_ARG
    assert f(2, *ok[1:]) == -1                                                         # no such mode
    assert f(PSA, *ok[1:]) == -1                                                       # PSA needs mag_noisy and cos_diff
    assert f(*ok[:10], P(ws) + 4, ws.nbytes - 4, None) == -3                           # ONSSEN_E_ALIGN: fp64 partial sums
    assert f(*ok[:11], ws.nbytes - 8, None) == -2                                      # ONSSEN_E_WORKSPACE
    assert f(*ok[:9], None, P(ws), ws.nbytes, None) == 0                               # total is optional
    gf = lib.dll.onssen_loss_enhance_grad_f32
    d = np.zeros((2, 40), np.float32)
    assert gf(PSA, P(c["est"]), P(c["x"]), P(c["s"]), P(c["c"]), 2, 40, 1.0, P(g), P(d), None) == 0
    assert gf(PSA, P(c["est"]), P(c["x"]), P(c["s"]), P(c["c"]), 2, 40, 1.0, None, P(d), None) == -1
    assert gf(PSA, P(c["est"]), None, P(c["s"]), P(c["c"]), 2, 40, 1.0, P(g), P(d), None) == -1


# ---- labels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 1000])
def test_labels_bits(lib, n_bins):
    a, b = R.labels_case(n_bins, seed=n_bins)
    mn, mc, cd = (np.full(n_bins, np.nan, np.float32) for _ in range(3))
    lib.labels_enhance(P(a), P(b), n_bins, P(mn), P(mc), P(cd), None)
    alone = np.full(n_bins, np.nan, np.float32)
    lib.cos_difference(P(a), P(b), n_bins, P(alone), None)
    assert cd.tobytes() == alone.tobytes()
    assert mn.tobytes() == np.hypot(a[:, 0], a[:, 1]).tobytes() and mc.tobytes() == np.hypot(b[:, 0], b[:, 1]).tobytes()
    rn, rc, rcos = R.labels(a, b)
    assert np.abs(mn - rn).max() <= 2 * R.EPS32 * rn.max() and np.abs(mc - rc).max() <= 2 * R.EPS32 * rc.max()
    assert np.abs(cd - rcos).max() <= 1e-6              # two atan2f, a difference of angles up to 2 pi, one cosf
    assert mn[0] == 0.0
    if n_bins > 2:
        assert cd[2] == -1.0                            # X = 0 against the negative real axis: cosf(0 - pi)
    # magnitudes alone: cos_diff NULL; the noisy magnitude alone: no clean spectrum at all
    mn2, mc2 = np.full(n_bins, np.nan, np.float32), np.full(n_bins, np.nan, np.float32)
    lib.labels_enhance(P(a), P(b), n_bins, P(mn2), P(mc2), None, None)
    assert mn2.tobytes() == mn.tobytes() and mc2.tobytes() == mc.tobytes()
    mn3 = np.full(n_bins, np.nan, np.float32)
    lib.labels_enhance(P(a), None, n_bins, P(mn3), None, None, None)
    assert mn3.tobytes() == mn.tobytes()


def test_labels_refusals(lib):
    a, b = R.labels_case(8, seed=0)
    o = [np.zeros(8, np.float32) for _ in range(3)]
    f = lib.dll.onssen_labels_enhance_f32
    assert f(None, P(b), 8, P(o[0]), P(o[1]), P(o[2]), None) == -1
    assert f(P(a), P(b), 8, None, P(o[1]), P(o[2]), None) == -1
    assert f(P(a), P(b), 8, P(o[0]), None, P(o[2]), None) == -1                        # a clean spectrum needs its magnitude map
    assert f(P(a), None, 8, P(o[0]), None, P(o[2]), None) == -1                        # no clean spectrum: no cos_diff
    assert f(P(a), P(b), 0, P(o[0]), P(o[1]), P(o[2]), None) == -1
    assert f(P(a) + 4, P(b), 7, P(o[0]), P(o[1]), P(o[2]), None) == -3                 # (re, im) pairs are read as 8-byte words
    assert f(P(a), P(b) + 4, 7, P(o[0]), P(o[1]), P(o[2]), None) == -3


# ---- magnitude mode of the inverse transform --------------------------------------------------------------------------------
def mag_istft(lib, ri, mags, n_fft, hop, length, frames=None, lengths=None):
    B, T, F, C = mags.shape
    out = np.full((B, C, length), np.nan, np.float32)
    st = [s // 4 for s in mags.strides]
    rag = {} if frames is None else dict(frames=P(frames), lengths=P(lengths))
    lib.mag_istft(P(ri), P(mags), st[0], st[3], st[1], st[2], B, C, T, n_fft, hop, length, P(out), None, **rag)
    return out


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n_fft,hop,n", SHAPES)
def test_mag_istft_matches_oracle(lib, n_fft, hop, n, C):
    ri, mags = R.mag_case(n_fft, hop, n, C)
    assert (ri[:, 1::3, 5::17] == 0).all()
    out = mag_istft(lib, ri, mags, n_fft, hop, n)
    ref = R.mag_reference(ri, mags, hop, n)
    print(f"n_fft {n_fft} hop {hop} C {C}: max |out - ref| {np.abs(out - ref).max():.3e}, bound {R.mag_atol(ref):.3e}")
    assert np.isfinite(out).all() and np.abs(out - ref).max() <= R.mag_atol(ref)
    # the same magnitudes as a strided view: speaker-major storage, every second frequency column of a wider buffer
    B, T, F, _ = mags.shape
    wide = np.full((B, C, T, 2 * F), np.nan, np.float32)
    wide[..., ::2] = mags.transpose(0, 3, 1, 2)
    view = wide[..., ::2].transpose(0, 2, 3, 1)
    assert not view.flags.c_contiguous and view.shape == mags.shape
    assert mag_istft(lib, ri, view, n_fft, hop, n).tobytes() == out.tobytes()


@pytest.mark.parametrize("n_fft,hop,n", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_mag_istft_ragged_rows_are_their_batch_1_results(lib, n_fft, hop, n):
    ri, mags = R.mag_case(n_fft, hop, n, 1, B=3)
    B, T = mags.shape[:2]
    lengths = np.array([n, n - 3 * hop - 5, n_fft // 2 + hop + 1], np.int32)
    frames = (1 + lengths // hop).astype(np.int32)
    out = mag_istft(lib, ri, mags, n_fft, hop, n, frames, lengths)
    ref = R.mag_reference(ri, mags, hop, n, frames, lengths)
    assert np.abs(out - ref).max() <= R.mag_atol(ref)
    for b in range(B):
        Tb, nb = int(frames[b]), int(lengths[b])
        alone = mag_istft(lib, np.ascontiguousarray(ri[b:b + 1, :Tb]), np.ascontiguousarray(mags[b:b + 1, :Tb]), n_fft, hop, nb)
        assert out[b, :, :nb].tobytes() == alone[0].tobytes(), b
        assert (out[b, :, nb:] == 0.0).all(), b


def test_mag_istft_refusals(lib):
    ri, mags = R.mag_case(256, 64, 768, 1)
    B, T, F, C = mags.shape
    out = np.zeros((B, C, 768), np.float32)
    fr, ln = np.full(B, T, np.int32), np.full(B, 768, np.int32)
    f, fr_ = lib.dll.onssen_mag_istft_f32, lib.dll.onssen_mag_istft_ragged_f32
    a = lambda ri_, m_, n_fft: (ri_, m_, T * F * C, 1, F * C, C, B, C, T, n_fft, 64, 768, P(out), None)
    assert f(*a(P(ri), P(mags), 256)) == 0
    assert f(*a(None, P(mags), 256)) == -1
    assert f(*a(P(ri), None, 256)) == -1                                               # no magnitude: that is onssen_mask_istft_f32
    assert f(*a(P(ri) + 4, P(mags), 256)) == -3
    for n_fft in (128, 384, 2048):
        assert f(*a(P(ri), P(mags), n_fft)) == -1
    r = lambda frames, lengths: (P(ri), P(mags), T * F * C, 1, F * C, C, B, C, T, frames, 256, 64, 768, lengths, P(out), None)
    assert fr_(*r(P(fr), P(ln))) == 0
    assert fr_(*r(None, P(ln))) == -1 and fr_(*r(P(fr), None)) == -1
