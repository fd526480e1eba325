"""The SI-SNR permutation-invariant training loss through the C ABI on the host-side emulation build (tests/emu):
onssen_sisnr_pit_f32 and onssen_sisnr_pit_backward_f32 against the NumPy fp64 restatement (tests/sisnr_pit_ref.py), which is
first pinned to fp64 autograd of loss.si_snr_loss.  Every comparison prints what it measured.

Bounds: value within 2 fp32 ulps of |V_ref| (0.5 from the final rounding, the rest for the fp64 evaluation),
loss within 2 ulps of max_b |V_b|, gradient elementwise within 2^-23 |g_ref| + 1e-9 (|A x| + |B s| + |C|): one rounding of an
expression evaluated in fp64.  Measured on this build (planted sources, every shape below): value <= 0.50 ulp, loss <= 0.43 ulp,
gradient <= 0.49 of its bound (the one rounding); beyond that rounding <= 1.3e-16 of the terms at 60 dB (noise 1e-3), 0 elsewhere."""
import os

import numpy as np
import pytest

from tests import sisnr_pit_ref as R
from tests.emu_build import load_emu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _rows(a, pad=0, offset=0):
    """A copy of a (N, S) whose rows are S + pad floats apart, its first element ``offset`` floats into a 16-byte aligned buffer;
    everything around the rows is NaN."""
    N, S = a.shape
    raw = np.full(N * (S + pad) + offset + 8, np.nan, dtype=np.float32)
    skip = (-raw.ctypes.data // 4) % 4                  # floats up to the next 16-byte boundary
    view = raw[skip + offset: skip + offset + N * (S + pad)].reshape(N, S + pad)[:, :S]
    view[:] = a
    assert (view.ctypes.data - 4 * offset) % 16 == 0
    return view


class Call:
    """One forward (and on request one backward) of the C ABI on host memory."""

    def __init__(self, lib, ests, refs, lengths=None, want_perm=True, want_total=True):
        self.lib, self.k = lib, len(ests)
        self.N, self.S = ests[0].shape
        assert all(e.strides[1] == 4 and e.dtype == np.float32 for e in list(ests) + list(refs))
        self.ests, self.refs = list(ests), list(refs)
        self.est = lib.sisnr_signals([e.ctypes.data for e in ests], [e.strides[0] // 4 for e in ests])
        self.ref = lib.sisnr_signals([r.ctypes.data for r in refs], [r.strides[0] // 4 for r in refs])
        self.lengths = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        self.nb = lib.sisnr_pit_workspace_bytes(self.N, self.k)
        self.ws = np.full(self.nb // 8 + 1, 0, dtype=np.float64).view(np.uint8)[:self.nb]
        self.ws[:] = 0xA5                                  # the workspace needs no zeroing
        self.value = np.full(self.N, np.nan, dtype=np.float32)
        self.perm = np.full(self.N, -7, dtype=np.int32) if want_perm else None
        self.total = np.full(1, np.nan, dtype=np.float32) if want_total else None
        lib.sisnr_pit(self.est, self.ref, self.k, self.N, self.S, self._p(self.lengths), self.value.ctypes.data, self._p(self.perm),
                      self._p(self.total), self.ws.ctypes.data, self.nb, None)

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data

    def backward(self, g_value=None, g_total=None):
        gv = None if g_value is None else np.ascontiguousarray(g_value, np.float32)
        gt = None if g_total is None else np.full(1, g_total, dtype=np.float32)
        d = np.full((self.k, self.N, self.S), np.nan, dtype=np.float32)
        self.lib.sisnr_pit_backward(self.est, self.ref, self.k, self.N, self.S, self._p(self.lengths), self._p(gv), self._p(gt),
                                    d.ctypes.data, self.ws.ctypes.data, self.nb, None)
        return d


def _planted_call(lib, k, N, S, seed, noise=0.3, pad=0, offset=0, lengths=None):
    ests, refs = R.planted(k, N, S, seed, noise)
    call = Call(lib, [_rows(e, pad, offset) for e in ests], [_rows(r, pad, offset) for r in refs], lengths)
    return ests, refs, call


# ---- the restatement itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N,S,noise", [(1, 3, 65, 0.3), (2, 3, 257, 0.3), (3, 1, 64, 0.3), (4, 3, 63, 0.3), (2, 3, 1030, 1e-3)])
def test_restatement_is_fp64_autograd_of_si_snr_loss(k, N, S, noise):
    """Bound: 1e-9 of the largest gradient entry: fp64's 1e-16 times the at most 1e6 cancellation of a 60 dB row, with margin."""
    import torch
    from onssen_amd import loss as L
    ests, refs = R.planted(k, N, S, 100 + k, noise)
    ref = R.reference(ests, refs)
    xs = [torch.from_numpy(e.astype(np.float64)).requires_grad_(True) for e in ests]
    loss = L.si_snr_loss(xs, [torch.from_numpy(r.astype(np.float64)) for r in refs])
    loss.backward()
    g = np.stack([x.grad.numpy() for x in xs])
    gmax = float(np.abs(g).max())
    print(f"k={k} N={N} S={S} noise={noise}: loss {ref['loss']:.9f} vs autograd {float(loss.detach()):.9f}, "
          f"gradient max |diff| / max |g| = {np.abs(ref['grad'] - g).max() / gmax:.2e} (bound 1e-9)")
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(ref["loss"]))
    assert np.abs(ref["grad"] - g).max() <= 1e-9 * gmax


# ---- items 1 and 2: values, loss, permutation, gradient --------------------------------------------------------------------
@pytest.mark.parametrize("S", R.SHAPES_S)
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_value_perm_loss_and_gradient(lib, k, S):
    for N in (1, 3):
        ests, refs, ref = R.planted_clear(k, N, S, seed=1000 * k + S + N)
        call = Call(lib, [_rows(e) for e in ests], [_rows(r) for r in refs])
        R.check_values(call.value, call.perm, call.total[0], ref, f"k={k} N={N} S={S}")
        R.check_grad(call.backward(g_total=1.0), ref, f"k={k} N={N} S={S}")


@pytest.mark.parametrize("pad,offset", [(3, 0), (0, 1), (3, 1), (4, 0)])
def test_row_strides_and_unaligned_bases_same_bits(lib, pad, offset):
    """Rows S + 3 apart, base pointers one float off a 16-byte boundary: the same bits as the contiguous aligned call, and right."""
    for k, N, S in ((2, 3, 257), (3, 3, 64), (4, 1, 513)):
        ests, refs, plain = _planted_call(lib, k, N, S, seed=7 + S)
        _, _, call = _planted_call(lib, k, N, S, seed=7 + S, pad=pad, offset=offset)
        ref = R.reference(ests, refs)
        R.check_values(call.value, call.perm, call.total[0], ref, f"k={k} N={N} S={S} pad={pad} offset={offset}")
        g = call.backward(g_total=1.0)
        R.check_grad(g, ref, f"k={k} N={N} S={S} pad={pad} offset={offset}")
        assert np.array_equal(call.value, plain.value) and np.array_equal(call.total, plain.total)
        assert np.array_equal(g, plain.backward(g_total=1.0))


def test_high_si_snr_and_both_incoming_gradients(lib):
    """Noise 1e-3 (about 60 dB): the terms of the gradient cancel; per-row and scalar incoming gradients together."""
    k, N, S = 2, 3, 1030
    ests, refs, call = _planted_call(lib, k, N, S, seed=5, noise=1e-3)
    gv = np.array([0.5, -2.0, 0.25], np.float32)
    ref = R.reference(ests, refs, g_value=gv, g_total=3.0)
    assert ref["value"].min() > 55.0
    R.check_values(call.value, call.perm, call.total[0], ref, "60 dB")
    R.check_grad(call.backward(g_value=gv, g_total=3.0), ref, "60 dB, g_value and g_total")
    R.check_grad(call.backward(g_value=gv), R.reference(ests, refs, g_value=gv, g_total=0.0), "60 dB, g_value alone")


def test_rows_longer_than_the_fixed_chunk_count(lib):
    """Above 64 x 512 samples a row's chunks grow instead of their number (the other branch of chunk_len)."""
    k, N, S = 2, 1, R.S_ABOVE_CHUNK_GROWTH
    ests, refs, call = _planted_call(lib, k, N, S, seed=9)
    ref = R.reference(ests, refs)
    R.check_values(call.value, call.perm, call.total[0], ref, f"S={S}")
    R.check_grad(call.backward(g_total=1.0), ref, f"S={S}")


def test_outputs_that_may_be_null(lib):
    ests, refs, call = _planted_call(lib, 2, 3, 65, seed=3)
    bare = Call(lib, call.ests, call.refs, want_perm=False, want_total=False)
    assert np.array_equal(bare.value, call.value)
    assert np.array_equal(bare.backward(g_total=1.0), call.backward(g_total=1.0))


# ---- item 3: ragged lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,S,lengths", [(2, 1030, (1030, 513, 5)), (3, 600, (64, 600, 511)), (4, 520, (512, 1, 519)), (1, 70, (70, 3, 65))])
def test_ragged_rows_are_the_one_row_calls_bit_for_bit(lib, k, S, lengths):
    N = len(lengths)
    ests, refs = R.planted(k, N, S, seed=40 + k)
    pe, pr = [_rows(e, 3, 1) for e in ests], [_rows(r, 3, 1) for r in refs]
    for arr in pe + pr:                                    # host padding beyond each row's length is NaN: never read
        for b, L in enumerate(lengths):
            arr[b, L:] = np.nan
    call = Call(lib, pe, pr, lengths)
    gv = np.linspace(0.5, 1.5, N).astype(np.float32)
    g = call.backward(g_value=gv, g_total=1.0)
    assert np.isfinite(call.value).all() and np.isfinite(call.total).all() and np.isfinite(g).all()
    ref = R.reference(ests, refs, lengths, g_value=gv, g_total=1.0)
    if min(lengths) >= 5:
        R.check_values(call.value, call.perm, call.total[0], ref, f"ragged k={k} {lengths}")
        R.check_grad(g, ref, f"ragged k={k} {lengths}")
    gb = call.backward(g_value=gv)
    for b, L in enumerate(lengths):
        one = Call(lib, [np.ascontiguousarray(e[b:b + 1, :L]) for e in ests], [np.ascontiguousarray(r[b:b + 1, :L]) for r in refs])
        assert call.value[b] == one.value[0] and call.perm[b] == one.perm[0]
        assert np.array_equal(gb[:, b, :L], one.backward(g_value=gv[b:b + 1])[:, 0, :])
        assert not g[:, b, L:].any() and not gb[:, b, L:].any()


# ---- item 4: degenerate rows ----------------------------------------------------------------------------------------------
def test_degenerate_rows(lib):
    rng = np.random.default_rng(2)
    S = 257
    s = rng.standard_normal((1, S)).astype(np.float32)
    x = (s + 0.3 * rng.standard_normal((1, S))).astype(np.float32)
    zero, const = np.zeros((1, S), np.float32), np.full((1, S), 0.3, np.float32)
    for name, est, ref in (("all-zero estimate", zero, s), ("constant estimate", const, s), ("all-zero reference", x, zero)):
        call = Call(lib, [est], [ref])
        g = call.backward(g_total=1.0)
        print(f"{name}: value {call.value[0]!r}, max |gradient| {np.abs(g).max()!r}")
        assert call.value[0] == np.float32(-160.0) and call.total[0] == np.float32(160.0) and not g.any()
        want = R.reference([est], [ref])
        assert abs(want["value"][0] + 160.0) < 1e-9
    # an exact multiple of the reference: the fp64 Gram floor is about 1e-14 of the power, that is 140 dB
    call = Call(lib, [(2.0 * s).astype(np.float32)], [s])
    g = call.backward(g_total=1.0)
    print(f"exact multiple: value {call.value[0]!r} dB, max |gradient| {np.abs(g).max():.3e}")
    assert np.isfinite(call.value[0]) and call.value[0] >= 120.0 and np.isfinite(g).all()
    # two speakers, one of them silent: the live pair still decides, everything stays finite
    call = Call(lib, [x, zero], [s, (0.5 * s[:, ::-1]).copy()])
    assert np.isfinite(call.value).all() and np.isfinite(call.backward(g_total=1.0)).all()


# ---- item 5: repeatability -------------------------------------------------------------------------------------------------
def test_two_runs_same_bits(lib):
    for k, N, S in ((2, 3, 1030), (4, 3, 65)):
        a = _planted_call(lib, k, N, S, seed=11)[2]
        b = _planted_call(lib, k, N, S, seed=11)[2]
        assert np.array_equal(a.value, b.value) and np.array_equal(a.perm, b.perm) and np.array_equal(a.total, b.total)
        assert np.array_equal(a.backward(g_total=1.0), b.backward(g_total=1.0))


# ---- item 6: refusals ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(lib):
    k, N, S = 2, 3, 65
    ests, refs = R.planted(k, N, S, seed=1)
    ests, refs = [_rows(e) for e in ests], [_rows(r) for r in refs]
    dll = lib.dll
    nb = lib.sisnr_pit_workspace_bytes(N, k)
    ws = np.full(nb, 0x5A, dtype=np.uint8)
    value, perm, total = np.full(N, 7.0, np.float32), np.full(N, 7, np.int32), np.full(1, 7.0, np.float32)
    d_est, gt = np.full((k, N, S), 7.0, np.float32), np.ones(1, np.float32)
    ep, es = lib.sisnr_signals([e.ctypes.data for e in ests], [S] * k)
    rp, rs = lib.sisnr_signals([r.ctypes.data for r in refs], [S] * k)

    def fwd(ep=ep, es=es, rp=rp, rs=rs, k=k, N=N, S=S, value=value.ctypes.data, ws=ws.ctypes.data, nb=nb):
        return dll.onssen_sisnr_pit_f32(ep, es, rp, rs, k, N, S, None, value, perm.ctypes.data, total.ctypes.data, ws, nb, None)

    def bwd(ep=ep, es=es, rp=rp, rs=rs, k=k, N=N, S=S, gv=None, gt=gt.ctypes.data, d=d_est.ctypes.data, ws=ws.ctypes.data, nb=nb):
        return dll.onssen_sisnr_pit_backward_f32(ep, es, rp, rs, k, N, S, None, gv, gt, d, ws, nb, None)

    short = lib.sisnr_signals([e.ctypes.data for e in ests], [S, S - 1])[1]
    holed = lib.sisnr_signals([ests[0].ctypes.data, None], [S] * k)[0]
    for f in (fwd, bwd):
        assert f(k=0) == -1 and f(k=5) == -1 and f(S=0) == -1 and f(N=0) == -1
        assert f(ep=None) == -1 and f(es=None) == -1 and f(rp=None) == -1 and f(rs=None) == -1 and f(ws=None) == -1
        assert f(es=short) == -1 and f(rs=short) == -1 and f(ep=holed) == -1 and f(rp=holed) == -1
        assert f(nb=nb - 1) == -2
    assert fwd(value=None) == -1 and bwd(d=None) == -1 and bwd(gt=None) == -1
    assert dll.onssen_sisnr_pit_workspace_bytes(N, 0) == 0 and dll.onssen_sisnr_pit_workspace_bytes(N, 5) == 0
    assert dll.onssen_sisnr_pit_workspace_bytes(0, 2) == 0
    assert (value == 7.0).all() and (perm == 7).all() and (total == 7.0).all() and (d_est == 7.0).all() and (ws == 0x5A).all()
    assert fwd() == 0 and bwd() == 0 and np.isfinite(d_est).all()


# ---- item 7: the reference's fixtures -----------------------------------------------------------------------------------
def test_loss_fixture(lib):
    """g8_tasnet_loss.npz: loss and gradient within that fixture's tolerance in tests/test_tasnet.py (1e-6 of the largest entry)."""
    z = np.load(os.path.join(GOLD, "g8_tasnet_loss.npz"))
    ests, refs = [np.ascontiguousarray(e, np.float32) for e in z["ests"]], [np.ascontiguousarray(r, np.float32) for r in z["refs"]]
    call = Call(lib, ests, refs)
    g = call.backward(g_total=1.0)
    want_g = z["grad"].astype(np.float64)
    print(f"loss {call.total[0]:.7f} vs fixture {float(z['loss']):.7f}; gradient max |diff| / max |g| = "
          f"{np.abs(g - want_g).max() / np.abs(want_g).max():.2e} (bound 1e-6)")
    assert abs(float(call.total[0]) - float(z["loss"])) <= 1e-6 * abs(float(z["loss"]))
    assert np.abs(g - want_g).max() <= 1e-6 * np.abs(want_g).max()


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_training_fixture_through_the_hip_loss(lib, prec, monkeypatch):
    """g8_tasnet_train.npz: training forward on the emulation -> the HIP loss and its gradient -> the HIP backward; the loss within
    1e-4 max(1, |loss|), every grad__* within the project's CEILING = 2e-3 under grad_error (tests/test_emu_tasnet_train.py)."""
    from tests import tasnet_ref
    from tests.tasnet_train_emu import Step, grad_error, param_names
    path = os.path.join(GOLD, "g8_tasnet_train.npz")
    z = np.load(path)
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(path)
    st = Step(lib, sd, cfg, z["x"].astype(np.float32), prec)
    refs = [np.ascontiguousarray(r, np.float32) for r in z["refs"]]
    call = Call(lib, [st.out[s] for s in range(st.out.shape[0])], refs)      # the k views of the (k, n, S_out) output
    print(f"{prec}: loss {float(call.total[0]):.6f} vs fixture {float(z['loss'][0]):.6f}")
    assert abs(float(call.total[0]) - float(z["loss"][0])) <= 1e-4 * max(1.0, abs(float(z["loss"][0])))
    got = st.backward(call.backward(g_total=1.0))
    ref = {k[6:]: z[k] for k in z.files if k.startswith("grad__")}
    assert set(ref) == set(param_names(cfg))
    e_hip, where = grad_error(got, ref)
    print(f"{prec}: HIP loss + HIP backward {e_hip:.2e} (worst: {where}), ceiling 2e-03")
    assert e_hip <= 2e-3
