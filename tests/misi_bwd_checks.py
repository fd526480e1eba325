"""Check bodies shared by the host-side and the GPU tests of the MISI half-step's backward (tests/test_emu_misi_bwd.py,
tests/test_gpu_misi_bwd.py): onssen_misi_phase_backward_f32 through the C ABI against the float64 adjoint of
tests/misi_grad_ref.py.  A ``backend`` (tests/wa_checks.py) carries the library and says where arrays live."""
import numpy as np

from tests import misi_cases as MC
from tests import misi_grad_ref as G
from tests.wa_checks import E_ALIGN, E_ARG, E_WORKSPACE, DeviceBackend, HostBackend  # noqa: F401  (re-exported for the tests)


def run_backward(be, mix, est, n_fft, hop, g_p, lengths=None, est_view=None, sentinel=np.nan):
    """g_est (B, C, n) float32 (sentinel-filled before the call, as the workspace is) through the C ABI.  ``est_view``: a function
    of the backend that returns the estimates as a strided view on the device instead of a copy of ``est``."""
    B, C, n = est.shape
    d_mix, d_gp = be.dev(mix), be.dev(g_p)
    d_est = est_view(be) if est_view else be.dev(est)
    sb, sc, one = be.strides(d_est)
    assert one == 1
    nbytes = be.lib.misi_phase_backward_workspace_bytes(B, C, n, n_fft, hop)
    assert nbytes == C * B * (1 + n // hop) * n_fft * 8
    ws = be.dev(np.full(nbytes // 8, np.nan, np.float64))
    g_est = be.dev(np.full((B, C, n), sentinel, np.float32))
    ln = None if lengths is None else be.dev(np.asarray(lengths, np.int32))
    be.lib.misi_phase_backward(be.ptr(d_mix), be.strides(d_mix)[0], be.ptr(d_est), sb, sc, B, C, n, n_fft, hop, be.ptr(d_gp),
                               be.ptr(g_est), be.ptr(ws), nbytes, None, n_per_utt=be.ptr(ln))
    return be.host(g_est)


def grad_error(be, shape):
    """(max |got - ref|, max |ref|) of one case against the float64 adjoint, over all samples."""
    n_fft, hop, n, C = shape
    k = MC.case(*shape)
    got = run_backward(be, k.mix, k.est, n_fft, hop, G.g_phase(*shape))
    ref = G.reference(*shape)
    assert np.isfinite(got).all()
    return np.abs(got - ref).max(), np.abs(ref).max()


def check_gradient(be, shape):
    err, top = grad_error(be, shape)
    print(f"misi_phase backward {shape}: max |got - ref| {err:.3e}, max |ref| {top:.3e} ({err / top:.3e} relative; bound "
          f"{G.GRAD_REL_BOUND:.3e}, ceiling 1e-5)")
    assert top > 0 and err <= 1e-5 * top, (err, top)
    assert err <= G.GRAD_REL_BOUND * top, (err / top, G.GRAD_REL_BOUND)


def check_ragged(be, shape):
    """Lengths [n, n - 3 hop - 5, n_fft/2 + hop + 1]: every row inside its own length is bit for bit its batch-1 call, exactly 0
    after it; NaN planted in est / mix beyond lengths[b] and in g_p at the frames past the row's own does not reach the result."""
    n_fft, hop, n, C = shape
    lengths = G.ragged_lengths(n_fft, hop, n)
    k = MC.case(n_fft, hop, n, C, B=3)
    gp = G.g_phase(n_fft, hop, n, C, 3)
    mix, est, g = k.mix.copy(), k.est.copy(), gp.copy()
    for b, nb in enumerate(lengths):
        mix[b, nb:] = np.nan
        est[b, :, nb:] = np.nan
        g[:, b, 1 + nb // hop:] = np.nan
    got = run_backward(be, mix, est, n_fft, hop, g, lengths=lengths)
    assert np.isfinite(got).all()
    ref = G.reference(n_fft, hop, n, C, 3, tuple(lengths))
    for b, nb in enumerate(lengths):
        Tb = 1 + nb // hop
        one = run_backward(be, np.ascontiguousarray(mix[b:b + 1, :nb]), np.ascontiguousarray(est[b:b + 1, :, :nb]), n_fft, hop,
                           np.ascontiguousarray(g[:, b:b + 1, :Tb]))
        assert got[b, :, :nb].tobytes() == one[0].tobytes(), b
        assert (got[b, :, nb:] == 0).all(), b
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"misi_phase backward {shape} ragged {lengths}: {err / top:.3e} relative (bound {G.GRAD_REL_BOUND:.3e})")
    assert err <= 1e-5 * top and err <= G.GRAD_REL_BOUND * top, (err, top)


def check_strided(be, shape):
    """The estimates as a view of a larger NaN-filled buffer with its own batch and speaker strides: the bits of the contiguous call."""
    n_fft, hop, n, C = shape
    k, g = MC.case(*shape), G.g_phase(*shape)

    def view(be):
        big = np.full((k.B, C + 1, n + 37), np.nan, np.float32)
        big[:, :C, :n] = k.est
        return be.dev(big)[:, :C, :n]

    assert run_backward(be, k.mix, k.est, n_fft, hop, g, est_view=view).tobytes() == run_backward(be, k.mix, k.est, n_fft, hop, g).tobytes()


def check_zero_speaker(be, shape):
    """est_0 = 0 and est_1 = mix (the rest, if any, 0): no residual, so u_0 = 0 exactly, its phases are the (1, 0) fallback and its
    g_p contributes nothing -- the result is finite and equals the float64 adjoint, which sees Z_0 = 0 as well; with every
    g_p but speaker 0's set to zero the whole gradient is exactly 0."""
    n_fft, hop, n, C = shape
    k, g = MC.case(*shape), G.g_phase(*shape)
    est = np.zeros_like(k.est)
    est[:, 1] = k.mix
    got = run_backward(be, k.mix, est, n_fft, hop, g)
    assert np.isfinite(got).all()
    ref = np.stack([G.half_step_adjoint(k.mix[b], est[b], n_fft, hop, g[:, b]) for b in range(k.B)])
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"misi_phase backward {shape}, a silent speaker: {err / top:.3e} relative (bound {G.GRAD_REL_BOUND:.3e})")
    assert top > 0 and err <= 1e-5 * top and err <= G.GRAD_REL_BOUND * top
    only0 = np.zeros_like(g)
    only0[0] = g[0]
    assert (run_backward(be, k.mix, est, n_fft, hop, only0) == 0).all()


def check_repeatable(be, shape):
    n_fft, hop, n, C = shape
    k, g = MC.case(*shape), G.g_phase(*shape)
    assert run_backward(be, k.mix, k.est, n_fft, hop, g).tobytes() == run_backward(be, k.mix, k.est, n_fft, hop, g).tobytes()


def check_refusals(be):
    """Every refused argument returns its code before anything is launched: the sentinel-filled output is unchanged."""
    n_fft, hop, n, C = 256, 64, 768, 2
    k, g = MC.case(n_fft, hop, n, C), G.g_phase(n_fft, hop, n, C)
    B = k.B
    mix, est, gp = be.dev(k.mix), be.dev(k.est), be.dev(g)
    size = be.lib.dll.onssen_misi_phase_backward_workspace_bytes
    nbytes = int(size(B, C, n, n_fft, hop))
    assert nbytes == C * B * (1 + n // hop) * n_fft * 8
    for a in [(0, C, n, n_fft, hop), (B, 1, n, n_fft, hop), (B, 9, n, n_fft, hop), (B, C, 128, n_fft, hop), (B, C, n, 128, hop),
              (B, C, n, 2048, hop), (B, C, n, 300, hop), (B, C, n, n_fft, 0), (B, C, n, n_fft, 257)]:
        assert size(*a) == 0, a
    ws = be.dev(np.zeros(nbytes // 8 + 1, np.float64))
    g_est = be.dev(np.full((B, C, n), 7.0, np.float32))
    lens = be.dev(np.full(B, n, np.int32))
    f, P = be.lib.dll.onssen_misi_phase_backward_f32, be.ptr

    def args(mix=P(mix), est=P(est), C=C, n=n, lens=None, n_fft=n_fft, hop=hop, gp=P(gp), g_est=P(g_est), ws=P(ws), nbytes=nbytes, B=B):
        return (mix, n, est, C * n, n, B, C, n, lens, n_fft, hop, gp, g_est, ws, nbytes, None)

    bad = [dict(mix=None), dict(est=None), dict(gp=None), dict(g_est=None), dict(ws=None), dict(B=0), dict(C=1), dict(C=9),
           dict(hop=0), dict(hop=-3), dict(hop=257), dict(n=128), dict(n_fft=128), dict(n_fft=2048), dict(n_fft=300)]
    for kw in bad:
        assert f(*args(**kw)) == E_ARG, kw
        assert f(*args(lens=P(lens), **kw)) == E_ARG, kw
    assert f(*args(nbytes=nbytes - 1)) == E_WORKSPACE and f(*args(nbytes=0)) == E_WORKSPACE
    assert f(*args(gp=P(gp) + 4)) == E_ALIGN and f(*args(ws=P(ws) + 4)) == E_ALIGN
    be.sync()
    assert (be.host(g_est) == 7.0).all()
    assert f(*args()) == 0 and f(*args(lens=P(lens))) == 0
    be.sync()
    assert np.isfinite(be.host(g_est)).all()


# ------------------------------------------------------------------------------------------------- the whole chain
def chain_through_abi(be, c, iters):
    """K unfolded iterations forward and backward through the C ABI alone on ``misi_grad_ref.chain_case``: mask_istft, (misi_phase,
    phase_istft) x K, the L1 PIT loss's gradient at the final estimates (sign pattern and assignment from the estimates this
    build formed), then the adjoints in reverse.  The mixture is the inverse transform of the spectrum, as loss_wa_misi takes it.
    -> (mix (B,n) f32, final estimates (B,C,n) f32, gy (B,C,n) f64, d loss / d masks (B,T,F,C) f32)."""
    from tests import istft_grad_ref as IR
    from tests import wa_checks as WC
    from tests import wa_pit_cases as W
    B, T, F, C, n, n_fft, hop = c.B, c.T, c.F, c.C, c.n, c.n_fft, c.hop
    lib = be.lib
    dummy = np.zeros((C, B, T, F, 2), np.float32)
    d_ri, d_mix = be.dev(c.ri), be.dev(np.full((B, 1, n), np.nan, np.float32))
    lib.mask_istft(be.ptr(d_ri), None, 0, 0, 0, 0, B, 1, T, n_fft, hop, n, be.ptr(d_mix), None)
    mix = np.ascontiguousarray(be.host(d_mix)[:, 0])
    ests, phs = [WC.run_forward(be, IR.MASK, c.ri, c.masks, dummy, n_fft, hop, n)], []
    for _ in range(iters):
        d_mix, d_est = be.dev(mix), be.dev(ests[-1])
        ph = be.dev(np.full((C, B, T, F, 2), np.nan, np.float32))
        lib.misi_phase(be.ptr(d_mix), n, be.ptr(d_est), C * n, n, B, C, n, n_fft, hop, be.ptr(ph), None)
        phs.append(be.host(ph))
        ests.append(WC.run_forward(be, IR.PHASE, c.ri, c.masks, phs[-1], n_fft, hop, n))
    _, _, _, gy, _ = W.reference(ests[-1], c.src, None, np.full(B, 1.0 / B))
    g = gy.astype(np.float32)
    g_masks = np.zeros((B, T, F, C), np.float64)
    for i in range(iters, 0, -1):
        g_op, g_ph = WC.run_backward(be, IR.PHASE, c.ri, c.masks, phs[i - 1], n_fft, hop, g)
        g_masks += g_op
        g = run_backward(be, mix, ests[i - 1], n_fft, hop, g_ph)
    g_op, _ = WC.run_backward(be, IR.MASK, c.ri, c.masks, dummy, n_fft, hop, g)
    return mix, ests[-1], gy, (g_masks + g_op).astype(np.float32)


def chain_error(got, c, iters, mix, gy, masks=None):
    """(max |got - ref|, max |ref|) of d loss / d masks (B,T,F,C) against torch float64 autograd through the whole chain with the
    float32 mixture ``mix`` (B,n) and the gradient ``gy`` (B,C,n) at the final estimates."""
    masks = c.masks if masks is None else masks
    ref = np.stack([G.unfolded_gradient(c.ri[b], masks[b], mix[b], c.hop, c.n, iters, gy[b])[1] for b in range(c.B)])
    return np.abs(got - ref).max(), np.abs(ref).max()
