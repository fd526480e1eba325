"""Check bodies shared by the host-side and the GPU tests of the waveform-approximation kernels (tests/test_emu_istft_bwd.py,
tests/test_gpu_istft_bwd.py, tests/test_emu_wa_pit.py, tests/test_gpu_wa_pit.py).  A ``backend`` carries the library and says
where arrays live: NumPy arrays for the host-side build, torch tensors on the device for the product library."""
import numpy as np

from tests import istft_grad_ref as R

E_ARG, E_WORKSPACE, E_ALIGN = -1, -2, -3          # include/onssen_hip.h


class HostBackend:
    def __init__(self, lib):
        self.lib = lib

    def dev(self, a):
        return np.array(a, copy=True)

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def strides(self, a):
        return [s // a.itemsize for s in a.strides]

    def host(self, a):
        return np.array(a, copy=True)

    def sync(self):
        pass


class DeviceBackend:
    def __init__(self, lib):
        import torch
        self.lib, self.torch = lib, torch

    def dev(self, a):
        return self.torch.from_numpy(np.array(a, copy=True)).cuda()

    def ptr(self, a):
        return None if a is None else a.data_ptr()

    def strides(self, a):
        return list(a.stride())

    def host(self, a):
        self.torch.cuda.synchronize()
        return a.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the inverse transforms
def run_forward(be, mode, ri, op, phases, n_fft, hop, length, frames=None, lengths=None):
    """(B, C, length) float32 through the C ABI: ri (B,T,F,2), op (B,T,F,C), phases (C,B,T,F,2) host arrays."""
    B, T, F, C = op.shape
    d_ri, d_op, d_ph = be.dev(ri), be.dev(op), be.dev(phases)
    out = be.dev(np.full((B, C, length), np.nan, np.float32))
    fr = None if frames is None else be.dev(np.asarray(frames, np.int32))
    ln = None if lengths is None else be.dev(np.asarray(lengths, np.int32))
    rag = {} if fr is None else dict(frames=be.ptr(fr), lengths=be.ptr(ln))
    a = (be.ptr(d_ri), be.ptr(d_op), T * F * C, 1, F * C, C)
    if mode == R.MASK:
        be.lib.mask_istft(*a, B, C, T, n_fft, hop, length, be.ptr(out), None, **rag)
    elif mode == R.PHASE:
        be.lib.phase_istft(*a, be.ptr(d_ph), B * T * F * 2, B, C, T, n_fft, hop, length, be.ptr(out), None, **rag)
    else:
        be.lib.mag_istft(*a, B, C, T, n_fft, hop, length, be.ptr(out), None, **rag)
    return be.host(out)


def run_backward(be, mode, ri, op, phases, n_fft, hop, gy, frames=None, lengths=None, op_view=None):
    """g_op (B,T,F,C), g_ph (C,B,T,F,2) float32 (NaN-filled before the call) through onssen_istft_backward_f32.  ``op_view``:
    a function of the backend that returns the operand as a strided view on the device instead of a copy of ``op``."""
    B, T, F, C = op.shape
    length = gy.shape[2]
    d_ri, d_ph, d_gy = be.dev(ri), be.dev(phases), be.dev(gy)
    d_op = op_view(be) if op_view else be.dev(op)
    sb, st, sf, sc = be.strides(d_op)
    g_op = be.dev(np.full((B, T, F, C), np.nan, np.float32))
    g_ph = be.dev(np.full((C, B, T, F, 2), np.nan, np.float32)) if mode == R.PHASE else None
    fr = None if frames is None else be.dev(np.asarray(frames, np.int32))
    ln = None if lengths is None else be.dev(np.asarray(lengths, np.int32))
    be.lib.istft_backward(be.ptr(d_ri), be.ptr(d_op) if mode == R.PHASE else None, sb, sc, st, sf,
                          be.ptr(d_ph) if mode == R.PHASE else None, B * T * F * 2, mode, B, C, T, n_fft, hop, length, be.ptr(d_gy),
                          be.ptr(g_op), be.ptr(g_ph), None, frames=be.ptr(fr), lengths=be.ptr(ln))
    return be.host(g_op), (be.host(g_ph) if g_ph is not None else None)


def grad_errors(be, mode, shape, ragged=False, op_view=None):
    """[(what, max |got - ref|, max |ref|)] of one case against the float64 adjoint."""
    k = R.case(*shape)
    frames, lengths = R.ragged_extents(k) if ragged else (None, None)
    g_op, g_ph = run_backward(be, mode, k.ri, R.operand_of(k, mode), k.phases, k.n_fft, k.hop, k.gy, frames, lengths, op_view)
    r_op, r_ph = R.reference(*shape, mode, ragged)
    assert np.isfinite(g_op).all()
    out = [("g_" + ("mag" if mode == R.MAG else "mask"), np.abs(g_op - r_op).max(), np.abs(r_op).max())]
    if mode == R.PHASE:
        assert np.isfinite(g_ph).all()
        out.append(("g_phase", np.abs(g_ph - r_ph).max(), np.abs(r_ph).max()))
    return out


def check_gradient(be, mode, shape, ragged=False, op_view=None):
    for what, err, top in grad_errors(be, mode, shape, ragged, op_view):
        bound = R.GRAD_BOUND[(mode, what)]
        print(f"{R.MODE_NAMES[mode]} {shape}{' ragged' if ragged else ''} {what}: max |got - ref| {err:.3e}, max |ref| {top:.3e} "
              f"({err / top:.2e} relative), bound {bound:.3e}, ceiling {1e-5 * top:.3e}")
        assert err <= 1e-5 * top, (what, err, top)
        assert err <= bound, (what, err, bound)
        assert err <= R.GRAD_REL_BOUND * top, (what, err / top, R.GRAD_REL_BOUND)


def check_dot_product(be, mode, shape, seed=0):
    """<istft(m), g> = <m, istft_bwd(g)> through the ABI alone, random float32 m and g, sums in float64; in the phase mode the map
    is bilinear: linear in the masks with the phases fixed, and in the phases with the masks fixed -- both are checked."""
    k = R.case(*shape)
    rng = np.random.default_rng(seed + 17)
    B, T, F, C, n = k.B, k.T, k.F, k.C, k.n
    m = rng.standard_normal((B, T, F, C)).astype(np.float32)
    p = rng.standard_normal((C, B, T, F, 2)).astype(np.float32)
    g = rng.standard_normal((B, C, n)).astype(np.float32)
    y = run_forward(be, mode, k.ri, m, p, k.n_fft, k.hop, n).astype(np.float64)
    g_op, g_ph = run_backward(be, mode, k.ri, m, p, k.n_fft, k.hop, g)
    lhs = float((y * g.astype(np.float64)).sum())
    scale = float(np.linalg.norm(y) * np.linalg.norm(g.astype(np.float64)))
    sides = [("operand", float((m.astype(np.float64) * g_op.astype(np.float64)).sum()))]
    if mode == R.PHASE:
        sides.append(("phases", float((p.astype(np.float64) * g_ph.astype(np.float64)).sum())))
    # the float64 restatement of the forward with the kernel's float32 rounding of the frames, against the float64 adjoint
    yr = np.stack([R.forward(k.ri[b], m[b], mode, k.hop, n, p[:, b], f32_frames=True) for b in range(B)])
    gr = sum(float((m[b].astype(np.float64) * R.adjoint(k.ri[b], m[b], mode, k.hop, g[b], p[:, b])[0]).sum()) for b in range(B))
    restated = abs(float((yr * g.astype(np.float64)).sum()) - gr) / scale
    for what, rhs in sides:
        rel = abs(lhs - rhs) / scale
        print(f"{R.MODE_NAMES[mode]} {shape} {what}: |<istft(m), g> - <m, istft_bwd(g)>| / (|istft(m)| |g|) = {rel:.3e} "
              f"(bound 1e-5; the float64 restatement with float32 frames gives {restated:.3e})")
        assert restated <= 1e-5, restated          # (otherwise the issue's fallback, 4 x restated, would apply)
        assert rel <= 1e-5, (what, rel)


def check_ragged(be, mode):
    """Row b inside frames[b] is bit for bit the batch-1 call on that utterance; exactly 0 for t >= frames[b]; gy beyond
    lengths[b] (NaN here) and X / operand / phases beyond frames[b] (NaN here) do not reach the result."""
    shape = R.RAGGED_SHAPE
    k = R.case(*shape)
    frames, lengths = R.ragged_extents(k)
    ri, op, ph, gy = k.ri.copy(), R.operand_of(k, mode).copy(), k.phases.copy(), k.gy.copy()
    for b, (Tb, nb) in enumerate(zip(frames, lengths)):
        ri[b, Tb:] = np.nan
        op[b, Tb:] = np.nan
        ph[:, b, Tb:] = np.nan
        gy[b, :, nb:] = np.nan
    g_op, g_ph = run_backward(be, mode, ri, op, ph, k.n_fft, k.hop, gy, frames, lengths)
    assert np.isfinite(g_op).all() and (g_ph is None or np.isfinite(g_ph).all())
    for b, (Tb, nb) in enumerate(zip(frames, lengths)):
        one_op, one_ph = run_backward(be, mode, np.ascontiguousarray(ri[b:b + 1, :Tb]), np.ascontiguousarray(op[b:b + 1, :Tb]),
                                      np.ascontiguousarray(ph[:, b:b + 1, :Tb]), k.n_fft, k.hop, np.ascontiguousarray(gy[b:b + 1, :, :nb]))
        assert g_op[b, :Tb].tobytes() == one_op[0].tobytes(), b
        assert (g_op[b, Tb:] == 0).all(), b
        if mode == R.PHASE:
            assert g_ph[:, b, :Tb].tobytes() == one_ph[:, 0].tobytes(), b
            assert (g_ph[:, b, Tb:] == 0).all(), b
    check_gradient(be, mode, shape, ragged=True)


def strided_view(k, mode):
    """The operand as a view of a larger NaN-filled buffer with its own batch, frame, bin and speaker strides."""
    def make(be):
        big = np.full((k.B, k.T + 2, k.F + 3, k.C + 1), np.nan, np.float32)
        big[:, :k.T, :k.F, :k.C] = R.operand_of(k, mode)
        return be.dev(big)[:, :k.T, :k.F, :k.C]
    return make


def check_repeatable(be, mode, shape):
    k = R.case(*shape)
    a = run_backward(be, mode, k.ri, R.operand_of(k, mode), k.phases, k.n_fft, k.hop, k.gy)
    b = run_backward(be, mode, k.ri, R.operand_of(k, mode), k.phases, k.n_fft, k.hop, k.gy)
    assert a[0].tobytes() == b[0].tobytes()
    assert mode != R.PHASE or a[1].tobytes() == b[1].tobytes()


def check_istft_bwd_refusals(be):
    """Every refused argument returns its code before anything is launched: the sentinel-filled outputs are unchanged."""
    k = R.case(256, 64, 12, 4)
    B, T, F, C, n = k.B, k.T, k.F, k.C, k.n
    ri, op, ph, gy = be.dev(k.ri), be.dev(k.masks), be.dev(k.phases), be.dev(k.gy)
    g_op = be.dev(np.full((B, T, F, C), 7.0, np.float32))
    g_ph = be.dev(np.full((C, B, T, F, 2), 7.0, np.float32))
    fr, ln = be.dev(np.full(B, T, np.int32)), be.dev(np.full(B, n, np.int32))
    f = be.lib.dll.onssen_istft_backward_f32
    P = be.ptr

    def args(mode=R.PHASE, ri=P(ri), op=P(op), ph=P(ph), p_sc=B * T * F * 2, B=B, C=C, T=T, frames=None, n_fft=256, hop=64, length=n,
             lengths=None, gy=P(gy), g_op=P(g_op), g_ph=P(g_ph)):
        return (ri, op, T * F * C, 1, F * C, C, ph, p_sc, mode, B, C, T, frames, n_fft, hop, length, lengths, gy, g_op, g_ph, None)

    bad = [dict(ri=None), dict(gy=None), dict(g_op=None), dict(op=None), dict(ph=None), dict(g_ph=None), dict(B=0), dict(C=0),
           dict(hop=0), dict(hop=-1), dict(hop=257), dict(n_fft=128), dict(n_fft=2048), dict(n_fft=300), dict(frames=P(fr)),
           dict(lengths=P(ln)), dict(mode=3), dict(mode=-1), dict(T=0), dict(length=0)]
    for kw in bad:
        assert f(*args(**kw)) == E_ARG, kw
    for mode in (R.MASK, R.MAG):
        for kw in [dict(ri=None), dict(gy=None), dict(g_op=None), dict(frames=P(fr)), dict(n_fft=2048)]:
            assert f(*args(mode=mode, **kw)) == E_ARG, (mode, kw)
    assert f(*args(ph=P(ph) + 4)) == E_ALIGN and f(*args(g_ph=P(g_ph) + 4)) == E_ALIGN
    g1, g2 = be.host(g_op), be.host(g_ph)
    assert (g1 == 7.0).all() and (g2 == 7.0).all()
    # what is not required is not asked for: no operand, phase or g_phase outside the phase mode; both extents together
    assert f(*args(mode=R.MASK, op=None, ph=None, g_ph=None)) == 0
    assert f(*args(mode=R.MAG, op=None, ph=None, g_ph=None)) == 0
    assert f(*args(frames=P(fr), lengths=P(ln))) == 0
    be.sync()


# ------------------------------------------------------------------------------------------------- the waveform loss
def run_wa(be, est, ref_view, lengths, g_value, sentinel=np.nan):
    """value (B,), perm (B,), total, d_est (B,C,n) through the C ABI; ``ref_view(be)`` returns the references on the device."""
    B, C, n = est.shape
    d_est_in, d_ref = be.dev(est), ref_view(be)
    r_sb, r_sc, one = be.strides(d_ref)
    assert one == 1
    nb = be.lib.wa_pit_workspace_bytes(B, C)
    ws = be.dev(np.full(nb // 8 + 1, np.nan, np.float64))            # needs no zeroing
    value, total = be.dev(np.full(B, sentinel, np.float32)), be.dev(np.full(1, sentinel, np.float32))
    perm = be.dev(np.full(B, -1, np.int32))
    ln = None if lengths is None else be.dev(np.asarray(lengths, np.int32))
    be.lib.wa_pit(be.ptr(d_est_in), be.ptr(d_ref), r_sb, r_sc, B, C, n, be.ptr(ln), be.ptr(value), be.ptr(perm), be.ptr(total),
                  be.ptr(ws), nb, None)
    gv = be.dev(np.asarray(g_value, np.float32))
    d_est = be.dev(np.full((B, C, n), sentinel, np.float32))
    be.lib.wa_pit_backward(be.ptr(d_est_in), be.ptr(d_ref), r_sb, r_sc, B, C, n, be.ptr(ln), be.ptr(gv), None, be.ptr(d_est), be.ptr(ws),
                           nb, None)
    return be.host(value), be.host(perm), be.host(total), be.host(d_est)


def check_wa(be, C, n, ragged=False, strided=False, tie=False):
    from tests import wa_pit_cases as W
    k = W.case(C, n, ragged, tie)
    view = W.strided_ref(k) if strided else (lambda be: be.dev(k.ref))
    value, perm, total, d_est = run_wa(be, k.est, view, k.lengths, k.g_value)
    rel = np.abs(value.astype(np.float64) - k.V) / np.abs(k.V)
    print(f"C {C} n {n}{' ragged' if ragged else ''}{' strided' if strided else ''}{' tie' if tie else ''}: max |V - V_ref| / |V_ref| "
          f"{rel.max():.3e} (bound 1e-6), perm {perm.tolist()}")
    assert (rel <= 1e-6).all(), rel
    assert perm.tolist() == k.perm_index, (perm.tolist(), k.perm_index)
    assert abs(float(total[0]) - k.V.mean()) <= 1e-6 * abs(k.V.mean())
    assert d_est.tobytes() == k.grad.astype(np.float32).tobytes()
    assert (d_est[k.planted] == 0).all()
    if k.lengths is not None:
        for b, nb in enumerate(k.lengths):
            assert (d_est[b, :, nb:] == 0).all()
    again = run_wa(be, k.est, view, k.lengths, k.g_value)
    assert value.tobytes() == again[0].tobytes() and d_est.tobytes() == again[3].tobytes() and total.tobytes() == again[2].tobytes()


def check_wa_refusals(be):
    from tests import wa_pit_cases as W
    k = W.case(2, 777)
    B, C, n = k.est.shape
    est, ref = be.dev(k.est), be.dev(k.ref)
    nb = be.lib.wa_pit_workspace_bytes(B, C)
    ws = be.dev(np.zeros(nb // 8 + 1, np.float64))
    value, total, perm = be.dev(np.full(B, 7.0, np.float32)), be.dev(np.full(1, 7.0, np.float32)), be.dev(np.full(B, 7, np.int32))
    d_est, gv = be.dev(np.full((B, C, n), 7.0, np.float32)), be.dev(np.ones(B, np.float32))
    P = be.ptr
    fwd, bwd = be.lib.dll.onssen_wa_pit_f32, be.lib.dll.onssen_wa_pit_backward_f32
    assert be.lib.dll.onssen_wa_pit_workspace_bytes(B, 5) == 0 and be.lib.dll.onssen_wa_pit_workspace_bytes(0, 2) == 0

    def fa(est=P(est), ref=P(ref), r_sb=C * n, r_sc=n, B=B, C=C, n=n, value=P(value), ws=P(ws), nb=nb):
        return (est, ref, r_sb, r_sc, B, C, n, None, value, P(perm), P(total), ws, nb, None)

    def ba(est=P(est), ref=P(ref), r_sb=C * n, r_sc=n, B=B, C=C, n=n, gv=P(gv), d_est=P(d_est), ws=P(ws), nb=nb):
        return (est, ref, r_sb, r_sc, B, C, n, None, gv, None, d_est, ws, nb, None)

    common = [dict(est=None), dict(ref=None), dict(ws=None), dict(B=0), dict(C=0), dict(C=5), dict(n=0), dict(r_sc=n - 1), dict(r_sb=n - 1)]
    for kw in common:
        assert fwd(*fa(**kw)) == E_ARG, kw
        assert bwd(*ba(**kw)) == E_ARG, kw
    assert fwd(*fa(value=None)) == E_ARG and bwd(*ba(d_est=None)) == E_ARG and bwd(*ba(gv=None)) == E_ARG
    assert fwd(*fa(nb=nb - 1)) == E_WORKSPACE and bwd(*ba(nb=nb - 1)) == E_WORKSPACE
    assert fwd(*fa(ws=P(ws) + 4)) == E_ALIGN and bwd(*ba(ws=P(ws) + 4)) == E_ALIGN
    be.sync()
    assert (be.host(value) == 7.0).all() and (be.host(total) == 7.0).all() and (be.host(perm) == 7).all() and (be.host(d_est) == 7.0).all()
    assert fwd(*fa()) == 0 and bwd(*ba()) == 0
    be.sync()
