"""onssen_loss_phase_f32 / onssen_loss_phase_grad_f32 in the host-side build (tests/emu) against the float64 restatement
(tests/loss_phase_ref.py): value of both terms, the assignment with its strict tie rule, the gradient of the masks and of the
phase estimates, bit-repeatability.  Bounds (none of them taken from the kernels' output):
  value     |out - ref| <= 1e-5 * sum_bins 2 x for either term: every bin contributes a few fp32 roundings of a quantity bounded
            by x (mask residual) or by 2 x (two cosines), summed in fp64 -- about 5e-7 relative at worst, a 20-fold margin; the
            grade of the chimera mask term's rtol = 1e-5
  d masks   exactly float32(g * x) * sign: the product of two floats rounds once whether it is formed in fp32 or in fp64, and
            the residual is a fused multiply-add, whose sign is the exact one
  d phases  within 1e-5 * |g| x / max(|p|, eps) elementwise: (q^ - <p^, q^> p^) has entries bounded by 1 and an absolute fp32
            error of a few 1e-7, divided by the (clamped) norm"""
import numpy as np
import pytest
import torch

from tests import loss_phase_ref as R
from tests.emu_build import load_emu


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return a.ctypes.data


def aligned_bytes(n, fill, align=256):
    raw = np.full(n + align, fill, np.uint8)
    off = -raw.ctypes.data % align
    return raw[off:off + n]


def run(lib, c, g_mask, g_phase):
    B = c["x"].shape[0]
    TF = c["x"][0].size
    masks = c["masks"]
    out_mask, out_phase, perm = np.full(B, np.nan, np.float32), np.full(B, np.nan, np.float32), np.full(B, -1, np.int32)
    ws = aligned_bytes(lib.loss_phase_workspace_bytes(B), 0xA5)          # the workspace needs no zeroing
    maps = (P(c["x"]), P(c["s1"]), P(c["s2"]), P(c["pA"]), P(c["pB"]), P(c["q1"]), P(c["q2"]))
    lib.loss_phase(P(masks), P(masks) + 4, 2 * TF, 2, *maps, B, TF, P(out_mask), P(out_phase), P(perm), P(ws), ws.nbytes, None)
    d = np.full(masks.shape, np.nan, np.float32)
    dpa, dpb = np.full(c["pA"].shape, np.nan, np.float32), np.full(c["pB"].shape, np.nan, np.float32)
    lib.loss_phase_grad(P(masks), P(masks) + 4, 2 * TF, 2, *maps, B, TF, P(g_mask), P(g_phase), P(perm), P(d), P(d) + 4, 2 * TF, 2,
                        P(dpa), P(dpb), None)
    return out_mask, out_phase, perm, d, dpa, dpb


def test_restatement_matches_float64_autograd():
    """tests/loss_phase_ref.py (closed forms) against torch autograd of the same loss written with F.cosine_similarity, in
    float64: values to 1e-12 relative, gradients to 1e-9 of their bound -- the bins at the clamp included."""
    import torch.nn.functional as F
    c = R.planted_case(4, (63,), seed=3)
    t = {k: torch.from_numpy(v).double() for k, v in c.items()}
    m, pA, pB = t["masks"].requires_grad_(True), t["pA"].requires_grad_(True), t["pB"].requires_grad_(True)
    mA, mB, x = m[..., 0], m[..., 1], t["x"]
    l1 = (mA * x - t["s1"]).abs().sum(1) + (mB * x - t["s2"]).abs().sum(1)
    l2 = (mB * x - t["s1"]).abs().sum(1) + (mA * x - t["s2"]).abs().sum(1)
    cs = lambda p, q: (x * F.cosine_similarity(p, q, dim=-1)).sum(1)
    p1, p2 = -cs(pA, t["q1"]) - cs(pB, t["q2"]), -cs(pB, t["q1"]) - cs(pA, t["q2"])
    amin = l1 < l2
    lm, lp = torch.where(amin, l1, l2), torch.where(amin, p1, p2)
    g_mask, g_phase = torch.tensor([0.7, -1.3, 0.4, 2.0]).double(), torch.tensor([-0.6, 1.1, 0.9, -1.7]).double()
    gm, gpa, gpb = torch.autograd.grad((lm * g_mask).sum() + (lp * g_phase).sum(), [m, pA, pB])
    args = (c["masks"][..., 0], c["masks"][..., 1], c["pA"], c["pB"], c["x"], c["s1"], c["s2"], c["q1"], c["q2"])
    rm, rp, perm = R.terms(*args)
    assert perm.tolist() == [0, 1, 1, int(perm[3])] and perm.tolist() == (~amin).int().tolist()
    np.testing.assert_allclose(rm.numpy(), lm.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(rp.numpy(), lp.detach().numpy(), rtol=1e-12)
    dA, dB, dpA, dpB = R.grads(*args, perm, g_mask, g_phase)
    np.testing.assert_array_equal(torch.stack([dA, dB], -1).numpy(), gm.numpy())
    for ref, got, p in ((dpA, gpa, t["pA"]), (dpB, gpb, t["pB"])):
        bound = 1e-9 * (x / R._norm(p.detach()).clamp_min(R.EPS)).unsqueeze(-1) * 2.0
        print("restatement vs autograd, phase gradient: max |diff| / bound", float(((ref - got).abs() / bound).max()))
        assert ((ref - got).abs() <= bound).all()
    zg, zr = (gpb, dpB) if int(perm[3]) else (gpa, dpA)          # the estimate that phase_s1 = (0, 0) is assigned to
    assert float(zg[3, 0].abs().max()) == 0.0 and float(zr[3, 0].abs().max()) == 0.0         # zero target: zero gradient
    assert float(dpA[3, 1].abs().max()) > 1e6                                                # |p| = 1e-9: divided by eps, not by |p|


@pytest.mark.parametrize("B,TF", [(4, 63), (3, 700)])
def test_loss_phase_value_and_gradient(lib, B, TF):
    c = R.planted_case(B, (TF,), seed=5 + B)
    rng = np.random.default_rng(B)
    g_mask, g_phase = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    out_mask, out_phase, perm, d, dpa, dpb = run(lib, c, g_mask, g_phase)
    args = (c["masks"][..., 0], c["masks"][..., 1], c["pA"], c["pB"], c["x"], c["s1"], c["s2"], c["q1"], c["q2"])
    rm, rp, rperm = R.terms(*args)
    np.testing.assert_array_equal(perm, rperm.numpy())
    assert perm[0] == 0 and perm[1] == 1 and perm[2] == 1, perm            # straight, swapped, and the tie swapped
    # the tie row's two assignments differ in the phase term (distinct phase labels): the value shows which one was taken
    _, p_straight, _ = R.terms(args[0], args[1], args[2], args[3], *args[4:7], c["q2"], c["q1"])
    assert abs(float(p_straight[2] - rp[2])) > 1.0
    bound = 1e-5 * 2.0 * c["x"].astype(np.float64).sum(1)
    print("mask term  |out - ref| / bound", np.abs(out_mask - rm.numpy()) / bound)
    print("phase term |out - ref| / bound", np.abs(out_phase - rp.numpy()) / bound)
    assert (np.abs(out_mask - rm.numpy()) <= bound).all() and (np.abs(out_phase - rp.numpy()) <= bound).all()
    dA, dB, dpA, dpB = R.grads(*args, rperm, g_mask, g_phase)
    np.testing.assert_array_equal(d, torch.stack([dA, dB], -1).numpy().astype(np.float32))
    assert d[B - 1, 2, perm[B - 1]] == 0.0                                   # the exactly-zero residual of the mask assigned to s1
    xg = np.abs(g_phase.astype(np.float64))[:, None] * c["x"]
    for got, ref, p in ((dpa, dpA, c["pA"]), (dpb, dpB, c["pB"])):
        pb = 1e-5 * xg / np.maximum(np.linalg.norm(p.astype(np.float64), axis=-1), R.EPS)
        err = np.abs(got - ref.numpy()).max(-1)
        print("phase gradient max |err| / bound", (err / pb).max())
        assert np.isfinite(got).all() and (err <= pb).all()
    assert np.all((dpb if perm[B - 1] else dpa)[B - 1, 0] == 0.0)            # phase_s1 = (0, 0): a zero target, a zero gradient
    # the same call again: identical bits
    again = run(lib, c, g_mask, g_phase)
    for a, b in zip((out_mask, out_phase, perm, d, dpa, dpb), again):
        assert a.tobytes() == b.tobytes()
