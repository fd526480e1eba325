"""The MISI half-step (csrc/misi.inc) restated in float64 with its explicit adjoint, a torch float64 forward that autograd
differentiates, and the reference of K unfolded iterations -- the reference of tests/test_emu_misi_bwd.py,
tests/test_gpu_misi_bwd.py, tests/test_misi_grad_api.py and tests/test_gpu_misi_train_e2e.py.

    forward :  u_c = s_c + (x - sum_j s_j) / C,  Z_c = rfft(w * frames(reflect-padded u_c)),  p_c = Z_c / |Z_c|, (1, 0) at Z = 0
               (tests/misi_ref.py: misi_spectra, unit)
    adjoint :  g_Z = (g_p - p (p . g_p)) / |Z|, 0 where Z = 0
               r_t = N w * irfft(H),  H = g_Z / 2 inside, Re g_Z at DC / Nyquist  (irfft divides by N and doubles the inside bins)
               g_u = overlap-add of r_t on the padded axis, the reflect padding folded back:
                     padded q < N/2 adds to sample N/2 - q,  q >= N/2 + n adds to sample 2 (n - 1) - (q - N/2)
               g_s_c = g_u_c - (1 / C) sum_j g_u_j

``self_check`` compares the adjoint with torch float64 autograd of ``torch_half_step`` on the CPU.  Every reference is built once
per process and must be left unchanged."""
import functools

import numpy as np

from oracle import np_oracle as O
from tests import istft_grad_ref as IR
from tests import misi_cases as MC
from tests import misi_ref as R

# (n_fft, hop, samples, speakers) of the half-step's gradient tests: the forward's shapes, the shortest legal signal (n = N/2 + 1:
# both mirrors fall on the same samples) and one with n not a multiple of hop, the 8-estimate fetch path and an odd C
SHAPES = list(MC.SHAPES) + [(256, 64, 129, 2), (256, 64, 777, 5)]
RAGGED_SHAPES = [(256, 64, 768, 2), (256, 100, 1500, 3)]     # three rows each, lengths ``ragged_lengths``


def ragged_lengths(n_fft, hop, n):
    return [n, n - 3 * hop - 5, n_fft // 2 + hop + 1]


def half_step_adjoint(mix, est, n_fft, hop, g_p):
    """One utterance: mix (n,), est (C, n), g_p (C, T, F, 2) the gradient at misi_ref.misi_phase's unit vectors -> the gradient
    at est (C, n), float64.  The float32 inputs are taken as they are; everything after them is float64."""
    est = np.asarray(est, dtype=np.float64)
    g_p = np.asarray(g_p, dtype=np.float64)
    C, n = est.shape
    half = n_fft // 2
    Z = R.misi_spectra(mix, est, n_fft, hop)                      # (C, T, F) complex128
    T = Z.shape[1]
    h = np.abs(Z)
    nz = h > 0
    safe = np.where(nz, h, 1.0)
    p = R.unit(Z)
    dot = (p * g_p).sum(-1)
    g_Z = np.where(nz[..., None], (g_p - p * dot[..., None]) / safe[..., None], 0.0)
    H = 0.5 * (g_Z[..., 0] + 1j * g_Z[..., 1])
    H[..., 0] = g_Z[..., 0, 0]
    H[..., -1] = g_Z[..., -1, 0]
    r = np.fft.irfft(H, n=n_fft, axis=-1) * n_fft * O.hann_periodic(n_fft)[None, None, :]
    y = np.zeros((C, n + n_fft))
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += r[:, t]
    g_u = y[:, half:half + n].copy()
    for q in range(half):
        g_u[:, half - q] += y[:, q]
    for q in range(half + n, n + n_fft):
        g_u[:, 2 * (n - 1) - (q - half)] += y[:, q]
    total = g_u[0].copy()
    for j in range(1, C):
        total = total + g_u[j]
    return g_u - total[None] / C


def torch_half_step(mix, est, n_fft, hop):
    """The half-step in torch float64 on the CPU: mix (n,) array or tensor, est (C, n) tensor (may require grad) ->
    (C, T, F, 2) unit vectors, (1, 0) where Z = 0."""
    import torch
    mix = torch.as_tensor(np.asarray(mix, dtype=np.float64)) if not torch.is_tensor(mix) else mix.double()
    C, n = est.shape
    total = est[0]
    for j in range(1, C):
        total = total + est[j]
    u = est + ((mix - total) / C)[None]
    pad = torch.nn.functional.pad(u[None], (n_fft // 2, n_fft // 2), mode="reflect")[0]
    fr = pad.unfold(-1, n_fft, hop) * torch.from_numpy(O.hann_periodic(n_fft))[None, None, :]
    Z = torch.fft.rfft(fr, dim=-1)
    zr, zi = Z.real, Z.imag
    nz = (zr != 0) | (zi != 0)
    h = torch.sqrt(torch.where(nz, zr * zr + zi * zi, torch.ones_like(zr)))
    return torch.stack([torch.where(nz, zr / h, torch.ones_like(zr)), torch.where(nz, zi / h, torch.zeros_like(zi))], -1)


@functools.lru_cache(maxsize=None)
def g_phase(n_fft, hop, n, C, B=2):
    """g_p (C, B, T, F, 2) float32 ~ N(0, 1): the gradient arriving at the phase maps of ``misi_cases.case``."""
    k = MC.case(n_fft, hop, n, C, B)
    g = np.random.default_rng(4100 + n_fft + hop + 7 * C + n).standard_normal((C, B, k.T, k.F, 2)).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(n_fft, hop, n, C, B=2, lengths=None):
    """g_est (B, C, n) float64 of the case; ``lengths``: a tuple of the rows' own lengths (zeros after them)."""
    k, g = MC.case(n_fft, hop, n, C, B), g_phase(n_fft, hop, n, C, B)
    out = np.zeros((B, C, n))
    for b in range(B):
        nb = n if lengths is None else lengths[b]
        Tb = 1 + nb // hop
        out[b, :, :nb] = half_step_adjoint(k.mix[b, :nb], k.est[b, :, :nb], n_fft, hop, g[:, b, :Tb])
    out.setflags(write=False)
    return out


def self_check():
    """The explicit adjoint against torch float64 autograd of ``torch_half_step``, three shapes (a hop that does not divide the
    window with an odd C; the 2 * 4^k length; the shortest legal signal).  Returns the largest relative difference."""
    import torch
    worst = 0.0
    for shape in [(256, 64, 768, 2), (256, 100, 1500, 3), (512, 128, 2048, 2), (256, 64, 129, 2)]:
        n_fft, hop, n, C = shape
        k, g = MC.case(*shape), g_phase(*shape)
        est = torch.from_numpy(k.est[0].astype(np.float64)).requires_grad_(True)
        p = torch_half_step(k.mix[0], est, n_fft, hop)
        np.testing.assert_allclose(p.detach().numpy(), R.misi_phase(k.mix[0], k.est[0], n_fft, hop)[0], rtol=0, atol=1e-9)
        (p * torch.from_numpy(g[:, 0].astype(np.float64))).sum().backward()
        ref = half_step_adjoint(k.mix[0], k.est[0], n_fft, hop, g[:, 0])
        worst = max(worst, np.abs(est.grad.numpy() - ref).max() / np.abs(ref).max())
    return worst


def unfolded_gradient(ri, masks, mix, hop, n, iters, gy, phases=None):
    """One utterance, torch float64 autograd through the whole chain: ri (T, F, 2) f32, masks (T, F, C), mix (n,) f32, gy (C, n)
    the gradient at the final estimates, ``phases`` (C, T, F, 2) starting phases or None for the mixture's ->
    (est (C, n), d<est, gy>/d masks (T, F, C), d/d phases or None), float64 arrays."""
    import torch
    n_fft = 2 * (ri.shape[1] - 1)
    m = torch.from_numpy(np.asarray(masks, dtype=np.float64)).requires_grad_(True)
    p0 = None if phases is None else torch.from_numpy(np.asarray(phases, dtype=np.float64)).requires_grad_(True)
    if p0 is None:
        est = IR.torch_forward(ri, m, IR.MASK, hop, n)
    else:
        est = IR.torch_forward(ri, m, IR.PHASE, hop, n, p0)
    for _ in range(iters):
        est = IR.torch_forward(ri, m, IR.PHASE, hop, n, torch_half_step(mix, est, n_fft, hop))
    (est * torch.from_numpy(np.asarray(gy, dtype=np.float64))).sum().backward()
    return est.detach().numpy(), m.grad.numpy(), None if p0 is None else p0.grad.numpy()


class Case:
    pass


@functools.lru_cache(maxsize=None)
def chain_case(C=2, B=2, T=13, n_fft=256, hop=64):
    """The inputs of the whole-chain tests: ri (B,T,F,2) f32 spectra of synthetic C-speaker mixtures of n = hop (T - 1) samples,
    src (B,C,n) f32 their sources, masks (B,T,F,C) f32 in [0, 1), phases (C,B,T,F,2) f32 unit vectors."""
    from onssen_amd.synthetic import synth_mixture_k
    rng = np.random.default_rng(5200 + 7 * C + T)
    c = Case()
    n = hop * (T - 1)
    sigs = [synth_mixture_k(70 + b, n, num_speaker=C) for b in range(B)]
    X = [O.stft(np.asarray(s[0], dtype=np.float32), n_fft, hop) for s in sigs]
    c.src = np.ascontiguousarray(np.stack([np.stack(s[1:]) for s in sigs]), dtype=np.float32)
    c.ri = np.ascontiguousarray(np.stack([np.stack([x.real, x.imag], -1) for x in X]), dtype=np.float32)
    c.F = n_fft // 2 + 1
    assert c.ri.shape == (B, T, c.F, 2)
    c.masks = rng.random((B, T, c.F, C)).astype(np.float32)
    p = rng.standard_normal((C, B, T, c.F, 2))
    c.phases = np.ascontiguousarray(p / np.linalg.norm(p, axis=-1, keepdims=True), dtype=np.float32)
    c.B, c.C, c.T, c.n, c.n_fft, c.hop = B, C, T, n, n_fft, hop
    for a in (c.src, c.ri, c.masks, c.phases):
        a.setflags(write=False)
    return c


# Bounds of the half-step's gradient tests: 4 x the largest max |got - ref| / max |ref| measured on the host-side build over all
# of SHAPES (the device's hypot and contraction differ from the host's); the hard ceiling per case is 1e-5 max |ref|.  The
# reference alone is stable on these inputs (float64-rounding-sized perturbations of est move it by <= 2e-11 max |ref|; the
# weakest bin has |Z| >= 5e-8 max |Z|), so nothing is left out.  Per-shape values: DESIGN section 25.
GRAD_MEASURED_REL = 4.73e-08       # (256, 64, 2000, 4); the smallest is 3.03e-08 at (256, 100, 1500, 3): one float32 rounding of the result
GRAD_REL_BOUND = 4 * GRAD_MEASURED_REL
# Whole chain (tests/test_emu_misi_bwd.py, tests/test_gpu_misi_train_e2e.py): the same rule on d loss / d masks of ``chain_case``
# through K unfolded iterations, ceiling 1e-4 max |ref| -- float32 estimates and phases between the iterations shift the point
# of linearisation (MC.ITER_BOUND's reasoning).  Measured on the host-side build: K = 1 3.32e-07, K = 2 1.69e-07.
CHAIN_MEASURED_REL = 3.32e-07
CHAIN_REL_BOUND = 4 * CHAIN_MEASURED_REL
