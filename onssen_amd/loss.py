"""Training losses needed by the data-parallel step.

Chimera losses (onssen/loss/loss_chimera.py): the deep-clustering term as below, the mask-inference term on
``onssen_loss_mask_f32`` (value; the winning speaker assignment) and ``onssen_loss_mask_grad_f32`` (gradient, one pass;
csrc/loss_mask.inc).
On a GPU the loss_dc value comes from ``onssen_loss_dc_f32`` (one pass over the embedding builds the Gram of ``[V | Y]``) and, when
autograd needs it, the gradient from ``onssen_loss_dc_grad_f32`` (``dV = Z M`` from the same Gram: one more pass); on the CPU
(tests, the gloo path) PyTorch ops with the same single-Gram forward and analytic backward.  ``ONSSEN_LOSS_HIP=0`` keeps the
PyTorch form on the GPU.
The phase network's loss (``loss_phase``): the same deep-clustering term, and the mask term and cosine phase term from
``onssen_loss_phase_f32`` / ``onssen_loss_phase_grad_f32`` (one pass over the eleven maps forward, one elementwise pass backward).
The enhancement losses (``loss_mask_msa`` / ``loss_mask_psa``, onssen/loss/loss_mask.py): one estimate against one target, value from
``onssen_loss_enhance_f32`` and gradient from ``onssen_loss_enhance_grad_f32`` (csrc/enhance.inc).
The uPIT losses (``loss_upit_msa`` / ``loss_upit_psa``; upstream has none): the permutation-invariant mask loss for 2 .. 4 speakers on
``onssen_loss_upit_f32`` / ``onssen_loss_upit_grad_f32`` (csrc/loss_upit.inc).

Routing.  The chimera mask term, the enhancement losses and the uPIT losses choose their form in ``_route``: "value" (ROCm tensors
and no gradient wanted: the value kernel alone), "grad" (a gradient wanted and option ``loss`` = "1": an autograd node over the value
and the gradient kernel), else "aten" (PyTorch ops; always on the CPU, and for what the kernels do not take).  Two losses route by
rules of their own: ``loss_dc`` (its kernels bound D + C and, for the gradient, C) and ``loss_phase`` (HIP whenever
option ``loss`` = "1", with or without a gradient: "hip" | "aten").  ``last_enhance_path`` / ``last_upit_path`` /
``last_phase_path`` / ``last_si_snr_path`` say which route the last call of a family took.

Plane buffers.  The mask networks write their S masks as the planes ``buf[..., k]`` of one contiguous fp32 (..., S) buffer.
``_planes_base`` hands that buffer itself to the kernels and to autograd when the masks are exactly its planes (the graph then runs
through the root tensor, not through S select views whose gradients would be scattered into zeros and added); anything else is
interleaved by ``torch.stack`` first.  Every mask-family node takes the (..., S) buffer; labels are detached fp32 contiguous maps,
workspaces are allocated per call (nothing cached: every route can be captured in a graph).
The waveform-approximation loss (``wa_pit`` / ``loss_wa``; upstream has none): the network's masks go through one differentiable
inverse transform (features.mask_istft / phase_istft / mag_istft, backward csrc/istft_bwd.inc) and the waveforms are compared in L1
under the best speaker permutation on ``onssen_wa_pit_f32`` / ``onssen_wa_pit_backward_f32`` (csrc/loss_wa.inc).
Semantics follow onssen/loss/loss_dc.py:6-44 and loss_util.py:4-11 exactly,
including their quirks: the affinity terms are Frobenius *norms* (not squared
norms) and the final product ``(B,) * (B,1)`` broadcasts to a (B, B) tensor
whose mean the trainer takes (onssen/utils/train.py:78-79).
"""
import os

import torch

from . import options


# ----------------------------------------------------------------------------- shared host path of the HIP routes
def _lib():
    from .hip import get_lib
    return get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _lab(t):
    """A label map as the kernels read it: detached (labels carry no gradient), fp32, contiguous.  None passes through."""
    return None if t is None else t.detach().float().contiguous()


def _grad_in(g):
    """An incoming gradient as the gradient kernels read it (None: that output was not used)."""
    return None if g is None else g.float().contiguous()


def _ws(nbytes, device):
    """A workspace of this call alone."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _no_grad_needed(*ts):
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in ts))


def _route(is_cuda, needs_grad, eligible=True):
    """Which form a mask-family loss takes: "value" (a ROCm tensor and no gradient wanted: the value kernel), "grad" (a gradient
    wanted and option ``loss`` = "1": the autograd node over the two kernels), else "aten" (PyTorch ops; always on the CPU, and
    when the kernels cannot take the call: ``eligible`` false)."""
    if not (is_cuda and eligible):
        return "aten"
    if not needs_grad:
        return "value"
    return "grad" if options.get("loss") == "1" else "aten"


_enhance_route = _route                 # (is_cuda, needs_grad): the name the enhancement losses introduced it under


def _planes_base(masks):
    """The contiguous fp32 (*mask.shape, S) buffer whose S planes the masks are: the network's own when every mask is plane k of
    one contiguous fp32 buffer of exactly S * numel elements (offset ``base.storage_offset() + k``, strides S times the dense
    ones, equal shapes; the root may be the head's flat (B, T, F S) output: the same memory), else ``torch.stack`` of them."""
    S, m0 = len(masks), masks[0]
    base = getattr(m0, "_base", None)
    dense, acc = [], S
    for n_i in reversed(m0.shape):
        dense.insert(0, acc)
        acc *= n_i
    dense = tuple(dense)
    if (base is not None and base.dtype == torch.float32 and base.is_contiguous() and base.numel() == S * m0.numel()
            and all(getattr(m, "_base", None) is base and m.stride() == dense and m.shape == m0.shape
                    and m.storage_offset() == base.storage_offset() + k for k, m in enumerate(masks))):
        return base if base.shape == (*m0.shape, S) else base.view(*m0.shape, S)
    return torch.stack([m.float() for m in masks], -1)


def _rows(t):
    """(B, elements per batch row) of a map (B, ...), without the view ``t[0]`` would make."""
    return t.shape[0], t.numel() // t.shape[0]


def _two_planes(t):
    """(plane 0, plane 1, batch stride, element stride in floats) of an interleaved fp32 (B, ..., 2) buffer, as the chimera and
    phase entries take their two mask maps."""
    p = t.data_ptr()
    return p, p + 4, _rows(t)[1], 2


def _fro(x):
    return torch.sqrt((x * x).flatten(1).sum(dim=1))


def loss_dc(output, label):
    assert len(output) == 1, "Number of output must be 1 for Deep Clustering"
    assert len(label) == 2, "Number of label must be 2 for Deep Clustering"
    embedding, = output
    one_hot, mag_mix = label
    one_hot = one_hot.float()
    B, T, F, C = one_hot.shape
    D = embedding.shape[-1]
    needs_grad = torch.is_grad_enabled() and embedding.requires_grad
    if embedding.is_cuda and D + C <= 34 and (not needs_grad or (C <= 4 and options.get("loss") == "1")):
        emb, oh, mag = embedding.float().contiguous(), one_hot.contiguous(), mag_mix.float().contiguous()
        if not needs_grad:
            return _loss_dc_hip(emb, oh, mag, B, T * F, D, C)
        per_utt, total = _LossDcHip.apply(emb.view(B, T * F, D), oh, mag)
        return per_utt * total.unsqueeze(1)              # (B,) * (B,1) -> (B,B), as upstream
    V = embedding.reshape(B, T * F, D)
    Y = one_hot.reshape(B, T * F, C)
    mag = mag_mix.detach().reshape(B, T * F)
    total = mag.sum(1, keepdim=True)
    w = torch.sqrt(mag / total).unsqueeze(-1)            # W_i = |x_i| / sum_j |x_j|, applied to both factors
    scale = Y.sum(2, keepdim=True) * w                   # silent TF bins do not contribute
    per_utt = _AffinityNorms.apply(V, scale.detach(), (Y * w).detach())      # (B,)
    return per_utt * total                               # (B,) * (B,1) -> (B,B), as upstream


class _AffinityNorms(torch.autograd.Function):
    """||Vm^T Vm||_F - 2 ||Vm^T Ym||_F + ||Ym^T Ym||_F per utterance with Vm = scale * V (onssen/loss/loss_dc.py:36-42),
    as ONE Gram product of Z = [Vm | Ym] forward and ONE product backward instead of the three `bmm`s (and six in
    autograd's backward) of the literal form -- each contracts over all T*F bins.  Same value and gradient:
      d||Vm^T Vm|| = 2 Vm (Vm^T Vm) / ||.||,   d||Vm^T Ym|| = Ym (Vm^T Ym)^T / ||.||."""

    @staticmethod
    def forward(ctx, V, scale, Ym):
        D = V.shape[2]
        Z = torch.cat([V * scale, Ym], 2)
        G = torch.bmm(Z.transpose(1, 2), Z)              # (B, D+C, D+C): blocks Vm^T Vm, Vm^T Ym, Ym^T Ym
        nvv, nvy, nyy = _fro(G[:, :D, :D]), _fro(G[:, :D, D:]), _fro(G[:, D:, D:])
        ctx.save_for_backward(Z, scale, G, nvv, nvy)
        ctx.D = D
        return nvv - 2 * nvy + nyy

    @staticmethod
    def backward(ctx, g):
        Z, scale, G, nvv, nvy = ctx.saved_tensors
        D = ctx.D
        # dL/dVm = Z M with M = [2 Gvv / ||Gvv|| ; -2 Gvy^T / ||Gvy||]   (a zero norm has a zero block: no contribution)
        top = 2 * G[:, :D, :D] / nvv.clamp_min(1e-30)[:, None, None]
        bot = -2 * G[:, :D, D:].transpose(1, 2) / nvy.clamp_min(1e-30)[:, None, None]
        dVm = torch.bmm(Z, torch.cat([top, bot], 1))
        return dVm * scale * g[:, None, None], None, None


_WS = {}


def _loss_dc_launch(emb, one_hot, mag, B, TF, D, C, own_ws=False):
    from .hip import get_lib
    lib = get_lib()
    dev = emb.device
    nbytes = lib.loss_dc_workspace_bytes(B)
    if own_ws:      # kept alive by the autograd graph: the backward pass reads the partial Grams the forward left in it
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        ws = _WS.get((dev, B))
        if ws is None:
            ws = _WS[(dev, B)] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    per_utt = torch.empty(B, device=dev, dtype=torch.float32)
    total = torch.empty(B, device=dev, dtype=torch.float32)
    lib.loss_dc(emb.data_ptr(), one_hot.data_ptr(), mag.data_ptr(), B, TF, D, C, per_utt.data_ptr(), total.data_ptr(),
                ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    return per_utt, total, ws


def _loss_dc_hip(emb, one_hot, mag, B, TF, D, C):
    per_utt, total, _ = _loss_dc_launch(emb, one_hot, mag, B, TF, D, C)
    return per_utt * total.unsqueeze(1)                  # (B,) * (B,1) -> (B,B), as upstream


class _LossDcHip(torch.autograd.Function):
    """(per_utt, total_mag) of loss_dc with the embedding's gradient from onssen_loss_dc_grad_f32 (one_hot and mag_mix are
    labels: no gradient, like upstream's detached weights)."""

    @staticmethod
    def forward(ctx, emb, one_hot, mag):
        B, TF, D = emb.shape
        C = one_hot.shape[-1]
        per_utt, total, ws = _loss_dc_launch(emb, one_hot, mag, B, TF, D, C, own_ws=True)
        ctx.save_for_backward(emb, one_hot, mag, ws)
        ctx.mark_non_differentiable(total)
        return per_utt, total

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_total):
        from .hip import get_lib
        emb, one_hot, mag, ws = ctx.saved_tensors
        B, TF, D = emb.shape
        d_emb = torch.empty_like(emb)
        g = g.float().contiguous()
        get_lib().loss_dc_grad(emb.data_ptr(), one_hot.data_ptr(), mag.data_ptr(), B, TF, D, one_hot.shape[-1], g.data_ptr(),
                               d_emb.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        return d_emb, None, None


# ----------------------------------------------------------------------------- chimera / chimera++ losses
def _l1(x):
    return x.reshape(x.shape[0], -1).abs().sum(dim=1)


def _mask_term(mask_A, mask_B, mag_mix, t1, t2):
    l_ab = _l1(mask_A * mag_mix - t1) + _l1(mask_B * mag_mix - t2)
    l_ba = _l1(mask_B * mag_mix - t1) + _l1(mask_A * mag_mix - t2)
    return torch.min(l_ab, l_ba)


def _mask_term_launch(mask_a, mask_b, m_sb, m_se, mag, s1, s2, c1, c2, want_perm):
    """onssen_loss_mask_f32 over two mask maps given as pointers, element (b, e) of each at b * m_sb + e * m_se floats ->
    (out (B,), the winning assignment (B,) int32 or None)."""
    lib = _lib()
    (B, TF), dev = _rows(mag), mag.device
    out = torch.empty(B, device=dev, dtype=torch.float32)
    perm = torch.empty(B, device=dev, dtype=torch.int32) if want_perm else None
    ws = _ws(lib.loss_mask_workspace_bytes(B), dev)
    lib.loss_mask(mask_a, mask_b, m_sb, m_se, mag.data_ptr(), s1.data_ptr(), s2.data_ptr(), _ptr(c1), _ptr(c2), B, TF,
                  out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(), perm=_ptr(perm))
    return out, perm


class _MaskTermHip(torch.autograd.Function):
    """The mask-inference term with its gradient on the device: ``onssen_loss_mask_f32`` picks the better
    speaker assignment per utterance in the forward pass, ``onssen_loss_mask_grad_f32`` writes d/d(mask_A, mask_B) in one pass
    over the maps.  ``masks`` is the interleaved (B, ..., 2) buffer both mask views come from (targets carry no gradient,
    like upstream's labels)."""

    @staticmethod
    def forward(ctx, masks, mag, s1, s2, c1, c2):
        out, perm = _mask_term_launch(*_two_planes(masks), mag, s1, s2, c1, c2, True)
        ctx.save_for_backward(masks, mag, s1, s2, perm, *([c1, c2] if c1 is not None else []))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        masks, mag, s1, s2, perm, *cs = ctx.saved_tensors
        c1, c2 = cs if cs else (None, None)
        d = torch.empty_like(masks)
        g = _grad_in(g)
        _lib().loss_mask_grad(*_two_planes(masks), mag.data_ptr(), s1.data_ptr(), s2.data_ptr(), _ptr(c1), _ptr(c2), *_rows(mag),
                              g.data_ptr(), perm.data_ptr(), *_two_planes(d), _stream())
        return d, None, None, None, None, None


def _mask_term_hip(route, mask_A, mask_B, mag_mix, s1, s2, c1=None, c2=None):
    """The mask-inference term on the device.  "grad": the node over the plane buffer.  "value" is the one place that does not
    go through ``_planes_base``: the kernel reads any two maps of one batch and one element stride, so two views of one base
    with common strides (the planes of a buffer of any width, say) and two separate contiguous tensors are read where they lie,
    without the copy an interleaved buffer would cost an evaluation."""
    mag, s1, s2, c1, c2 = _lab(mag_mix), _lab(s1), _lab(s2), _lab(c1), _lab(c2)
    if route == "grad":
        return _MaskTermHip.apply(_planes_base((mask_A, mask_B)), mag, s1, s2, c1, c2)
    base = getattr(mask_A, "_base", None)
    if (base is None or getattr(mask_B, "_base", None) is not base or mask_A.stride() != mask_B.stride()
            or mask_A.stride(2) * mask_A.shape[2] != mask_A.stride(1)):
        mask_A, mask_B = mask_A.contiguous(), mask_B.contiguous()
    if mask_A.dtype != torch.float32 or mask_B.dtype != torch.float32:   # autocast / a user-supplied half estimate: the kernel reads fp32
        mask_A, mask_B = mask_A.float().contiguous(), mask_B.float().contiguous()
    # element (b, e = t*F + f) of a mask view sits at b*stride(0) + e*stride(2) when stride(1) = F*stride(2)
    return _mask_term_launch(mask_A.data_ptr(), mask_B.data_ptr(), mask_A.stride(0), mask_A.stride(2), mag, s1, s2, c1, c2, False)[0]


def _loss_chimera(embedding, mask_A, mask_B, one_hot, mag_mix, mag_s1, mag_s2, cos_s1=None, cos_s2=None):
    le = loss_dc([embedding], [one_hot, mag_mix])
    route = _route(mask_A.is_cuda, not _no_grad_needed(mask_A, mask_B))
    if route != "aten":
        lm = _mask_term_hip(route, mask_A, mask_B, mag_mix, mag_s1, mag_s2, cos_s1, cos_s2)
    elif cos_s1 is None:
        lm = _mask_term(mask_A, mask_B, mag_mix, mag_s1, mag_s2)
    else:
        lm = _mask_term(mask_A, mask_B, mag_mix, torch.min(mag_mix, torch.relu(mag_s1 * cos_s1)),
                        torch.min(mag_mix, torch.relu(mag_s2 * cos_s2)))
    return le * 0.975 + lm * 0.025


def loss_chimera_msa(output, label):
    """onssen/loss/loss_chimera.py:6-31: 0.975 * loss_dc + 0.025 * magnitude-spectrum-approximation mask loss with the
    better of the two speaker assignments ((B,B) like loss_dc, as upstream)."""
    (embedding, mask_A, mask_B), (one_hot, mag_mix, mag_s1, mag_s2) = output, label
    return _loss_chimera(embedding, mask_A, mask_B, one_hot, mag_mix, mag_s1, mag_s2)


def loss_chimera_psa(output, label):
    """onssen/loss/loss_chimera.py:33-59: as MSA with the phase-sensitive targets min(|x|, relu(|s| cos(theta)))."""
    (embedding, mask_A, mask_B), (one_hot, mag_mix, mag_s1, mag_s2, cos_s1, cos_s2) = output, label
    return _loss_chimera(embedding, mask_A, mask_B, one_hot, mag_mix, mag_s1, mag_s2, cos_s1, cos_s2)


# ----------------------------------------------------------------------------- enhancement losses
last_enhance_path = None


def _enhance_launch(mode, est, mag_noisy, mag_clean, cos_diff, scale):
    """onssen_loss_enhance_f32 -> MSA: the scalar ``scale * sum (est - clean)^2``; PSA (mag_noisy given): the sums (B,)."""
    lib = _lib()
    (B, TF), dev = _rows(est), est.device
    per_utt = torch.empty(B, device=dev, dtype=torch.float32)
    total = torch.empty((), device=dev, dtype=torch.float32) if mag_noisy is None else None
    ws = _ws(lib.loss_enhance_workspace_bytes(B), dev)
    lib.loss_enhance(mode, est.data_ptr(), _ptr(mag_noisy), mag_clean.data_ptr(), _ptr(cos_diff), B, TF, scale, per_utt.data_ptr(),
                     _ptr(total), ws.data_ptr(), ws.numel(), _stream())
    return per_utt if total is None else total


class _EnhanceLossHip(torch.autograd.Function):
    """An enhancement loss with the estimate's gradient on the device (csrc/enhance.inc): ``onssen_loss_enhance_f32`` forward,
    ``onssen_loss_enhance_grad_f32`` backward, one elementwise pass.  MSA returns the scalar ``scale * sum (est - clean)^2``, PSA
    the per-utterance sums (B,); the labels carry no gradient."""

    @staticmethod
    def forward(ctx, mode, scale, est, mag_noisy, mag_clean, cos_diff):
        ctx.geom = (mode, scale)
        ctx.save_for_backward(est, mag_clean, *([] if mag_noisy is None else [mag_noisy, cos_diff]))
        return _enhance_launch(mode, est, mag_noisy, mag_clean, cos_diff, scale)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        mode, scale = ctx.geom
        est, mag_clean, *rest = ctx.saved_tensors
        mag_noisy, cos_diff = rest if rest else (None, None)
        d = torch.empty_like(est)
        g = _grad_in(g)
        _lib().loss_enhance_grad(mode, est.data_ptr(), _ptr(mag_noisy), mag_clean.data_ptr(), _ptr(cos_diff), *_rows(est), scale,
                                 g.data_ptr(), d.data_ptr(), _stream())
        return None, None, d, None, None, None


def _loss_enhance(est, mag_noisy, mag_clean, cos_diff, aten):
    """One estimate against one target: MSA (mag_noisy and cos_diff None) or PSA; ``aten()`` is the form on PyTorch ops."""
    global last_enhance_path
    from . import _abi
    same = all(t is None or t.shape == est.shape for t in (mag_noisy, mag_clean, cos_diff))
    route = last_enhance_path = _route(est.is_cuda, not _no_grad_needed(est), same and est.dim() >= 2)
    if route == "aten":
        return aten()
    mode, scale = (_abi.ENHANCE_MSA, 1.0 / est.numel()) if mag_noisy is None else (_abi.ENHANCE_PSA, 1.0)
    mag_noisy, mag_clean, cos_diff = _lab(mag_noisy), _lab(mag_clean), _lab(cos_diff)
    x = est.float().contiguous()
    if route == "grad":
        return _EnhanceLossHip.apply(mode, scale, x, mag_noisy, mag_clean, cos_diff)
    return _enhance_launch(mode, x.detach(), mag_noisy, mag_clean, cos_diff, scale)


def loss_mask_msa(output, label):
    """onssen/loss/loss_mask.py:6-22, magnitude spectrum approximation for enhancement: ``MSELoss()(clean_est, mag_clean)``, a
    scalar -- the mean over all B T F bins.  ``output`` = [clean_est (B,T,F)] (the ``enhance`` network returns the clean
    magnitude itself, no mask is applied here), ``label`` = [mag_clean, cos_diff] as ``daps_enhance_dataloader`` yields them;
    cos_diff is not used, as upstream.  This is the loss of the recipe (egs/daps/run.py).

    On ROCm tensors the value comes from ``onssen_loss_enhance_f32`` when no gradient is wanted, value and gradient from the
    autograd node over the enhancement loss kernels with option ``loss`` = "1"; otherwise, and always on the CPU, PyTorch ops.
    ``last_enhance_path`` ("value" | "grad" | "aten") says which route the last call took."""
    assert len(output) == 1, "There must be 1 tensor in the output"
    assert len(label) == 2, "There must be 2 tensors in the label"
    clean_est, = output
    mag_clean, _cos_diff = label
    return _loss_enhance(clean_est, None, mag_clean, None, lambda: torch.nn.functional.mse_loss(clean_est, mag_clean))


def loss_mask_psa(output, label):
    """onssen/loss/loss_mask.py:25-40, phase-sensitive spectrum approximation: per utterance
    ``sum |mask * mag_noisy - min(mag_noisy, relu(mag_clean * cos_diff))|``, (B,).  ``output`` = [mask (B,T,F)], ``label`` =
    [mag_noisy, mag_clean, cos_diff].  Restated as upstream has it -- which is NOT what the DAPS loader yields (its label is
    [mag_clean, cos_diff], mag_noisy travels with the input) nor what ``enhance`` returns (a magnitude, not a mask): upstream's
    recipe trains with ``loss_mask_msa``, and so does this one; a caller with a mask-valued model builds the label list itself.
    Routes as ``loss_mask_msa``."""
    assert len(output) == 1, "There must be 1 tensor in the output"
    assert len(label) == 3, "There must be 3 tensors in the label"
    mask, = output
    mag_noisy, mag_clean, cos_diff = label
    return _loss_enhance(mask, mag_noisy, mag_clean, cos_diff,
                         lambda: _l1(mask * mag_noisy - torch.min(mag_noisy, torch.relu(mag_clean * cos_diff))))


# ----------------------------------------------------------------------------- uPIT losses (2 .. 4 speakers)
last_upit_path = None
UPIT_MAX_SPEAKERS = 4                 # upit::SMAX


def _upit_aten(masks, mag_mix, targets):
    """The plain restatement on PyTorch ops: the pair matrix by broadcasting, then the minimum over itertools.permutations (the
    first minimum wins).  Returns (out (B,), perm (B,) int64)."""
    from itertools import permutations
    S = len(masks)
    est = torch.stack([m * mag_mix for m in masks], 1)                       # (B, S, ...)
    tgt = torch.stack(list(targets), 1)
    pair = (est.unsqueeze(2) - tgt.unsqueeze(1)).abs().flatten(3).sum(-1)    # (B, S, S): pair[b][k][j]
    totals = torch.stack([sum(pair[:, k, p[k]] for k in range(S)) for p in permutations(range(S))], 1)
    out = totals.min(dim=1).values
    # torch.min's index among equal values is unspecified: take the first occurrence, as the kernels do
    perm = (totals == out.unsqueeze(1)).int().argmax(dim=1)
    return out, perm


def _upit_maps(maps):
    """S label maps of one shape -> (first pointer's tensor list kept alive, pointer, distance in floats): the maps as they lie
    when they sit at one common distance (slices of one tensor, say), else stacked first."""
    maps = [_lab(t) for t in maps]
    ptrs = [t.data_ptr() for t in maps]
    d = ptrs[1] - ptrs[0]
    if d % 4 == 0 and all(ptrs[j] - ptrs[0] == j * d for j in range(len(maps))):
        return maps, ptrs[0], d // 4
    st = torch.stack(maps, 0)
    return [st], st.data_ptr(), maps[0].numel()


def _upit_frames(frames, B, T, device):
    if frames is None:
        return None
    from .nn._core import as_frames
    return as_frames(frames, B, T, device)


def _upit_launch(base, S, mag, src, cs, frames, F):
    lib = _lib()
    (B, TF), dev = _rows(mag), mag.device
    out = torch.empty(B, device=dev, dtype=torch.float32)
    perm = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _ws(lib.loss_upit_workspace_bytes(B, S), dev)
    lib.loss_upit(base.data_ptr(), TF * S, S, 1, mag.data_ptr(), src[1], src[2], cs[1] if cs else None, cs[2] if cs else 0,
                  _ptr(frames), F, B, TF, S, out.data_ptr(), perm.data_ptr(), None, ws.data_ptr(), ws.numel(), _stream())
    return out, perm


class _UpitLossHip(torch.autograd.Function):
    """The uPIT mask loss with the masks' gradient on the device (csrc/loss_upit.inc): ``onssen_loss_upit_f32`` picks the
    assignment per utterance in the forward pass, ``onssen_loss_upit_grad_f32`` writes d/d masks in one elementwise pass.
    ``base`` is the interleaved (B, ..., S) buffer (see _MaskTermHip); the labels carry no gradient.  Returns (out, perm)."""

    @staticmethod
    def forward(ctx, base, S, mag, src, cs, frames, F):
        out, perm = _upit_launch(base, S, mag, src, cs, frames, F)
        ctx.save_for_backward(base, mag, perm, *src[0], *(cs[0] if cs else []), *([frames] if frames is not None else []))
        ctx.geom = (S, src[1:], cs[1:] if cs else None, frames is not None, F)
        ctx.mark_non_differentiable(perm)
        return out, perm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_perm):
        S, src, cs, ragged, F = ctx.geom
        base, mag, perm, *rest = ctx.saved_tensors
        frames = rest[-1] if ragged else None
        B, TF = _rows(mag)
        d = torch.empty_like(base)
        g = _grad_in(g)
        _lib().loss_upit_grad(base.data_ptr(), TF * S, S, 1, mag.data_ptr(), src[0], src[1], cs[0] if cs else None,
                              cs[1] if cs else 0, _ptr(frames), F, B, TF, S, g.data_ptr(), perm.data_ptr(), d.data_ptr(),
                              TF * S, S, 1, _stream())
        return d, None, None, None, None, None, None


def _loss_upit(name, output, label, psa, frames, return_perm):
    global last_upit_path
    masks = list(output)
    S = len(masks)
    want = 1 + (2 if psa else 1) * S
    if S < 2 or len(label) != want:
        raise ValueError(f"{name}: {len(label)} label tensors for {S} masks; {S} masks take {want} "
                         f"([mag_mix, mag_s1 .. mag_s{S}" + (f", cos_s1 .. cos_s{S}])" if psa else "])"))
    mag_mix, mags, coss = label[0], list(label[1:1 + S]), (list(label[1 + S:]) if psa else None)
    m0 = masks[0]
    same = all(t.shape == m0.shape for t in masks + [mag_mix] + mags + (coss or []))
    route = last_upit_path = _route(m0.is_cuda, not _no_grad_needed(*masks), S <= UPIT_MAX_SPEAKERS and same and m0.dim() >= 2)
    if route == "aten":
        if frames is not None:
            raise RuntimeError(f"{name}: frames=... (ragged batch) needs the HIP kernels (ROCm tensors, at most "
                               f"{UPIT_MAX_SPEAKERS} speakers, option loss = \"1\" when a gradient is wanted)")
        mag = mag_mix.detach()
        tg = [t.detach() for t in mags] if not psa else [torch.min(mag, torch.relu(s.detach() * c.detach()))
                                                         for s, c in zip(mags, coss)]
        out, perm = _upit_aten(masks, mag, tg)
        return (out, perm) if return_perm else out
    B = m0.shape[0]
    F = m0.shape[-1]
    frames = _upit_frames(frames, B, _rows(m0)[1] // F, m0.device)
    mag = _lab(mag_mix)
    src, cs = _upit_maps(mags), (_upit_maps(coss) if psa else None)
    base = _planes_base(masks)
    if route == "grad":
        out, perm = _UpitLossHip.apply(base, S, mag, src, cs, frames, F)
    else:
        out, perm = _upit_launch(base.detach(), S, mag, src, cs, frames, F)
    return (out, perm.long()) if return_perm else out


def loss_upit_msa(output, label, frames=None, return_perm=False):
    """Utterance-level permutation-invariant mask loss, magnitude spectrum approximation, for S = len(output) speakers (upstream
    has the uPIT network, onssen/nn/uPIT-LSTM.py, and no loss for it): ``output`` = the S masks (B,T,F), ``label`` = [mag_mix,
    mag_s1 .. mag_sS].  Per utterance ``min_p sum_k sum_bins |m_k mag_mix - mag_s_p[k]|`` over the S! assignments p, (B,) -- the
    trainer takes the mean; for S = 2 the mask term of ``loss_chimera_msa``.  ``return_perm``: also the index (B,) int64 of each
    row's assignment in the order of ``itertools.permutations(range(S))`` (the first minimum wins).  ``frames`` (B,): a ragged
    batch, row b is its first frames[b] frames (HIP kernels only).

    On ROCm tensors the value comes from ``onssen_loss_upit_f32`` when no gradient is wanted, value and gradient from the autograd
    node over the two kernels (csrc/loss_upit.inc) with option ``loss`` = "1"; otherwise -- CPU tensors, ``loss`` = "torch", more
    than four speakers -- PyTorch ops.  ``last_upit_path`` ("value" | "grad" | "aten") says which route the last call took."""
    return _loss_upit("loss_upit_msa", output, label, False, frames, return_perm)


def loss_upit_psa(output, label, frames=None, return_perm=False):
    """As ``loss_upit_msa`` with the phase-sensitive targets ``min(mag_mix, relu(mag_s_j cos_s_j))``: ``label`` = [mag_mix,
    mag_s1 .. mag_sS, cos_s1 .. cos_sS]; for S = 2 the mask term of ``loss_chimera_psa``."""
    return _loss_upit("loss_upit_psa", output, label, True, frames, return_perm)


# ----------------------------------------------------------------------------- phase network loss
last_phase_path = None


def _phase_terms(mask_A, mask_B, phase_A, phase_B, mag_mix, mag_s1, mag_s2, phase_s1, phase_s2):
    """(mask term, phase term), (B,) each, on PyTorch ops: the straight assignment where l1 < l2 strictly, else the swapped one."""
    import torch.nn.functional as F
    l1 = _l1(mask_A * mag_mix - mag_s1) + _l1(mask_B * mag_mix - mag_s2)
    l2 = _l1(mask_B * mag_mix - mag_s1) + _l1(mask_A * mag_mix - mag_s2)
    cos = lambda p, q: (mag_mix * F.cosine_similarity(p, q, dim=-1)).flatten(1).sum(dim=1)
    p1 = -cos(phase_A, phase_s1) - cos(phase_B, phase_s2)
    p2 = -cos(phase_B, phase_s1) - cos(phase_A, phase_s2)
    straight = l1 < l2
    return torch.where(straight, l1, l2), torch.where(straight, p1, p2)


def _phase_terms_launch(masks, pa, pb, mag, s1, s2, q1, q2):
    lib = _lib()
    (B, TF), dev = _rows(mag), mag.device
    out_mask = torch.empty(B, device=dev, dtype=torch.float32)
    out_phase = torch.empty(B, device=dev, dtype=torch.float32)
    perm = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _ws(lib.loss_phase_workspace_bytes(B), dev)
    lib.loss_phase(*_two_planes(masks), mag.data_ptr(), s1.data_ptr(), s2.data_ptr(), pa.data_ptr(), pb.data_ptr(), q1.data_ptr(),
                   q2.data_ptr(), B, TF, out_mask.data_ptr(), out_phase.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel(),
                   _stream())
    return out_mask, out_phase, perm


class _PhaseTermsHip(torch.autograd.Function):
    """(mask term, phase term) of loss_phase with their gradients on the device: ``onssen_loss_phase_f32`` reads the eleven maps
    once and picks the assignment, ``onssen_loss_phase_grad_f32`` writes d/d(masks, phase_A, phase_B) in one pass.  ``masks`` is
    the interleaved (B, ..., 2) buffer (see _MaskTermHip); the labels carry no gradient."""

    @staticmethod
    def forward(ctx, masks, pa, pb, mag, s1, s2, q1, q2):
        out_mask, out_phase, perm = _phase_terms_launch(masks, pa, pb, mag, s1, s2, q1, q2)
        ctx.save_for_backward(masks, pa, pb, mag, s1, s2, q1, q2, perm)
        return out_mask, out_phase

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mask, g_phase):
        masks, pa, pb, mag, s1, s2, q1, q2, perm = ctx.saved_tensors
        d, dpa, dpb = torch.empty_like(masks), torch.empty_like(pa), torch.empty_like(pb)
        g_mask, g_phase = _grad_in(g_mask), _grad_in(g_phase)
        _lib().loss_phase_grad(*_two_planes(masks), mag.data_ptr(), s1.data_ptr(), s2.data_ptr(), pa.data_ptr(), pb.data_ptr(),
                               q1.data_ptr(), q2.data_ptr(), *_rows(mag), g_mask.data_ptr(), g_phase.data_ptr(),
                               perm.data_ptr(), *_two_planes(d), dpa.data_ptr(), dpb.data_ptr(), _stream())
        return d, dpa, dpb, None, None, None, None, None


def _phase_terms_hip(mask_A, mask_B, phase_A, phase_B, mag_mix, mag_s1, mag_s2, phase_s1, phase_s2, needs_grad):
    labels = [_lab(t) for t in (mag_mix, mag_s1, mag_s2, phase_s1, phase_s2)]
    masks = _planes_base((mask_A, mask_B))
    pa, pb = phase_A.float().contiguous(), phase_B.float().contiguous()
    if needs_grad:
        return _PhaseTermsHip.apply(masks, pa, pb, *labels)
    return _phase_terms_launch(masks.detach(), pa.detach(), pb.detach(), *labels)[:2]


def loss_phase(output, label):
    """onssen/loss/loss_phase.py:6-37 with its two defects repaired (it asserts six outputs and unpacks five, and hands loss_dc
    its arguments in the wrong groups): 0.975 * loss_dc + 0.025 * mask term + 0.025 * phase term, (B,B) like the chimera losses.
    The mask term is the L1 mask-inference term of the assignment with l1 < l2 strictly (a tie takes the swapped one, as
    upstream's index does); the phase term is -sum |x| (cos(phase_A, t_A) + cos(phase_B, t_B)) under the same assignment, cos =
    F.cosine_similarity over the (re, im) axis (each norm clamped at 1e-8; ``phase_s*`` are raw STFT values, 0 in silent bins).

    On ROCm tensors with option ``loss`` = "1" both terms come from the loss_phase kernels (csrc/loss_phase.inc), with their
    gradient when autograd needs it; on CPU tensors or with ``loss`` = "torch" from PyTorch ops.  ``last_phase_path`` ("hip" |
    "aten") says which route the last call took.  The labels get no gradient."""
    global last_phase_path
    assert len(output) == 5, "There must be 5 tensors in the output"
    assert len(label) == 6, "There must be 6 tensors in the label"
    embedding, mask_A, mask_B, phase_A, phase_B = output
    one_hot, mag_mix, mag_s1, mag_s2, phase_s1, phase_s2 = label
    le = loss_dc([embedding], [one_hot, mag_mix])
    if mask_A.is_cuda and options.get("loss") == "1":
        last_phase_path = "hip"
        lm, lp = _phase_terms_hip(mask_A, mask_B, phase_A, phase_B, mag_mix, mag_s1, mag_s2, phase_s1, phase_s2,
                                  not _no_grad_needed(mask_A, mask_B, phase_A, phase_B))
    else:
        last_phase_path = "aten"
        lm, lp = _phase_terms(mask_A, mask_B, phase_A, phase_B, mag_mix.detach(), mag_s1.detach(), mag_s2.detach(),
                              phase_s1.detach(), phase_s2.detach())
    return le * 0.975 + lm * 0.025 + lp * 0.025


# ---- time-domain losses of Conv-TasNet (onssen/loss/loss_e2e.py:7-87) ------------------------------------------------------
# Reductions used in training: PyTorch ops, same placement of eps, zero mean and permutation search as the reference.

def SI_SNR(_s, s, zero_mean=True):
    """SI-SNR in dB of one estimate ``_s`` against one reference ``s`` (1-D tensors), no eps (loss_e2e.py:7-23)."""
    est, ref = (_s - _s.mean(), s - s.mean()) if zero_mean else (_s, s)
    target = (est * ref).sum() * ref / ref.norm() ** 2          # projection of the estimate on the reference
    return 20 * torch.log10(target.norm() / (est - target).norm())


def permute_SI_SNR(_s_lists, s_lists):
    """The largest speaker-averaged SI_SNR over all assignments of estimates to references (loss_e2e.py:26-43)."""
    from itertools import permutations
    k = len(_s_lists)
    return max(sum(SI_SNR(_s_lists[i], s_lists[p[i]]) for i in range(k)) / k for p in permutations(range(k)))


def sisnr(x, s, eps=1e-8):
    """Per-row SI-SNR in dB of x against s, both (N, S), eps as in loss_e2e.py:46-69: added to the squared reference norm, to
    the noise norm and to the ratio inside the logarithm."""
    if x.shape != s.shape:
        raise RuntimeError(f"sisnr: shapes differ, {tuple(x.shape)} vs {tuple(s.shape)}")
    est = x - x.mean(dim=-1, keepdim=True)
    ref = s - s.mean(dim=-1, keepdim=True)
    scale = (est * ref).sum(dim=-1, keepdim=True) / (ref.norm(dim=-1, keepdim=True) ** 2 + eps)
    target = scale * ref
    return 20 * torch.log10(eps + target.norm(dim=-1) / ((est - target).norm(dim=-1) + eps))


def si_snr_loss(ests, refs):
    """Negative SI-SNR training loss (loss_e2e.py:72-87): per utterance the speaker-averaged sisnr of the best assignment of
    estimates to references, summed over the batch and divided by its size.

    Option ``tasnet_loss`` (default "aten": the PyTorch ops below): under "hip" the value and the estimates' gradient come from
    the SI-SNR PIT kernels (``sisnr_pit``; csrc/loss_sisnr.inc) as one autograd node, except for what ``sisnr_pit_limits`` lists,
    which stays on the PyTorch ops by itself.  ``last_si_snr_path`` ("hip" | "aten") says which route the last call took."""
    global last_si_snr_path
    if options.get("tasnet_loss") == "hip" and not sisnr_pit_limits(ests, refs):
        last_si_snr_path = "hip"
        return _sisnr_pit_apply(list(ests), list(refs), None)[1]
    last_si_snr_path = "aten"
    from itertools import permutations
    k = len(refs)
    per_perm = torch.stack([sum(sisnr(ests[i], refs[p[i]]) for i in range(k)) / k for p in permutations(range(k))])
    return -per_perm.max(dim=0).values.sum() / refs[0].shape[0]


# ---- the same loss on the SI-SNR PIT kernels (csrc/loss_sisnr.inc) ---------------------------------------------------------
last_si_snr_path = None
SISNR_PIT_MAX_SPEAKERS = 4            # sisnr::CMAX
SISNR_PIT_MAX_ROWS = 65535


def sisnr_pit_limits(ests, refs):
    """Reasons the SI-SNR PIT kernels cannot take these estimates and references (empty: they can).  Under
    ``tasnet_loss = "hip"`` such a call stays on the PyTorch ops by itself; ``sisnr_pit`` raises with this list."""
    ests, refs = list(ests), list(refs)
    ts = ests + refs
    why = []
    if any(not t.is_cuda for t in ts):
        why.append("CPU tensors: the kernels read ROCm device memory")
    bad = sorted({str(t.dtype) for t in ts if t.dtype != torch.float32})
    if bad:
        why.append(f"dtype {', '.join(bad)}: the kernels take fp32")
    if torch.is_grad_enabled() and any(r.requires_grad for r in refs):
        why.append("a reference requires a gradient: the backward gives the estimates' gradient only")
    if len(refs) > SISNR_PIT_MAX_SPEAKERS:
        why.append(f"k = {len(refs)} > {SISNR_PIT_MAX_SPEAKERS} speakers")
    if torch.is_anomaly_enabled():
        why.append("autograd anomaly mode")
    if any(t.dim() != 2 for t in ts):
        why.append("signals that are not (N, S) matrices")
    elif ts and ts[0].shape[0] > SISNR_PIT_MAX_ROWS:
        why.append(f"N = {ts[0].shape[0]} > {SISNR_PIT_MAX_ROWS} rows")
    return why


def _pit_lengths(lengths, N, S, device):
    """``lengths`` of a ragged batch as an int32 device tensor: host integers (a sequence or a CPU tensor) are validated and
    copied; a device tensor is taken as it is (its values cannot be checked without reading them back: the kernels clamp them to
    [1, S])."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.is_cuda:
        if lengths.dtype != torch.int32 or lengths.dim() != 1:
            raise TypeError(f"sisnr_pit: a device lengths tensor must be 1-D int32, got {lengths.dtype} with {lengths.dim()} dimensions")
        if lengths.numel() != N:
            raise ValueError(f"sisnr_pit: {lengths.numel()} lengths for a batch of {N} rows")
        return lengths.contiguous()
    if torch.is_tensor(lengths):
        if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
            raise TypeError(f"sisnr_pit: lengths must be integers, got {lengths.dtype}")
        lengths = lengths.reshape(-1).tolist()
    lengths = list(lengths)
    if any(isinstance(v, bool) or int(v) != v for v in lengths):
        raise TypeError(f"sisnr_pit: lengths must be integers, got {lengths!r}")
    if len(lengths) != N:
        raise ValueError(f"sisnr_pit: {len(lengths)} lengths for a batch of {N} rows")
    for b, v in enumerate(lengths):
        if not 1 <= v <= S:
            raise ValueError(f"sisnr_pit: lengths[{b}] = {v} lies outside [1, {S}], the samples of a row")
    return torch.tensor([int(v) for v in lengths], dtype=torch.int32, device=device)


def _pit_rows(t):
    """(tensor, row stride in floats) as the kernels read it: unit inner stride, rows at least S apart (any stride for one row)."""
    N, S = t.shape
    if t.stride(1) != 1 or (N > 1 and t.stride(0) < S):
        t = t.contiguous()
    return t, (t.stride(0) if N > 1 else S)


def _pit_stacked_base(ests):
    """The (k, N, S) tensor whose k slices the estimates are (what ConvTasNet's training forward returns), or None.  The node is
    then applied to that tensor itself: the gradient (k, N, S) goes to it as it is written, not through k select views whose
    gradients autograd would scatter into zeros and add (as _planes_base does for the mask networks)."""
    base = getattr(ests[0], "_base", None)
    k, (N, S) = len(ests), ests[0].shape
    if base is None or not base.requires_grad or base.dtype != torch.float32 or not base.is_contiguous():
        return None
    if base.numel() != k * N * S or base.dim() != 3 or tuple(base.shape) != (k, N, S):
        return None
    for i, e in enumerate(ests):
        if getattr(e, "_base", None) is not base or e.storage_offset() != base.storage_offset() + i * N * S:
            return None
        if e.stride(1) != 1 or (N > 1 and e.stride(0) != S):
            return None
    return base


class _SisnrPitHip(torch.autograd.Function):
    """(V (N,), loss, perm (N,) int32) of the SI-SNR PIT loss on onssen_sisnr_pit_f32, with the estimates' gradient from
    onssen_sisnr_pit_backward_f32.  Two outputs carry a gradient, as _LossDcHip's: the per-row values and the scalar loss
    -sum(V) / N, so ``si_snr_loss`` adds no reduction of its own.  ``stacked``: the first tensor is the (k, N, S) tensor
    whose slices are the estimates; otherwise the k estimates come one by one.  The references follow; they get no gradient."""

    @staticmethod
    def forward(ctx, k, lengths, stacked, *ts):
        lib = _lib()
        if stacked:
            base, refs = ts[0], ts[1:]
            ests = [base[i] for i in range(k)]
        else:
            ests, refs = ts[:k], ts[k:]
        ests = [_pit_rows(e.detach()) for e in ests]
        refs = [_pit_rows(r.detach()) for r in refs]
        N, S = ests[0][0].shape
        dev = ests[0][0].device
        est = lib.sisnr_signals([e.data_ptr() for e, _ in ests], [st for _, st in ests])
        ref = lib.sisnr_signals([r.data_ptr() for r, _ in refs], [st for _, st in refs])
        nbytes = lib.sisnr_pit_workspace_bytes(N, k)
        ws = _ws(nbytes, dev)                    # owned by the graph: the backward reads the coefficients in it
        value = torch.empty(N, device=dev, dtype=torch.float32)
        total = torch.empty((), device=dev, dtype=torch.float32)
        perm = torch.empty(N, device=dev, dtype=torch.int32)
        lib.sisnr_pit(est, ref, k, N, S, _ptr(lengths), value.data_ptr(), perm.data_ptr(), total.data_ptr(), ws.data_ptr(), nbytes,
                      _stream())
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(perm)
        ctx.sig = ([e for e, _ in ests], [r for r, _ in refs], est, ref, ws, lengths)
        ctx.geom = (k, N, S, stacked, len(ts))
        return value, total, perm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value, g_total, _g_perm):
        k, N, S, stacked, n_in = ctx.geom
        if g_value is None and g_total is None:
            return (None,) * (3 + n_in)
        ests, refs, est, ref, ws, lengths = ctx.sig
        g_value, g_total = _grad_in(g_value), _grad_in(g_total)
        d = torch.empty(k, N, S, device=ws.device, dtype=torch.float32)
        _lib().sisnr_pit_backward(est, ref, k, N, S, _ptr(lengths), _ptr(g_value), _ptr(g_total), d.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream())
        grads = [d] if stacked else [d[i] for i in range(k)]
        return (None, None, None, *grads, *([None] * (n_in - len(grads))))


def _sisnr_pit_apply(ests, refs, lengths):
    """Checks that do not depend on the route (counts, shapes: ``sisnr``'s RuntimeError text), then the node."""
    if not ests or len(ests) != len(refs):
        raise ValueError(f"sisnr_pit: {len(ests)} estimates for {len(refs)} references")
    for t in ests + refs:
        if t.shape != ests[0].shape:
            raise RuntimeError(f"sisnr: shapes differ, {tuple(ests[0].shape)} vs {tuple(t.shape)}")
    why = sisnr_pit_limits(ests, refs)
    if why:
        raise RuntimeError("sisnr_pit: the HIP kernels cannot take these inputs: " + "; ".join(why))
    N, S = ests[0].shape
    if S < 1 or N < 1:
        raise RuntimeError(f"sisnr_pit: empty signals, {tuple(ests[0].shape)}")
    lengths = _pit_lengths(lengths, N, S, ests[0].device)
    k = len(ests)
    base = _pit_stacked_base(ests) if torch.is_grad_enabled() else None
    if base is not None:
        return _SisnrPitHip.apply(k, lengths, True, base, *refs)
    return _SisnrPitHip.apply(k, lengths, False, *ests, *refs)


def sisnr_pit(ests, refs, lengths=None, return_perm=False):
    """The speaker-averaged SI-SNR in dB of the best assignment of ``ests`` to ``refs`` (k tensors (N, S) each, k <= 4, fp32 on a
    ROCm device), per row: V (N,) fp32, differentiable with respect to the estimates -- ``-V.sum() / N`` is ``si_snr_loss``.
    ``return_perm``: also the index (N,) int64 of each row's assignment in the order of ``itertools.permutations(range(k))`` (the
    first maximum wins).  ``lengths`` (N,), host integers or an int32 device tensor: row b is its first lengths[b] samples;
    its value and gradient are bit for bit those of the one-row call on ``x[b, :lengths[b]]`` and the gradient beyond is zero.
    Runs on the SI-SNR PIT kernels (csrc/loss_sisnr.inc): one pass over the signals forward, one elementwise pass backward,
    nothing read back by the host, bit-repeatable, capturable in a graph.  Raises, with the reasons, on anything the kernels
    cannot take (``sisnr_pit_limits``); shapes that differ raise ``sisnr``'s RuntimeError."""
    value, _, perm = _sisnr_pit_apply(list(ests), list(refs), lengths)
    return (value, perm.long()) if return_perm else value


# ----------------------------------------------------------------------------- waveform approximation
WA_PIT_MAX_SPEAKERS = 4
WA_KINDS = ("chimera", "upit", "phase", "enhance")


def _wa_ref_rows(ref, n):
    """The references as the kernels read them: fp32, unit sample stride, rows (batch and speaker) at least n samples apart."""
    ref = ref.detach().float()
    B, C, _ = ref.shape
    if ref.stride(2) != 1 or (C > 1 and abs(ref.stride(1)) < n) or (B > 1 and abs(ref.stride(0)) < n):
        ref = ref.contiguous()
    return ref


def _wa_pit_launch(est, ref, lengths):
    lib = _lib()
    B, C, n = est.shape
    dev = est.device
    nbytes = lib.wa_pit_workspace_bytes(B, C)
    ws = _ws(nbytes, dev)
    value = torch.empty(B, device=dev, dtype=torch.float32)
    perm = torch.empty(B, device=dev, dtype=torch.int32)
    lib.wa_pit(est.data_ptr(), ref.data_ptr(), ref.stride(0) if B > 1 else C * n, ref.stride(1) if C > 1 else n, B, C, n,
               _ptr(lengths), value.data_ptr(), perm.data_ptr(), None, ws.data_ptr(), nbytes, _stream())
    return value, perm, ws


class _WaPitHip(torch.autograd.Function):
    """(V (B,), perm (B,) int32) of the waveform L1 loss with the best permutation on ``onssen_wa_pit_f32``; the estimates'
    gradient comes from ``onssen_wa_pit_backward_f32``, which reads the assignment the forward left in its workspace
    (csrc/loss_wa.inc).  ``est`` (B, C, n) contiguous fp32; the references get no gradient."""

    @staticmethod
    def forward(ctx, est, ref, lengths):
        est = est.detach()
        value, perm, ws = _wa_pit_launch(est, ref, lengths)
        ctx.mark_non_differentiable(perm)
        ctx.sig = (est, ref, lengths, ws)            # the workspace is owned by the graph: the backward reads the assignment in it
        return value, perm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value, _g_perm):
        est, ref, lengths, ws = ctx.sig
        B, C, n = est.shape
        g_value = _grad_in(g_value)
        d = torch.empty_like(est)
        _lib().wa_pit_backward(est.data_ptr(), ref.data_ptr(), ref.stride(0) if B > 1 else C * n, ref.stride(1) if C > 1 else n,
                               B, C, n, _ptr(lengths), g_value.data_ptr(), None, d.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        return d, None, None


def wa_pit(est, ref, lengths=None, return_perm=False):
    """The waveform-approximation objective of Wang, Le Roux, Wang & Hershey 2018 per row: est, ref (B, C, n) fp32 on a ROCm device,
    C <= 4 ->  V (B,) = min over the C! assignments p of sum_i sum_t |est_i[t] - ref_p(i)[t]| / (C n_b), differentiable with
    respect to ``est`` (d est = sign(est - ref_p) / (C n_b), 0 at equality).  ``return_perm``: also the index (B,) int64 of each
    row's assignment in the order of ``itertools.permutations(range(C))`` (the first minimum wins).  ``lengths`` (B,), host
    integers or an int32 device tensor: row b is its first n_b = lengths[b] samples; the gradient beyond them is zero.
    ``ref`` is read where it is with any batch and speaker strides (unit sample stride); it gets no gradient.
    Runs on the kernels of csrc/loss_wa.inc: one pass over the signals forward (fp64 sums, fixed order), one elementwise pass
    backward, nothing read back by the host, bit-repeatable, capturable in a graph.  There is no PyTorch-op route."""
    if est.dim() != 3 or ref.dim() != 3 or est.shape != ref.shape:
        raise ValueError(f"wa_pit: expected est and ref of one shape (B, C, n), got {tuple(est.shape)} and {tuple(ref.shape)}")
    B, C, n = est.shape
    if not 1 <= C <= WA_PIT_MAX_SPEAKERS:
        raise ValueError(f"wa_pit: {C} speakers; the kernels take 1 .. {WA_PIT_MAX_SPEAKERS}")
    if B < 1 or n < 1:
        raise ValueError(f"wa_pit: empty signals, {tuple(est.shape)}")
    if torch.is_grad_enabled() and ref.requires_grad:
        raise RuntimeError("wa_pit: a reference requires a gradient; the backward gives the estimates' gradient only")
    if not est.is_cuda or not ref.is_cuda:
        raise RuntimeError("wa_pit: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    lengths = _pit_lengths(lengths, B, n, est.device)
    ref = _wa_ref_rows(ref, n)
    est = est.float().contiguous()
    if torch.is_grad_enabled() and est.requires_grad:
        value, perm = _WaPitHip.apply(est, ref, lengths)
    else:
        value, perm, _ = _wa_pit_launch(est.detach(), ref, lengths)
    return (value, perm.long()) if return_perm else value


def loss_wa(output, label, hop_size=64, frames=None, lengths=None, kind="chimera", misi_iters=0):
    """Waveform-approximation training loss (Wang, Le Roux, Wang & Hershey 2018; upstream has none): the network's output goes
    through ONE inverse transform and is compared with the source waveforms, ``wa_pit(...).mean()``.

    ``label`` = [stft_ri_mix (B,T,F,2), sig_ref (B,C,n)] (the "chimera-wa" / "upit-wa" loaders); n is the length of the
    reconstruction (``hop_size * (T - 1)`` from those loaders).  ``kind`` says what ``output`` is -- the arity alone cannot (a
    chimera output and three uPIT masks are both three tensors):
      "chimera"  [embedding, mask_A, mask_B] of chimera / chimera++: the two masks through ``mask_istft``, the embedding ignored
      "upit"     the S masks of the uPIT network, through ``mask_istft``
      "phase"    [embedding, mask_A, mask_B, phase_A, phase_B] of the phase network, through ``phase_istft``
      "enhance"  [magnitude] of the enhancement network, through ``mag_istft``: one channel, the identity assignment
    ``frames`` / ``lengths`` (B,): a ragged batch as in ``mask_istft`` (both or neither); ``lengths`` also bounds the loss's sums.
    ``misi_iters``: this loss is the single inverse transform; anything but 0 raises NotImplementedError -- unfolded MISI
    iterations as training layers (the adjoint of misi_phase) are ``loss_wa_misi``.  The mixture's spectrum is data: a
    ``stft_ri`` that requires a gradient raises."""
    from . import features
    if misi_iters != 0:
        raise NotImplementedError(f"loss_wa: misi_iters = {misi_iters!r}; this loss goes through ONE inverse transform and has no use for "
                                  f"the adjoint of misi_phase -- training through unfolded MISI iterations is loss_wa_misi(output, label, "
                                  f"iters, ...)")
    stft_ri, sig_ref, masks, phases = _wa_args("loss_wa", output, label, frames, lengths, kind)
    n = sig_ref.shape[2]
    rag = dict(frames=frames, lengths=lengths)
    if kind == "enhance":
        est = features.mag_istft(stft_ri, masks[0], hop_size, n, **rag)
    else:
        base = _planes_base(masks)               # the network's own interleaved buffer when the masks are its planes
        if kind == "phase":
            est = features.phase_istft(stft_ri, base, phases, hop_size, n, **rag)
        else:
            est = features.mask_istft(stft_ri, base, hop_size, n, **rag)
    return wa_pit(est, sig_ref, lengths).mean()


def _wa_args(who, output, label, frames, lengths, kind):
    """The argument checks of the waveform-approximation losses -> (stft_ri, sig_ref, masks, phase maps or None)."""
    if kind not in WA_KINDS:
        raise ValueError(f"{who}: unknown kind {kind!r}; one of {WA_KINDS}")
    output = list(output)
    want = {"chimera": (3,), "phase": (5,), "enhance": (1,), "upit": (2, 3, 4)}[kind]
    if len(output) not in want:
        raise ValueError(f"{who}: {len(output)} output tensors for kind {kind!r}, which has {' or '.join(map(str, want))}")
    if len(label) != 2:
        raise ValueError(f"{who}: {len(label)} label tensors; the label is [stft_ri_mix (B,T,F,2), sig_ref (B,C,n)]")
    stft_ri, sig_ref = label
    if stft_ri.dim() != 4 or stft_ri.shape[-1] != 2 or sig_ref.dim() != 3:
        raise ValueError(f"{who}: expected stft_ri_mix (B,T,F,2) and sig_ref (B,C,n), got {tuple(stft_ri.shape)} and {tuple(sig_ref.shape)}")
    if stft_ri.requires_grad:
        raise RuntimeError(f"{who}: stft_ri_mix requires a gradient; the mixture's spectrum is data")
    masks = output[1:3] if kind in ("chimera", "phase") else output
    B, T, F = stft_ri.shape[:3]
    for m in masks:
        if tuple(m.shape) != (B, T, F):
            raise ValueError(f"{who}: an output of shape {tuple(m.shape)} for a spectrum of {(B, T, F)} bins")
    if tuple(sig_ref.shape[:2]) != (B, len(masks)):
        raise ValueError(f"{who}: sig_ref {tuple(sig_ref.shape)} for a batch of {B} with {len(masks)} estimates")
    if (frames is None) != (lengths is None):
        raise ValueError(f"{who}: a ragged batch needs both frames= and lengths=")
    phases = None
    if kind == "phase":
        phases = output[3:]
        for p in phases:
            if tuple(p.shape) != (B, T, F, 2):
                raise ValueError(f"{who}: a phase map of shape {tuple(p.shape)}, expected {(B, T, F, 2)}")
    return stft_ri, sig_ref, masks, phases


def loss_wa_misi(output, label, iters, hop_size=64, frames=None, lengths=None, kind="chimera"):
    """``loss_wa`` through ``iters`` unfolded MISI iterations (Wang, Le Roux, Wang & Hershey 2018: the phase reconstruction as
    training layers): the network's masks go through the inverse transform, then ``iters`` times through ``features.misi_phase``
    and ``features.phase_istft`` (``separation.misi`` with autograd on: every launch a node, the half-step's backward
    csrc/misi_bwd.inc), and the final estimates are compared with the source waveforms, ``wa_pit(...).mean()``.

    ``output``, ``label`` = [stft_ri_mix (B,T,F,2), sig_ref (B,C,n)], ``frames`` / ``lengths`` and the kinds "chimera", "upit" and
    "phase" (whose network phases start the iterations) as in ``loss_wa``; "enhance" raises: with one source there is no
    residual to redistribute.  The mixture waveform MISI needs is the inverse transform of ``stft_ri_mix``
    (``mask_istft(stft_ri, None, ...)``, as the testers take it), so the "chimera-wa" / "upit-wa" loaders serve as they are; it
    and the spectrum are data.  ``iters`` = 0 is exactly ``loss_wa``: the same launches, value and gradients."""
    from . import features
    from .separation import _misi_iters, misi
    iters = _misi_iters(iters, "loss_wa_misi")
    if kind == "enhance":
        raise ValueError("loss_wa_misi: kind 'enhance' has one source: MISI spreads the mixture's residual over several, there is "
                         "nothing to redistribute -- use loss_wa")
    stft_ri, sig_ref, masks, phases = _wa_args("loss_wa_misi", output, label, frames, lengths, kind)
    if iters == 0:
        return loss_wa(output, label, hop_size, frames, lengths, kind)
    n = sig_ref.shape[2]
    with torch.no_grad():
        wav = features.mask_istft(stft_ri, None, hop_size, n, frames=frames, lengths=lengths)[:, 0]
    est = misi(stft_ri, _planes_base(masks), wav, iters, hop_size, frames=frames, lengths=lengths, phases=phases)
    return wa_pit(est, sig_ref, lengths).mean()
