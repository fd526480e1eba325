"""GPU front end / back end of the separation path (K1, K2, K10).

Counterparts of onssen/data/feature_utils.py (get_stft, get_log_magnitude,
get_phase) and of the mask-apply + librosa.istft tail of
egs/wsj0-2mix/*/evaluate.py, operating on device tensors."""
import torch

from .hip import get_lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lengths_i32(lengths, B, hi, device, what, lo=1):
    """Per-row extents of a ragged batch as an int32 device tensor.  Values that come from the host are validated there; a
    device tensor is taken as it is (checking it would cost a synchronisation per call): its values must lie in [lo, hi]."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        out = lengths.to(device=device, dtype=torch.int32).contiguous()
    else:
        host = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
        if host.numel() != B or int(host.min()) < lo or int(host.max()) > hi:
            raise ValueError(f"{what}: expected {B} values in [{lo}, {hi}], got {host.tolist()}")
        out = host.to(device=device, dtype=torch.int32)
    if out.numel() != B:
        raise ValueError(f"{what}: expected {B} values, got {out.numel()}")
    return out


def stft_logmag(wav, window_size=256, hop_size=64, epsilon=1e-7, return_stft=True, lengths=None):
    """wav (B, n) or (n,) float32 cuda tensor ->
    (log_magnitude (B,T,F) float32, stft_ri (B,T,F,2) float32 | None).

    stft_ri[..., 0] + 1j*stft_ri[..., 1] is what feature_utils.get_stft
    returns per utterance (frame x frequency complex64; librosa<0.10 defaults:
    periodic Hann, centred, reflect padding); stft_ri itself is get_phase.

    ``lengths`` (B,): a RAGGED batch -- row b holds lengths[b] <= n valid samples (the rest is padding and is never
    read); its 1 + lengths[b] // hop frames are bit for bit those of a batch-1 call on wav[b, :lengths[b]], the frames
    after them are silence."""
    if wav.dim() == 1:
        wav = wav[None]
    if not wav.is_cuda:
        raise RuntimeError("stft_logmag: needs a tensor on a ROCm device; onssen_amd has no CPU fallback")
    wav = wav.float()
    if wav.stride(1) != 1:
        wav = wav.contiguous()
    B, n = wav.shape
    T, F = 1 + n // hop_size, window_size // 2 + 1
    logmag = torch.empty(B, T, F, device=wav.device, dtype=torch.float32)
    ri = torch.empty(B, T, F, 2, device=wav.device, dtype=torch.float32) if return_stft else None
    if lengths is not None:      # (every utterance must be longer than window_size / 2 samples: reflect padding)
        lengths = _lengths_i32(lengths, B, n, wav.device, "lengths", lo=window_size // 2 + 1)
    get_lib().stft_logmag(wav.data_ptr(), B, n, wav.stride(0), window_size, hop_size, float(epsilon),
                          logmag.data_ptr(), ri.data_ptr() if ri is not None else None, _stream(),
                          n_per_utt=lengths.data_ptr() if lengths is not None else None)
    return logmag, ri


_RESAMPLE_WS = {}      # (device, up, down) -> the ratio's phase-major tap image on that device


def resample(wav, rate_in, rate_out, lengths=None, sub=None):
    """wav (B, n) or (n,) float32 cuda tensor at ``rate_in`` -> (y (B, n_out) float32, lengths_out (B,) int32) at ``rate_out``:
    ``scipy.signal.resample_poly(wav, rate_out / g, rate_in / g)`` (default window) in one launch, products and sums in fp64,
    one rounding to fp32 (csrc/resample.inc).  n_out = ceil(n * rate_out / rate_in).

    ``lengths`` (B,): a RAGGED batch -- row b holds lengths[b] <= n samples (nothing beyond them is read); its
    lengths_out[b] = ceil(lengths[b] * rate_out / rate_in) outputs are bit for bit those of a batch-1 call on wav[b, :lengths[b]],
    zeros follow them.  ``sub`` (same shape as wav): the filter's input is wav - sub, formed in fp64 on load
    (``get_stft_from_subtraction``: the noise of a noisy / clean pair without a pass of its own).

    The tap image of a ratio is built on its first use (one blocking copy) and kept per device: use a ratio once before
    capturing it into a graph."""
    if not wav.is_cuda or (sub is not None and not sub.is_cuda):
        raise RuntimeError("resample: needs a tensor on a ROCm device; onssen_amd has no CPU fallback")
    if wav.dim() == 1:
        wav = wav[None]
        sub = sub[None] if sub is not None and sub.dim() == 1 else sub
    if sub is not None and sub.shape != wav.shape:
        raise ValueError(f"resample: sub has shape {tuple(sub.shape)}, wav {tuple(wav.shape)}")
    wav = wav.float()
    if wav.stride(1) != 1 or wav.stride(0) < wav.shape[1]:
        wav = wav.contiguous()
    if sub is not None:
        sub = sub.to(device=wav.device, dtype=torch.float32)
        if sub.stride() != wav.stride():
            wav, sub = wav.contiguous(), sub.contiguous()
    B, n = wav.shape
    lib, dev = get_lib(), wav.device
    up, down, _, n_out = lib.resample_geometry(int(rate_in), int(rate_out), n)
    ws = _RESAMPLE_WS.get((dev, up, down))
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"resample: the tap image of {rate_in} -> {rate_out} Hz is not built yet; call resample once before capturing")
        ws = torch.empty(lib.resample_workspace_bytes(up, down) // 8, dtype=torch.float64, device=dev)
        lib.resample_prepare(up, down, ws.data_ptr(), ws.numel() * 8, _stream())
        _RESAMPLE_WS[(dev, up, down)] = ws
    if lengths is not None:
        lengths = _lengths_i32(lengths, B, n, dev, "lengths", lo=0)
    y = torch.empty(B, n_out, device=dev, dtype=torch.float32)
    lengths_out = torch.empty(B, device=dev, dtype=torch.int32)
    lib.resample(wav.data_ptr(), sub.data_ptr() if sub is not None else None, wav.stride(0),
                 lengths.data_ptr() if lengths is not None else None, B, n, up, down, y.data_ptr(), n_out, lengths_out.data_ptr(),
                 ws.data_ptr(), ws.numel() * 8, _stream())
    return y, lengths_out


# ---- training through the inverse transforms (waveform approximation: csrc/istft_bwd.inc) ----------------------------------------
ISTFT_MASK, ISTFT_PHASE, ISTFT_MAG = 0, 1, 2


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in ts)


def _refuse_spectrum_grad(name, stft_ri):
    if torch.is_grad_enabled() and stft_ri.requires_grad:
        raise RuntimeError(f"{name}: stft_ri requires a gradient; the mixture's spectrum is data -- the backward gives the gradient "
                           f"of the masks / magnitudes (and phases) only")


def _phase_maps(phases, C, shape):
    """C phase maps (a list, or one (C,B,T,F,2) tensor) -> (tensors kept alive until the launch is queued, pointer, distance in
    floats): read where they are when they lie at one common 8-byte-aligned distance, otherwise stacked first."""
    phases = [p.float().contiguous() for p in (phases.unbind(0) if torch.is_tensor(phases) else phases)]
    if len(phases) != C or any(tuple(p.shape) != shape for p in phases):
        raise ValueError(f"phase_istft: expected {C} phase maps of shape {shape}, got {[tuple(p.shape) for p in phases]}")
    step = {phases[c + 1].data_ptr() - phases[c].data_ptr() for c in range(C - 1)}
    if len(step) > 1 or any(d % 8 for d in step) or phases[0].data_ptr() % 8:
        stacked = torch.stack(phases)                    # kept alive until the launch is queued
        phases = list(stacked.unbind(0))
        step = {phases[1].data_ptr() - phases[0].data_ptr()}
    return phases, phases[0].data_ptr(), (step.pop() // 4 if step else 0)


class _IstftGrad(torch.autograd.Function):
    """mask_istft / phase_istft / mag_istft with their backward on the device.  The forward is the plain call on the detached
    inputs (the same launch, the same bits); the backward is ``onssen_istft_backward_f32``: one launch from the gradient at the
    (B, C, length) waveforms to the gradient at the masks / magnitudes (B,T,F,C) and, in the phase mode, at the C phase maps.
    ``operand`` is (B,T,F,C) with any strides; the phase maps follow one by one, or as one (C,B,T,F,2) tensor (``stacked``)."""

    @staticmethod
    def forward(ctx, mode, hop, length, frames, lengths, stacked, stft_ri, operand, *phases):
        stft_ri, operand = stft_ri.detach(), operand.detach()
        ph = None
        if mode == ISTFT_PHASE:
            ph = phases[0].detach() if stacked else [p.detach() for p in phases]
            out = phase_istft(stft_ri, operand, ph, hop, length, frames, lengths)
        elif mode == ISTFT_MAG:
            out = mag_istft(stft_ri, operand, hop, length, frames, lengths)
        else:
            out = mask_istft(stft_ri, operand, hop, length, frames, lengths)
        ctx.saved = (stft_ri, operand, ph, frames, lengths)
        ctx.geom = (mode, hop, out.shape[2], stacked, len(phases))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        mode, hop, length, stacked, n_ph = ctx.geom
        stft_ri, operand, ph, frames, lengths = ctx.saved
        stft_ri, operand = stft_ri.float().contiguous(), operand.float()
        B, T, F, C = operand.shape
        g = g.float().contiguous()
        g_op = torch.empty(B, T, F, C, device=g.device, dtype=torch.float32)
        g_ph, keep, p_ptr, p_sc = None, None, None, 0
        if mode == ISTFT_PHASE:
            keep, p_ptr, p_sc = _phase_maps(ph, C, (B, T, F, 2))
            g_ph = torch.empty(C, B, T, F, 2, device=g.device, dtype=torch.float32)
        rag = {}
        if frames is not None:
            rag = dict(frames=frames.data_ptr(), lengths=lengths.data_ptr())      # (int32 device tensors, kept by the node)
        get_lib().istft_backward(stft_ri.data_ptr(), operand.data_ptr(), operand.stride(0), operand.stride(3), operand.stride(1),
                                 operand.stride(2), p_ptr, p_sc, mode, B, C, T, 2 * (F - 1), hop, length, g.data_ptr(), g_op.data_ptr(),
                                 g_ph.data_ptr() if g_ph is not None else None, _stream(), **rag)
        d_ph = () if mode != ISTFT_PHASE else ((g_ph,) if stacked else tuple(g_ph.unbind(0)))
        return (None, None, None, None, None, None, None, g_op, *d_ph, *([None] * (n_ph - len(d_ph))))


def _ragged_for_grad(name, frames, lengths, B, T, length, device):
    """The ragged extents as the int32 device tensors both passes of the node read (validated once)."""
    if (frames is None) != (lengths is None):
        raise ValueError(f"{name}: a ragged batch needs both frames= and lengths=")
    if frames is None:
        return None, None
    return _lengths_i32(frames, B, T, device, "frames"), _lengths_i32(lengths, B, length, device, "lengths")


def mask_istft(stft_ri, masks, hop_size=64, length=None, frames=None, lengths=None):
    """stft_ri (B,T,F,2); masks (B,T,F,C) (any strides) or None ->
    (B, C, length) float32: istft(stft * mask_c) per speaker, librosa
    semantics (hop, length=nsample).

    ``frames`` / ``lengths`` (B,): a RAGGED batch -- row b has frames[b] <= T frames and lengths[b] <= length output
    samples (zeros after them); inside them the result is bit for bit that of a batch-1 call on that utterance.

    Differentiable with respect to ``masks``: when autograd is on and they require a gradient, the same launch runs inside an
    autograd node whose backward is ``onssen_istft_backward_f32`` (csrc/istft_bwd.inc); a ``stft_ri`` that requires one raises."""
    if not stft_ri.is_cuda:
        raise RuntimeError("mask_istft: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    _refuse_spectrum_grad("mask_istft", stft_ri)
    if _wants_grad(masks):
        B, T = stft_ri.shape[:2]
        n = hop_size * (T - 1) if length is None else length
        frames, lengths = _ragged_for_grad("mask_istft", frames, lengths, B, T, n, stft_ri.device)
        return _IstftGrad.apply(ISTFT_MASK, hop_size, n, frames, lengths, False, stft_ri, masks.float())
    stft_ri = stft_ri.float().contiguous()
    B, T, F, _ = stft_ri.shape
    n_fft = 2 * (F - 1)
    if length is None:
        length = hop_size * (T - 1)
    lib = get_lib()
    rag = {}
    if (frames is None) != (lengths is None):
        raise ValueError("mask_istft: a ragged batch needs both frames= and lengths=")
    if frames is not None:
        frames = _lengths_i32(frames, B, T, stft_ri.device, "frames")
        lengths = _lengths_i32(lengths, B, length, stft_ri.device, "lengths")
        rag = dict(frames=frames.data_ptr(), lengths=lengths.data_ptr())
    if masks is None:
        out = torch.empty(B, 1, length, device=stft_ri.device, dtype=torch.float32)
        lib.mask_istft(stft_ri.data_ptr(), None, 0, 0, 0, 0, B, 1, T, n_fft, hop_size, length, out.data_ptr(),
                       _stream(), **rag)
        return out
    masks = masks.float()
    C = masks.shape[3]
    out = torch.empty(B, C, length, device=stft_ri.device, dtype=torch.float32)
    lib.mask_istft(stft_ri.data_ptr(), masks.data_ptr(), masks.stride(0), masks.stride(3), masks.stride(1),
                   masks.stride(2), B, C, T, n_fft, hop_size, length, out.data_ptr(), _stream(), **rag)
    return out


def phase_istft(stft_ri, masks, phases, hop_size=64, length=None, frames=None, lengths=None, out=None):
    """stft_ri (B,T,F,2); masks (B,T,F,C) (any strides); phases: C tensors (B,T,F,2), or one (C,B,T,F,2) ->
    (B, C, length) float32: istft(mask_c * |stft| * (phase_c.re + i phase_c.im)) per speaker -- phase_net's reconstruction from
    its masks and unit phase vectors (mask_istft re-uses the mixture's phase instead).

    The phase maps are read where they are when they lie at one common distance from each other (two slices of one buffer,
    as phase_net's forward returns them; any two fp32 tensors); otherwise they are stacked first.

    ``frames`` / ``lengths`` (B,): a RAGGED batch exactly as in ``mask_istft`` (both or neither).  ``out``: a (B, C, length)
    float32 contiguous tensor to write into instead of a new one (``separation.misi`` re-uses one across its iterations).

    Differentiable with respect to ``masks`` and ``phases`` as ``mask_istft`` is with respect to its masks (``out=`` together
    with an input that requires a gradient raises)."""
    if (frames is None) != (lengths is None):
        raise ValueError("phase_istft: a ragged batch needs both frames= and lengths=")
    if not stft_ri.is_cuda:
        raise RuntimeError("phase_istft: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    _refuse_spectrum_grad("phase_istft", stft_ri)
    if _wants_grad(masks, *([phases] if torch.is_tensor(phases) else phases)):
        if out is not None:
            raise ValueError("phase_istft: out= cannot be combined with inputs that require a gradient")
        B, T = stft_ri.shape[:2]
        n = hop_size * (T - 1) if length is None else length
        frames, lengths = _ragged_for_grad("phase_istft", frames, lengths, B, T, n, stft_ri.device)
        stacked = torch.is_tensor(phases)
        return _IstftGrad.apply(ISTFT_PHASE, hop_size, n, frames, lengths, stacked, stft_ri, masks.float(),
                                *([phases.float()] if stacked else [p.float() for p in phases]))
    stft_ri = stft_ri.float().contiguous()
    B, T, F, _ = stft_ri.shape
    n_fft = 2 * (F - 1)
    if length is None:
        length = hop_size * (T - 1)
    rag = {}
    if frames is not None:
        frames = _lengths_i32(frames, B, T, stft_ri.device, "frames")
        lengths = _lengths_i32(lengths, B, length, stft_ri.device, "lengths")
        rag = dict(frames=frames.data_ptr(), lengths=lengths.data_ptr())
    masks = masks.float()
    C = masks.shape[3]
    phases, p_ptr, p_sc = _phase_maps(phases, C, (B, T, F, 2))
    if out is None:
        out = torch.empty(B, C, length, device=stft_ri.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, C, length) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != stft_ri.device:
        raise ValueError(f"phase_istft: out must be a contiguous float32 tensor of shape {(B, C, length)} on {stft_ri.device}")
    get_lib().phase_istft(stft_ri.data_ptr(), masks.data_ptr(), masks.stride(0), masks.stride(3), masks.stride(1), masks.stride(2),
                          p_ptr, p_sc, B, C, T, n_fft, hop_size, length, out.data_ptr(),
                          _stream(), **rag)
    return out


class _MisiPhaseGrad(torch.autograd.Function):
    """misi_phase with its backward on the device.  The forward is the plain call on the detached inputs (the same launch, the
    same bits); the backward is ``onssen_misi_phase_backward_f32`` (csrc/misi_bwd.inc): two launches from the gradient at the
    (C,B,T,F,2) phase maps to the gradient at the (B,C,n) estimates, the Jacobian at the float32 estimates evaluated in fp64.
    The mixture is data and gets no gradient; the workspace is allocated per backward call (the caching allocator: no
    synchronisation, capturable)."""

    @staticmethod
    def forward(ctx, window_size, hop, lengths, mix, est):
        mix, est = mix.detach(), est.detach()
        out = misi_phase(mix, est, window_size, hop, lengths)
        ctx.saved = (mix, est, lengths)
        ctx.geom = (window_size, hop)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        window_size, hop = ctx.geom
        mix, est, lengths = ctx.saved
        mix, est = mix.float(), est.float()
        if mix.stride(1) != 1:
            mix = mix.contiguous()
        if est.stride(2) != 1:
            est = est.contiguous()
        B, C, n = est.shape
        g = g.float().contiguous()
        lib = get_lib()
        nbytes = lib.misi_phase_backward_workspace_bytes(B, C, n, window_size, hop)
        ws = torch.empty(nbytes // 8, device=g.device, dtype=torch.float64)
        g_est = torch.empty(B, C, n, device=g.device, dtype=torch.float32)
        lib.misi_phase_backward(mix.data_ptr(), mix.stride(0), est.data_ptr(), est.stride(0), est.stride(1), B, C, n, window_size, hop,
                                g.data_ptr(), g_est.data_ptr(), ws.data_ptr(), nbytes, _stream(),
                                n_per_utt=lengths.data_ptr() if lengths is not None else None)
        return None, None, None, None, g_est


def misi_phase(mix, est, window_size=256, hop_size=64, lengths=None, out=None):
    """The half-step of MISI (multiple input spectrogram inversion) between two inverse transforms, one launch (csrc/misi.inc):
    mix (B, n), est (B, C, n) float32 cuda tensors, 2 <= C <= 8 -> (C, B, T, F, 2) float32 unit phase vectors, T = 1 + n // hop,
    F = window_size // 2 + 1 -- what ``phase_istft`` takes as ``phases``.  Per sample, in fp64, the mixture's residual is spread
    evenly over the speakers, u_c = est_c + (mix - sum_j est_j) / C, and the phase of STFT(u_c) (the framing of ``stft_logmag``)
    is kept: Z / |Z|, (1, 0) where Z = 0.  ``est`` is read where it is with any batch and speaker strides (unit sample stride).

    ``lengths`` (B,): a RAGGED batch as in ``stft_logmag`` -- nothing beyond lengths[b] is read, row b's own 1 + lengths[b] // hop
    frames are bit for bit those of a batch-1 call, the frames after them are silence, (1, 0).  ``out``: a (C, B, T, F, 2) float32
    contiguous tensor to write into instead of a new one.

    Differentiable with respect to ``est``: when autograd is on and it requires a gradient, the same launch runs inside an autograd
    node whose backward is ``onssen_misi_phase_backward_f32`` (csrc/misi_bwd.inc) -- what training through unfolded MISI
    iterations needs (``separation.misi``, ``loss.loss_wa_misi``); ``out=`` together with such an input raises, and so does a
    ``mix`` that requires a gradient: the mixture is data."""
    if _wants_grad(mix):
        raise RuntimeError("misi_phase: mix requires a gradient; the mixture is data -- the backward gives the gradient of the estimates only")
    if _wants_grad(est) and out is not None:
        raise ValueError("misi_phase: out= cannot be combined with inputs that require a gradient")
    if not mix.is_cuda or not est.is_cuda:
        raise RuntimeError("misi_phase: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    if mix.dim() != 2 or est.dim() != 3 or est.shape[0] != mix.shape[0] or est.shape[2] != mix.shape[1]:
        raise ValueError(f"misi_phase: expected mix (B, n) and est (B, C, n), got {tuple(mix.shape)} and {tuple(est.shape)}")
    if _wants_grad(est):
        if not 2 <= est.shape[1] <= 8:
            raise ValueError(f"misi_phase: {est.shape[1]} speakers; the kernel takes 2 .. 8")
        if lengths is not None:
            lengths = _lengths_i32(lengths, est.shape[0], est.shape[2], mix.device, "lengths", lo=window_size // 2 + 1)
        return _MisiPhaseGrad.apply(window_size, hop_size, lengths, mix, est.float())
    mix, est = mix.float(), est.float()
    if mix.stride(1) != 1:
        mix = mix.contiguous()
    if est.stride(2) != 1:
        est = est.contiguous()
    B, C, n = est.shape
    if not 2 <= C <= 8:
        raise ValueError(f"misi_phase: {C} speakers; the kernel takes 2 .. 8")
    T, F = 1 + n // hop_size, window_size // 2 + 1
    if lengths is not None:      # (every utterance must be longer than window_size / 2 samples: reflect padding)
        lengths = _lengths_i32(lengths, B, n, mix.device, "lengths", lo=window_size // 2 + 1)
    if out is None:
        out = torch.empty(C, B, T, F, 2, device=mix.device, dtype=torch.float32)
    elif tuple(out.shape) != (C, B, T, F, 2) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != mix.device:
        raise ValueError(f"misi_phase: out must be a contiguous float32 tensor of shape {(C, B, T, F, 2)} on {mix.device}")
    get_lib().misi_phase(mix.data_ptr(), mix.stride(0), est.data_ptr(), est.stride(0), est.stride(1), B, C, n, window_size, hop_size,
                         out.data_ptr(), _stream(), n_per_utt=lengths.data_ptr() if lengths is not None else None)
    return out


def training_labels(stft_mix, stft_s1, stft_s2, feature_mix, db_threshold=40.0, with_cos=False):
    """Label-side features of a batch of chunks on the GPU: counterparts of get_one_hot,
    np.abs and get_cos_difference (onssen/data/feature_utils.py:77-95, wsj0_2mix.py:130-152).
    Inputs: (B,T,F,2) float32 STFTs as returned by stft_logmag, feature_mix (B,T,F).
    Returns one_hot (B,T,F,2) float32, mag_mix, mag_s1, mag_s2 (B,T,F) [, cos_s1, cos_s2]."""
    if not stft_mix.is_cuda:
        raise RuntimeError("training_labels: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    B, T, F, _ = stft_mix.shape
    dev = stft_mix.device
    stft_mix, stft_s1, stft_s2 = stft_mix.contiguous(), stft_s1.contiguous(), stft_s2.contiguous()
    feature_mix = feature_mix.contiguous()
    mk = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    one_hot, mm, m1, m2, umax = mk(B, T, F, 2), mk(B, T, F), mk(B, T, F), mk(B, T, F), mk(B)
    c1, c2 = (mk(B, T, F), mk(B, T, F)) if with_cos else (None, None)
    get_lib().labels(stft_mix.data_ptr(), stft_s1.data_ptr(), stft_s2.data_ptr(), feature_mix.data_ptr(), B, T, F,
                     float(db_threshold), umax.data_ptr(), one_hot.data_ptr(), mm.data_ptr(), m1.data_ptr(),
                     m2.data_ptr(), c1.data_ptr() if with_cos else None, c2.data_ptr() if with_cos else None, _stream())
    return (one_hot, mm, m1, m2, c1, c2) if with_cos else (one_hot, mm, m1, m2)


def mag_istft(stft_ri, mags, hop_size=64, length=None, frames=None, lengths=None):
    """stft_ri (B,T,F,2); mags (B,T,F,C) (any strides), or (B,T,F) for one channel -> (B, C, length) float32:
    istft(mags_c * exp(i angle(stft))) per channel -- an estimated MAGNITUDE put back on the mixture's phase, the
    reconstruction of the enhancement recipe (the ``enhance`` network returns a clean magnitude, not a mask).  A bin whose
    spectrum is exactly 0 has phase 0, as np.angle gives it.

    ``frames`` / ``lengths`` (B,): a RAGGED batch exactly as in ``mask_istft``.  Differentiable with respect to ``mags`` as
    ``mask_istft`` is with respect to its masks."""
    if not stft_ri.is_cuda:
        raise RuntimeError("mag_istft: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    _refuse_spectrum_grad("mag_istft", stft_ri)
    if _wants_grad(mags):
        B, T, F = stft_ri.shape[:3]
        if mags.dim() == 3:
            mags = mags.unsqueeze(-1)
        if tuple(mags.shape[:3]) != (B, T, F):
            raise ValueError(f"mag_istft: expected magnitudes of shape {(B, T, F)} (+ channels), got {tuple(mags.shape)}")
        n = hop_size * (T - 1) if length is None else length
        frames, lengths = _ragged_for_grad("mag_istft", frames, lengths, B, T, n, stft_ri.device)
        return _IstftGrad.apply(ISTFT_MAG, hop_size, n, frames, lengths, False, stft_ri, mags.float())
    stft_ri = stft_ri.float().contiguous()
    B, T, F, _ = stft_ri.shape
    n_fft = 2 * (F - 1)
    if length is None:
        length = hop_size * (T - 1)
    if (frames is None) != (lengths is None):
        raise ValueError("mag_istft: a ragged batch needs both frames= and lengths=")
    rag = {}
    if frames is not None:
        frames = _lengths_i32(frames, B, T, stft_ri.device, "frames")
        lengths = _lengths_i32(lengths, B, length, stft_ri.device, "lengths")
        rag = dict(frames=frames.data_ptr(), lengths=lengths.data_ptr())
    mags = mags.float()
    if mags.dim() == 3:
        mags = mags.unsqueeze(-1)
    if tuple(mags.shape[:3]) != (B, T, F):
        raise ValueError(f"mag_istft: expected magnitudes of shape {(B, T, F)} (+ channels), got {tuple(mags.shape)}")
    C = mags.shape[3]
    out = torch.empty(B, C, length, device=stft_ri.device, dtype=torch.float32)
    get_lib().mag_istft(stft_ri.data_ptr(), mags.data_ptr(), mags.stride(0), mags.stride(3), mags.stride(1), mags.stride(2),
                        B, C, T, n_fft, hop_size, length, out.data_ptr(), _stream(), **rag)
    return out


def enhance_labels(stft_noisy, stft_clean, with_cos=True):
    """Label-side features of the enhancement recipe on the GPU, one pass (onssen/data/daps_enhance.py:104-106: np.abs, np.abs,
    get_cos_difference): (..., 2) float32 spectra of the noisy and the clean signal, as ``stft_logmag`` returns them ->
    (mag_noisy, mag_clean, cos_diff), each of the spectra's shape without the last axis; ``with_cos=False`` leaves cos_diff out
    (None): evaluation needs the magnitudes only.  ``stft_clean=None`` (separation has no clean signal): (mag_noisy, None, None)."""
    if not stft_noisy.is_cuda:
        raise RuntimeError("enhance_labels: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    if stft_noisy.shape[-1] != 2 or (stft_clean is not None and stft_clean.shape != stft_noisy.shape):
        raise ValueError(f"enhance_labels: expected two (..., 2) spectra of one shape, got {tuple(stft_noisy.shape)} and "
                         f"{None if stft_clean is None else tuple(stft_clean.shape)}")
    stft_noisy = stft_noisy.float().contiguous()
    shape, dev = stft_noisy.shape[:-1], stft_noisy.device
    mk = lambda: torch.empty(shape, device=dev, dtype=torch.float32)
    mag_noisy = mk()
    if stft_clean is None:
        get_lib().labels_enhance(stft_noisy.data_ptr(), None, mag_noisy.numel(), mag_noisy.data_ptr(), None, None, _stream())
        return mag_noisy, None, None
    stft_clean = stft_clean.float().contiguous()
    mag_clean, cos_diff = mk(), (mk() if with_cos else None)
    get_lib().labels_enhance(stft_noisy.data_ptr(), stft_clean.data_ptr(), mag_noisy.numel(), mag_noisy.data_ptr(),
                             mag_clean.data_ptr(), cos_diff.data_ptr() if with_cos else None, _stream())
    return mag_noisy, mag_clean, cos_diff
