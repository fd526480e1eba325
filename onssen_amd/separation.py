"""End-to-end separation: waveform -> K1..K10 -> waveforms.

Counterpart of tester.eval + get_est_sig (onssen/utils/test.py:29-41,
egs/wsj0-2mix/chimera/evaluate.py:23-45, deep_clustering/evaluate.py:22-47)
with the device->host->device hop removed for the mask-inference models."""
import numpy as np
import torch

from . import options
from .features import mask_istft, stft_logmag
from .nn._core import _XcdStatus, recovering


def _ragged(wav, lengths, hop_size):
    """(lengths, frames) as int32 device tensors for a ragged batch of waveforms, or (None, None)."""
    if lengths is None:
        return None, None
    from .features import _lengths_i32
    lengths = _lengths_i32(lengths, wav.shape[0], wav.shape[-1], wav.device, "lengths", lo=hop_size)
    return lengths, (1 + lengths // hop_size).to(torch.int32)


def _misi_iters(iters, who):
    """``iters`` as a non-negative int, or ValueError."""
    import numbers
    if isinstance(iters, bool) or not isinstance(iters, numbers.Integral) or iters < 0:
        raise ValueError(f"{who}: the number of MISI iterations must be a non-negative integer, got {iters!r}")
    return int(iters)


def misi(stft_ri, masks, wav, iters, hop_size=64, frames=None, lengths=None, phases=None):
    """MISI (multiple input spectrogram inversion: Gunawan & Sen 2010; the phase reconstruction of Wang, Le Roux, Wang & Hershey
    2018 after a chimera++ network) on the device: stft_ri (B,T,F,2) the mixture's spectrum, masks (B,T,F,C) (any strides), wav
    (B, n) the mixture -> (B, C, n) float32.  The estimated magnitudes mask_c |X| stay fixed; the phases start as the mixture's
    (``mask_istft``) -- or as ``phases``, C maps (B,T,F,2) of unit vectors such as phase_net's, through ``phase_istft`` -- and every
    iteration is two launches: ``features.misi_phase`` (the residual mix - sum of the estimates spread evenly over the speakers,
    STFT, Z / |Z|: csrc/misi.inc) and ``features.phase_istft`` with those phases.

    ``iters`` = 0 returns exactly ``mask_istft(...)`` (``phase_istft(...)`` with ``phases``) and launches nothing else.  ``frames``
    / ``lengths`` (B,): a ragged batch as in ``mask_istft`` (both or neither).  Nothing is read back by the host and the
    phase buffer and the estimates are allocated once per call, so a call can be captured in a hipGraph.

    Unfolded MISI as training layers (Wang et al. 2018): when autograd is on and ``masks`` or ``phases`` require a gradient, the
    same launches run as a chain of autograd nodes (``mask_istft`` / ``phase_istft`` -> ``misi_phase`` -> ``phase_istft`` -> ...)
    with fresh buffers per iteration, and the result is differentiable with respect to them; the mixture (``stft_ri``, ``wav``)
    is data.  Otherwise nothing is recorded and the buffers are re-used as above."""
    from .features import _wants_grad
    iters = _misi_iters(iters, "misi")
    if (frames is None) != (lengths is None):
        raise ValueError("misi: a ragged batch needs both frames= and lengths=")
    if not stft_ri.is_cuda or not wav.is_cuda:
        raise RuntimeError("misi: needs tensors on a ROCm device; onssen_amd has no CPU fallback")
    if wav.dim() == 1:
        wav = wav[None]
    track = _wants_grad(masks, *(() if phases is None else [phases] if torch.is_tensor(phases) else phases))
    with torch.enable_grad() if track else torch.no_grad():
        return _misi(stft_ri, masks, wav, iters, hop_size, frames, lengths, phases, track)


def _misi(stft_ri, masks, wav, iters, hop_size, frames, lengths, phases, track):
    """``misi`` after its checks; ``track``: every launch is an autograd node with buffers of its own."""
    from .features import misi_phase, phase_istft
    n = wav.shape[-1]
    if phases is not None:
        est = phase_istft(stft_ri, masks, phases, hop_size, n, frames=frames, lengths=lengths)
    else:
        est = mask_istft(stft_ri, masks, hop_size, n, frames=frames, lengths=lengths)
    if iters == 0:
        return est
    if frames is not None:       # validated once, passed on as device tensors
        from .features import _lengths_i32
        frames = _lengths_i32(frames, est.shape[0], stft_ri.shape[1], est.device, "frames")
        lengths = _lengths_i32(lengths, est.shape[0], n, est.device, "lengths")
    stft_ri, masks = stft_ri.float().contiguous(), masks.float()
    n_fft = 2 * (stft_ri.shape[2] - 1)
    ph = None
    for _ in range(iters):
        ph = misi_phase(wav, est, n_fft, hop_size, lengths=lengths, out=None if track else ph)
        est = phase_istft(stft_ri, masks, ph, hop_size, n, frames=frames, lengths=lengths, out=None if track else est)
    return est


@recovering
@torch.no_grad()
def separate_chimera(model, wav, window_size=256, hop_size=64, lengths=None, misi_iters=0):
    """wav (B, n) cuda float32 -> (B, 2, n): masks straight from the network.  ``lengths`` (B,): a ragged batch of whole
    utterances padded to n samples (see separate_dc).  ``misi_iters`` = K > 0: K iterations of MISI phase reconstruction after
    the masks (``misi``; two launches each); 0 is the mixture's phase, the reference's result."""
    misi_iters = _misi_iters(misi_iters, "separate_chimera")
    lengths, frames = _ragged(wav, lengths, hop_size)
    logmag, ri = stft_logmag(wav, window_size, hop_size, lengths=lengths)
    _, masks = model.embedding_and_masks(logmag, frames)
    if misi_iters:
        out = misi(ri, masks, wav, misi_iters, hop_size, frames=frames, lengths=lengths)
    else:
        out = mask_istft(ri, masks, hop_size, wav.shape[-1], frames=frames, lengths=lengths)
    _XcdStatus.flush()            # an aborted recurrence is caught HERE (and the call re-run, see `recovering`), not by the next call
    return out


@recovering
@torch.no_grad()
def separate_upit(model, wav, window_size=256, hop_size=64, lengths=None, misi_iters=0):
    """wav (B, n) cuda float32 -> (B, S, n), S = ``model.num_speaker`` (2 .. 4): STFT -> ``uPIT_LSTM.masks`` -> ``mask_istft``.
    Nothing is read back by the host, so a call can be captured in a hipGraph.  ``lengths`` (B,): a ragged batch of whole
    utterances padded to n samples; every row inside its own length is bit for bit its batch-1 result, zeros after it (see
    separate_dc).  ``misi_iters`` = K > 0: K iterations of MISI phase reconstruction after the masks (``misi``)."""
    misi_iters = _misi_iters(misi_iters, "separate_upit")
    lengths, frames = _ragged(wav, lengths, hop_size)
    logmag, ri = stft_logmag(wav, window_size, hop_size, lengths=lengths)
    masks = model.masks(logmag, frames)
    if misi_iters:
        out = misi(ri, masks, wav, misi_iters, hop_size, frames=frames, lengths=lengths)
    else:
        out = mask_istft(ri, masks, hop_size, wav.shape[-1], frames=frames, lengths=lengths)
    _XcdStatus.flush()            # an aborted recurrence is caught HERE (and the call re-run, see `recovering`), not by the next call
    return out


@recovering
@torch.no_grad()
def separate_phase(model, wav, window_size=256, hop_size=64, misi_iters=0):
    """wav (B, n) cuda float32 -> (B, 2, n): phase_net's masks AND its phase estimates go into the inverse transform
    (features.phase_istft); the mixture's phase is only the network's input.  Uniform batches (phase_net has no ragged forward).
    ``misi_iters`` = K > 0: K iterations of MISI after that, starting from the network's phases (``misi(..., phases=)``)."""
    from .features import phase_istft
    misi_iters = _misi_iters(misi_iters, "separate_phase")
    logmag, ri = stft_logmag(wav, window_size, hop_size)
    _, mask_A, mask_B, phase_A, phase_B = model([logmag, ri])
    base = getattr(mask_A, "_base", None)            # the network's (B,T,F,2) mask buffer, when both masks are its planes
    if base is None or getattr(mask_B, "_base", None) is not base or base.shape != mask_A.shape + (2,):
        base = torch.stack([mask_A, mask_B], -1)
    if misi_iters:
        out = misi(ri, base, wav, misi_iters, hop_size, phases=[phase_A, phase_B])
    else:
        out = phase_istft(ri, base, [phase_A, phase_B], hop_size, wav.shape[-1])
    _XcdStatus.flush()            # an aborted recurrence is caught HERE (and the call re-run, see `recovering`), not by the next call
    return out


@recovering
@torch.no_grad()
def separate_enhance(model, wav, window_size=256, hop_size=64, lengths=None):
    """Speech enhancement, waveform in -> (B, n) waveform out (egs/daps: ``enhance`` estimates the clean MAGNITUDE, which goes
    back to a waveform on the noisy signal's phase): STFT -> |X| -> ``model([logmag, |X|])`` -> ``features.mag_istft``.  Nothing is
    read back by the host, so a call can be captured in a hipGraph.  ``lengths`` (B,): a ragged batch of whole utterances padded
    to n samples; every row inside its own length is bit for bit its batch-1 result, zeros after it (see separate_dc)."""
    from .features import enhance_labels, mag_istft
    lengths, frames = _ragged(wav, lengths, hop_size)
    logmag, ri = stft_logmag(wav, window_size, hop_size, lengths=lengths)
    mag = enhance_labels(ri, None)[0]
    clean, = model([logmag, mag]) if frames is None else model([logmag, mag], frames=frames)
    out = mag_istft(ri, clean, hop_size, wav.shape[-1], frames=frames, lengths=lengths)
    _XcdStatus.flush()            # an aborted recurrence is caught HERE (and the call re-run, see `recovering`), not by the next call
    return out[:, 0]


@torch.no_grad()
def separate_tasnet(model, waves):
    """Time-domain separation of whole utterances: ``waves`` a list of 1-D waveforms of any lengths (one device) -> a list of
    (num_spks, S_out_k) tensors, S_out_k = min(S_k, (T_k - 1) L/2 + L) as ``tester_tasnet`` cuts them (trailing samples that
    fill no encoder frame are dropped).  The utterances go through ``ConvTasNet.forward(..., lengths=)`` in the order given,
    ``model.RAGGED_MAX`` per forward; each result is bit for bit the one-utterance forward's."""
    from torch.nn.utils.rnn import pad_sequence
    K = int(model.RAGGED_MAX)
    waves = list(waves)
    if any(w.dim() != 1 for w in waves):
        raise ValueError("separate_tasnet: every waveform must be 1-D (samples,)")
    hop, out = model.L // 2, []
    for at in range(0, len(waves), K):
        chunk = waves[at:at + K]
        lens = [int(w.shape[0]) for w in chunk]
        est = model([pad_sequence(chunk, batch_first=True)], lengths=lens)
        for b, S in enumerate(lens):
            S_out = min(S, ((S - model.L) // hop) * hop + model.L)
            out.append(torch.stack([e[b, :S_out] for e in est]))
    return out


@torch.no_grad()
def separate_tasnet_stream(model, x, chunk):
    """A whole signal through the STREAMING path of a causal ConvTasNet: x (n, S), or (S,), fed to ``model.stream(n)`` in
    pushes of ``chunk`` hops (hop = L/2; the last push is shorter when the hops do not divide), then flushed.  Returns what
    ``model([x])`` returns, bit for bit: the one hop of delay is trimmed and the samples beyond the last whole hop are dropped, as
    the forward drops them.  Shows how the pieces of a stream fit together; an online caller keeps the stream object and
    calls ``push`` as audio arrives."""
    if x.dim() == 1:
        x = x.unsqueeze(0)
    hop, chunk = model.L // 2, int(chunk)
    if chunk < 1:
        raise ValueError(f"separate_tasnet_stream: chunk must be at least one hop, got {chunk}")
    n, S = x.shape
    hops = S // hop
    if hops < 2:
        raise RuntimeError(f"ConvTasNet: {S} samples is shorter than one encoder frame (L = {model.L})")
    st = model.stream(n)
    pieces = [st.push(x[:, at * hop:min(at + chunk, hops) * hop]) for at in range(0, hops, chunk)]
    tail = st.flush()
    return [torch.squeeze(torch.cat([p[s] for p in pieces] + [tail[s]], dim=1)[:, hop:]) for s in range(model.num_spks)]


def tasnet_long_geometry(L, S, window, step):
    """Windows of a long-form separation -> (S_out, K, v_last): K windows of ``window`` samples start at k ``step``; all are
    full but the last, which holds ``v_last`` samples; S_out is what the plain forward returns for S samples.  K = 1 with
    v_last = S_out when the signal fits one window.  Raises ValueError naming the violated requirement (hop = L/2,
    overlap = window - step):  hop | step;  hop | (window - L), so that a window's output has exactly ``window`` samples;
    L <= overlap <= window / 2, so that at most two windows ever cover a sample."""
    L, S, W, step = int(L), int(S), int(window), int(step)
    hop = L // 2
    if step < 1 or step % hop:
        raise ValueError(f"separate_tasnet_long: step = {step} must be a positive multiple of hop = {hop}")
    if W < L or (W - L) % hop:
        raise ValueError(f"separate_tasnet_long: window = {W} must be L = {L} plus a multiple of hop = {hop}, so that a "
                         "window's output has as many samples as the window")
    O = W - step
    if not L <= O <= W // 2:
        raise ValueError(f"separate_tasnet_long: overlap = window - step = {O} must lie in [L, window / 2] = [{L}, {W // 2}], "
                         "so that consecutive windows share a frame and at most two windows cover a sample")
    if S < L:
        raise RuntimeError(f"ConvTasNet: {S} samples is shorter than one encoder frame (L = {L})")
    S_out = (S - L) // hop * hop + L
    if S_out <= W:
        return S_out, 1, S_out
    K = 1 + -(-(S_out - W) // step)
    # K - 1 = ceil((S_out - W) / step):  (K - 1) step >= S_out - W gives v_last <= W, and (K - 2) step < S_out - W gives
    # v_last = S_out - (K - 1) step > W - step = overlap.  hop divides S_out - L, step and window - L, so the last window is
    # L plus whole hops too and its forward returns exactly v_last samples.
    return S_out, K, S_out - (K - 1) * step


@torch.no_grad()
def separate_tasnet_long(model, wav, window, step=None, batch=16, return_windows=False):
    """Long-form time-domain separation: ``wav`` (S,) on a ROCm device, of any length, is cut into windows of ``window`` samples
    that start ``step`` apart (default: ``window // 2`` rounded down to a multiple of hop = L/2), every window is separated on
    its own -- the gLN statistics see what they saw in training, the activations are those of ``batch`` windows -- and the
    estimates are put back together on the device (csrc/tasnet_stitch.inc): a model assigns speakers to output rows per window,
    so consecutive windows are permutation-aligned on their overlap (maximal summed inner product, ties to the identity) and
    then cross-faded linearly.  Returns (num_spks, S_out), S_out what ``model([wav])`` returns; a signal that fits one window
    IS ``model([wav])``, bit for bit.  ``return_windows=True``: also the window estimates (num_spks, K, window) -- the last
    window holds ``S_out - (K - 1) step`` samples and zeros after them -- and ``perm`` (K, num_spks) int32, the row of window k
    that carries output channel c.  The full windows go through the eval forward ``batch`` rows at a time, a shorter last window
    through a forward of its own; nothing is read back by the host, so a call can be captured in a hipGraph.  Every ``norm``,
    causal or not, up to 4 speakers; eval mode and no autograd, like ``forward(..., lengths=)``.  ``tasnet_long_geometry``
    states the requirements on ``window`` and ``step``."""
    from .hip import get_lib
    from .nn._core import _stream, needs_graph, require_device, use_hip_path
    if model.training or not use_hip_path(model) or needs_graph(wav):
        raise RuntimeError("ConvTasNet: separate_tasnet_long is an inference call: it needs eval mode and no autograd "
                           "(torch.no_grad(), or frozen parameters)")
    if not torch.is_tensor(wav) or wav.dim() != 1:
        raise ValueError("separate_tasnet_long: wav must be a 1-D tensor (samples,)")
    model._require_hip_forward()
    C = model.num_spks
    if C > 4:
        raise ValueError(f"separate_tasnet_long: num_spks = {C} > 4 (the permutation search is exhaustive)")
    hop, W, batch = model.L // 2, int(window), int(batch)
    if batch < 1:
        raise ValueError(f"separate_tasnet_long: batch must be at least 1, got {batch}")
    step = W // 2 // hop * hop if step is None else int(step)
    S_out, K, v_last = tasnet_long_geometry(model.L, wav.shape[0], W, step)
    require_device(wav, "ConvTasNet")
    dev = wav.device
    if K == 1:
        est = model._hip_forward_rows(wav.unsqueeze(0))                    # (C, 1, S_out)
        if return_windows:
            return est[:, 0], est, torch.arange(C, dtype=torch.int32, device=dev).unsqueeze(0)
        return est[:, 0]
    lib, st = get_lib(), _stream()
    wav = wav.float().contiguous()
    win = torch.empty(K, W, device=dev, dtype=torch.float32)
    lib.tasnet_windows(wav.data_ptr(), S_out, K, W, step, win.data_ptr(), st)
    est = torch.empty(C, K, W, device=dev, dtype=torch.float32)
    full = K if v_last == W else K - 1
    for at in range(0, full, batch):
        rows = model._hip_forward_rows(win[at:at + min(batch, full - at)])
        if rows.shape[1] == K:
            est = rows                                                      # one forward covered every window
        else:
            est[:, at:at + rows.shape[1]].copy_(rows)                       # (the forward writes speaker-major per call)
    if full < K:
        est[:, K - 1, :v_last].copy_(model._hip_forward_rows(win[K - 1:, :v_last])[:, 0])
        est[:, K - 1, v_last:].zero_()
    out = torch.empty(C, S_out, device=dev, dtype=torch.float32)
    perm = torch.empty(K, C, device=dev, dtype=torch.int32)
    nb = lib.tasnet_stitch_workspace_bytes(C, K, W, step, v_last)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    lib.tasnet_stitch(est.data_ptr(), C, K, W, step, v_last, out.data_ptr(), perm.data_ptr(), ws.data_ptr(), nb, st)
    return (out, est, perm) if return_windows else out


_CLUSTER_WS = {}           # (device, B, T, F, D[, "compact"], stream) -> buffer of a uniform shape
_CLUSTER_SCRATCH = {}      # (device, stream) -> grow-only buffer of the ragged / shape-changing calls (see dc_masks)
_CLUSTER_PINNED = set()    # keys of _CLUSTER_WS handed out for / during a hipGraph capture: never evicted


def _cluster_ws(device, key, nb, head, ragged):
    """Workspace of the clustering back end, private to the calling STREAM (round 5: every call rewrites the header --
    centroids, counters, the status word -- so two streams of one process separating at once must not share a buffer; work
    on one stream is ordered and reuses its own).  Uniform shapes: one buffer per (shape, stream) (hipGraph-capturable),
    most recently used last, at most 8 that no graph points into.  Ragged batches bring a new longest utterance every time:
    ONE grow-only buffer per (device, stream).  Either way it is allocated uninitialised and only its first ``head`` bytes
    (the library's ``comp_offset``: everything in front of the compacted array, which is as large as the embedding and is
    written before it is read) are zeroed."""
    capturing = torch.cuda.is_current_stream_capturing()
    stream = torch.cuda.current_stream(device).cuda_stream
    if ragged:
        if capturing:
            raise RuntimeError("dc_masks: ragged batches (frames=...) cannot be captured in a hipGraph (shared grow-only workspace)")
        ws = _CLUSTER_SCRATCH.get((device, stream))
        if ws is None or ws.numel() < nb:
            ws = _CLUSTER_SCRATCH[(device, stream)] = torch.empty(max(nb, int(nb * 1.25)), dtype=torch.uint8, device=device)
        ws[:head].zero_()                  # (the status word of an earlier call was examined by _XcdStatus before this one is issued)
        return ws
    if capturing:
        # a capture replays on whatever stream the graph is launched on: the buffer of the eager warm-up call of this shape
        # (any stream) is the one to capture, and from then on it belongs to the graph
        hit = next((k for k in _CLUSTER_WS if k[:-1] == key), None)
        if hit is None:
            raise RuntimeError("dc_masks: call it once eagerly for this shape before capturing it in a hipGraph (workspace allocation)")
        _CLUSTER_PINNED.add(hit)
        return _CLUSTER_WS[hit]
    key = key + (stream,)
    ws = _CLUSTER_WS.pop(key, None)
    if ws is None:
        loose = [k for k in _CLUSTER_WS if k not in _CLUSTER_PINNED]
        while len(loose) >= 8:
            _CLUSTER_WS.pop(loose.pop(0))
        ws = torch.empty(nb, dtype=torch.uint8, device=device)
        ws[:head].zero_()                  # status word starts out zero
    _CLUSTER_WS[key] = ws
    return ws


def _dc_compact_route(B, H, D):
    """The compacted device-side clustering can end this forward: ``dc_cluster`` / ``dc_compact`` on, an embedding width the GEMM's
    register epilogue holds, and a head GEMM that reads the recurrence's x3 image."""
    from .nn._core import heads_take_image
    return options.get("dc_cluster") == "1" and options.get("dc_compact") == "1" and D <= 32 and heads_take_image(B, H, (D,))


def dc_masks_from_features(model, logmag, db_threshold=40.0, iters=20, frames=None, tol=1e-4):
    """Deep-clustering masks (B,T,F,2) straight from the mixture's log-magnitude WITHOUT materialising the embedding
    (round 4): the active bins are known before the network runs (evaluate.py:36-37), so the threshold is turned into a
    target map first (onssen_dc_index_f32), ``model``'s fc_dc GEMM stores only the active bins' normalised rows -- straight
    into the compacted array the clustering reads (onssen_linear_x3p_compact) -- and threshold / initialisation / Lloyd /
    masks run on that (onssen_dc_cluster_compact_f32).  Bit-identical masks to ``dc_masks(model([logmag])[0], logmag)``,
    minus the 10 320 B/frame embedding write, its re-read and the compaction pass.

    Returns None when this forward cannot take that route (not an eval-mode ``deep_clustering`` on the persistent split-bf16
    path, an embedding width the GEMM's register epilogue does not hold, a forced launch-per-step re-run): the caller then
    computes the embedding and calls ``dc_masks``."""
    from .hip import get_lib
    from .nn._core import _XcdPolicy, _XcdSerial, _XcdStatus, as_frames, precision, run_blstm, use_hip_path
    from .nn.deep_clustering import deep_clustering
    B, T, F = logmag.shape
    D = getattr(model, "embedding_dim", 0)
    if (not isinstance(model, deep_clustering) or not use_hip_path(model) or F != model.input_dim or precision() == "f32"
            or (frames is not None and precision() == "bf16") or _XcdPolicy.force_steps != 0
            or not _dc_compact_route(B, model.hidden_dim, D)):
        return None
    lib = get_lib()
    logmag = logmag.float().contiguous()
    if frames is not None:
        frames = as_frames(frames, B, T, logmag.device)
    nb, comp_off, dest_off = lib.dc_compact_layout(B, T, F, D)
    ws = _cluster_ws(logmag.device, (logmag.device, B, T, F, D, "compact"), nb, comp_off, frames is not None)
    st = torch.cuda.current_stream().cuda_stream
    fr = frames.data_ptr() if frames is not None else None
    # (round 5 measured "no": the map depends on the features only, so its three small launches were put on a side stream under
    #  the first layer's recurrence -- 1.888 / 1.879 ms against 1.875 / 1.882 ms per step in the captured graph, and the map's
    #  kernels, squeezed onto the 16 CUs the recurrence leaves, took 135 us instead of 10: profiles/NOTES.md)
    lib.dc_index(logmag.data_ptr(), B, T, F, D, float(db_threshold), ws.data_ptr(), nb, st, frames=fr)
    y = run_blstm(model._packed, model._ws, logmag, need_y=False, frames=frames)
    img = getattr(y, "x3_image", None)
    if img is None:                            # (the recurrence fell back between the check above and its own plan)
        return None
    wsb, off = img
    Hp = y.shape[3]
    hd = model._head.get(Hp)
    lib.linear_x3p_compact(wsb.data_ptr() + off, T * B, 2 * Hp, hd.img.data_ptr(), hd.b.data_ptr(), hd.N, D, 1e-12,
                           ws.data_ptr() + dest_off, T * F, F, ws.data_ptr() + comp_off, B, T * F * D, precision() == "bf16", st)
    masks = torch.empty(B, T, F, 2, device=logmag.device, dtype=torch.float32)
    _XcdSerial.before(logmag.device)            # the persistent Lloyd launch wants its workgroups resident together too
    lib.dc_cluster_compact(B, T, F, D, iters, masks.data_ptr(), ws.data_ptr(), nb, st, tol=float(tol))
    _XcdSerial.after(logmag.device)
    _XcdStatus.post_cluster(ws, int(lib.dll.onssen_dc_cluster_status_offset(B, D)))
    return masks


def dc_masks(emb, logmag, db_threshold=40.0, iters=20, frames=None, tol=1e-4, num_speaker=2):
    """Binary deep-clustering masks (B,T,F,2) on the device: threshold at max - db/20, 2-means on the active
    bins' embeddings (counterpart of evaluate.py:36-41, where it is sklearn on the host).

    ``num_speaker`` = 3 or 4: K-means for that many speakers (evaluate.py:33-44 takes the count from ``sig_ref``) and masks
    (B,T,F,K), channel k = the cluster grown from the k-th centroid of a deterministic farthest-point initialisation
    (``onssen_dc_cluster_k_f32``).  That route has the launch-per-iteration form only -- no persistent
    launch, no waits, nothing to recover -- and takes ``frames`` like the two-speaker one.  Anything but 2, 3, 4: ValueError.

    Default: the active bins are compacted once and all Lloyd iterations run in ONE persistent launch (8 workgroups per
    utterance meeting at a counter); its waits are bounded, and a wait that gave up is reported like an aborted recurrence
    (``_XcdStatus``: the owning call is re-run with the launch-per-iteration form, which is also what runs inside
    ``_XcdPolicy.forced_steps()`` and with ONSSEN_DC_PERSISTENT=0).  ``iters`` / ``tol``: at most that many Lloyd iterations,
    stopped earlier at the exact fixed point or by sklearn's rule (``KMeans(tol=1e-4)``, upstream's default: summed squared
    centroid shift <= tol x mean per-feature variance); ``tol=0`` iterates to the fixed point.

    ``frames`` (B,): a ragged batch -- utterance b owns its first frames[b] frames; its padding is never active, takes no
    part in the threshold or the sums, and gets zero masks.  Such calls (a new longest utterance per batch) share ONE
    grow-only workspace per device, allocated uninitialised with only its header zeroed."""
    from . import _abi
    from .features import _lengths_i32
    from .hip import get_lib
    from .nn._core import _XcdPolicy, _XcdSerial, _XcdStatus
    K = int(num_speaker)
    if K not in (2, 3, 4):
        raise ValueError(f"dc_masks: num_speaker must be 2, 3 or 4, got {num_speaker}")
    lib = get_lib()
    B, T, F, D = emb.shape
    emb, logmag = emb.contiguous(), logmag.contiguous()
    if frames is not None:
        frames = _lengths_i32(frames, B, T, emb.device, "frames")
    if K > 2:
        nb = int(lib.dll.onssen_dc_cluster_k_workspace_bytes(B, T, F, D, K))
        if nb == 0:
            raise ValueError(f"dc_masks: unsupported shape for num_speaker = {K}: embedding {tuple(emb.shape)} (embedding_dim <= 32)")
        ws = _cluster_ws(emb.device, (emb.device, B, T, F, D, "k", K), nb, 0, frames is not None)      # (rewritten by every call)
        masks = torch.empty(B, T, F, K, device=emb.device, dtype=torch.float32)
        lib.dc_cluster_k(emb.data_ptr(), logmag.data_ptr(), B, T, F, D, K, float(db_threshold), iters, masks.data_ptr(),
                         ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream,
                         frames=frames.data_ptr() if frames is not None else None, tol=float(tol))
        return masks
    nb = int(lib.dll.onssen_dc_cluster_workspace_bytes(B, T, F, D))
    head = lib.dc_compact_layout(B, T, F, D)[1]        # the library's own offset of the compacted array = the header's size
    ws = _cluster_ws(emb.device, (emb.device, B, T, F, D), nb, head, frames is not None)
    persistent = options.get("dc_cluster") == "1" and _XcdPolicy.force_steps == 0
    masks = torch.empty(B, T, F, 2, device=emb.device, dtype=torch.float32)
    if persistent:
        _XcdSerial.before(emb.device)
    lib.dc_cluster(emb.data_ptr(), logmag.data_ptr(), B, T, F, D, float(db_threshold), iters, masks.data_ptr(),
                   ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream,
                   flags=0 if persistent else _abi.DC_CLUSTER_LAUNCH_PER_ITERATION,
                   frames=frames.data_ptr() if frames is not None else None, tol=float(tol))
    if persistent:
        _XcdSerial.after(emb.device)
        _XcdStatus.post_cluster(ws, int(lib.dll.onssen_dc_cluster_status_offset(B, D)))
    return masks


def _host_label_masks(label, K, device):
    """sklearn labels of the active bins -> their mask rows (n, K): (label, 1 - label) for two speakers, as ever; one-hot
    (``mask[i, embedding_labels == i] = 1``, evaluate.py:39-41) for more."""
    lab = torch.from_numpy(label.astype(np.int64)).to(device)
    if K == 2:
        return torch.stack([lab.float(), 1.0 - lab.float()], -1)
    return torch.nn.functional.one_hot(lab, K).float()


@recovering
@torch.no_grad()
def separate_dc(model, wav, window_size=256, hop_size=64, db_threshold=40.0, host_kmeans=False, lengths=None, num_speaker=2):
    """Deep-clustering separation, waveform in -> (B, 2, n) waveforms out, entirely on the GPU
    (STFT -> network -> threshold + 2-means -> binary masks -> mask-apply + iSTFT).  ``host_kmeans=True``
    clusters with sklearn KMeans(n_clusters=num_speaker, random_state=0) on the host exactly as upstream does
    (egs/wsj0-2mix/deep_clustering/evaluate.py:36-38); the two differ only in the arbitrary cluster
    numbering and in bins that sit between the clusters.

    ``num_speaker`` = 3 or 4 -> (B, num_speaker, n): the same network, K-means for that many speakers on its embedding
    (``dc_masks(num_speaker=)``; the route that skips the embedding is two-speaker, so the embedding is materialised).

    ``lengths`` (B,): a RAGGED batch of whole utterances -- row b holds lengths[b] valid samples of the n it is padded to
    (the reference separates them one at a time, onssen/utils/test.py:29-41; together they fill the chip).  Every row's
    result inside its own length is bit for bit what the batch-1 call on wav[b:b+1, :lengths[b]] returns; zeros after it."""
    K = int(num_speaker)
    if K not in (2, 3, 4):
        raise ValueError(f"separate_dc: num_speaker must be 2, 3 or 4, got {num_speaker}")
    lengths, frames = _ragged(wav, lengths, hop_size)
    logmag, ri = stft_logmag(wav, window_size, hop_size, lengths=lengths)
    if not host_kmeans:
        masks = dc_masks_from_features(model, logmag, db_threshold, frames=frames) if K == 2 else None   # the embedding never leaves the GEMM ...
        if masks is None:                                                                 # ... unless this forward cannot do that
            emb, = model([logmag]) if frames is None else model([logmag], frames=frames)
            masks = dc_masks(emb, logmag, db_threshold, frames=frames, num_speaker=K)
        out = mask_istft(ri, masks, hop_size, wav.shape[-1], frames=frames, lengths=lengths)
        _XcdStatus.flush()        # an aborted recurrence is reported by THIS call, not by the next one
        return out
    if frames is not None:
        raise ValueError("separate_dc: host_kmeans=True takes uniform batches only")
    emb, = model([logmag])
    _XcdStatus.flush()
    from sklearn.cluster import KMeans
    B, T, F, D = emb.shape
    masks = torch.zeros(B, T, F, K, device=wav.device, dtype=torch.float32)
    for b in range(B):   # upstream evaluates with batch 1 (evaluate.py:34-35)
        feat = logmag[b]
        act = feat >= (feat.max() - db_threshold / 20.0)
        label = KMeans(n_clusters=K, random_state=0, n_init=10).fit_predict(emb[b][act].cpu().numpy())
        masks[b][act] = _host_label_masks(label, K, wav.device)
    return mask_istft(ri, masks, hop_size, wav.shape[-1])


def _dc_pipe_why_not(model, B, window_size, rows):
    """None if this model / batch size / mode can run on a pipeline of at most ``rows`` rows (32 uniform, 16 ragged), else what
    is missing (no allocation, no launch)."""
    from .nn._core import _XcdPolicy, precision
    from .nn.deep_clustering import deep_clustering
    if not isinstance(model, deep_clustering) or model.num_layers != 2:
        return "a deep_clustering model with num_layers = 2"
    if model.training or next(model.parameters()).device.type != "cuda":
        return "an eval-mode model on a ROCm device"
    if window_size // 2 + 1 != model.input_dim:
        return f"window_size // 2 + 1 == input_dim ({model.input_dim})"
    if not 1 <= B <= rows or model.hidden_dim > 640:
        return f"1 <= B <= {rows}{' (ragged rows run on stacked tiles)' if rows < 32 else ''} and hidden_dim <= 640"
    if precision() != "bf16x3" or options.get("recurrence") != "1" or not _XcdPolicy.persistent_allowed():
        return "the default split-bf16 arithmetic on the persistent recurrence"
    if not _dc_compact_route(B, model.hidden_dim, model.embedding_dim):
        return "the compacted device-side clustering (embedding_dim in 4, 8, 16, 20; dc_cluster / dc_compact on)"
    return None


class _DCPipeCore:
    """What ``DCPipeline`` and ``DCRaggedPipeline`` share: the geometry, the two clustering workspaces (one per parity, headers
    zeroed once) and the pair-launch workspace, the status posts, the drain's bookkeeping, and the back end of a step."""

    def __init__(self, model, B, T, window_size, hop_size, db_threshold, iters, tol):
        """``T``: the frames the workspaces are sized for."""
        from . import _abi
        from .hip import get_lib
        self.model, self.lib, self.dev = model, get_lib(), next(model.parameters()).device
        self.B, self.nfft, self.hop = int(B), int(window_size), int(hop_size)
        self.F, self.D = window_size // 2 + 1, model.embedding_dim
        self.db, self.iters, self.tol = float(db_threshold), int(iters), float(tol)
        self.H, self.ug = model.hidden_dim, 4 * -(-model.hidden_dim // 128)
        self.flags = _abi.BLSTM_BF16X3 | _abi.BLSTM_XCD
        lib, F, D = self.lib, self.F, self.D
        self.cnb, self.comp_off, self.dest_off = lib.dc_compact_layout(B, T, F, D)
        self.cws = []
        for _ in range(2):
            w = torch.empty(self.cnb, dtype=torch.uint8, device=self.dev)
            w[:self.comp_off].zero_()
            self.cws.append(w)
        self.cstat = int(lib.dll.onssen_dc_cluster_status_offset(B, D))
        self.wnb = lib.blstm_pipe2_workspace_bytes(B, T, F, self.H, self.ug)
        self.ws = torch.zeros(self.wnb, dtype=torch.uint8, device=self.dev)     # zeroed ONCE (ABI)
        self.img_off, _ = lib.blstm_pipe2_y_image(B, T, F, self.H, self.ug)
        self.count = 0               # batches pushed since the last reset

    def _back_end(self, pk, q, T, comp_off, dest_off, ri, strides, n, out, st, frames=None, lengths=None):
        """Head GEMM (active bins only, straight into the compacted array of parity ``q``), 2-means, masks and iSTFT of the batch
        whose layer-1 output the pair launch has just left in ``ws``: T frames, spectrum ``ri``, ``n`` samples into ``out``."""
        lib, B, F, D = self.lib, self.B, self.F, self.D
        hd = self.model._head.get(pk.Hp)
        cw = self.cws[q]
        lib.linear_x3p_compact(self.ws.data_ptr() + self.img_off, T * B, 2 * pk.Hp, hd.img.data_ptr(), hd.b.data_ptr(), hd.N, D, 1e-12,
                               cw.data_ptr() + dest_off, T * F, F, cw.data_ptr() + comp_off, B, T * F * D, False, st)
        lib.dc_cluster_compact(B, T, F, D, self.iters, self.masks.data_ptr(), cw.data_ptr(), self.cnb, st, tol=self.tol)
        lib.mask_istft(ri.data_ptr(), self.masks.data_ptr(), *strides, B, 2, T, self.nfft, self.hop, n, out.data_ptr(), st,
                       frames=frames, lengths=lengths)

    def _post(self, parities):
        """Status words to examine: the pair launch's, and the clustering's of the parities whose back end ran."""
        from .nn._core import _XcdStatus
        _XcdStatus.post(self.ws)
        for q in parities:
            _XcdStatus.post_cluster(self.cws[q], self.cstat)

    @torch.no_grad()
    def flush(self):
        """Drain: the separated LAST batch (or None if nothing is in flight); the pipeline is empty afterwards."""
        from .nn._core import _XcdStatus
        if self.count == 0:
            return None
        out = self._drain(self.count & 1)
        self.count = 0
        _XcdStatus.flush()
        return out

    def reset(self):
        """Forget the batch in flight (after an aborted step: the exchange header was zeroed by the status poll)."""
        self.count = 0


class DCPipeline(_DCPipeCore):
    """Deep-clustering separation of a STREAM of equally shaped batches, software-pipelined over consecutive batches (round 6;
    the evaluation loop of onssen/utils/test.py:29-41 / egs/wsj0-2mix/deep_clustering/evaluate.py:31-45 hands over one batch after
    the other).  A two-layer BLSTM of <= 32 rows fills the chip's 8 XCDs only with 8-row recurrence groups, whose time step costs
    nearly what a 16-row group's does -- so ``push(batch n)`` runs, in ONE persistent launch, layer 1 of batch n-1 on half of the
    XCDs and layer 0 of batch n on the other half (``onssen_blstm_pipe2_forward_f32``), with the rest of both batches' work around it:

        STFT, input projection of batch n -> [ layer 1 (n-1) || layer 0 (n) || target map (n) ] -> layer 1's projection of batch n;
        fc_dc (active bins only) + 2-means + masks + iSTFT of batch n-1

    (the target map of batch n is first read by batch n's fc_dc, one step later: the persistent launch builds it in workgroups of
    its own on the CUs its members leave free, ``onssen_blstm_pipe2_map_forward_f32``; ``aux_map=False`` builds it in front of the
    launch with ``onssen_dc_index_f32`` instead -- the same bytes, three launches more on the critical path)

    and returns the separated batch n-1 -- (B, 2, n_samples), valid until the next-but-one ``push`` -- or None for the first
    batch; ``flush()`` drains the last one.  Every batch gets exactly the arithmetic ``separate_dc`` gives it on 16-row recurrence
    groups without the fused first layer (bit for bit what the same rows get inside a 64-row ``separate_dc`` call; last-bit
    differences against the default 32-row call, inside the same tolerance); the price is one batch of latency.  Both parities of
    the step are captured as hipGraphs (``graph=True``).

    Needs an eval-mode ``deep_clustering`` with num_layers = 2, hidden <= 640, B <= 32 in the default split-bf16 arithmetic on the
    persistent recurrence; anything else raises (use ``separate_dc``).  A launch that gave up a bounded wait is reported by the
    next ``push`` / ``flush`` (XcdAborted; ``separate_dc_stream`` re-runs the affected batches with ``separate_dc``).
    Two speakers only (the compacted clustering it ends in is the 2-means): ``separate_dc(num_speaker=)`` separates three or four."""

    def __init__(self, model, B, n_samples, window_size=256, hop_size=64, db_threshold=40.0, iters=20, tol=1e-4, graph=True, aux_map=True):
        from .nn._core import _version_key
        why = _dc_pipe_why_not(model, B, window_size, 32)
        if why:
            raise RuntimeError(f"DCPipeline needs {why}; use separate_dc")
        self.n = int(n_samples)
        self.T = T = 1 + self.n // int(hop_size)
        super().__init__(model, B, T, window_size, hop_size, db_threshold, iters, tol)
        dev, F = self.dev, self.F
        mk = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        self.wav = [torch.zeros(B, self.n, device=dev) for _ in range(2)]
        self.logmag = [mk(B, T, F) for _ in range(2)]
        self.ri = [mk(B, T, F, 2) for _ in range(2)]
        self.out = [torch.zeros(B, 2, self.n, device=dev) for _ in range(2)]
        self.masks = mk(B, T, F, 2)
        self.graphs = [None, None]
        self.use_graph = bool(graph)
        self.aux_map = bool(aux_map)
        self._wkey = None
        self._version_key = _version_key
        self._prime()

    # -- one pipeline step on the current stream: buffers of parity p take batch n, those of 1 - p hold batch n - 1
    def _enqueue(self, p, back_end=True):
        lib, B, T, F = self.lib, self.B, self.T, self.F
        st = torch.cuda.current_stream().cuda_stream
        pk = self.model._packed.get(self.ug)
        lib.stft_logmag(self.wav[p].data_ptr(), B, self.n, self.n, self.nfft, self.hop, 1e-7, self.logmag[p].data_ptr(),
                        self.ri[p].data_ptr(), st)
        weights = [t.data_ptr() for t in pk.wih_img], [t.data_ptr() for t in pk.whh_x3], [t.data_ptr() for t in pk.bias]
        if self.aux_map:
            lib.blstm_pipe2_map_forward(self.logmag[p].data_ptr(), T * F, F, B, T, F, self.H, self.ug, *weights, self.ws.data_ptr(), self.wnb,
                                        self.flags, self.db, self.D, self.cws[p].data_ptr(), self.cnb, st)
        else:
            lib.dc_index(self.logmag[p].data_ptr(), B, T, F, self.D, self.db, self.cws[p].data_ptr(), self.cnb, st)
            lib.blstm_pipe2_forward(self.logmag[p].data_ptr(), T * F, F, B, T, F, self.H, self.ug, *weights, self.ws.data_ptr(), self.wnb,
                                    self.flags, st)
        if back_end:
            m = self.masks
            self._back_end(pk, 1 - p, T, self.comp_off, self.dest_off, self.ri[1 - p], (m.stride(0), m.stride(3), m.stride(1), m.stride(2)),
                           self.n, self.out[p], st)

    def _prime(self):
        """Two eager steps on silence: every kernel has run once, both target maps and the layer-1 projection hold finite data."""
        from .nn._core import _XcdStatus
        _XcdStatus.poll()
        for p in (0, 1):
            self._enqueue(p, back_end=p == 1)
        self._post((0, 1))
        self.count = 0

    def _capture(self):
        key = self._version_key(self.model.rnn.flat_weights() + [self.model.fc_dc.weight, self.model.bn.running_mean])
        if self._wkey == key and self.graphs[0] is not None:
            return
        pk = self.model._packed.get(self.ug)         # (re)pack eagerly: inside the capture these only mark the images as captured
        self.model._head.get(pk.Hp)
        torch.cuda.synchronize(self.dev)
        self.graphs = [None, None]
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        for p in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                self._enqueue(p)
            self.graphs[p] = g
        torch.cuda.current_stream(self.dev).wait_stream(s)
        self._wkey = key

    def step(self, p):
        if self.use_graph:
            self.graphs[p].replay()
        else:
            self._enqueue(p)

    def replay(self):
        """One steady-state step on the input buffers as they are (``self.wav[parity]``: bench.py fills them once and times this):
        no copy, no status traffic.  At least one batch must be in flight (the parities alternate from there)."""
        if self.count == 0:
            raise RuntimeError("DCPipeline.replay: push a batch first")
        if self.use_graph:
            self._capture()
        self.step(self.count & 1)
        self.count += 1

    @torch.no_grad()
    def push(self, wav, check=True):
        """Hand over batch n (B, n_samples) float32 on the device; returns the separated batch n-1 (B, 2, n_samples) or None."""
        from .nn._core import _XcdStatus
        if tuple(wav.shape) != (self.B, self.n) or not wav.is_cuda:
            raise ValueError(f"DCPipeline.push: expected a ({self.B}, {self.n}) tensor on {self.dev}, got {tuple(wav.shape)} on {wav.device}")
        if check:
            _XcdStatus.poll()                      # reports of earlier steps that have landed (raises XcdAborted)
        if self.use_graph:
            self._capture()
        p = self.count & 1
        self.wav[p].copy_(wav, non_blocking=True)
        if self.count == 0:
            # the first batch of a stream has nothing behind it: no back end (the other parity's clustering workspace holds a map that
            # was consumed by the drain, or none) -- an eager step, the captured graphs are the steady state
            self._enqueue(p, back_end=False)
        else:
            self.step(p)
        if check:
            self._post((0, 1))
        self.count += 1
        return self.out[p] if self.count > 1 else None

    def _drain(self, p):
        self.wav[p].zero_()
        if self.use_graph:
            self._capture()
        self.step(p)
        self._post((0, 1))
        return self.out[p]


class DCRaggedPipeline(_DCPipeCore):
    """``DCPipeline`` for a stream of RAGGED batches of whole utterances (round 6c) -- the shape the reference evaluates one by one
    (onssen/utils/test.py:29-41) and ``separate_dc(..., lengths=)`` runs K at a time: every batch is B <= 16 rows padded to ITS OWN
    longest utterance.  A ragged batch of <= 16 rows runs on stacked 4-row recurrence groups, whose time step costs what an 8-row
    group's does, one layer after the other; here ``push(batch n)`` runs layer 1 of batch n-1 and layer 0 of batch n in ONE persistent
    launch on stacked 8-row groups (``onssen_blstm_pipe2_forward_ragged_f32``: each half of the launch has its own number of time steps
    and its own row lengths), with the rest of both batches' work around it exactly as in ``DCPipeline``, and returns the separated batch
    n-1 -- (B, 2, n_{n-1}), valid until the next-but-one ``push`` -- or None for the first batch; ``flush()`` drains the last one.

    Every utterance's result inside its own length is bit for bit what ``separate_dc(model, wav, lengths=lengths)`` gives it (stacked
    tiles in both: a tile column never sees its neighbours), i.e. what the batch-1 call on that utterance returns; zeros after it.
    Eager launches (a new longest utterance per batch: nothing to capture); buffers are sized once for ``n_cap`` samples per row.
    Needs what ``DCPipeline`` needs, with B <= 16; two speakers only, like it (``tester_dc.eval`` sends a forward whose references
    hold another number of sources through its plain loop)."""

    @staticmethod
    def why_not(model, B, window_size=256):
        """None if this model / batch size / mode can run here, else what is missing (no allocation, no launch)."""
        return _dc_pipe_why_not(model, B, window_size, 16)

    def __init__(self, model, B, n_cap, window_size=256, hop_size=64, db_threshold=40.0, iters=20, tol=1e-4):
        why = self.why_not(model, B, window_size)
        if why is None and n_cap < hop_size:
            why = "n_cap >= hop_size"
        if why:
            raise RuntimeError(f"DCRaggedPipeline needs {why}; use separate_dc(..., lengths=)")
        self.n_cap = int(n_cap)
        self.T_cap = T = 1 + self.n_cap // int(hop_size)
        super().__init__(model, B, T, window_size, hop_size, db_threshold, iters, tol)
        dev, F = self.dev, self.F
        mk = lambda k: torch.empty(k, device=dev, dtype=torch.float32)
        self.logmag = [torch.zeros(B * T * F, device=dev) for _ in range(2)]
        self.ri = [mk(B * T * F * 2) for _ in range(2)]
        self.out = [mk(B * 2 * self.n_cap) for _ in range(2)]
        self.masks = mk(B * T * F * 2)
        self.meta = [None, None]     # per parity: (T, n, frames, lengths, logmag, ri) of the batch its buffers hold

    def _step(self, p, cur, back_end):
        """The pair launch for the batch ``cur`` = (T, n, frames, lengths, logmag, ri) beside the batch of parity 1 - p, then
        (``back_end``) that batch's head GEMM, clustering, masks and iSTFT into ``out[p]``; the status posts."""
        lib, B, F = self.lib, self.B, self.F
        st = torch.cuda.current_stream().cuda_stream
        pk = self.model._packed.get(self.ug)
        q = 1 - p
        T, n, frames, lengths, x, _ = cur
        Tq, nq, frames_q, lengths_q, _, ri_q = self.meta[q] if back_end else cur
        lib.blstm_pipe2_forward_ragged(x.data_ptr(), T * F, F, B, self.T_cap, T, frames.data_ptr(), Tq, frames_q.data_ptr(), F, self.H,
                                       self.ug, [t.data_ptr() for t in pk.wih_img], [t.data_ptr() for t in pk.whh_x3],
                                       [t.data_ptr() for t in pk.bias], self.ws.data_ptr(), self.wnb, self.flags, st)
        if not back_end:
            return None
        _, comp_off, dest_off = lib.dc_compact_layout(B, Tq, F, self.D)
        self._back_end(pk, q, Tq, comp_off, dest_off, ri_q, (Tq * F * 2, 1, F * 2, 2), nq, self.out[p], st,
                       frames_q.data_ptr(), lengths_q.data_ptr())
        return self.out[p][:B * 2 * nq].view(B, 2, nq)

    def _advance(self, cur, check):
        """Target map of ``cur`` (the features are in place), the pipeline step, the status posts."""
        T, n, frames, lengths, x, _ = cur
        p = self.count & 1
        self.lib.dc_index(x.data_ptr(), self.B, T, self.F, self.D, self.db, self.cws[p].data_ptr(), self.cnb,
                          torch.cuda.current_stream().cuda_stream, frames=frames.data_ptr())
        back_end = self.count > 0
        out = self._step(p, cur, back_end)
        self.meta[p] = cur
        if check:
            self._post((1 - p,) if back_end else ())
        self.count += 1
        return out

    @torch.no_grad()
    def push(self, wav, lengths, check=True):
        """Hand over batch n: ``wav`` (B, n) float32 on the device, row b holding ``lengths[b]`` <= n valid samples (n <= n_cap);
        returns the separated batch n-1 (B, 2, n_{n-1}) or None."""
        from .features import _lengths_i32
        from .nn._core import _XcdStatus
        if wav.dim() != 2 or wav.shape[0] != self.B or not wav.is_cuda or not self.hop <= wav.shape[1] <= self.n_cap:
            raise ValueError(f"DCRaggedPipeline.push: expected a ({self.B}, n <= {self.n_cap}) tensor on {self.dev}, got "
                             f"{tuple(wav.shape)} on {wav.device}")
        wav = wav.float()
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        B, n = wav.shape
        lengths = _lengths_i32(lengths, B, n, self.dev, "lengths", lo=max(self.hop, self.nfft // 2 + 1))
        frames = (1 + lengths // self.hop).to(torch.int32)
        if check:
            _XcdStatus.poll()                      # reports of earlier steps that have landed (raises XcdAborted)
        p = self.count & 1
        T = 1 + n // self.hop
        self.lib.stft_logmag(wav.data_ptr(), B, n, wav.stride(0), self.nfft, self.hop, 1e-7, self.logmag[p].data_ptr(),
                             self.ri[p].data_ptr(), torch.cuda.current_stream().cuda_stream, n_per_utt=lengths.data_ptr())
        return self._advance((T, n, frames, lengths, self.logmag[p], self.ri[p]), check)

    @torch.no_grad()
    def push_features(self, logmag, stft_ri, frames, lengths, n, check=True):
        """``push`` for a batch whose features come from elsewhere (the evaluation loader's items, onssen/data/wsj0_2mix.py:231-245,
        collated by ``evaluate.tester.collate``): ``logmag`` (B, T, F) and ``stft_ri`` (B, T, F, 2) float32 on the device, row b owning
        its first ``frames[b]`` <= T frames and ``lengths[b]`` <= n output samples.  The tensors are used where they are (no copy) and
        kept until their batch has left the pipeline."""
        from .features import _lengths_i32
        from .nn._core import _XcdStatus
        B, T, F = logmag.shape
        if (B != self.B or F != self.F or T > self.T_cap or n > self.n_cap or tuple(stft_ri.shape) != (B, T, F, 2) or not logmag.is_cuda
                or not stft_ri.is_cuda):
            raise ValueError(f"DCRaggedPipeline.push_features: expected ({self.B}, T <= {self.T_cap}, {self.F}) features and their "
                             f"(..., 2) spectrum on {self.dev}, n <= {self.n_cap}; got {tuple(logmag.shape)}, {tuple(stft_ri.shape)}, n = {n}")
        logmag, stft_ri = logmag.float().contiguous(), stft_ri.float().contiguous()
        frames = _lengths_i32(frames, B, T, self.dev, "frames")
        lengths = _lengths_i32(lengths, B, n, self.dev, "lengths")
        if check:
            _XcdStatus.poll()
        return self._advance((T, int(n), frames, lengths, logmag, stft_ri), check)

    def _drain(self, p):
        # the launch's other half needs SOME batch: the last one's own features again (its layer-0 output is not used)
        out = self._step(p, self.meta[1 - p], True)
        self._post((1 - p,))
        return out


def dc_stream(items, fit, push, release, rerun, fallback, how):
    """The loop behind ``separate_dc_stream``, ``separate_dc_ragged_stream`` and ``tester_dc.eval``: generator of one result per item
    of ``items``, in order, through a pipeline that returns item k-1's estimate when item k is pushed.  At most two items are held
    (pushed, result not released yet); the order per item is push -> compute the result -> ``_XcdStatus.flush()`` -> release, so a
    result whose step gave up a bounded wait (``XcdAborted``, from the push, the flush or that status check) is never released:
    the recovery counts ``_XcdPolicy.recovered``, warns, resets the pipeline and re-runs everything held.  What differs per caller:

      fit(item, pipe)     the pipeline that takes ``item``: ``pipe`` itself, another one (the held items are drained through
                          ``pipe.flush()`` first), or None -- the item then goes through ``fallback(item)`` after the same drain
      push(pipe, item)    hand the item over; the previous item's estimate, or None
      release(est, item)  what the estimate ``est`` of ``item`` becomes (a clone; its SI-SDR sum): computed before the status check
      rerun(held, e)      the results (a list) of the held items after the abort ``e``, without the pipeline
      how                 the end of the warning: how ``rerun`` does it."""
    import warnings
    from .nn._core import XcdAborted, _XcdPolicy, _XcdStatus
    pipe, held = None, []

    def recover(e):
        nonlocal held
        _XcdPolicy.recovered += 1
        warnings.warn(f"onssen_amd: {e}  Re-running {len(held)} batch(es) of that pipeline step {how}.", RuntimeWarning)
        pipe.reset()
        todo, held = held, []
        return rerun(todo, e)

    def drain():
        nonlocal held
        if not held:
            return []
        try:
            res = release(pipe.flush(), held[0])       # (flush() examines the status itself)
            held = []
            return [res]
        except XcdAborted as e:
            return recover(e)

    for item in items:
        fitted = fit(item, pipe)
        if fitted is not pipe:
            yield from drain()
            pipe = fitted
        if pipe is None:
            yield fallback(item)
            continue
        held.append(item)
        try:
            est = push(pipe, item)
            if est is None:
                continue
            res = release(est, held[0])
            _XcdStatus.flush()                 # the step that produced it has completed cleanly (the next one is not enqueued yet)
            held.pop(0)
        except XcdAborted as e:
            yield from recover(e)
            continue
        yield res
    yield from drain()


@torch.no_grad()
def separate_dc_ragged_stream(model, batches, window_size=256, hop_size=64, db_threshold=40.0):
    """Generator: ``separate_dc(model, wav, lengths=lengths)`` over an iterable of ragged batches ``(wav (B, n), lengths (B,))`` --
    B <= 16 whole utterances each, every batch padded to its own longest one -- through ``DCRaggedPipeline``: yields one (B, 2, n)
    result per batch, in order (a fresh tensor each), bit for bit what ``separate_dc`` returns for it.  The pipeline's buffers are
    sized for the longest batch seen so far (a longer one drains it and starts a larger one); a batch it cannot take (another B,
    more than 16 rows, a model or mode ``DCRaggedPipeline`` refuses) goes through ``separate_dc``; a step whose persistent launch
    gave up a bounded wait is recovered by separating the batches it touched again with ``separate_dc`` (``dc_stream``)."""
    sep = lambda item: separate_dc(model, item[0], window_size, hop_size, db_threshold, lengths=item[1])

    def fit(item, pipe):
        B, n = item[0].shape
        if pipe is not None and B == pipe.B and n <= pipe.n_cap:
            return pipe
        try:
            return DCRaggedPipeline(model, B, int(n * 1.25) if B <= 16 else n, window_size, hop_size, db_threshold)
        except RuntimeError:
            return None

    yield from dc_stream(batches, fit, lambda pipe, item: pipe.push(*item), lambda est, item: est.clone(),
                         lambda held, e: [sep(item) for item in held], sep, "with separate_dc")


@torch.no_grad()
def separate_dc_stream(model, batches, window_size=256, hop_size=64, db_threshold=40.0, graph=True):
    """Generator: ``separate_dc`` over an iterable of equally shaped (B, n) device batches, through ``DCPipeline`` -- yields one
    (B, 2, n) result per batch, in order (a fresh tensor each).  A step whose persistent launch gave up a bounded wait is
    recovered (``dc_stream``): the batches it touched are separated again with ``separate_dc`` and the pipeline restarts.  Batches
    the pipeline cannot take (see DCPipeline; another shape than the first batch's) go through ``separate_dc`` one by one, after
    the batch in flight has been drained."""
    sep = lambda wav: separate_dc(model, wav, window_size, hop_size, db_threshold)
    made = []                                  # the ONE pipeline of this stream, sized for the first batch; False: refused

    def fit(wav, pipe):
        if not made:
            try:
                made.append(DCPipeline(model, wav.shape[0], wav.shape[1], window_size, hop_size, db_threshold, graph=graph))
            except RuntimeError:
                made.append(False)
        return made[0] if made[0] and tuple(wav.shape) == (made[0].B, made[0].n) else None

    yield from dc_stream(batches, fit, lambda pipe, wav: pipe.push(wav), lambda est, wav: est.clone(),
                         lambda held, e: [sep(wav) for wav in held], sep, "with separate_dc")
