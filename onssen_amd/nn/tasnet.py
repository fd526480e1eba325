import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _abi, options
from ._core import (PackedWeightsMixin, _Workspaces, _park_if_captured, _stream, _version_key, needs_graph, precision,
                    require_device, use_hip_path)
from ..hip import get_lib

_NORMS = {"gln": _abi.TASNET_GLN, "cln": _abi.TASNET_CLN, "bn": _abi.TASNET_BN}
_ACTS = {"relu": _abi.TASNET_RELU, "sigmoid": _abi.TASNET_SIGMOID, "softmax": _abi.TASNET_SOFTMAX}
_PRECS = {"f32": _abi.TASNET_F32, "bf16x3": _abi.TASNET_BF16X3, "bf16": _abi.TASNET_BF16}


class GlobalLayerNorm(nn.Module):
    """gLN of the reference (onssen/nn/tasnet.py:5-44): per-utterance mean and biased variance over all (channel, frame)
    pairs, eps inside the square root, weight and bias shaped (C, 1)."""

    def __init__(self, dim, eps=1e-05):
        super().__init__()
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim, 1))
        self.bias = nn.Parameter(torch.zeros(dim, 1))

    def forward(self, x):                      # x: n x C x T
        if x.dim() != 3:
            raise RuntimeError("GlobalLayerNorm accepts 3D tensors")
        mean = torch.mean(x, (1, 2), keepdim=True)
        var = torch.mean((x - mean) ** 2, (1, 2), keepdim=True)
        return self.weight * (x - mean) / torch.sqrt(var + self.eps) + self.bias


class CumulativeLayerNorm(nn.LayerNorm):
    """cLN of the reference (tasnet.py:47-67): LayerNorm over the channels of each frame."""

    def forward(self, x):                      # x: n x C x T
        return super().forward(x.transpose(1, 2)).transpose(1, 2)


def _select_norm(norm, dim):
    if norm == "gln":
        return GlobalLayerNorm(dim)
    if norm == "cln":
        return CumulativeLayerNorm(dim)
    return nn.BatchNorm1d(dim)


class Conv1DBlock(nn.Module):
    """One separation block (tasnet.py:126-163).  PReLU_2 and norm_2 are parameters of the reference's block that its forward
    never uses: they are kept so that checkpoints load, and stay out of the computation."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation, norm, causal):
        super().__init__()
        self.conv1x1 = nn.Conv1d(in_channels, out_channels, 1)
        self.PReLU_1 = nn.PReLU()
        self.norm_1 = _select_norm(norm, out_channels)
        self.pad = dilation * (kernel_size - 1) if causal else dilation * (kernel_size - 1) // 2
        self.dwconv = nn.Conv1d(out_channels, out_channels, kernel_size, groups=out_channels, padding=self.pad, dilation=dilation)
        self.PReLU_2 = nn.PReLU()
        self.norm_2 = _select_norm(norm, out_channels)
        self.Sc_conv = nn.Conv1d(out_channels, in_channels, 1, bias=True)
        self.causal = causal

    def forward(self, x):
        c = self.norm_1(self.PReLU_1(self.conv1x1(x)))
        c = self.dwconv(c)
        if self.causal:
            c = c[:, :, :-self.pad]
        return x + self.Sc_conv(c)


class _SavedSlot:
    """One buffer of saved activations of the HIP training forward.  ``owner`` is the generation number of the forward whose
    graph still needs it (0: free); ``gen`` counts the forwards that wrote it."""

    def __init__(self, buf):
        self.buf, self.owner, self.gen = buf, 0, 0


class _Lease:
    """Held by the autograd node of one training forward: gives the slot back after that node's backward, or when the graph is
    dropped without one (a training forward under no_grad, a loss that is never differentiated)."""

    def __init__(self, slot):
        slot.gen += 1
        slot.owner = self.gen = slot.gen
        self.slot = slot

    def release(self):
        if self.slot.owner == self.gen:
            self.slot.owner = 0

    def valid(self):
        return self.slot.gen == self.gen

    __del__ = release


class _TasNetTrainFunction(torch.autograd.Function):
    """The network of ConvTasNet as ONE autograd node on HIP kernels (csrc/tasnet_bwd.inc): forward(model, x, *parameters in
    the order of model._packed_params()) -> (num_spks, n, S_out); backward -> the parameters' gradients as views of ONE flat
    buffer, allocated per call (autograd may keep the views as ``p.grad``, and a second backward before ``zero_grad()`` has to
    add to them).  No gradient with respect to x.

    Saved activations live in buffers the model caches per shape.  A forward takes a free one and its graph owns it until its
    backward has run or the graph is dropped; a second forward while the first graph is alive gets a buffer of its own (two graphs
    alive = two buffers, both kept for reuse).  Backward through a retained graph (``retain_graph=True``) works as long as no
    later forward has taken the buffer over; after that it raises instead of differentiating somebody else's activations."""

    @staticmethod
    def forward(ctx, model, x, *params):
        lib, cfg, image, x, x_stride = model._hip_inputs(x)
        n, S = x.shape
        hop = model.L // 2
        S_out = ((S - model.L) // hop) * hop + model.L
        dev = x.device
        nb = lib.tasnet_workspace_bytes(cfg, n, S)
        ws = model._ws.get(("tasnet", str(dev), n, S), nb, dev)
        sb = lib.tasnet_saved_bytes(cfg, n, S)
        slots = model._train_saved.setdefault((str(dev), n, S), [])
        slot = next((s for s in slots if s.owner == 0 and s.buf.numel() >= sb), None)
        if slot is None:
            slot = _SavedSlot(torch.empty(sb, dtype=torch.uint8, device=dev))
            slots.append(slot)
        ctx.lease = _Lease(slot)
        out = torch.empty(model.num_spks, n, S_out, device=dev, dtype=torch.float32)
        lib.tasnet_train_forward(cfg, image.data_ptr(), x.data_ptr(), n, S, x_stride, out.data_ptr(), slot.buf.data_ptr(), sb,
                                 ws.data_ptr(), nb, _stream())
        ctx.model, ctx.cfg, ctx.image, ctx.x, ctx.geom = model, cfg, image, x, (n, S, x_stride, sb)
        ctx.shapes = [p.shape for p in params]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        lease, model = ctx.lease, ctx.model
        if not lease.valid():
            raise RuntimeError("ConvTasNet: the saved activations of this forward were taken over by a later forward "
                               "(backward through a retained graph after its buffer was released)")
        lib = get_lib()
        n, S, x_stride, sb = ctx.geom
        d_out = d_out.contiguous().float()
        dev = d_out.device
        nb = lib.tasnet_backward_workspace_bytes(ctx.cfg, n, S)
        ws = model._ws.get(("tasnet_bwd", str(dev), n, S), nb, dev)
        flat = torch.empty(lib.tasnet_param_floats(ctx.cfg), device=dev, dtype=torch.float32)
        lib.tasnet_backward(ctx.cfg, ctx.image.data_ptr(), ctx.x.data_ptr(), n, S, x_stride, lease.slot.buf.data_ptr(), sb,
                            d_out.data_ptr(), flat.data_ptr(), ws.data_ptr(), nb, _stream())
        lease.release()
        grads, at = [], 0
        for i, shape in enumerate(ctx.shapes):
            size = shape.numel()
            grads.append(flat[at:at + size].view(shape) if ctx.needs_input_grad[2 + i] else None)
            at += size
        return (None, None, *grads)


class TasNetStream:
    """``n`` concurrent streams of a causal ConvTasNet that advance in lockstep (``ConvTasNet.stream(n)``; csrc/tasnet_stream.inc).

    ``push(x)``: x (n, F hop), or (F hop,) for n = 1, hop = L/2, any F >= 1 (it may change from call to call) -> ``num_spks``
    tensors (n, F hop).  The stream has an algorithmic delay of exactly one hop (``delay``): the first hop of output after a
    reset is zero, and ``concat(pushes)[..., hop:]`` followed by ``flush()`` (``num_spks`` tensors (n, hop)) is bit for bit
    ``model([x])`` of the whole signal.  ``reset(slots=None)`` starts all streams, or the given ones, over; the others are not
    disturbed.  State (per stream: one hop of samples, every block's last (P - 1) 2^x frames, one hop of decoder taps, a frame
    counter) and workspaces live on the device and belong to this object; a workspace is kept per F and never freed, so a
    captured graph of a push stays valid.  ``push`` works under ``torch.cuda.graph``: the frame counters are device data,
    so replaying the graph on a refilled static input advances the stream.  Needs eval mode and no autograd, like
    ``forward(..., lengths=)``; the packed weights follow the parameters as for ``forward``."""

    def __init__(self, model, n=1):
        why = model.stream_limits()
        if why:
            raise RuntimeError("ConvTasNet: this configuration cannot stream: " + "; ".join(why))
        if int(n) != n or not 1 <= n <= 65535:
            raise ValueError(f"ConvTasNet.stream: n must be an integer in [1, 65535], got {n!r}")
        self.model, self.n, self.hop = model, int(n), model.L // 2
        self._state = None        # (device, buffer)
        self._ws = {}             # (device, F) -> buffer

    @property
    def delay(self):
        return self.hop

    def _check_mode(self, x=None):
        m = self.model
        if m.training or not use_hip_path(m) or (x is not None and needs_graph(x)):
            raise RuntimeError("ConvTasNet: streaming is an inference call: it needs eval mode and no autograd "
                               "(torch.no_grad(), or frozen parameters)")

    def _get_state(self, lib, cfg, device):
        if self._state is None or self._state[0] != device:
            nb = lib.tasnet_stream_state_bytes(cfg, self.n)
            buf = torch.empty(nb, dtype=torch.uint8, device=device)
            lib.tasnet_stream_reset(cfg, buf.data_ptr(), nb, self.n, None, _stream())
            self._state = (device, buf)
        return self._state[1]

    def reset(self, slots=None):
        if slots is not None:
            slots = [int(v) for v in (slots.reshape(-1).tolist() if torch.is_tensor(slots) else slots)]
            if any(not 0 <= v < self.n for v in slots):
                raise ValueError(f"ConvTasNet stream: slots must lie in [0, {self.n}), got {slots!r}")
            if not slots:
                return
        lib = get_lib()
        if self._state is None:                      # nothing pushed yet: the state is created (reset) where the weights live
            dev = self.model.encoder.weight.device
            if dev.type == "cuda":
                self._get_state(lib, self.model._cfg(precision()), dev)
            return
        buf = self._state[1]
        lib.tasnet_stream_reset(self.model._cfg(precision()), buf.data_ptr(), buf.numel(), self.n, slots, _stream())

    def push(self, x):
        self._check_mode(x)
        if not torch.is_tensor(x) or x.dim() not in (1, 2):
            raise ValueError("ConvTasNet stream: push takes a 1-D or 2-D tensor of samples")
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.shape[0] != self.n:
            raise ValueError(f"ConvTasNet stream: {x.shape[0]} rows pushed into {self.n} streams")
        if x.shape[1] == 0 or x.shape[1] % self.hop:
            raise ValueError(f"ConvTasNet stream: a push takes a positive multiple of hop = {self.hop} samples per stream, "
                             f"got {x.shape[1]} (the caller buffers the remainder)")
        require_device(x, "ConvTasNet")
        m, n, F = self.model, self.n, x.shape[1] // self.hop
        lib, cfg, image, x, x_stride = m._hip_inputs(x)
        if torch.cuda.is_current_stream_capturing() and (self._state is None or self._state[0] != x.device):
            raise RuntimeError("ConvTasNet stream: call reset() (or push once) before capturing a push: creating the state "
                               "resets it, and a captured reset would start the stream over at every replay")
        state = self._get_state(lib, cfg, x.device)
        ws = self._ws.get((x.device, F))
        if ws is None:
            ws = self._ws[(x.device, F)] = torch.empty(lib.tasnet_stream_workspace_bytes(cfg, n, F), dtype=torch.uint8, device=x.device)
        out = torch.empty(m.num_spks, n, F * self.hop, device=x.device, dtype=torch.float32)
        lib.tasnet_stream_step(cfg, image.data_ptr(), x.data_ptr(), n, F, x_stride, out.data_ptr(), state.data_ptr(), state.numel(),
                               ws.data_ptr(), ws.numel(), _stream())
        return [out[s] for s in range(m.num_spks)]

    def flush(self):
        self._check_mode()
        m = self.model
        if self._state is None:
            raise RuntimeError("ConvTasNet stream: flush before the first push")
        lib = get_lib()
        cfg = m._cfg(precision())
        image = m._get_image(cfg)
        dev, state = self._state
        out = torch.empty(m.num_spks, self.n, self.hop, device=dev, dtype=torch.float32)
        lib.tasnet_stream_flush(cfg, image.data_ptr(), state.data_ptr(), state.numel(), self.n, out.data_ptr(), _stream())
        return [out[s] for s in range(m.num_spks)]


class ConvTasNet(PackedWeightsMixin, nn.Module):
    """Drop-in for onssen.nn.ConvTasNet (onssen/nn/tasnet.py:166-264): same constructor, defaults, submodule / parameter names
    and shapes, and forward contract.

    forward([x]) with x (S,) or (n, S) -> list of ``num_spks`` tensors, each torch.squeeze-d as upstream: (S_out,) for n = 1,
    (n, S_out) otherwise; T = (S - L) // (L/2) + 1 frames, S_out = (T - 1) L/2 + L (trailing samples are dropped).

    forward([x], lengths=...) (extension, eval only): a RAGGED batch of whole utterances -- x (n, S_max) zero-padded (what lies
    beyond a row's own length is never read), ``lengths`` a sequence of n ints or a CPU integer tensor, n <= RAGGED_MAX.
    Returns ``num_spks`` tensors (n, S_out_max), never squeezed; row b holds the estimate of utterance b in [0, S_out_b) and
    zeros after it, bit for bit what ``forward([x[b, :lengths[b]]])`` returns (gLN statistics, the depthwise convolution's
    padding and the overlap-add use the utterance's own frames; the activations are compact rows, so a batch costs what its
    frames cost).  The lengths are kernel arguments, not device data: a device tensor is refused (reading it would stall the
    stream), and a captured graph is tied to the lengths it was captured with.  Workspace: one grow-only buffer per model
    (the largest batch seen, times 1.25 at most), so a loop over batches of ever different lengths allocates a handful of
    times and then never; under graph capture a buffer per tuple of lengths instead (a regrowth must not free memory a
    captured graph points into).

    In eval mode without autograd, on ROCm tensors: the HIP forward (csrc/tasnet.inc) -- the encoder + LayerNorm, every 1x1
    convolution as a row GEMM (exact fp32 under ``precision`` f32 and bf16x3, plain bf16 products under the opt-in bf16: see
    EXACT_KINDS), PReLU + norm statistics, the normalised
    dilated depthwise convolution, the masks and the overlap-add decoder.  A shape it cannot run raises (odd L, L > 64,
    N > 1024, P > 32, an even P without ``causal``, more than 8 speakers); nothing falls back to ATen.

    Training (train mode, or a parameter gradient needed) on ROCm tensors with fp32 parameters: the network's forward AND
    backward run on HIP kernels behind one autograd node (_TasNetTrainFunction, csrc/tasnet_bwd.inc; option ``tasnet_train``,
    default "hip"), so ``loss.backward()``, ``dist.train_step``, the fused clip + Adam and the gradient reducer work on it as on
    any module; the training forward's output is bit-identical to the eval forward's.  The loss (``loss.si_snr_loss``) runs on
    PyTorch ops by default and, under the option ``tasnet_loss = "hip"``, on the SI-SNR PIT kernels (csrc/loss_sisnr.inc) as one
    more autograd node applied to this forward's (num_spks, n, S_out) output: a training step then runs on HIP kernels throughout.
    ``hip_train_limits()`` lists what sends a training forward to ATen autograd instead (``_autograd_forward``): what
    ``hip_limits()`` lists, ``norm="bn"``, an input that requires a gradient, anomaly mode; double backward is not offered.
    ``last_train_path`` ("hip" | "aten") says which path the last training forward took.  A CPU tensor raises unless
    ONSSEN_CPU_AUTOGRAD=1 (test scaffolding) is set."""

    def __init__(self, N=512, L=16, B=128, H=512, P=3, X=8, R=3, norm="gln", num_spks=2, activate="relu", causal=False,
                 **hip_options):
        super().__init__()
        options.constructor_options(type(self).__name__, hip_options)
        if norm not in _NORMS:
            raise ValueError(f"norm must be one of {sorted(_NORMS)}, got {norm!r}")
        if activate not in _ACTS:
            raise KeyError(activate)
        self.N, self.L, self.B, self.H, self.P, self.X, self.R = N, L, B, H, P, X, R
        self.norm, self.num_spks, self.activation_type, self.causal = norm, num_spks, activate, bool(causal)
        self.encoder = nn.Conv1d(1, N, L, stride=L // 2, padding=0)
        self.LayerN_S = CumulativeLayerNorm(N)
        self.BottleN_S = nn.Conv1d(N, B, 1)
        self.separation = nn.Sequential(*[
            nn.Sequential(*[Conv1DBlock(B, H, P, 2 ** x, norm, causal) for x in range(X)]) for _ in range(R)])
        self.gen_masks = nn.Conv1d(B, num_spks * N, 1)
        self.decoder = nn.ConvTranspose1d(N, 1, L, stride=L // 2)
        self._ws = _Workspaces()
        self._init_packed_hooks()
        self._image = None        # (key, image tensor)
        self._train_saved = {}    # (device, n, S) -> [_SavedSlot]: saved activations of the HIP training forward
        self.last_train_path = None

    # ---- HIP path ---------------------------------------------------------------------------------------------------
    def hip_limits(self):
        """Reasons the HIP forward cannot run this configuration (empty: it can)."""
        why = []
        if self.L % 2 or not 2 <= self.L <= 64:
            why.append(f"L = {self.L}: the HIP forward needs an even L in [2, 64]")
        if self.N > 1024:
            why.append(f"N = {self.N} > 1024 (encoder: one wave per frame, 16 channels per lane)")
        if self.P > 32:
            why.append(f"P = {self.P} > 32")
        if self.P % 2 == 0 and not self.causal:
            why.append(f"P = {self.P} is even without causal: the reference's block changes the frame count there")
        if self.num_spks > 8:
            why.append(f"num_spks = {self.num_spks} > 8")
        if self.X > 30:
            why.append(f"X = {self.X} > 30")
        return why

    STREAM_MAX_HISTORY = 1 << 24              # ONSSEN_TASNET_STREAM_MAX_HISTORY: frames of the deepest block's history

    def stream_limits(self):
        """Reasons this model cannot run as a stream (empty: ``stream()`` works)."""
        why = self.hip_limits()
        if not self.causal:
            why.append("causal = False: a non-causal block looks ahead of the frame it computes")
        if self.norm == "gln":
            why.append("norm = 'gln': its statistics span the whole utterance (cln and bn are local to a frame)")
        if (self.P - 1) << max(self.X - 1, 0) > self.STREAM_MAX_HISTORY:
            why.append(f"(P - 1) 2^(X - 1) = {(self.P - 1) << (self.X - 1)} frames of history > {self.STREAM_MAX_HISTORY}")
        return why

    def stream(self, n=1):
        """``n`` lockstep streams of this (causal, cln / bn) model: see TasNetStream."""
        return TasNetStream(self, n)

    # 1x1 convolutions kept on exact fp32 per precision (ONSSEN_TASNET_EXACT_* bits, include/onssen_hip.h).  bf16x3 keeps all four
    # kinds there: split-bf16 products (~1e-5 relative per dot product) compound over the 50 chained GEMMs of the recipe to a
    # relative L2 of 1.8e-5 at the output (measured, MI355X, 3 x 32 000), outside the 1e-5 contract, and no subset of the kinds
    # brings it back with margin (every kind contributes about equally: profiles/tasnet_exact_probe.jsonl); exact fp32 costs 12 %
    # of the forward there (the narrow GEMMs are not what bounds it).  bf16 (opt-in, bf16-grade) keeps plain bf16 products.
    EXACT_KINDS = {"f32": 0, "bf16x3": 15, "bf16": 0}
    RAGGED_MAX = _abi.TASNET_RAGGED_MAX       # utterances of one ragged forward (the kernels take their table by value)

    def _cfg(self, prec):
        return _abi.Lib.tasnet_cfg(self.N, self.L, self.B, self.H, self.P, self.X, self.R, _NORMS[self.norm], self.num_spks,
                                   _ACTS[self.activation_type], self.causal, _PRECS[prec] | (self.EXACT_KINDS[prec] << 8))

    def _packed_params(self):
        ts = [self.encoder.weight, self.encoder.bias, self.LayerN_S.weight, self.LayerN_S.bias, self.BottleN_S.weight,
              self.BottleN_S.bias]
        for rep in self.separation:
            for blk in rep:
                ts += [blk.conv1x1.weight, blk.conv1x1.bias, blk.PReLU_1.weight, blk.norm_1.weight, blk.norm_1.bias]
                if self.norm == "bn":
                    ts += [blk.norm_1.running_mean, blk.norm_1.running_var]
                ts += [blk.dwconv.weight, blk.dwconv.bias, blk.Sc_conv.weight, blk.Sc_conv.bias]
        return ts + [self.gen_masks.weight, self.gen_masks.bias, self.decoder.weight, self.decoder.bias]

    def _get_image(self, cfg):
        ts = self._packed_params()
        key = _version_key(ts)
        capturing = torch.cuda.is_current_stream_capturing()
        if self._image is not None and self._image[0] == key:
            self._in_graph = getattr(self, "_in_graph", False) or capturing
            return self._image[1]
        _park_if_captured(self, ("_image",))
        self._in_graph = capturing
        lib = get_lib()
        dev = ts[0].device
        flat = torch.cat([t.detach().reshape(-1).float() for t in ts]).contiguous()
        assert flat.numel() == lib.tasnet_param_floats(cfg)
        nb = lib.tasnet_image_bytes(cfg)
        image = torch.empty(nb, dtype=torch.uint8, device=dev)
        lib.tasnet_pack(cfg, flat.data_ptr(), image.data_ptr(), nb, _stream())
        self._image = (key, image, flat)            # flat stays alive until the stream-ordered pack has read it
        return image

    def _hip_inputs(self, x):
        """What every HIP entry takes -> (lib, cfg, packed image, x, x_stride): x (n, S) as fp32 with unit inner stride and rows at
        least S apart; a size-1 batch dimension may carry any stride, so its x_stride is S."""
        lib = get_lib()
        cfg = self._cfg(precision())
        image = self._get_image(cfg)
        n, S = x.shape
        x = x.float()
        if x.stride(1) != 1 or (n > 1 and x.stride(0) < S):
            x = x.contiguous()
        return lib, cfg, image, x, (x.stride(0) if n > 1 else S)

    def _require_hip_forward(self):
        why = self.hip_limits()
        if why:
            raise RuntimeError("ConvTasNet: the HIP forward cannot run this configuration: " + "; ".join(why))

    def _hip_forward(self, x):
        out = self._hip_forward_rows(x)
        return [torch.squeeze(out[s]) for s in range(self.num_spks)]

    def _hip_forward_rows(self, x):
        """The eval forward of x (n, S) as ONE tensor (num_spks, n, S_out), as the library writes it."""
        self._require_hip_forward()
        require_device(x, "ConvTasNet")
        n, S = x.shape
        if S < self.L:
            raise RuntimeError(f"ConvTasNet: {S} samples is shorter than one encoder frame (L = {self.L})")
        lib, cfg, image, x, x_stride = self._hip_inputs(x)
        hop = self.L // 2
        T = (S - self.L) // hop + 1
        S_out = (T - 1) * hop + self.L
        nb = lib.tasnet_workspace_bytes(cfg, n, S)
        ws = self._ws.get(("tasnet", str(x.device), n, S), nb, x.device)
        out = torch.empty(self.num_spks, n, S_out, device=x.device, dtype=torch.float32)
        lib.tasnet_forward(cfg, image.data_ptr(), x.data_ptr(), n, S, x_stride, out.data_ptr(), ws.data_ptr(), nb, _stream())
        return out

    def _ragged_lengths(self, x, lengths):
        """``lengths`` of a ragged forward of x (n, S_max) as a list of host ints, validated."""
        if torch.is_tensor(lengths):
            if lengths.is_cuda:
                raise TypeError("ConvTasNet: lengths must be host integers (a sequence or a CPU tensor): they size the launches "
                                "and travel as kernel arguments, so a device tensor would force a synchronisation per forward")
            if lengths.is_floating_point() or lengths.is_complex() or lengths.dtype == torch.bool:
                raise TypeError(f"ConvTasNet: lengths must be an integer tensor, got {lengths.dtype}")
            lengths = lengths.reshape(-1).tolist()
        lengths = list(lengths)
        if any(isinstance(v, bool) or int(v) != v for v in lengths):
            raise TypeError(f"ConvTasNet: lengths must be integers, got {lengths!r}")
        lengths = [int(v) for v in lengths]
        n, S = x.shape
        if len(lengths) != n:
            raise ValueError(f"ConvTasNet: {len(lengths)} lengths for a batch of {n} rows")
        if n > self.RAGGED_MAX:
            raise ValueError(f"ConvTasNet: a ragged forward takes at most {self.RAGGED_MAX} utterances, got {n} "
                             "(separation.separate_tasnet splits a longer list)")
        for b, v in enumerate(lengths):
            if v < self.L:
                raise ValueError(f"ConvTasNet: lengths[{b}] = {v} samples is shorter than one encoder frame (L = {self.L})")
            if v > S:
                raise ValueError(f"ConvTasNet: lengths[{b}] = {v} exceeds the {S} samples of a row of the input")
        return lengths

    def _hip_forward_ragged(self, x, lengths):
        if self.training or not use_hip_path(self) or needs_graph(x):
            raise RuntimeError("ConvTasNet: lengths= (a ragged batch of whole utterances) is an inference call: it needs eval "
                               "mode and no autograd (torch.no_grad(), or frozen parameters); training uses fixed-size chunks")
        self._require_hip_forward()
        lengths = self._ragged_lengths(x, lengths)
        require_device(x, "ConvTasNet")
        n, S = x.shape
        lib, cfg, image, x, x_stride = self._hip_inputs(x)
        hop = self.L // 2
        S_out = max((v - self.L) // hop for v in lengths) * hop + self.L
        ln = lib.tasnet_lengths(lengths)
        nb = lib.tasnet_ragged_workspace_bytes(cfg, n, ln)
        if torch.cuda.is_current_stream_capturing():
            ws = self._ws.get(("tasnet_ragged", str(x.device), tuple(lengths)), nb, x.device)
        else:
            ws = self._ws.scratch("tasnet_ragged", nb, 0, x.device)
        out = torch.empty(self.num_spks, n, S_out, device=x.device, dtype=torch.float32)
        lib.tasnet_forward_ragged(cfg, image.data_ptr(), x.data_ptr(), n, ln, x_stride, out.data_ptr(), S_out, ws.data_ptr(),
                                  ws.numel(), _stream())
        return [out[s] for s in range(self.num_spks)]

    def hip_train_limits(self, x=None):
        """Reasons a training forward (of ``x``, if given) cannot run on the HIP training kernels (empty: it can)."""
        why = self.hip_limits()
        if self.norm == "bn":
            why.append("norm = 'bn': train-mode BatchNorm (batch statistics, running-statistics updates) stays on ATen")
        if x is not None and needs_graph(x):
            why.append("the input requires a gradient: the HIP backward gives parameter gradients only")
        if torch.is_anomaly_enabled():
            why.append("autograd anomaly mode")
        return why

    def _hip_train_forward(self, x):
        n, S = x.shape
        if S < self.L:
            raise RuntimeError(f"ConvTasNet: {S} samples is shorter than one encoder frame (L = {self.L})")
        out = _TasNetTrainFunction.apply(self, x, *self._packed_params())
        return [torch.squeeze(out[s]) for s in range(self.num_spks)]

    # ---- forward ------------------------------------------------------------------------------------------------------
    def forward(self, input, lengths=None):
        x, = input
        if x.dim() >= 3:
            raise RuntimeError(f"ConvTasNet accepts 1/2D tensors as input, but got {x.dim()}D")
        if x.dim() == 1:
            x = torch.unsqueeze(x, 0)
        if lengths is not None:
            return self._hip_forward_ragged(x, lengths)
        if use_hip_path(self) and not needs_graph(x):
            return self._hip_forward(x)
        if (options.get("tasnet_train") == "hip" and x.is_cuda and all(p.dtype == torch.float32 for p in self._packed_params())
                and not self.hip_train_limits(x)):
            self.last_train_path = "hip"
            return self._hip_train_forward(x)
        self.last_train_path = "aten"
        return self._autograd_forward(x)

    def _autograd_forward(self, x):
        """ATen training path: autograd over PyTorch ops (ROCm device only; a CPU tensor needs ONSSEN_CPU_AUTOGRAD=1)."""
        if not x.is_cuda and options.get("cpu_autograd") != "1":
            raise RuntimeError("onssen_amd: ConvTasNet needs tensors on a ROCm device; there is no CPU fallback "
                               "(ONSSEN_CPU_AUTOGRAD=1 is test scaffolding, never a product path)")
        w = self.encoder(x.unsqueeze(1))
        e = self.BottleN_S(self.LayerN_S(w))
        e = self.separation(e)
        m = self.gen_masks(e)
        m = torch.stack(torch.chunk(m, chunks=self.num_spks, dim=1), dim=0)
        if self.activation_type == "relu":
            m = F.relu(m)
        elif self.activation_type == "sigmoid":
            m = torch.sigmoid(m)
        else:
            m = torch.softmax(m, dim=0)
        return [torch.squeeze(self.decoder(w * m[i])) for i in range(self.num_spks)]
