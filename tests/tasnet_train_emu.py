"""Drive the Conv-TasNet training C ABI (training forward + backward) on host memory (the emulation build of tests/emu), and the
fp64 yardstick for its gradients: autograd of the module's unchanged ATen path on the CPU in double precision."""
import numpy as np

from tests import tasnet_emu, tasnet_ref


def param_names(cfg):
    """Names of the flat parameter / gradient buffer's entries, in its order (BatchNorm is not offered for training)."""
    c = dict(tasnet_ref.DEFAULTS, **cfg)
    names = ["encoder.weight", "encoder.bias", "LayerN_S.weight", "LayerN_S.bias", "BottleN_S.weight", "BottleN_S.bias"]
    for r in range(c["R"]):
        for x in range(c["X"]):
            p = f"separation.{r}.{x}."
            names += [p + "conv1x1.weight", p + "conv1x1.bias", p + "PReLU_1.weight", p + "norm_1.weight", p + "norm_1.bias",
                      p + "dwconv.weight", p + "dwconv.bias", p + "Sc_conv.weight", p + "Sc_conv.bias"]
    return names + ["gen_masks.weight", "gen_masks.bias", "decoder.weight", "decoder.bias"]


class Step:
    """pack + training forward of one batch; ``backward(d_out)`` -> {name: gradient, shaped like the state dict entry}."""

    def __init__(self, lib, sd, cfg, x, prec):
        self.lib, self.sd = lib, sd
        self.c = c = dict(tasnet_ref.DEFAULTS, **cfg)
        self.x = x = np.ascontiguousarray(x, np.float32)
        self.n, self.S = x.shape
        self.cf = cf = tasnet_emu.lib_cfg(lib, c, prec)
        flat = tasnet_emu.flat_params(sd, c)
        self.nparam = lib.tasnet_param_floats(cf)
        assert flat.size == self.nparam
        nb = lib.tasnet_image_bytes(cf)
        self.image = tasnet_emu.aligned(nb)
        lib.tasnet_pack(cf, flat.ctypes.data, self.image.ctypes.data, nb, None)
        T = tasnet_ref.frames(self.S, c["L"])
        self.S_out = (T - 1) * (c["L"] // 2) + c["L"]
        self.saved_bytes = lib.tasnet_saved_bytes(cf, self.n, self.S)
        self.saved = tasnet_emu.aligned(self.saved_bytes)
        wsb = lib.tasnet_workspace_bytes(cf, self.n, self.S)
        ws = tasnet_emu.aligned(wsb)
        self.out = np.full((c["num_spks"], self.n, self.S_out), np.nan, dtype=np.float32)
        lib.tasnet_train_forward(cf, self.image.ctypes.data, x.ctypes.data, self.n, self.S, self.S, self.out.ctypes.data,
                                 self.saved.ctypes.data, self.saved_bytes, ws.ctypes.data, wsb, None)

    def backward_flat(self, d_out):
        lib = self.lib
        d_out = np.ascontiguousarray(d_out, np.float32)
        assert d_out.shape == self.out.shape
        wsb = lib.tasnet_backward_workspace_bytes(self.cf, self.n, self.S)
        ws = tasnet_emu.aligned(wsb)
        ws[:] = 0xA5                                     # the workspace needs no zeroing
        g = np.full(self.nparam, np.nan, dtype=np.float32)
        lib.tasnet_backward(self.cf, self.image.ctypes.data, self.x.ctypes.data, self.n, self.S, self.S, self.saved.ctypes.data,
                            self.saved_bytes, d_out.ctypes.data, g.ctypes.data, ws.ctypes.data, wsb, None)
        return g

    def backward(self, d_out):
        g, out, at = self.backward_flat(d_out), {}, 0
        for k in param_names(self.c):
            shape = np.asarray(self.sd[k]).shape
            size = int(np.prod(shape))
            out[k] = g[at:at + size].reshape(shape)
            at += size
        assert at == g.size
        return out


def aten_model(cfg, sd, dtype):
    import torch
    from onssen_amd import nn as onn
    m = onn.ConvTasNet(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dtype).train()


def aten_grads(cfg, sd, x, dtype, d_out=None, loss_fn=None):
    """Gradients of the module's ATen path on the CPU (ONSSEN_CPU_AUTOGRAD=1 must be set) in ``dtype``: of sum(out * d_out), or
    of loss_fn(estimates).  -> (stacked outputs, {name: gradient}, loss value)"""
    import torch
    m = aten_model(cfg, sd, dtype)
    ests = m._autograd_forward(torch.from_numpy(np.asarray(x)).to(dtype))
    n = x.shape[0]
    ests = [e.reshape(n, -1) for e in ests]
    if loss_fn is None:
        loss = sum((e * torch.from_numpy(np.asarray(d_out[i])).to(dtype)).sum() for i, e in enumerate(ests))
    else:
        loss = loss_fn(ests)
    loss.backward()
    grads = {k: p.grad.detach().numpy() for k, p in m.named_parameters() if p.grad is not None}
    return np.stack([e.detach().numpy() for e in ests]), grads, float(loss.detach())


def grad_error(got, ref):
    """The project's metric for these gradients (tests/test_gpu_tasnet.py): per parameter max |g - g_ref| relative to
    max(max |g_ref|, 1e-3 of the largest gradient of the model); -> (worst value, its parameter)."""
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    worst, where = 0.0, None
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    for k, g in ref.items():
        err = float(np.abs(np.asarray(got[k], np.float64).reshape(g.shape) - g).max()) / max(float(np.abs(g).max()), 1e-3 * gmax)
        if err >= worst:
            worst, where = err, k
    return worst, where
