"""Drive the ragged Conv-TasNet entry points (onssen_tasnet_forward_ragged_f32) on host memory beside tests/tasnet_emu.py: one
packed weight image serves the ragged call and the one-utterance rectangular calls it is compared with."""
import ctypes as C

import numpy as np

from tests import tasnet_emu, tasnet_ref


class Packed:
    def __init__(self, lib, sd, cfg, prec):
        self.lib, self.c = lib, dict(tasnet_ref.DEFAULTS, **cfg)
        self.cf = tasnet_emu.lib_cfg(lib, self.c, prec)
        flat = tasnet_emu.flat_params(sd, self.c)
        self.nb = lib.tasnet_image_bytes(self.cf)
        self.image = tasnet_emu.aligned(self.nb)
        lib.tasnet_pack(self.cf, flat.ctypes.data, self.image.ctypes.data, self.nb, None)

    def s_out(self, S):
        L = self.c["L"]
        return (tasnet_ref.frames(S, L) - 1) * (L // 2) + L

    def one(self, x):
        """x (S,) or (n, S) -> (spk, n, S_out): the rectangular forward."""
        x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
        n, S = x.shape
        wsb = self.lib.tasnet_workspace_bytes(self.cf, n, S)
        ws = tasnet_emu.aligned(wsb)
        out = np.full((self.c["num_spks"], n, self.s_out(S)), np.nan, dtype=np.float32)
        self.lib.tasnet_forward(self.cf, self.image.ctypes.data, x.ctypes.data, n, S, S, out.ctypes.data, ws.ctypes.data, wsb, None)
        return out

    def ragged(self, xs, out_extra=3, pad=np.nan):
        """xs: list of 1-D waveforms -> (spk, n, out_stride); the padding of the input rows is `pad`, `out` starts as NaN."""
        n = len(xs)
        lens = [len(v) for v in xs]
        stride = max(lens) + 5
        x = np.full((n, stride), pad, dtype=np.float32)
        for b, v in enumerate(xs):
            x[b, :len(v)] = v
        ln = self.lib.tasnet_lengths(lens)
        wsb = self.lib.tasnet_ragged_workspace_bytes(self.cf, n, ln)
        ws = tasnet_emu.aligned(wsb)
        out_stride = max(self.s_out(s) for s in lens) + out_extra
        out = np.full((self.c["num_spks"], n, out_stride), np.nan, dtype=np.float32)
        self.lib.tasnet_forward_ragged(self.cf, self.image.ctypes.data, x.ctypes.data, n, ln, stride, out.ctypes.data, out_stride,
                                       ws.ctypes.data, wsb, None)
        return out

    def raw(self, n, lens, x_stride, out_stride, ws_bytes=None):
        """The return code of the ragged forward on scratch buffers sized generously (refusal tests: nothing may be launched)."""
        ln = (C.c_int32 * max(1, len(lens)))(*lens)
        x = np.zeros((max(1, len(lens)), max(1, x_stride, *lens)), dtype=np.float32)
        out = np.zeros((self.c["num_spks"], max(1, len(lens)), max(1, out_stride, *lens)), dtype=np.float32)
        ok = [max(s, self.c["L"]) for s in lens][:64] or [self.c["L"]]
        wsb = self.lib.tasnet_ragged_workspace_bytes(self.cf, len(ok), (C.c_int32 * len(ok))(*ok))
        ws = tasnet_emu.aligned(wsb)
        return self.lib.dll.onssen_tasnet_forward_ragged_f32(self.cf, self.image.ctypes.data, x.ctypes.data, n, ln, x_stride,
                                                             out.ctypes.data, out_stride, ws.ctypes.data,
                                                             wsb if ws_bytes is None else ws_bytes, None)
