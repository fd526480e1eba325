"""Drive the streaming Conv-TasNet entry points (onssen_tasnet_stream_*) on host memory beside tests/tasnet_ragged_emu.py: one
packed weight image (Packed) serves the stream and the offline forward it is compared with."""
import numpy as np

from tests import tasnet_emu


class Stream:
    """n lockstep streams over a Packed image.  The state buffer starts as ``fill`` bytes (0xFF: NaN everywhere) and is reset
    through the ABI before the first step."""

    def __init__(self, pk, n, fill=0xFF):
        self.pk, self.n, self.dll = pk, n, pk.lib.dll
        self.hop, self.spk = pk.c["L"] // 2, pk.c["num_spks"]
        self.sb = pk.lib.tasnet_stream_state_bytes(pk.cf, n)
        self.state = tasnet_emu.aligned(self.sb)
        self.state[:] = fill
        self.reset()

    def reset(self, slots=None):
        self.pk.lib.tasnet_stream_reset(self.pk.cf, self.state.ctypes.data, self.sb, self.n, slots, None)

    def push(self, x):
        """x (n, F hop) -> (spk, n, F hop); the workspace is new and NaN-filled at every step (nothing survives in it)."""
        x = np.ascontiguousarray(x, np.float32)
        F = x.shape[1] // self.hop
        assert x.shape == (self.n, F * self.hop)
        wsb = self.pk.lib.tasnet_stream_workspace_bytes(self.pk.cf, self.n, F)
        ws = tasnet_emu.aligned(wsb)
        ws[:] = 0xFF
        out = np.full((self.spk, self.n, F * self.hop), np.nan, dtype=np.float32)
        self.pk.lib.tasnet_stream_step(self.pk.cf, self.pk.image.ctypes.data, x.ctypes.data, self.n, F, x.shape[1],
                                       out.ctypes.data, self.state.ctypes.data, self.sb, ws.ctypes.data, wsb, None)
        return out

    def flush(self):
        out = np.full((self.spk, self.n, self.hop), np.nan, dtype=np.float32)
        self.pk.lib.tasnet_stream_flush(self.pk.cf, self.pk.image.ctypes.data, self.state.ctypes.data, self.sb, self.n,
                                        out.ctypes.data, None)
        return out

    def run(self, x, schedule):
        """The whole (n, sum(schedule) hop) signal through steps of `schedule` hops -> (concatenated step outputs, flush)."""
        assert sum(schedule) * self.hop == x.shape[1]
        outs, at = [], 0
        for F in schedule:
            outs.append(self.push(x[:, at:at + F * self.hop]))
            at += F * self.hop
        return np.concatenate(outs, axis=-1), self.flush()


def stitched(steps, tail, hop):
    """What the stream says the offline forward is: the step outputs without the hop of delay, then the flush."""
    return np.concatenate([steps[..., hop:], tail], axis=-1)
