"""Drive the Conv-TasNet C ABI on host memory (the emulation build of tests/emu): the flat parameter buffer in the order of
include/onssen_hip.h, built from a state dict of NumPy arrays."""
import numpy as np

from tests import tasnet_ref

NORMS = {"gln": 0, "cln": 1, "bn": 2}
ACTS = {"relu": 0, "sigmoid": 1, "softmax": 2}
PRECS = {"f32": 0, "bf16x3": 1, "bf16": 2}


def flat_params(sd, cfg):
    c = dict(tasnet_ref.DEFAULTS, **cfg)
    names = ["encoder.weight", "encoder.bias", "LayerN_S.weight", "LayerN_S.bias", "BottleN_S.weight", "BottleN_S.bias"]
    for r in range(c["R"]):
        for x in range(c["X"]):
            p = f"separation.{r}.{x}."
            names += [p + "conv1x1.weight", p + "conv1x1.bias", p + "PReLU_1.weight", p + "norm_1.weight", p + "norm_1.bias"]
            if c["norm"] == "bn":
                names += [p + "norm_1.running_mean", p + "norm_1.running_var"]
            names += [p + "dwconv.weight", p + "dwconv.bias", p + "Sc_conv.weight", p + "Sc_conv.bias"]
    names += ["gen_masks.weight", "gen_masks.bias", "decoder.weight", "decoder.bias"]
    return np.ascontiguousarray(np.concatenate([np.asarray(sd[k], np.float32).reshape(-1) for k in names]))


def lib_cfg(lib, cfg, prec):
    c = dict(tasnet_ref.DEFAULTS, **cfg)
    return lib.tasnet_cfg(c["N"], c["L"], c["B"], c["H"], c["P"], c["X"], c["R"], NORMS[c["norm"]], c["num_spks"],
                          ACTS[c["activate"]], c["causal"], PRECS[prec])


def aligned(nbytes):
    buf = np.zeros(nbytes + 256, dtype=np.uint8)
    off = (-buf.ctypes.data) % 256
    return buf[off:off + nbytes]


def forward(lib, sd, cfg, x, prec):
    """x (n, S) float32 -> (spk, n, S_out) through onssen_tasnet_pack_f32 + onssen_tasnet_forward_f32 on host memory."""
    c = dict(tasnet_ref.DEFAULTS, **cfg)
    x = np.ascontiguousarray(x, np.float32)
    n, S = x.shape
    cf = lib_cfg(lib, c, prec)
    flat = flat_params(sd, c)
    assert flat.size == lib.tasnet_param_floats(cf)
    nb = lib.tasnet_image_bytes(cf)
    image = aligned(nb)
    lib.tasnet_pack(cf, flat.ctypes.data, image.ctypes.data, nb, None)
    T = tasnet_ref.frames(S, c["L"])
    S_out = (T - 1) * (c["L"] // 2) + c["L"]
    wsb = lib.tasnet_workspace_bytes(cf, n, S)
    ws = aligned(wsb)
    out = np.full((c["num_spks"], n, S_out), np.nan, dtype=np.float32)
    lib.tasnet_forward(cf, image.ctypes.data, x.ctypes.data, n, S, S, out.ctypes.data, ws.ctypes.data, wsb, None)
    return out
