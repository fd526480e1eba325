"""fp64 NumPy restatement of the Conv-TasNet forward (onssen/nn/tasnet.py:166-264), written from its semantics:

encoder Conv1d(1, N, L, stride L/2) without activation; LayerN_S = LayerNorm(N) per frame; BottleN_S 1x1; R x X blocks
``x + Sc_conv(dwconv(norm_1(PReLU_1(conv1x1(x)))))`` (PReLU_2 / norm_2 unused) with dilation 2^x and zero padding of the
normalised signal (causal: left padding only); gen_masks split into num_spks chunks of N channels, relu / sigmoid / softmax
across speakers; d_i = w * m_i; decoder ConvTranspose1d(N, 1, L, stride L/2); torch.squeeze of each output.

``state`` maps the reference's state_dict names to arrays.  Also: a seeded weight generator for any configuration."""
import numpy as np

RECIPE = dict(N=512, L=16, B=128, H=512, P=3, X=8, R=3, norm="gln", num_spks=2, activate="relu", causal=False)
DEFAULTS = dict(RECIPE)
EPS = 1e-5


def _cfg(cfg):
    c = dict(DEFAULTS)
    c.update(cfg or {})
    return c


def state_names(cfg=None):
    """(name, shape) of every state_dict entry in the reference's order."""
    c = _cfg(cfg)
    N, L, B, H, P = c["N"], c["L"], c["B"], c["H"], c["P"]
    out = [("encoder.weight", (N, 1, L)), ("encoder.bias", (N,)), ("LayerN_S.weight", (N,)), ("LayerN_S.bias", (N,)),
           ("BottleN_S.weight", (B, N, 1)), ("BottleN_S.bias", (B,))]

    def norm(prefix):
        if c["norm"] == "gln":
            return [(prefix + ".weight", (H, 1)), (prefix + ".bias", (H, 1))]
        if c["norm"] == "cln":
            return [(prefix + ".weight", (H,)), (prefix + ".bias", (H,))]
        return [(prefix + ".weight", (H,)), (prefix + ".bias", (H,)), (prefix + ".running_mean", (H,)),
                (prefix + ".running_var", (H,)), (prefix + ".num_batches_tracked", ())]

    for r in range(c["R"]):
        for x in range(c["X"]):
            p = f"separation.{r}.{x}."
            out += [(p + "conv1x1.weight", (H, B, 1)), (p + "conv1x1.bias", (H,)), (p + "PReLU_1.weight", (1,))]
            out += norm(p + "norm_1")
            out += [(p + "dwconv.weight", (H, 1, P)), (p + "dwconv.bias", (H,)), (p + "PReLU_2.weight", (1,))]
            out += norm(p + "norm_2")
            out += [(p + "Sc_conv.weight", (B, H, 1)), (p + "Sc_conv.bias", (B,))]
    out += [("gen_masks.weight", (c["num_spks"] * N, B, 1)), ("gen_masks.bias", (c["num_spks"] * N,)),
            ("decoder.weight", (N, 1, L)), ("decoder.bias", (1,))]
    return out


def make_state(cfg=None, seed=0):
    """Seeded weights with the scales of PyTorch's default initialisation (uniform +-1/sqrt(fan_in)), non-trivial norm affines
    and BatchNorm running statistics."""
    c = _cfg(cfg)
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in state_names(c):
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[name] = np.array(7, dtype=np.int64)
            continue
        if "PReLU" in name:
            v = np.full(shape, 0.25) + 0.05 * rng.standard_normal(shape)
        elif "norm" in name or "LayerN_S" in name:
            if leaf == "weight":
                v = 1.0 + 0.1 * rng.standard_normal(shape)
            elif leaf == "running_var":
                v = 0.5 + rng.random(shape)
            else:
                v = 0.1 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else None
            if name.startswith("decoder"):
                fan_in = c["L"]       # ConvTranspose1d: weight (in, out, k) -> fan_in = out * k
            if fan_in is None:        # a bias: the fan-in of its weight
                w = name[:-len("bias")] + "weight"
                wshape = dict(state_names(c))[w]
                fan_in = wshape[2] if name.startswith("decoder") else int(np.prod(wshape[1:]))
            bound = 1.0 / np.sqrt(fan_in)
            v = rng.uniform(-bound, bound, shape)
        sd[name] = np.asarray(v, dtype=np.float32)
    return sd


def _norm(c, sd, prefix, y):
    """y (n, T, C) -> normalised (n, T, C)."""
    g = np.asarray(sd[prefix + ".weight"], np.float64).reshape(-1)
    b = np.asarray(sd[prefix + ".bias"], np.float64).reshape(-1)
    if c["norm"] == "gln":
        mean = y.mean(axis=(1, 2), keepdims=True)
        var = ((y - mean) ** 2).mean(axis=(1, 2), keepdims=True)
        return g * (y - mean) / np.sqrt(var + EPS) + b
    if c["norm"] == "cln":
        mean = y.mean(axis=2, keepdims=True)
        var = ((y - mean) ** 2).mean(axis=2, keepdims=True)
        return (y - mean) / np.sqrt(var + EPS) * g + b
    mu = np.asarray(sd[prefix + ".running_mean"], np.float64)
    var = np.asarray(sd[prefix + ".running_var"], np.float64)
    return (y - mu) / np.sqrt(var + EPS) * g + b


def frames(S, L):
    return (S - L) // (L // 2) + 1


def forward(sd, x, cfg=None):
    """x (S,) or (n, S) -> list of num_spks arrays, each squeezed like the reference ((S_out,) for n = 1)."""
    c = _cfg(cfg)
    x = np.asarray(x, np.float64)
    if x.ndim >= 3:
        raise RuntimeError("ConvTasNet accepts 1/2D tensors")
    if x.ndim == 1:
        x = x[None]
    f = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    N, L, P, X, spk = c["N"], c["L"], c["P"], c["X"], c["num_spks"]
    hop = L // 2
    n, S = x.shape
    T = frames(S, L)
    idx = np.arange(T)[:, None] * hop + np.arange(L)[None, :]
    fr = x[:, idx]                                                           # (n, T, L)
    w = fr @ f["encoder.weight"][:, 0, :].T + f["encoder.bias"]              # (n, T, N)
    mean = w.mean(axis=2, keepdims=True)
    var = ((w - mean) ** 2).mean(axis=2, keepdims=True)
    e = (w - mean) / np.sqrt(var + EPS) * f["LayerN_S.weight"] + f["LayerN_S.bias"]
    e = e @ f["BottleN_S.weight"][:, :, 0].T + f["BottleN_S.bias"]          # (n, T, B)
    for r in range(c["R"]):
        for xb in range(X):
            p = f"separation.{r}.{xb}."
            d = 2 ** xb
            y = e @ f[p + "conv1x1.weight"][:, :, 0].T + f[p + "conv1x1.bias"]
            a = f[p + "PReLU_1.weight"][0]
            y = np.where(y >= 0, y, a * y)
            y = _norm(c, f, p + "norm_1", y)
            pad_l = d * (P - 1) if c["causal"] else d * (P - 1) // 2
            ypad = np.zeros((n, T + d * (P - 1), y.shape[2]))
            ypad[:, pad_l:pad_l + T] = y
            wd = f[p + "dwconv.weight"][:, 0, :]                             # (H, P)
            z = np.zeros_like(y) + f[p + "dwconv.bias"]
            for k in range(P):
                z += ypad[:, k * d:k * d + T] * wd[:, k]
            e = e + (z @ f[p + "Sc_conv.weight"][:, :, 0].T + f[p + "Sc_conv.bias"])
    m = e @ f["gen_masks.weight"][:, :, 0].T + f["gen_masks.bias"]          # (n, T, spk N)
    m = np.stack([m[:, :, s * N:(s + 1) * N] for s in range(spk)])           # (spk, n, T, N)
    if c["activate"] == "relu":
        m = np.maximum(m, 0)
    elif c["activate"] == "sigmoid":
        m = 1.0 / (1.0 + np.exp(-m))
    else:
        m = np.exp(m - m.max(axis=0, keepdims=True))
        m = m / m.sum(axis=0, keepdims=True)
    S_out = (T - 1) * hop + L
    wdec = f["decoder.weight"][:, 0, :]                                      # (N, L)
    outs = []
    for s in range(spk):
        fr_out = (w * m[s]) @ wdec                                           # (n, T, L)
        o = np.zeros((n, S_out)) + f["decoder.bias"][0]
        o[:, :T * hop] += fr_out[:, :, :hop].reshape(n, T * hop)             # first half of frame t -> block t
        o[:, hop:(T + 1) * hop] += fr_out[:, :, hop:].reshape(n, T * hop)   # second half -> block t + 1
        outs.append(np.squeeze(o))
    return outs


def load_fixture(path):
    """(cfg, state dict, x, out64, out32) of a g8_tasnet_* fixture."""
    z = np.load(path)
    cfg = {k[5:]: z[k].item() for k in z.files if k.startswith("cfg__")}
    for k in ("norm", "activate"):
        cfg[k] = str(cfg[k])
    cfg["causal"] = bool(cfg["causal"])
    sd = {k[4:]: z[k] for k in z.files if k.startswith("sd__")}
    get = lambda k: z[k] if k in z.files else None                          # noqa: E731
    return cfg, sd, z["x"], get("out64"), get("out32")
