#!/usr/bin/env python
"""Golden vectors for ConvTasNet and the time-domain losses: imports the reference's own onssen.nn.ConvTasNet and
onssen.loss (loss_e2e) in the build container (the reference never travels) and commits arrays and names only under
tests/golden/ (g8_tasnet_*).  Run from the repo root: PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_tasnet.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.gen_golden import OUT, load_ref_pkg, to_torch_sd   # noqa: E402
from tests import tasnet_ref                                   # noqa: E402

# small configurations: every norm, causal and not, every activation, 2 and 3 speakers, P 3 and 5, 1-D and 2-D inputs, and
# lengths where (S - L) is not a multiple of L/2
SMALL = [
    ("gln_relu", dict(N=24, L=8, B=12, H=20, P=3, X=3, R=2, norm="gln", num_spks=2, activate="relu", causal=False), (2, 203)),
    ("cln_sigmoid_causal", dict(N=20, L=4, B=16, H=24, P=3, X=2, R=2, norm="cln", num_spks=2, activate="sigmoid", causal=True),
     (1, 150)),
    ("bn_softmax_p5", dict(N=16, L=6, B=10, H=18, P=5, X=2, R=1, norm="bn", num_spks=3, activate="softmax", causal=False), (3, 121)),
    ("gln_softmax_causal_1d", dict(N=18, L=8, B=8, H=16, P=3, X=3, R=1, norm="gln", num_spks=2, activate="softmax", causal=True),
     (0, 97)),
    ("cln_relu_spk3_p5", dict(N=16, L=4, B=12, H=12, P=5, X=2, R=2, norm="cln", num_spks=3, activate="relu", causal=False), (2, 90)),
    ("bn_sigmoid_causal", dict(N=12, L=8, B=8, H=16, P=3, X=2, R=1, norm="bn", num_spks=2, activate="sigmoid", causal=True),
     (2, 133)),
]


def build(ref_nn, cfg, sd):
    m = ref_nn.ConvTasNet(**cfg)
    m.load_state_dict(to_torch_sd(sd), strict=True)
    return m.eval()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_nn = load_ref_pkg("ref_nn", "nn")
    ref_loss = load_ref_pkg("ref_loss", "loss")
    e2e = ref_loss
    for i, (name, cfg, (n, S)) in enumerate(SMALL):
        sd = tasnet_ref.make_state(cfg, seed=100 + i)
        rng = np.random.default_rng(200 + i)
        x = (0.5 * rng.standard_normal((n, S) if n else (S,))).astype(np.float32)
        m = build(ref_nn, cfg, sd)
        with torch.no_grad():
            out32 = [o.numpy() for o in m([torch.from_numpy(x)])]
            out64 = [o.numpy() for o in m.double()([torch.from_numpy(x).double()])]
        arrays = {"sd__" + k: np.asarray(v) for k, v in sd.items()}
        cfg_arr = {"cfg__" + k: np.asarray(v) for k, v in cfg.items()}
        fn = f"{OUT}/g8_tasnet_{name}.npz"
        np.savez_compressed(fn, x=x, out64=np.stack(out64), out32=np.stack(out32), **arrays, **cfg_arr)
        print("wrote", fn, np.stack(out64).shape, os.path.getsize(fn))
    # recipe configuration: state_dict names and shapes only
    m = ref_nn.ConvTasNet(**tasnet_ref.RECIPE)
    names = list(m.state_dict().keys())
    shapes = np.array([",".join(str(d) for d in v.shape) for v in m.state_dict().values()])
    fn = f"{OUT}/g8_tasnet_recipe_names.npz"
    np.savez_compressed(fn, names=np.array(names), shapes=shapes, n_params=sum(p.numel() for p in m.parameters()))
    print("wrote", fn, len(names))
    # losses: values and the gradient of si_snr_loss
    rng = np.random.default_rng(7)
    N, S, spk = 3, 400, 2
    refs = rng.standard_normal((spk, N, S))
    ests = 0.6 * refs[::-1] + 0.4 * rng.standard_normal((spk, N, S))
    ests[:, 1] = 0.7 * refs[:, 1] + 0.3 * rng.standard_normal((spk, S))     # utterance 1 prefers the identity permutation
    ests_t = [torch.tensor(e, requires_grad=True) for e in ests]
    refs_t = [torch.tensor(r) for r in refs]
    loss = e2e.si_snr_loss(ests_t, refs_t)
    loss.backward()
    vals = dict(
        si_snr=np.array([float(e2e.SI_SNR(torch.tensor(ests[0, 0]), torch.tensor(refs[0, 0])))]),
        si_snr_nozm=np.array([float(e2e.SI_SNR(torch.tensor(ests[0, 0]), torch.tensor(refs[0, 0]), zero_mean=False))]),
        permute=np.array([float(e2e.permute_SI_SNR([torch.tensor(ests[s, 0]) for s in range(spk)],
                                                   [torch.tensor(refs[s, 0]) for s in range(spk)]))]),
        sisnr=e2e.sisnr(torch.tensor(ests[0]), torch.tensor(refs[0])).numpy(),
        loss=np.array([float(loss)]), grad=np.stack([e.grad.numpy() for e in ests_t]))
    fn = f"{OUT}/g8_tasnet_loss.npz"
    np.savez_compressed(fn, ests=ests, refs=refs, **vals)
    print("wrote", fn)
    # training: parameter gradients of si_snr_loss through one small model (fp64)
    name, cfg, (n, S) = SMALL[0]
    sd = tasnet_ref.make_state(cfg, seed=100)
    m = ref_nn.ConvTasNet(**cfg)
    m.load_state_dict(to_torch_sd(sd), strict=True)
    m = m.double().train()
    rng = np.random.default_rng(300)
    x = 0.5 * rng.standard_normal((n, S))
    est = m([torch.from_numpy(x)])
    T = (S - cfg["L"]) // (cfg["L"] // 2) + 1
    S_out = (T - 1) * (cfg["L"] // 2) + cfg["L"]
    refs = rng.standard_normal((cfg["num_spks"], n, S_out))
    loss = e2e.si_snr_loss(est, [torch.from_numpy(r) for r in refs])
    loss.backward()
    grads = {"grad__" + k: p.grad.numpy() for k, p in m.named_parameters() if p.grad is not None}
    fn = f"{OUT}/g8_tasnet_train.npz"
    np.savez_compressed(fn, x=x, refs=refs, loss=np.array([float(loss)]), **grads,
                        **{"sd__" + k: np.asarray(v) for k, v in sd.items()}, **{"cfg__" + k: np.asarray(v) for k, v in cfg.items()})
    print("wrote", fn, os.path.getsize(fn))


if __name__ == "__main__":
    main()
