"""ConvTasNet without a GPU: the fp64 restatement (tests/tasnet_ref.py) against the g8 fixtures of the reference, the module's
state_dict surface, the SI-SNR losses, the time-domain loaders and the recipe config."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from onssen_amd import loss as L
from onssen_amd import nn as onn
from tests import tasnet_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLD, "g8_tasnet_*.npz"))
                  if not f.endswith(("_loss.npz", "_train.npz", "_names.npz")))
TD_FO = {"data_path": "synthetic", "batch_size": 3, "sampling_rate": 8000, "chunk_size": 400}


def test_fixture_set_is_complete():
    cfgs = [tasnet_ref.load_fixture(f)[0] for f in FIXTURES]
    assert {c["norm"] for c in cfgs} == {"gln", "cln", "bn"}
    assert {c["activate"] for c in cfgs} == {"relu", "sigmoid", "softmax"}
    assert {c["causal"] for c in cfgs} == {True, False} and {c["num_spks"] for c in cfgs} == {2, 3} and {c["P"] for c in cfgs} == {3, 5}
    shapes = [tasnet_ref.load_fixture(f)[2].shape for f in FIXTURES]
    assert any(len(s) == 1 for s in shapes) and any(len(s) == 2 for s in shapes)
    cfg_of = dict(zip(FIXTURES, cfgs))
    assert any((s[-1] - cfg_of[f]["L"]) % (cfg_of[f]["L"] // 2) for f, s in zip(FIXTURES, shapes))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[10:-4])
def test_ref_reproduces_fixture(path):
    cfg, sd, x, out64, out32 = tasnet_ref.load_fixture(path)
    out = np.stack(tasnet_ref.forward(sd, x, cfg))
    assert out.shape == out64.shape == out32.shape
    assert np.abs(out - out64).max() <= 1e-9 * max(1.0, np.abs(out64).max())
    assert np.abs(out - out32).max() <= 5e-6


def test_recipe_state_dict_names_and_shapes():
    z = np.load(os.path.join(GOLD, "g8_tasnet_recipe_names.npz"))
    m = onn.ConvTasNet(**tasnet_ref.RECIPE)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in z["names"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in z["shapes"]]
    assert sum(p.numel() for p in m.parameters()) == int(z["n_params"]) == 3475121
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in tasnet_ref.state_names(tasnet_ref.RECIPE)]


@pytest.mark.parametrize("path", FIXTURES + [os.path.join(GOLD, "g8_tasnet_train.npz")], ids=lambda p: os.path.basename(p)[10:-4])
def test_fixture_loads_strict_both_ways(path):
    cfg, sd, _, _, _ = tasnet_ref.load_fixture(path)
    m = onn.ConvTasNet(**cfg)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    back = m.state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert np.array_equal(back[k].numpy(), np.asarray(v)), k


def test_aten_forward_matches_fixture_on_cpu(monkeypatch):
    monkeypatch.setenv("ONSSEN_CPU_AUTOGRAD", "1")
    for path in FIXTURES:
        cfg, sd, x, out64, _ = tasnet_ref.load_fixture(path)
        m = onn.ConvTasNet(**cfg)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m.eval()
        xt = torch.from_numpy(x).requires_grad_(True)           # a gradient wanted: the training (ATen) path
        out = np.stack([o.detach().numpy() for o in m([xt])])
        assert out.shape == out64.shape and np.abs(out - out64).max() <= 5e-6


def test_cpu_tensor_raises_without_the_switch(monkeypatch):
    monkeypatch.delenv("ONSSEN_CPU_AUTOGRAD", raising=False)
    from onssen_amd import options
    if options.get("cpu_autograd") == "1":
        pytest.skip("the test session sets ONSSEN_CPU_AUTOGRAD")
    m = onn.ConvTasNet(N=8, L=4, B=4, H=8, P=3, X=1, R=1)
    with pytest.raises(RuntimeError):
        m([torch.zeros(2, 100)])
    m.eval()
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            m([torch.zeros(2, 100)])


def test_three_d_input_raises():
    m = onn.ConvTasNet(N=8, L=4, B=4, H=8, P=3, X=1, R=1)
    with pytest.raises(RuntimeError, match="1/2D"):
        m([torch.zeros(1, 2, 100)])


def test_hip_limits_name_the_limit():
    assert onn.ConvTasNet(**tasnet_ref.RECIPE).hip_limits() == []
    assert any("L = 15" in w for w in onn.ConvTasNet(N=8, L=15, B=4, H=8, X=1, R=1).hip_limits())
    assert any("L = 66" in w for w in onn.ConvTasNet(N=8, L=66, B=4, H=8, X=1, R=1).hip_limits())
    assert any("P = 4" in w for w in onn.ConvTasNet(N=8, L=4, B=4, H=8, P=4, X=1, R=1).hip_limits())
    assert onn.ConvTasNet(N=8, L=4, B=4, H=8, P=4, X=1, R=1, causal=True).hip_limits() == []


def test_exports():
    import onssen_amd.nn as pkg
    assert "ConvTasNet" in pkg.__all__ and pkg.ConvTasNet is onn.ConvTasNet
    for name in ("SI_SNR", "permute_SI_SNR", "sisnr", "si_snr_loss"):
        assert callable(getattr(L, name))


def test_losses_match_fixture():
    z = np.load(os.path.join(GOLD, "g8_tasnet_loss.npz"))
    ests, refs = z["ests"], z["refs"]
    t = torch.from_numpy
    rel = lambda a, b: np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)   # noqa: E731
    assert rel(float(L.SI_SNR(t(ests[0, 0]), t(refs[0, 0]))), z["si_snr"]) <= 1e-6
    assert rel(float(L.SI_SNR(t(ests[0, 0]), t(refs[0, 0]), zero_mean=False)), z["si_snr_nozm"]) <= 1e-6
    assert rel(float(L.permute_SI_SNR([t(ests[s, 0]) for s in range(2)], [t(refs[s, 0]) for s in range(2)])), z["permute"]) <= 1e-6
    assert rel(L.sisnr(t(ests[0]), t(refs[0])).numpy(), z["sisnr"]) <= 1e-6
    e = [t(ests[s].copy()).requires_grad_(True) for s in range(2)]
    loss = L.si_snr_loss(e, [t(refs[s]) for s in range(2)])
    loss.backward()
    assert rel(float(loss.detach()), z["loss"]) <= 1e-6
    assert rel(np.stack([x.grad.numpy() for x in e]), z["grad"]) <= 1e-6
    with pytest.raises(RuntimeError):
        L.sisnr(t(ests[0]), t(refs[0][:, :-1]))


def test_synthetic_time_domain_loader_layouts():
    from onssen_amd.data import SyntheticWsj02mix, wsj0_2mix_dataloader
    for name in ("conv-tasnet", "lstm-tasnet"):
        dl = wsj0_2mix_dataloader(name, TD_FO, "tr", device="cpu")
        assert isinstance(dl, SyntheticWsj02mix)
        batches = list(dl)
        assert len(batches) == len(dl)
        for inp, lab in batches:
            assert len(inp) == 1 and len(lab) == 2
            assert inp[0].shape == lab[0].shape == lab[1].shape == (3, 400) and inp[0].dtype == torch.float32
        again = list(wsj0_2mix_dataloader(name, TD_FO, "tr", device="cpu"))   # seeded crops
        assert all(torch.equal(a[0][0], b[0][0]) for a, b in zip(batches, again))
        padded = [(inp[0][:, -10:] == 0).all(dim=1) for inp, _ in batches]      # utterances shorter than the chunk: zero tail
        assert any(p.any() for p in padded) and any((~p).any() for p in padded)
    tt = list(wsj0_2mix_dataloader("conv-tasnet", TD_FO, "tt", device="cpu"))
    for it, (inp, lab) in enumerate(tt):
        S = 400 + 7 * it
        Sp = S + 32 - S % 32
        assert inp[0].shape == (1, Sp) and lab[0].shape == (1, 2, Sp)
        assert (inp[0][0, S:] == 0).all() and (lab[0][0, :, S:] == 0).all()
    assert tt[0][0][0].shape == (1, 416)                 # 400 % 32 == 16 -> 16 samples of padding


def test_time_domain_helpers_crop_pad_and_pad32():
    from onssen_amd.data import time_domain as td
    rng = np.random.default_rng(0)
    a = np.arange(10, dtype=np.float32)
    c = td.crop_or_pad([a, a + 100, a + 200], 4, rng)
    assert len(c[0]) == 4 and np.array_equal(c[1] - 100, c[0]) and np.array_equal(c[2] - 200, c[0]) and c[0][1] == c[0][0] + 1
    p = td.crop_or_pad([a[:3]] * 3, 5, rng)
    assert np.array_equal(p[0], [0, 1, 2, 0, 0])
    inp, lab = td.eval_item(np.ones(64, np.float32), np.ones(64, np.float32), np.ones(64, np.float32), "cpu")
    assert inp[0].shape == (1, 96) and lab[0].shape == (1, 2, 96)      # S % 32 == 0: a full 32 samples of padding
    with pytest.raises(ValueError, match="chunk_size"):
        td.options_of("conv-tasnet", {"batch_size": 2, "sampling_rate": 8000})


def _corpus(root, part, lengths):
    from onssen_amd.data import write_wav
    rng = np.random.default_rng(3)
    sigs = []
    for i, n in enumerate(lengths):
        trip = [(0.3 * rng.standard_normal(n)).astype(np.float32) for _ in range(3)]
        for d, s in zip(("mix", "s1", "s2"), trip):
            os.makedirs(os.path.join(root, "wav8k", "min", part, d), exist_ok=True)
            write_wav(os.path.join(root, "wav8k", "min", part, d, f"u{i}.wav"), s, 8000, subtype="FLOAT")
        sigs.append(trip)
    return sigs


def test_file_time_domain_loader_layouts(tmp_path):
    from onssen_amd.data import Wsj02mixFiles, wsj0_2mix_dataloader
    fo = dict(TD_FO, data_path=str(tmp_path), batch_size=2)
    sigs = _corpus(str(tmp_path), "tr", [500, 300, 450])
    dl = wsj0_2mix_dataloader("conv-tasnet", fo, "tr", device="cpu")
    assert isinstance(dl, Wsj02mixFiles) and len(dl) == 2
    dl = Wsj02mixFiles("conv-tasnet", fo, "tr", device="cpu", shuffle=False, seed=4)
    batches = list(dl)
    assert [b[0][0].shape for b in batches] == [(2, 400), (1, 400)]
    rng = np.random.default_rng(4)                          # the crops the seeded generator draws, in file order
    start0 = int(rng.integers(0, 500 - 400 + 1))
    np.testing.assert_allclose(batches[0][0][0][0].numpy(), sigs[0][0][start0:start0 + 400], atol=1e-7)
    np.testing.assert_allclose(batches[0][1][1][0].numpy(), sigs[0][2][start0:start0 + 400], atol=1e-7)
    np.testing.assert_allclose(batches[0][0][0][1, :300].numpy(), sigs[1][0], atol=1e-7)
    assert (batches[0][0][0][1, 300:] == 0).all()
    _corpus(str(tmp_path), "tt", [320, 333])
    tt = list(Wsj02mixFiles("lstm-tasnet", fo, "tt", device="cpu"))
    assert [(i[0].shape, l[0].shape) for i, l in tt] == [((1, 352), (1, 2, 352)), ((1, 352), (1, 2, 352))]
    with pytest.raises(ValueError, match="chunk_size"):
        Wsj02mixFiles("conv-tasnet", {k: v for k, v in fo.items() if k != "chunk_size"}, "tr")


def test_recipe_config_builds_model_and_loaders():
    from onssen_amd import options
    from onssen_amd.data import wsj0_2mix_dataloader
    with open(os.path.join(GOLD, "config_conv_tasnet.json")) as f:
        args = json.load(f)
    assert args["model_name"] == "conv-tasnet"
    kwargs = options.split_model_options(args["model_options"])[0]
    m = onn.ConvTasNet(**kwargs)
    assert sum(p.numel() for p in m.parameters()) == 3475121 and m.activation_type == "sigmoid"
    fo = dict(args["feature_options"], data_path="synthetic")
    for part in ("tr", "cv"):
        dl = wsj0_2mix_dataloader(args["model_name"], fo, part, device="cpu")
        inp, lab = next(iter(dl))
        assert inp[0].shape == (3, 32000) and lab[1].shape == (3, 32000)
