"""The uPIT surface that needs no GPU: the model's parameters, the PyTorch-ops route of the two losses, the synthetic mixtures for
S speakers and the loader's argument checks."""
import os

import numpy as np
import pytest
import torch

from tests import upit_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_model_is_exported_with_the_reference_parameter_names():
    from onssen_amd import nn as onn
    from onssen_amd.synthetic import make_state_dict
    assert "uPIT_LSTM" in onn.__all__
    for S in (2, 3):
        fx = np.load(os.path.join(GOLDEN, f"g10_upit_H16_L2_S{S}.npz"))
        assert str(fx["kind"]) == "upit" and int(fx["C"]) == S
        F, H, L = int(fx["F"]), int(fx["H"]), int(fx["L"])
        sd = make_state_dict("upit", F, H, L, 20, S, seed=int(fx["seed"]), gain=float(fx["gain"]))
        m = onn.uPIT_LSTM(F, F, H, 20, L, num_speaker=S)
        own = m.state_dict()
        assert list(own) == list(sd)
        assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in sd.items()}
        assert sd["fc_mi.weight"].shape == (F * S, 2 * H)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        assert fx["mask_A"].shape == fx["mask_B"].shape == fx["x"].shape == (2, 12, 129)


def test_upit_kind_leaves_the_other_kinds_draws_alone():
    from onssen_amd.synthetic import make_state_dict
    a, u = make_state_dict("chimera", 9, 4, 1, 5, 2, seed=3), make_state_dict("upit", 9, 4, 1, 5, 2, seed=3)
    for k in u:
        if k.startswith("rnn."):
            assert u[k].tobytes() == a[k].tobytes()       # the same generator, the same order: rnn first in both


def test_cpu_forward_raises_without_the_scaffolding_switch(monkeypatch):
    from onssen_amd import nn as onn
    m = onn.uPIT_LSTM(129, 129, 8, num_layers=1, dropout=0.0, num_speaker=3)
    x = torch.randn(2, 5, 129)
    monkeypatch.setenv("ONSSEN_CPU_AUTOGRAD", "0")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train()([x])
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            m.eval()([x])
    monkeypatch.setenv("ONSSEN_CPU_AUTOGRAD", "1")
    out = m.train()([x])
    assert len(out) == 3 and all(o.shape == (2, 5, 129) for o in out)
    assert all(o._base is out[0]._base and o.stride() == (5 * 129 * 3, 129 * 3, 3) for o in out)
    with pytest.raises(RuntimeError, match="inference-path extension"):
        m([x], frames=[5, 3])


def _case(S, psa, TF=387, seed=5):
    c = R.loss_case(S, TF, seed, psa)
    t = lambda a: torch.from_numpy(np.array(a))
    masks = [t(c["masks"][k]).view(-1, 3, TF // 3) for k in range(S)]
    label = [t(c["x"]).view(-1, 3, TF // 3)] + [t(c["src"][j]).view(-1, 3, TF // 3) for j in range(S)]
    if psa:
        label += [t(c["cos"][j]).view(-1, 3, TF // 3) for j in range(S)]
    return c, masks, label


@pytest.mark.parametrize("psa", [False, True])
@pytest.mark.parametrize("S", [2, 3, 4, 5])
def test_cpu_route_is_aten_and_matches_the_reference(S, psa):
    from onssen_amd import loss
    if S == 5:                  # beyond the kernels' four speakers: random maps, the restatement against itself
        rng = np.random.default_rng(9)
        c = dict(masks=rng.random((5, 2, 12)).astype(np.float32), x=rng.random((2, 12)).astype(np.float32) + 0.1,
                 src=rng.random((5, 2, 12)).astype(np.float32), cos=rng.uniform(-1, 1, (5, 2, 12)).astype(np.float32) if psa else None)
        masks = [torch.from_numpy(m).view(2, 3, 4) for m in c["masks"]]
        label = ([torch.from_numpy(c["x"]).view(2, 3, 4)] + [torch.from_numpy(s).view(2, 3, 4) for s in c["src"]]
                 + ([torch.from_numpy(q).view(2, 3, 4) for q in c["cos"]] if psa else []))
    else:
        c, masks, label = _case(S, psa)
    fn = loss.loss_upit_psa if psa else loss.loss_upit_msa
    out, perm = fn(masks, label, return_perm=True)
    assert loss.last_upit_path == "aten" and out.shape == (len(out),) and perm.dtype == torch.int64
    ref_out, ref_perm = R.best(R.pair_matrix(c["masks"], c["x"], c["src"], c["cos"]))
    np.testing.assert_allclose(out.numpy(), ref_out, rtol=2e-5)
    if S < 5:
        assert (perm.numpy() == ref_perm).all() and (ref_perm == np.arange(len(ref_perm))).all()
    if S == 2:                  # the chimera mask term, exactly
        x, s1, s2 = label[0], label[1], label[2]
        if psa:
            s1, s2 = torch.min(x, torch.relu(s1 * label[3])), torch.min(x, torch.relu(s2 * label[4]))
        assert torch.equal(out, loss._mask_term(masks[0], masks[1], x, s1, s2))
    # gradients through autograd: x sign(m_k x - t_p[k]) per bin, for the sum of the rows
    leaves = [m.clone().requires_grad_(True) for m in masks]
    fn(leaves, label).sum().backward()
    assert loss.last_upit_path == "aten"
    sign = R.grad_sign(c["masks"], c["x"], c["src"], c["cos"], perm.numpy())
    for k, m in enumerate(leaves):
        np.testing.assert_array_equal(m.grad.reshape(sign[k].shape).numpy(), (c["x"] * sign[k]).astype(np.float32))


def test_wrong_label_counts_raise_and_name_both_counts():
    from onssen_amd import loss
    _, masks, label = _case(3, True)
    with pytest.raises(ValueError, match=r"6 label tensors for 3 masks.*take 7"):
        loss.loss_upit_psa(masks, label[:6])
    with pytest.raises(ValueError, match=r"7 label tensors for 3 masks.*take 4"):
        loss.loss_upit_msa(masks, label)
    with pytest.raises(ValueError, match=r"4 label tensors for 2 masks.*take 3"):
        loss.loss_upit_msa(masks[:2], label[:4])


def test_synth_mixture_k():
    from onssen_amd.synthetic import synth_mixture, synth_mixture_k
    two, ref = synth_mixture_k(77, 4000, 8000, 2), synth_mixture(77, 4000, 8000, return_sources=True)
    assert len(two) == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(two, ref))
    mix, *srcs = synth_mixture_k(77, 4000, 8000, 3)
    assert len(srcs) == 3 and all(s.dtype == np.float32 and s.shape == (4000,) for s in [mix] + srcs)
    assert abs(np.abs(mix).max() - 0.9) < 1e-6
    noise = mix.astype(np.float64) - sum(s.astype(np.float64) for s in srcs)
    clean = sum(s.astype(np.float64) for s in srcs)
    assert 0.005 < noise.std() / clean.std() < 0.02                   # the 1e-2 noise floor, not a fourth voice
    lev = [20 * np.log10(s.std() / srcs[0].std()) for s in srcs[1:]]
    assert all(abs(v) <= 2.5 + 1e-3 for v in lev)
    with pytest.raises(ValueError):
        synth_mixture_k(1, 100, 8000, 1)


def test_loaders_check_num_speaker():
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.data.wsj0_2mix import Wsj02mixFiles
    fo = dict(batch_size=2, frame_length=20, sampling_rate=8000, window_size=256, hop_size=64, db_threshold=40)
    for bad in (5, 1, "3", True):
        with pytest.raises(ValueError, match="num_speaker"):
            SyntheticWsj02mix("upit", dict(fo, num_speaker=bad), "tr", "cpu")
    assert SyntheticWsj02mix("upit", fo, "tr", "cpu").num_speaker == 2
    assert SyntheticWsj02mix("upit-psa", dict(fo, num_speaker=4), "tr", "cpu").num_speaker == 4
    with pytest.raises(ValueError, match="num_speaker"):
        Wsj02mixFiles("upit", dict(fo, num_speaker=3, data_path="/nonexistent"), "tr", "cpu")
    assert Wsj02mixFiles("upit-psa", dict(fo, data_path="/nonexistent"), "tr", "cpu").file_list == []
