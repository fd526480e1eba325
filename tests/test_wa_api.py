"""The public surface of waveform-approximation training without a GPU: names, signatures, argument errors, loader names."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FO = dict(batch_size=2, frame_length=40, sampling_rate=8000, window_size=256, hop_size=64, db_threshold=40.0)


def test_exports_and_abi():
    from onssen_amd import _abi, features, loss
    assert _abi.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "onssen_hip.h")).read()
    for name, n_args in (("onssen_istft_backward_f32", 21), ("onssen_wa_pit_workspace_bytes", 2), ("onssen_wa_pit_f32", 14),
                         ("onssen_wa_pit_backward_f32", 14)):
        assert name in _abi.SIGNATURES, name
        assert len(_abi.SIGNATURES[name][1]) == n_args, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\s*\(([^;]*?)\)\s*;", header, re.S | re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name      # the header agrees
    for f in ("istft_backward", "wa_pit_workspace_bytes", "wa_pit", "wa_pit_backward"):
        assert callable(getattr(_abi.Lib, f)), f
    par = lambda f: inspect.signature(f).parameters
    assert list(par(loss.wa_pit)) == ["est", "ref", "lengths", "return_perm"]
    assert list(par(loss.loss_wa))[:5] == ["output", "label", "hop_size", "frames", "lengths"]
    assert par(loss.loss_wa)["hop_size"].default == 64 and par(loss.loss_wa)["misi_iters"].default == 0
    assert par(loss.loss_wa)["kind"].default == "chimera" and loss.WA_KINDS == ("chimera", "upit", "phase", "enhance")
    assert issubclass(features._IstftGrad, torch.autograd.Function) and issubclass(loss._WaPitHip, torch.autograd.Function)


def _chimera_io(B=1, T=13, F=129, n=768, C=2):
    out = [torch.zeros(B, T, F, 20)] + [torch.zeros(B, T, F) for _ in range(C)]
    return out, [torch.zeros(B, T, F, 2), torch.zeros(B, C, n)]


@pytest.mark.parametrize("iters", [1, -1, 3])
def test_misi_iterations_are_not_built(iters):
    from onssen_amd.loss import loss_wa
    out, lab = _chimera_io()
    with pytest.raises(NotImplementedError, match="adjoint of misi_phase"):
        loss_wa(out, lab, misi_iters=iters)


def test_the_mixture_is_data():
    from onssen_amd.loss import loss_wa
    out, lab = _chimera_io()
    lab[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="spectrum is data"):
        loss_wa(out, lab)


def test_mismatched_shapes():
    from onssen_amd.loss import loss_wa, wa_pit
    out, lab = _chimera_io()
    with pytest.raises(ValueError, match="2 output tensors for kind 'chimera'"):
        loss_wa(out[:2], lab)
    with pytest.raises(ValueError, match="label tensors"):
        loss_wa(out, lab + lab[:1])
    with pytest.raises(ValueError, match="sig_ref"):
        loss_wa(out, [lab[0], torch.zeros(1, 3, 768)])
    with pytest.raises(ValueError, match="sig_ref"):
        loss_wa(out, [lab[0], torch.zeros(2, 2, 768)])
    with pytest.raises(ValueError, match="an output of shape"):
        loss_wa([out[0], out[1], torch.zeros(1, 13, 128)], lab)
    with pytest.raises(ValueError, match="expected stft_ri_mix"):
        loss_wa(out, [torch.zeros(1, 13, 129), lab[1]])
    with pytest.raises(ValueError, match="unknown kind"):
        loss_wa(out, lab, kind="dc")
    with pytest.raises(ValueError, match="1 output tensors|3 output tensors"):
        loss_wa(out, lab, kind="enhance")
    with pytest.raises(ValueError, match="a phase map of shape"):
        loss_wa(out + [torch.zeros(1, 13, 129), torch.zeros(1, 13, 129)], lab, kind="phase")
    with pytest.raises(ValueError, match="both frames= and lengths="):
        loss_wa(out, lab, frames=[13])
    with pytest.raises(ValueError, match="one shape"):
        wa_pit(torch.zeros(2, 2, 100), torch.zeros(2, 2, 99))
    with pytest.raises(ValueError, match="5 speakers"):
        wa_pit(torch.zeros(2, 5, 100), torch.zeros(2, 5, 100))
    with pytest.raises(RuntimeError, match="ROCm device"):
        wa_pit(torch.zeros(2, 2, 100), torch.zeros(2, 2, 100))
    with pytest.raises(RuntimeError, match="reference requires a gradient"):
        wa_pit(torch.zeros(2, 2, 100), torch.zeros(2, 2, 100, requires_grad=True))


def test_inverse_transforms_refuse_a_spectrum_that_requires_grad():
    from onssen_amd import features
    ri = torch.zeros(1, 13, 129, 2, requires_grad=True)
    m = torch.zeros(1, 13, 129, 2)
    # (CPU tensors are refused first, as before: the device check is the first thing each of them does)
    for call in (lambda: features.mask_istft(ri, m), lambda: features.mag_istft(ri, m), lambda: features.phase_istft(ri, m, [ri, ri])):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


def test_loader_names(tmp_path):
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.data.wsj0_2mix import Wsj02mixFiles
    for name in ("chimera-wa", "upit-wa"):
        assert SyntheticWsj02mix(name, FO, "tr", device="cpu").num_speaker == 2
        assert SyntheticWsj02mix(name, FO, "tt", device="cpu").model_name == name
        assert Wsj02mixFiles(name, dict(FO, data_path=str(tmp_path)), "tr", device="cpu").model_name == name
    assert SyntheticWsj02mix("upit-wa", dict(FO, num_speaker=3), "tr", device="cpu").num_speaker == 3
    assert SyntheticWsj02mix("chimera-wa", dict(FO, num_speaker=3), "tr", device="cpu").num_speaker == 2
    with pytest.raises(ValueError, match="num_speaker"):
        SyntheticWsj02mix("upit-wa", dict(FO, num_speaker=5), "tr", device="cpu")
    with pytest.raises(ValueError, match="two speakers"):
        Wsj02mixFiles("upit-wa", dict(FO, data_path=str(tmp_path), num_speaker=3), "tr", device="cpu")
    with pytest.raises(ValueError, match="unknown model_name"):
        Wsj02mixFiles("chimera-wb", dict(FO, data_path=str(tmp_path)), "tr", device="cpu")
