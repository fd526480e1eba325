"""The public surface of unfolded-MISI training without a GPU: names, signatures, argument errors, and the float64 adjoint of
tests/misi_grad_ref.py against torch autograd."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_abi():
    from onssen_amd import _abi, features, loss
    assert _abi.ABI_VERSION == 14                     # additive: the version stays
    header = open(os.path.join(ROOT, "include", "onssen_hip.h")).read()
    for name, n_args in (("onssen_misi_phase_backward_workspace_bytes", 5), ("onssen_misi_phase_backward_f32", 16)):
        assert name in _abi.SIGNATURES, name
        assert len(_abi.SIGNATURES[name][1]) == n_args, name
        decl = re.search(r"^(?:int|size_t) " + name + r"\s*\(([^;]*?)\)\s*;", header, re.S | re.M)
        assert decl is not None and len(decl.group(1).split(",")) == n_args, name      # the header agrees
    for f in ("misi_phase_backward_workspace_bytes", "misi_phase_backward"):
        assert callable(getattr(_abi.Lib, f)), f
    par = lambda f: inspect.signature(f).parameters
    assert list(par(loss.loss_wa_misi)) == ["output", "label", "iters", "hop_size", "frames", "lengths", "kind"]
    assert par(loss.loss_wa_misi)["hop_size"].default == 64 and par(loss.loss_wa_misi)["kind"].default == "chimera"
    assert par(loss.loss_wa_misi)["iters"].default is inspect.Parameter.empty
    assert list(par(features.misi_phase)) == ["mix", "est", "window_size", "hop_size", "lengths", "out"]
    assert issubclass(features._MisiPhaseGrad, torch.autograd.Function)


def _chimera_io(B=1, T=13, F=129, n=768, C=2):
    out = [torch.zeros(B, T, F, 20)] + [torch.zeros(B, T, F) for _ in range(C)]
    return out, [torch.zeros(B, T, F, 2), torch.zeros(B, C, n)]


def test_loss_wa_points_to_loss_wa_misi():
    from onssen_amd.loss import loss_wa
    out, lab = _chimera_io()
    with pytest.raises(NotImplementedError, match="adjoint of misi_phase.*loss_wa_misi"):
        loss_wa(out, lab, misi_iters=2)


def test_loss_wa_misi_argument_errors():
    from onssen_amd.loss import loss_wa_misi
    out, lab = _chimera_io()
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="non-negative integer"):
            loss_wa_misi(out, lab, bad)
    with pytest.raises(ValueError, match="nothing to redistribute"):
        loss_wa_misi(out[1:2], [lab[0], lab[1][:, :1]], 1, kind="enhance")
    with pytest.raises(ValueError, match="unknown kind"):
        loss_wa_misi(out, lab, 1, kind="dc")
    with pytest.raises(ValueError, match="2 output tensors for kind 'chimera'"):
        loss_wa_misi(out[:2], lab, 1)
    with pytest.raises(ValueError, match="label tensors"):
        loss_wa_misi(out, lab + lab[:1], 1)
    with pytest.raises(ValueError, match="sig_ref"):
        loss_wa_misi(out, [lab[0], torch.zeros(1, 3, 768)], 1)
    with pytest.raises(ValueError, match="an output of shape"):
        loss_wa_misi([out[0], out[1], torch.zeros(1, 13, 128)], lab, 1)
    with pytest.raises(ValueError, match="a phase map of shape"):
        loss_wa_misi(out + [torch.zeros(1, 13, 129), torch.zeros(1, 13, 129)], lab, 1, kind="phase")
    with pytest.raises(ValueError, match="both frames= and lengths="):
        loss_wa_misi(out, lab, 1, frames=[13])
    lab[0].requires_grad_(True)
    with pytest.raises(RuntimeError, match="spectrum is data"):
        loss_wa_misi(out, lab, 1)


def test_misi_phase_argument_errors():
    from onssen_amd import features
    mix, est = torch.zeros(1, 768), torch.zeros(1, 2, 768)
    with pytest.raises(RuntimeError, match="the mixture is data"):
        features.misi_phase(mix.clone().requires_grad_(True), est)
    with pytest.raises(ValueError, match="out= cannot be combined"):
        features.misi_phase(mix, est.clone().requires_grad_(True), out=torch.zeros(2, 1, 13, 129, 2))
    with pytest.raises(RuntimeError, match="ROCm device"):          # no CPU route, with or without a gradient
        features.misi_phase(mix, est.clone().requires_grad_(True))
    with torch.no_grad():                                           # nothing changes without autograd
        with pytest.raises(RuntimeError, match="ROCm device"):
            features.misi_phase(mix.clone().requires_grad_(True), est)


def test_the_fp64_adjoint_agrees_with_autograd():
    from tests import misi_grad_ref as G
    worst = G.self_check()
    print(f"half-step adjoint against torch float64 autograd: largest relative difference {worst:.3e} (bound 1e-10)")
    assert worst <= 1e-10


def test_the_bounds_are_the_measured_values_times_four():
    from tests import misi_grad_ref as G
    assert G.GRAD_REL_BOUND == 4 * G.GRAD_MEASURED_REL <= 1e-5 and G.CHAIN_REL_BOUND == 4 * G.CHAIN_MEASURED_REL <= 1e-4
    assert (256, 64, 129, 2) in G.SHAPES and (256, 64, 777, 5) in G.SHAPES
