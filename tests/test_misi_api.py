"""MISI's public surface without a GPU: names, signatures, argument errors, and the float64 restatement (tests/misi_ref.py) doing
what MISI is for -- more SI-SDR at every iteration on oracle magnitudes."""
import inspect

import numpy as np
import pytest
import torch

from tests import misi_cases as MC
from tests import misi_ref as R


def test_exports_and_abi():
    from onssen_amd import _abi, evaluate, features, separation
    assert _abi.ABI_VERSION == 14
    for name in ("onssen_misi_phase_f32", "onssen_misi_phase_ragged_f32", "onssen_phase_istft_ragged_f32"):
        assert name in _abi.SIGNATURES, name
    assert len(_abi.SIGNATURES["onssen_misi_phase_f32"][1]) == 12
    assert len(_abi.SIGNATURES["onssen_misi_phase_ragged_f32"][1]) == 13
    assert len(_abi.SIGNATURES["onssen_phase_istft_ragged_f32"][1]) == len(_abi.SIGNATURES["onssen_phase_istft_f32"][1]) + 2
    assert callable(features.misi_phase) and callable(separation.misi) and callable(_abi.Lib.misi_phase)
    par = lambda f: inspect.signature(f).parameters
    assert list(par(features.misi_phase))[:5] == ["mix", "est", "window_size", "hop_size", "lengths"]
    assert par(features.phase_istft)["frames"].default is None and par(features.phase_istft)["lengths"].default is None
    assert list(par(separation.misi)) == ["stft_ri", "masks", "wav", "iters", "hop_size", "frames", "lengths", "phases"]
    assert par(separation.misi)["hop_size"].default == 64
    for f in (separation.separate_chimera, separation.separate_upit, separation.separate_phase, evaluate.tester_chimera.__init__,
              evaluate.tester_upit.__init__):
        assert par(f)["misi_iters"].default == 0, f


@pytest.mark.parametrize("iters", [-1, 1.5, "2", None])
def test_bad_iteration_counts(iters):
    from onssen_amd.evaluate import tester_chimera, tester_upit
    from onssen_amd.separation import misi, separate_chimera, separate_phase, separate_upit
    z = torch.zeros(1, 13, 129, 2)
    with pytest.raises(ValueError, match="non-negative integer"):
        misi(z, z, torch.zeros(1, 768), iters)
    for sep in (separate_chimera, separate_upit, separate_phase):
        with pytest.raises(ValueError, match="non-negative integer"):
            sep(None, torch.zeros(1, 768), misi_iters=iters)
    for t in (tester_chimera, tester_upit):
        with pytest.raises(ValueError, match="non-negative integer"):
            t(dict(model=torch.nn.Identity(), device="cpu"), misi_iters=iters)


def test_frames_without_lengths():
    from onssen_amd.features import phase_istft
    from onssen_amd.separation import misi
    z = torch.zeros(1, 13, 129, 2)
    with pytest.raises(ValueError, match="both frames= and lengths="):
        misi(z, z, torch.zeros(1, 768), 1, frames=[13])
    with pytest.raises(ValueError, match="both frames= and lengths="):
        misi(z, z, torch.zeros(1, 768), 1, lengths=[768])
    with pytest.raises(ValueError, match="both frames= and lengths="):
        phase_istft(z, z, [z, z], frames=[13])


def test_cpu_tensors_are_refused():
    from onssen_amd.features import misi_phase, phase_istft
    from onssen_amd.separation import misi
    z = torch.zeros(1, 13, 129, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        misi_phase(torch.zeros(1, 768), torch.zeros(1, 2, 768))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        misi(z, z, torch.zeros(1, 768), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        phase_istft(z, z, [z, z], frames=[13], lengths=[768])


def reference_gains(n_fft, hop, n, C, K=3):
    """Mean SI-SDR (dB) over utterances and speakers after 0 .. K reference iterations on oracle magnitudes, mixture phase."""
    k = MC.oracle_case(n_fft, hop, n, C)
    means = np.zeros(K + 1)
    for b in range(k.B):
        mag = np.stack([np.abs(MC.O.stft(k.src[b, c], n_fft, hop)) for c in range(C)]).astype(np.float64)
        p0 = R.unit(k.X[b].astype(np.complex128))
        ests = R.misi(mag, np.stack([p0[..., 0] + 1j * p0[..., 1]] * C), k.mix[b], hop, K)
        for i, e in enumerate(ests):
            means[i] += np.mean([R.si_sdr(e[c], k.src[b, c]) for c in range(C)]) / k.B
    return means


@pytest.mark.parametrize("n_fft,hop,n,C", MC.SHAPES)
def test_reference_gains_si_sdr_at_every_iteration(n_fft, hop, n, C):
    means = reference_gains(n_fft, hop, n, C)
    print(f"n_fft {n_fft} hop {hop} n {n} C {C}: mean SI-SDR at K = 0..3 {np.round(means, 2)} dB")
    assert (np.diff(means) > 0).all(), means
    assert means[3] - means[0] >= 1.0, means
