"""MISI on the device: the half-step kernel and the ragged phase-aware iSTFT against tests/misi_ref.py at the shapes and with the
bounds of tests/test_emu_misi.py, the driver ``separation.misi`` (its parts, a graph capture, its effect on SI-SDR), and the
switches on the separators and testers."""
import numpy as np
import pytest
import torch

from tests import misi_cases as MC
from tests import misi_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def to(dev, a):
    return torch.from_numpy(np.array(a)).to(dev)


# ------------------------------------------------------------------------------------------------- (a) the half-step
@pytest.mark.parametrize("n_fft,hop,n,C", MC.SHAPES)
def test_misi_phase_matches_fp64_reference(dev, n_fft, hop, n, C):
    from onssen_amd.features import misi_phase
    k = MC.case(n_fft, hop, n, C)
    got = misi_phase(to(dev, k.mix), to(dev, k.est), n_fft, hop)
    assert tuple(got.shape) == (C, k.B, k.T, k.F, 2) and got.dtype == torch.float32
    MC.check_phase(got.cpu().numpy(), MC.reference_spectra(k), f"n_fft {n_fft} hop {hop} n {n} C {C}")


def test_misi_phase_reads_strided_estimates_in_place(dev):
    """Five speakers (the 8-estimate instantiation) in a larger buffer with NaN around them: the same bytes as from a compact copy."""
    from onssen_amd.features import misi_phase
    k = MC.case(256, 64, 768, 2)
    rng = np.random.default_rng(5)
    big = torch.full((2, 6, 800), float("nan"), device=dev)
    big[:, :5, :768] = to(dev, (0.2 * rng.standard_normal((2, 5, 768))).astype(np.float32))
    est = big[:, :5, :768]
    got = misi_phase(to(dev, k.mix), est, 256, 64)
    assert torch.isfinite(got).all()
    assert torch.equal(got, misi_phase(to(dev, k.mix), est.contiguous(), 256, 64))
    Z = np.stack([R.misi_spectra(k.mix[b], est[b].cpu().numpy(), 256, 64) for b in range(2)])
    MC.check_phase(got.cpu().numpy(), Z, "C 5, strided")


# ------------------------------------------------------------------------------------------------- (c) ragged batches
RAG_LENGTHS = (1500, 1100, 700)


def test_ragged_rows_are_their_batch1_bytes(dev):
    from onssen_amd.features import misi_phase, phase_istft
    k = MC.case(256, 100, 1500, 3, B=3)
    mix, est = k.mix.copy(), k.est.copy()
    for b, nb in enumerate(RAG_LENGTHS):          # nothing beyond a row's own length may be read
        mix[b, nb:] = np.nan
        est[b, :, nb:] = np.nan
    mix, est = to(dev, mix), to(dev, est)
    got = misi_phase(mix, est, 256, 100, lengths=RAG_LENGTHS)
    assert torch.isfinite(got).all()
    frames = [1 + nb // 100 for nb in RAG_LENGTHS]
    for b, (Tb, nb) in enumerate(zip(frames, RAG_LENGTHS)):
        one = misi_phase(mix[b:b + 1, :nb], est[b:b + 1, :, :nb], 256, 100)
        assert torch.equal(got[:, b, :Tb], one[:, 0]), b
        assert (got[:, b, Tb:, :, 0] == 1).all() and (got[:, b, Tb:, :, 1] == 0).all(), b
    # the ragged phase-aware iSTFT on those phases, NaN in every input after a row's own frames
    ri, masks, ph = k.ri.copy(), k.masks.copy(), got.clone()
    for b, Tb in enumerate(frames):
        ri[b, Tb:] = np.nan
        masks[b, Tb:] = np.nan
        ph[:, b, Tb:] = float("nan")
    ri, masks = to(dev, ri), to(dev, masks)
    out = phase_istft(ri, masks, ph, 100, 1500, frames=frames, lengths=RAG_LENGTHS)
    for b, (Tb, nb) in enumerate(zip(frames, RAG_LENGTHS)):
        one = phase_istft(ri[b:b + 1, :Tb], masks[b:b + 1, :Tb], ph[:, b:b + 1, :Tb], 100, nb)
        assert torch.isfinite(one).all()
        assert torch.equal(out[b, :, :nb], one[0]), b
        assert (out[b, :, nb:] == 0).all(), b


# ------------------------------------------------------------------------------------------------- (d) whole iterations
def reference_iterations(k, K):
    X = k.ri[..., 0].astype(np.float64) + 1j * k.ri[..., 1].astype(np.float64)
    out = []
    for b in range(k.B):
        mag = np.moveaxis(k.masks[b].astype(np.float64), -1, 0) * np.abs(X[b])[None]
        p0 = R.unit(X[b])
        out.append(R.misi(mag, np.stack([p0[..., 0] + 1j * p0[..., 1]] * k.C), k.mix[b], k.hop, K)[-1])
    return np.stack(out)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n_fft,hop,n,C", MC.SHAPES)
def test_whole_iterations_match_fp64_reference(dev, n_fft, hop, n, C, K):
    """``separation.misi`` against the float64 restatement with the bound measured on the host-side build
    (tests/test_emu_misi.py::test_whole_iterations_match_fp64_reference): MC.ITER_BOUND = 4 x 1.118e-07."""
    from onssen_amd.separation import misi
    k = MC.case(n_fft, hop, n, C)
    out = misi(to(dev, k.ri), to(dev, k.masks), to(dev, k.mix), K, hop).cpu().numpy()
    ref = reference_iterations(k, K)
    err, top = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"n_fft {n_fft} hop {hop} n {n} C {C} K {K}: max |out - ref| {err:.3e}, max |ref| {top:.3f}, bound {MC.ITER_BOUND:.3e}")
    assert np.isfinite(out).all()
    assert err <= 1e-4 * top
    assert err <= MC.ITER_BOUND


# ------------------------------------------------------------------------------------------------- the driver
def test_misi_is_the_sequence_of_its_public_parts(dev):
    from onssen_amd.features import mask_istft, misi_phase, phase_istft
    from onssen_amd.separation import misi
    k = MC.case(256, 100, 1500, 3)
    ri, masks, mix = to(dev, k.ri), to(dev, k.masks), to(dev, k.mix)
    plain = mask_istft(ri, masks, 100, k.n)
    assert torch.equal(misi(ri, masks, mix, 0, 100), plain)
    est = plain
    for _ in range(2):
        est = phase_istft(ri, masks, misi_phase(mix, est, 256, 100), 100, k.n)
    assert torch.equal(misi(ri, masks, mix, 2, 100), est)
    assert not torch.equal(est, plain)
    # from given phases: iters = 0 is phase_istft
    rng = np.random.default_rng(3)
    p = rng.standard_normal((3, k.B, k.T, k.F, 2))
    ph = to(dev, (p / np.linalg.norm(p, axis=-1, keepdims=True)).astype(np.float32))
    start = phase_istft(ri, masks, ph, 100, k.n)
    assert torch.equal(misi(ri, masks, mix, 0, 100, phases=ph), start)
    step = phase_istft(ri, masks, misi_phase(mix, start, 256, 100), 100, k.n)
    assert torch.equal(misi(ri, masks, mix, 1, 100, phases=list(ph.unbind(0))), step)
    # a ragged batch: rows are their batch-1 calls
    lengths = [1500, 1100]
    frames = [1 + nb // 100 for nb in lengths]
    rag = misi(ri, masks, mix, 2, 100, frames=frames, lengths=lengths)
    one = misi(ri[1:, :frames[1]], masks[1:, :frames[1]], mix[1:, :1100], 2, 100)
    assert torch.equal(rag[1, :, :1100], one[0]) and (rag[1, :, 1100:] == 0).all()


def test_misi_in_a_graph(dev):
    from onssen_amd.separation import misi
    k = MC.case(256, 64, 2000, 4)
    ri, masks, mix = to(dev, k.ri), to(dev, k.masks), to(dev, k.mix)
    eager = misi(ri, masks, mix, 2)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        misi(ri, masks, mix, 2)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = misi(ri, masks, mix, 2)
    for _ in range(2):
        captured.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, eager)


def test_misi_gains_si_sdr_on_oracle_magnitudes(dev):
    from onssen_amd.evaluate import batch_SDR_torch
    from onssen_amd.separation import misi
    n_fft, hop, n, C = MC.EFFECT_SHAPE
    k = MC.oracle_case(n_fft, hop, n, C)
    ri, ratio, mix, src = to(dev, k.ri), to(dev, k.ratio), to(dev, k.mix), to(dev, k.src)
    sdr = [float(batch_SDR_torch(misi(ri, ratio, mix, K, hop), src).mean()) for K in (0, 3)]
    print(f"mean SI-SDR on oracle magnitudes: K = 0 {sdr[0]:.2f} dB, K = 3 {sdr[1]:.2f} dB")
    assert sdr[1] - sdr[0] >= 1.0, sdr


# ------------------------------------------------------------------------------------------------- the switches
def _chimera(dev, F=129, H=32, L=1, D=20):
    from onssen_amd import nn as onn
    from onssen_amd.synthetic import make_state_dict
    sd = make_state_dict("chimera", F, H, L, D, 2, seed=1, gain=2.0)
    m = onn.chimera(F, H, L, D)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(dev).eval()


def test_separate_chimera_switch(dev):
    from onssen_amd.features import stft_logmag
    from onssen_amd.separation import misi, separate_chimera
    from onssen_amd.synthetic import synth_mixture
    m = _chimera(dev)
    wav = to(dev, np.stack([synth_mixture(40 + b, 64 * 23) for b in range(2)]))
    plain = separate_chimera(m, wav)
    assert torch.equal(separate_chimera(m, wav, misi_iters=0), plain)
    two = separate_chimera(m, wav, misi_iters=2)
    assert two.shape == plain.shape and torch.isfinite(two).all() and not torch.equal(two, plain)
    with torch.no_grad():
        logmag, ri = stft_logmag(wav, 256, 64)
        _, masks = m.embedding_and_masks(logmag)
    assert torch.equal(two, misi(ri, masks, wav, 2))
    lengths = [64 * 23, 64 * 15 + 7]
    rag = separate_chimera(m, wav, lengths=lengths, misi_iters=2)
    one = separate_chimera(m, wav[1:, :lengths[1]].contiguous(), misi_iters=2)
    assert torch.equal(rag[1, :, :lengths[1]], one[0]) and (rag[1, :, lengths[1]:] == 0).all()


def test_tester_upit_switch(dev):
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.evaluate import tester_upit
    from onssen_amd.nn import uPIT_LSTM
    from onssen_amd.synthetic import make_state_dict
    fo = dict(batch_size=4, frame_length=20, sampling_rate=8000, window_size=256, hop_size=64, db_threshold=40, num_speaker=3)
    loader = list(SyntheticWsj02mix("upit", fo, "tt", dev, num_batches=2, seed=0))
    m = uPIT_LSTM(129, 129, 32, 20, 2, dropout=0.0, num_speaker=3)
    sd = make_state_dict("upit", 129, 32, 2, 20, 3, seed=0, gain=2.0)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    args = dict(model=m.to(dev).eval(), test_loader=loader, device=str(dev), model_name="upit")
    plain = tester_upit(args).eval(batch=2)
    score = tester_upit(args, misi_iters=1).eval(batch=2)
    print(f"tester_upit: mean SI-SDR {plain:.3f} dB without, {score:.3f} dB with one MISI iteration")
    assert np.isfinite(score) and score != plain
