"""Speech enhancement end to end on the GPU: the enhancement losses on the HIP kernels (value, gradient, autograd node), the label
kernel, the magnitude mode of the inverse transform, separate_enhance (uniform, ragged, 512/128, graph capture), tester_enhance,
the DAPS loader on a temporary tree, and one training step through the HIP loss.  Cases and bounds are those of
tests/test_emu_enhance.py (reasoned there), for the shapes used here."""
import os

import numpy as np
import pytest
import torch

from onssen_amd import loss as L
from tests import enhance_ref as R
from tests.phase_istft_cases import SHAPES

LOSS_SHAPES = R.LOSS_SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _model(dev, F=129, H=32, layers=2, seed=0):
    from onssen_amd.nn.enhancement import enhance
    torch.manual_seed(seed)
    return enhance(F, H, layers, dropout=0.0).to(dev).eval()


# ---- losses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,TF", LOSS_SHAPES)
def test_msa_on_device(dev, monkeypatch, B, TF):
    monkeypatch.setenv("ONSSEN_LOSS_HIP", "1")
    c = R.loss_case(B, TF, seed=11 + B)
    t = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    ref_utt, ref_total = R.msa(c["est"], c["s"])
    scale = float(np.float32(1.0 / (B * TF)))
    bound = scale * 1e-5 * ref_utt.sum()
    with torch.no_grad():
        val = L.loss_mask_msa([t["est"]], [t["s"], t["c"]])
        assert L.last_enhance_path == "value" and val.dim() == 0
        again = L.loss_mask_msa([t["est"]], [t["s"], t["c"]])
    want = scale * ref_utt.sum()
    print("MSA value |out - ref| / bound", abs(float(val) - want) / bound)
    assert abs(float(val) - want) <= bound and torch.equal(val, again)
    est = t["est"].clone().requires_grad_(True)
    got = L.loss_mask_msa([est], [t["s"], t["c"]])
    assert L.last_enhance_path == "grad" and torch.equal(got.detach(), val)
    d, = torch.autograd.grad(got * -1.7, [est])
    ref_d = float(np.float32(-1.7)) * 2.0 * scale * (R.f64(c["est"]) - R.f64(c["s"]))
    err = np.abs(d.cpu().numpy() - ref_d)
    print("MSA gradient max |err| / bound", (err / np.maximum(4 * R.EPS32 * np.abs(ref_d), 1e-300)).max())
    assert (err <= 4 * R.EPS32 * np.abs(ref_d)).all()


@pytest.mark.parametrize("B,TF", LOSS_SHAPES)
def test_psa_on_device(dev, monkeypatch, B, TF):
    monkeypatch.setenv("ONSSEN_LOSS_HIP", "1")
    c = R.loss_case(B, TF, seed=23 + B)
    t = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    ref_utt = R.psa(c["est"], c["x"], c["s"], c["c"])
    bound = 1e-5 * 2.0 * R.f64(c["x"]).sum(1)
    label = [t["x"], t["s"], t["c"]]
    with torch.no_grad():
        val = L.loss_mask_psa([t["est"]], label)
        assert L.last_enhance_path == "value" and tuple(val.shape) == (B,)
        assert torch.equal(val, L.loss_mask_psa([t["est"]], label))
    print("PSA value |out - ref| / bound", np.abs(val.cpu().numpy() - ref_utt) / bound)
    assert (np.abs(val.cpu().numpy() - ref_utt) <= bound).all()
    mask = t["est"].clone().requires_grad_(True)
    got = L.loss_mask_psa([mask], label)
    assert L.last_enhance_path == "grad" and torch.equal(got.detach(), val)
    g = torch.from_numpy(np.random.default_rng(B).standard_normal(B).astype(np.float32)).to(dev)
    d, = torch.autograd.grad(got, [mask], [g])
    sign = np.sign(R.psa_grad(c["est"], c["x"], c["s"], c["c"], np.ones(B))).astype(np.float32)
    want = (g.cpu().numpy()[:, None] * c["x"]).astype(np.float32) * sign
    np.testing.assert_array_equal(d.cpu().numpy(), want)
    assert (d[:, 0] == 0).all()                                             # the planted residual of exactly 0


def test_autograd_node_against_float64_autograd(dev, monkeypatch):
    """The node's gradients at (3, 7, 129) against float64 autograd of the PyTorch form, and the PyTorch route on the device
    under ``loss`` = "torch"."""
    import torch.nn.functional as F
    monkeypatch.setenv("ONSSEN_LOSS_HIP", "1")
    c = {k: v.reshape(3, 7, 129) for k, v in R.loss_case(3, 7 * 129, seed=5).items()}
    t = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    t64 = {k: torch.from_numpy(v).double() for k, v in c.items()}
    e64 = t64["est"].clone().requires_grad_(True)
    g_msa64, = torch.autograd.grad(F.mse_loss(e64, t64["s"]), [e64])
    r = e64 * t64["x"] - torch.min(t64["x"], F.relu(t64["s"] * t64["c"]))
    w = torch.tensor([0.7, -1.3, 0.4]).double()
    g_psa64, = torch.autograd.grad((r.flatten(1).abs().sum(1) * w).sum(), [e64])
    est = t["est"].clone().requires_grad_(True)
    msa = L.loss_mask_msa([est], [t["s"], t["c"]])
    assert L.last_enhance_path == "grad"
    g_msa, = torch.autograd.grad(msa, [est])
    assert ((g_msa.cpu().double() - g_msa64).abs() <= 4 * R.EPS32 * g_msa64.abs()).all()
    psa = L.loss_mask_psa([est], [t["x"], t["s"], t["c"]])
    g_psa, = torch.autograd.grad((psa * w.float().to(dev)).sum(), [est])
    # float32(float32(w) x) * sign against the float64 product: two roundings; the sign is exact (one fused multiply-add)
    assert ((g_psa.cpu().double() - g_psa64).abs() <= 2 * R.EPS32 * g_psa64.abs()).all()
    monkeypatch.setenv("ONSSEN_LOSS_HIP", "0")
    aten = L.loss_mask_msa([est], [t["s"], t["c"]])
    assert L.last_enhance_path == "aten" and abs(float(aten.detach()) - float(msa.detach())) <= 1e-5 * float(msa.detach())


# ---- labels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", [1, 1000])
def test_labels_bits_on_device(dev, n_bins):
    from onssen_amd.features import enhance_labels, training_labels
    from onssen_amd.hip import get_lib
    a, b = R.labels_case(n_bins, seed=n_bins)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    mn, mc, cd = enhance_labels(ta, tb)
    alone = torch.empty(n_bins, device=dev)
    get_lib().cos_difference(ta.data_ptr(), tb.data_ptr(), n_bins, alone.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert torch.equal(cd, alone)
    # hypotf as the labels kernel computes it
    shape = (1, 1, n_bins, 2)
    _, mm, m1, _ = training_labels(ta.view(shape), tb.view(shape), tb.view(shape), torch.zeros(1, 1, n_bins, device=dev))
    assert torch.equal(mn, mm.view(-1)) and torch.equal(mc, m1.view(-1))
    rn, rc, rcos = R.labels(a, b)
    assert np.abs(mn.cpu().numpy() - rn).max() <= 2 * R.EPS32 * rn.max() and np.abs(mc.cpu().numpy() - rc).max() <= 2 * R.EPS32 * rc.max()
    assert np.abs(cd.cpu().numpy() - rcos).max() <= 1e-6 and float(mn[0]) == 0.0
    m2, c2, none = enhance_labels(ta, tb, with_cos=False)
    assert none is None and torch.equal(m2, mn) and torch.equal(c2, mc)
    m3, n1, n2 = enhance_labels(ta, None)
    assert n1 is None and n2 is None and torch.equal(m3, mn)


# ---- magnitude mode of the inverse transform --------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n_fft,hop,n", SHAPES)
def test_mag_istft_matches_oracle(dev, n_fft, hop, n, C):
    from onssen_amd.features import mag_istft
    ri, mags = R.mag_case(n_fft, hop, n, C)
    d = lambda a: torch.from_numpy(a).to(dev)
    out = mag_istft(d(ri), d(mags), hop, n)
    ref = R.mag_reference(ri, mags, hop, n)
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"n_fft {n_fft} hop {hop} C {C}: max |out - ref| {err:.3e}, bound {R.mag_atol(ref):.3e}")
    assert tuple(out.shape) == (2, C, n) and torch.isfinite(out).all() and err <= R.mag_atol(ref)
    B, T, F, _ = mags.shape
    wide = torch.full((B, C, T, 2 * F), float("nan"), device=dev)
    wide[..., ::2] = d(mags).permute(0, 3, 1, 2)
    view = wide[..., ::2].permute(0, 2, 3, 1)
    assert not view.is_contiguous() and torch.equal(mag_istft(d(ri), view, hop, n), out)
    if C == 1:
        assert torch.equal(mag_istft(d(ri), d(mags)[..., 0], hop, n), out)          # (B,T,F): one channel


@pytest.mark.parametrize("n_fft,hop,n", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_mag_istft_ragged_rows_are_their_batch_1_results(dev, n_fft, hop, n):
    from onssen_amd.features import mag_istft
    ri, mags = R.mag_case(n_fft, hop, n, 1, B=3)
    lengths = np.array([n, n - 3 * hop - 5, n_fft // 2 + hop + 1], np.int32)
    frames = (1 + lengths // hop).astype(np.int32)
    d = lambda a: torch.from_numpy(a).to(dev)
    out = mag_istft(d(ri), d(mags), hop, n, frames=frames.tolist(), lengths=lengths.tolist())
    ref = R.mag_reference(ri, mags, hop, n, frames, lengths)
    assert np.abs(out.cpu().numpy() - ref).max() <= R.mag_atol(ref)
    for b in range(3):
        Tb, nb = int(frames[b]), int(lengths[b])
        alone = mag_istft(d(ri[b:b + 1, :Tb]), d(mags[b:b + 1, :Tb]), hop, nb)
        assert torch.equal(out[b, :, :nb], alone[0]) and (out[b, :, nb:] == 0).all(), b
    with pytest.raises(ValueError, match="both frames= and lengths="):
        mag_istft(d(ri), d(mags), hop, n, frames=frames.tolist())


# ---- separate_enhance ------------------------------------------------------------------------------------------------------
def _wav(dev, B, n, seed=50):
    from onssen_amd.synthetic import synth_mixture
    return torch.from_numpy(np.stack([synth_mixture(seed + b, n) for b in range(B)])).to(dev)


@pytest.mark.parametrize("window,hop,F", [(256, 64, 129), (512, 128, 257)])
def test_separate_enhance_is_the_composition_of_its_parts(dev, window, hop, F):
    from onssen_amd.features import enhance_labels, stft_logmag
    from onssen_amd.separation import separate_enhance
    model = _model(dev, F)
    wav = _wav(dev, 3, 2000)
    out = separate_enhance(model, wav, window, hop)
    assert tuple(out.shape) == (3, 2000) and torch.isfinite(out).all()
    with torch.no_grad():
        logmag, ri = stft_logmag(wav, window, hop)
        clean, = model([logmag, enhance_labels(ri, None)[0]])
    assert float(clean.max()) > 0                                           # (a ReLU output: not all zero for these weights)
    ref = R.mag_reference(ri.cpu().numpy(), clean.cpu().numpy()[..., None], hop, 2000)[:, 0]
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"separate_enhance {window}/{hop}: max |out - ref| {err:.3e}, bound {R.mag_atol(ref):.3e}")
    assert err <= R.mag_atol(ref)


def test_separate_enhance_ragged_rows_are_their_batch_1_calls(dev):
    from onssen_amd.separation import separate_enhance
    model = _model(dev)
    wav = _wav(dev, 3, 2000)
    lengths = [2000, 1300, 700]
    out = separate_enhance(model, wav, lengths=lengths)
    for b, nb in enumerate(lengths):
        alone = separate_enhance(model, wav[b:b + 1, :nb])
        assert torch.equal(out[b, :nb], alone[0]), b
        assert (out[b, nb:] == 0).all(), b
    assert float(out.abs().max()) > 0


def test_separate_enhance_in_a_graph(dev):
    from onssen_amd.separation import separate_enhance
    model = _model(dev)
    wav = _wav(dev, 3, 2000)
    eager = separate_enhance(model, wav)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        separate_enhance(model, wav)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = separate_enhance(model, wav)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


# ---- tester and loader -----------------------------------------------------------------------------------------------------
def test_eval_batched_equals_the_one_by_one_loop(dev):
    from onssen_amd.data import daps_enhance_dataloader
    from onssen_amd.evaluate import batch_SDR_torch, tester_enhance
    fo = dict(data_path="synthetic", batch_size=1, frame_length=20, sampling_rate=8000, window_size=256, hop_size=64)
    loader = list(daps_enhance_dataloader(6, fo, "tt", dev))
    assert len(loader) == 6 and len({item[1][2].shape[-1] for item in loader}) == 6      # six different lengths
    (feat, mag), (sr, si, ref) = loader[0]
    assert feat.shape == mag.shape == sr.shape == si.shape and feat.shape[0] == 1 and ref.shape[:2] == (1, 1)
    t = tester_enhance(dict(model=_model(dev), test_loader=loader, device=str(dev), model_name="enhance"))
    one_by_one = t.eval(batch=1)
    assert np.isfinite(one_by_one)
    assert t.eval(batch=3) == one_by_one                                    # the same six values summed in the same order
    with torch.no_grad():
        inp, lab, (frames, lengths) = t.collate(loader[:3])
        assert inp[1].shape == inp[0].shape                                 # mag_noisy is padded along the frames like the features
        sdr = t._one(inp, lab, (frames, lengths))
        for b in range(3):
            assert torch.equal(sdr[b:b + 1], t._one(*loader[b], None)), b


def test_daps_loader_on_a_tree(dev, tmp_path):
    from onssen_amd.data import DapsEnhanceFiles, daps_enhance_dataloader, write_wav
    from onssen_amd.features import enhance_labels, stft_logmag
    from onssen_amd.synthetic import synth_mixture, synth_voice
    hop, L = 64, 10
    os.makedirs(tmp_path / "noisy")
    os.makedirs(tmp_path / "clean")
    names, sigs = [], {}
    # frames 1 + n // 64: 26 (two chunks), 12 (one), 8 (none: skipped), 16 kHz file of 2 x 1500 samples -> 1500 at 8 kHz: 24 (two)
    for k, (n, rate) in enumerate([(1600, 8000), (704, 8000), (448, 8000), (3000, 16000)]):
        clean = 0.5 * synth_voice(900 + k, n, rate)
        noisy = 0.5 * synth_mixture(70 + k, n, rate)
        name = f"s{k}_script{k}_dev_room.wav"
        write_wav(str(tmp_path / "noisy" / name), noisy, rate)
        write_wav(str(tmp_path / "clean" / f"s{k}_script{k}_clean.wav"), clean, rate)
        names.append("noisy/" + name)
    (tmp_path / "train").write_text("\n".join(names) + "\n")
    fo = dict(data_path=str(tmp_path), batch_size=2, frame_length=L, sampling_rate=8000, window_size=256, hop_size=hop)
    assert isinstance(daps_enhance_dataloader(3, fo, "train", dev), DapsEnhanceFiles)
    ld = DapsEnhanceFiles(3, fo, "train", dev, shuffle=False)
    batches = list(ld)
    assert len(batches) == 3 == len(ld)
    for (feature, mag_noisy), (mag_clean, cos_diff) in batches:
        for x in (feature, mag_noisy, mag_clean, cos_diff):
            assert tuple(x.shape) == (2, L, 129) and x.dtype == torch.float32 and x.device.type == "cuda"
    # the stream: file 0 frames [0, 10), [10, 20) | file 1 [0, 10) ; file 2 skipped ; file 3 [0, 10) | file 3 [10, 20) ; file 0 again
    assert ld.opened == [names[0], names[1], names[3], names[0]]
    want = [(0, 0), (0, 10), (1, 0), (3, 0), (3, 10), (0, 0)]
    from onssen_amd.data.wsj0_2mix import _load
    for i, (k, at) in enumerate(want):
        noisy, clean = (_load(p, 8000) for p in ld.paths(names[k]))
        if k == 3:
            assert len(noisy) == 1500                                           # resampled
        logmag, ri = stft_logmag(torch.from_numpy(np.stack([noisy, clean])).to(dev), 256, hop)
        mn, mc, cd = enhance_labels(ri[0, at:at + L], ri[1, at:at + L])
        (feature, mag_noisy), (mag_clean, cos_diff) = batches[i // 2]
        b = i % 2
        assert torch.equal(feature[b], logmag[0, at:at + L]) and torch.equal(mag_noisy[b], mn), (i, k, at)
        assert torch.equal(mag_clean[b], mc) and torch.equal(cos_diff[b], cd), (i, k, at)
    # the evaluation partition: whole recordings in the tester's contract
    (tmp_path / "tt").write_text(names[1] + "\n" + names[3] + "\n")
    items = list(daps_enhance_dataloader(1, fo, "tt", dev))
    assert len(items) == 2
    (feat, mag), (sr, si, ref) = items[1]
    assert tuple(feat.shape) == (1, 24, 129) == tuple(mag.shape) == tuple(sr.shape) and tuple(ref.shape) == (1, 1, 1500 + 32 - 1500 % 32)


# ---- training --------------------------------------------------------------------------------------------------------------
def test_training_step_through_the_hip_loss(dev, monkeypatch):
    """One step of enhance(129, 32, 1) on a synthetic batch (4, 50, 129): the parameter gradients with the loss on the HIP kernels
    against the same step with the PyTorch loss, each tensor to 1e-4 of its largest entry."""
    from onssen_amd.data import daps_enhance_dataloader
    fo = dict(data_path="synthetic", batch_size=4, frame_length=50, sampling_rate=8000, window_size=256, hop_size=64)
    input, label = next(iter(daps_enhance_dataloader(1, fo, "train", dev)))
    assert tuple(input[0].shape) == (4, 50, 129)
    model = _model(dev, 129, 32, 1, seed=3).train()
    grads = {}
    for how in ("1", "0"):
        monkeypatch.setenv("ONSSEN_LOSS_HIP", how)
        model.zero_grad(set_to_none=True)
        loss = L.loss_mask_msa(model(input), label)
        assert L.last_enhance_path == ("grad" if how == "1" else "aten")
        loss.backward()
        grads[how] = (float(loss), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert abs(grads["1"][0] - grads["0"][0]) <= 1e-5 * abs(grads["0"][0])
    assert grads["1"][1].keys() == grads["0"][1].keys() and len(grads["1"][1]) >= 8
    for k, g in grads["0"][1].items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        assert float((grads["1"][1][k] - g).abs().max()) <= 1e-4 * float(g.abs().max()), k
