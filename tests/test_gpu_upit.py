"""uPIT end to end on the GPU: the two losses on the HIP kernels (value route, gradient route) against tests/upit_ref.py, the
network against the fixtures recorded from the reference and against a float64 restatement, the ragged forward, separate_upit
(uniform, ragged, graph capture), tester_upit, the loader's items, and training through the HIP loss.  Cases and bounds are those of
tests/test_emu_upit.py (reasoned there)."""
import os
from math import factorial

import numpy as np
import pytest
import torch

from onssen_amd import loss as L
from tests import upit_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


def _model(dev, S, F=129, H=32, layers=2, seed=0, sd=None):
    from onssen_amd.nn import uPIT_LSTM
    from onssen_amd.synthetic import make_state_dict
    m = uPIT_LSTM(F, F, H, 20, layers, dropout=0.0, num_speaker=S)
    sd = sd if sd is not None else make_state_dict("upit", F, H, layers, 20, S, seed=seed, gain=2.0)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def _wav(dev, B, n, seed=60):
    from onssen_amd.synthetic import synth_mixture
    return torch.from_numpy(np.stack([synth_mixture(seed + b, n) for b in range(B)])).to(dev)


# ---- losses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,TF,psa", R.SHAPES + [R.LONG])
def test_losses_on_device(dev, monkeypatch, S, TF, psa):
    monkeypatch.setenv("ONSSEN_LOSS_HIP", "1")
    c = R.loss_case(S, TF, seed=100 * S + int(psa), psa=psa)
    B = factorial(S)
    fn = L.loss_upit_psa if psa else L.loss_upit_msa
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)
    x, src = to(c["x"]), to(c["src"])
    label = [x] + [src[j] for j in range(S)]                  # slices of one tensor: read where they lie
    if psa:
        cos = to(c["cos"])
        label += [cos[j].clone() for j in range(S)]           # separate allocations: stacked first unless they happen to line up
    inter = to(np.ascontiguousarray(c["masks"].transpose(1, 2, 0)))          # (B, TF, S): the network's layout
    masks = [inter[..., k] for k in range(S)]
    ref_pair = R.pair_matrix(c["masks"], c["x"], c["src"], c["cos"])
    ref_out, ref_perm = R.best(ref_pair)
    ob = R.out_bound(c["x"], c["src"], c["cos"], ref_perm)
    with torch.no_grad():
        val, perm = fn(masks, label, return_perm=True)
        assert L.last_upit_path == "value" and tuple(val.shape) == (B,) and perm.dtype == torch.int64
        again = fn(masks, label)
        apart = fn([m.contiguous() for m in masks], label)    # S separate maps: stacked into the same layout
    assert torch.equal(val, again) and torch.equal(val, apart)
    print("out |out - ref| / bound", np.abs(val.cpu().numpy() - ref_out) / ob)
    assert (np.abs(val.cpu().numpy() - ref_out) <= ob).all()
    perm = perm.cpu().numpy()
    if TF >= 387:
        mg = R.margin(ref_pair) / ob
        assert (mg >= 100).all() and (ref_perm == np.arange(B)).all()
        assert (perm == np.arange(B)).all()
    else:
        tot = R.totals(ref_pair)
        assert (np.abs(tot[np.arange(B), perm] - tot.min(1)) <= ob).all()      # ties: perm attains the minimum, to the bound
    # the gradient route: the node on the interleaved buffer itself, and on stacked separate leaves
    g = torch.from_numpy(np.random.default_rng(S).standard_normal(B).astype(np.float32)).to(dev)
    leaf = inter.clone().requires_grad_(True)
    got, perm_g = fn([leaf[..., k] for k in range(S)], label, return_perm=True)
    assert L.last_upit_path == "grad" and torch.equal(got.detach(), val) and (perm_g.cpu().numpy() == perm).all()
    d, = torch.autograd.grad((got * g).sum(), [leaf])
    sign = R.grad_sign(c["masks"], c["x"], c["src"], c["cos"], perm)
    want = (g.cpu().numpy()[None, :, None] * c["x"][None]).astype(np.float32) * sign.astype(np.float32)
    np.testing.assert_array_equal(d.cpu().numpy().transpose(2, 0, 1), want)
    if TF == 387:
        leaves = [to(c["masks"][k]).requires_grad_(True) for k in range(S)]
        got2 = fn(leaves, label)
        assert L.last_upit_path == "grad" and torch.equal(got2.detach(), val)
        ds = torch.autograd.grad((got2 * g).sum(), leaves)
        for k in range(S):
            np.testing.assert_array_equal(ds[k].cpu().numpy(), want[k])
        monkeypatch.setenv("ONSSEN_LOSS_HIP", "0")
        aten = fn([l for l in leaves], label)
        assert L.last_upit_path == "aten"
        assert (np.abs(aten.detach().cpu().numpy() - ref_out) <= 20 * ob).all()          # fp32 sums of the PyTorch route


def test_ragged_loss_rows_are_their_batch_1_calls(dev):
    S, T, F = 3, 5, 129
    c = R.loss_case(S, T * F, seed=31, psa=True)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)
    frames = [1, T - 1, T]
    masks = [to(c["masks"][k][:3]).view(3, T, F) for k in range(S)]
    label = [to(c["x"][:3]).view(3, T, F)] + [to(c["src"][j][:3]).view(3, T, F) for j in range(S)] \
        + [to(c["cos"][j][:3]).view(3, T, F) for j in range(S)]
    with torch.no_grad():
        val = L.loss_upit_psa(masks, label, frames=frames)
        for b, fb in enumerate(frames):
            one = L.loss_upit_psa([m[b:b + 1, :fb] for m in masks], [t[b:b + 1, :fb] for t in label])
            assert torch.equal(val[b:b + 1], one), b


# ---- the network -----------------------------------------------------------------------------------------------------------
def _f64_masks(sd, x, F, H, layers, S):
    """(B, T, F, S) float64: nn.LSTM + Linear + sigmoid on the CPU with the same weights."""
    rnn = torch.nn.LSTM(F, H, layers, bidirectional=True, batch_first=True).double()
    fc = torch.nn.Linear(2 * H, F * S).double()
    rnn.load_state_dict({k[4:]: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if k.startswith("rnn.")})
    fc.load_state_dict({k[6:]: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if k.startswith("fc_mi.")})
    with torch.no_grad():
        y, _ = rnn(torch.from_numpy(x).double())
        return torch.sigmoid(fc(y)).reshape(x.shape[0], x.shape[1], F, S).numpy()


@pytest.mark.parametrize("precision,atol", [(None, 3e-5), ("f32", 1e-5)])
@pytest.mark.parametrize("S", [2, 3, 4])
def test_network_against_the_fixtures_and_float64(dev, monkeypatch, S, precision, atol):
    from onssen_amd.synthetic import make_state_dict
    if precision:
        monkeypatch.setenv("ONSSEN_PRECISION", precision)
    monkeypatch.setenv("ONSSEN_CHECK", "1")
    fx = np.load(os.path.join(GOLDEN, f"g10_upit_H16_L2_S{min(S, 3)}.npz"))
    F, H, layers, x = int(fx["F"]), int(fx["H"]), int(fx["L"]), fx["x"]
    sd = make_state_dict("upit", F, H, layers, 20, S, seed=int(fx["seed"]), gain=float(fx["gain"]))
    m = _model(dev, S, F, H, layers, sd=sd)
    xt = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        out = m([xt])
        buf = m.masks(xt)
    assert len(out) == S and buf.shape == (2, 12, F, S) and buf.is_contiguous()
    for k, o in enumerate(out):
        assert o.shape == (2, 12, F) and o.stride() == buf[..., k].stride() and torch.equal(o, buf[..., k])
    close = lambda a, b: (np.abs(a - b) <= atol + 1e-4 * np.abs(b)).all()
    got = [o.cpu().numpy() for o in out]
    if S <= 3:                                                  # the reference's two masks (the first two of three at S = 3)
        print("max |mask - fixture|", max(np.abs(got[0] - fx["mask_A"]).max(), np.abs(got[1] - fx["mask_B"]).max()))
        assert close(got[0], fx["mask_A"]) and close(got[1], fx["mask_B"])
    ref = _f64_masks(sd, x, F, H, layers, S)
    for k in range(S):                                          # every mask, the third and fourth among them
        assert close(got[k], ref[..., k]), k
    # the training-path forward (dropout 0) equals the inference forward
    tr = m.train()([xt])
    assert tr[0].requires_grad and tr[0]._base is tr[S - 1]._base
    for k in range(S):
        assert close(tr[k].detach().cpu().numpy(), got[k]), k
    m.eval()


def test_ragged_forward_rows_are_their_batch_1_forwards(dev):
    S, T = 3, 12
    m = _model(dev, S, H=32)
    from onssen_amd.features import stft_logmag
    logmag, _ = stft_logmag(_wav(dev, 3, 64 * (T - 1)))
    assert logmag.shape[1] == T
    frames = [12, 7, 3]
    with torch.no_grad():
        rag = m([logmag], frames=frames)
        for b, fb in enumerate(frames):
            one = m([logmag[b:b + 1, :fb].contiguous()])
            for k in range(S):
                assert torch.equal(rag[k][b, :fb], one[k][0]), (b, k)


# ---- separation ------------------------------------------------------------------------------------------------------------
def test_separate_upit(dev):
    from onssen_amd.features import mask_istft, stft_logmag
    from onssen_amd.separation import separate_upit
    S, n = 3, 2000
    m = _model(dev, S)
    wav = _wav(dev, 3, n)
    out = separate_upit(m, wav)
    assert out.shape == (3, S, n) and torch.isfinite(out).all()
    with torch.no_grad():
        logmag, ri = stft_logmag(wav, 256, 64)
        parts = mask_istft(ri, m.masks(logmag), 64, n)
    assert torch.equal(out, parts)                              # the composition of its parts, bit for bit
    lengths = [2000, 1500, 700]
    rag = separate_upit(m, wav, lengths=lengths)
    for b, nb in enumerate(lengths):
        one = separate_upit(m, wav[b:b + 1, :nb].contiguous())
        assert torch.equal(rag[b, :, :nb], one[0]), b
        assert (rag[b, :, nb:] == 0).all(), b


def test_separate_upit_in_a_graph(dev):
    from onssen_amd.separation import separate_upit
    m = _model(dev, 3)
    wav = _wav(dev, 3, 2000)
    eager = separate_upit(m, wav)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        separate_upit(m, wav)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = separate_upit(m, wav)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


# ---- tester and loader -----------------------------------------------------------------------------------------------------
FO = dict(batch_size=4, frame_length=50, sampling_rate=8000, window_size=256, hop_size=64, db_threshold=40)


def test_eval_batched_equals_the_one_by_one_loop(dev):
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.evaluate import tester_upit
    # three items each from two loaders: within one, the padding of sig_ref to a multiple of 32 samples makes lengths coincide
    loader = [item for fl, seed in ((20, 0), (26, 1))
              for item in SyntheticWsj02mix("upit", dict(FO, frame_length=fl, num_speaker=3), "tt", dev, num_batches=3, seed=seed)]
    assert len(loader) == 6 and len({item[1][2].shape[-1] for item in loader}) == 6      # six different lengths
    assert len({item[0][0].shape[1] for item in loader}) == 6                            # ... and frame counts
    (feat,), (sr, si, ref) = loader[0]
    assert feat.shape == sr.shape == si.shape and feat.shape[0] == 1 and ref.shape[:2] == (1, 3)
    t = tester_upit(dict(model=_model(dev, 3), test_loader=loader, device=str(dev), model_name="upit"))
    one_by_one = t.eval(batch=1)
    assert np.isfinite(one_by_one)
    assert t.eval(batch=3) == one_by_one                        # the same six values summed in the same order


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("name", ["upit", "upit-psa"])
def test_loader_items(dev, name, S):
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    from onssen_amd.features import enhance_labels, stft_logmag
    fo = dict(FO, num_speaker=S) if S != 2 else FO
    ld = SyntheticWsj02mix(name, fo, "tr", dev, num_batches=1)
    (feat,), label = next(iter(ld))
    psa = name == "upit-psa"
    assert tuple(feat.shape) == (4, 50, 129) and len(label) == 1 + (2 if psa else 1) * S
    assert all(t.shape == feat.shape and t.dtype == torch.float32 and t.is_cuda for t in [feat] + label)
    # the same maps from the same signals, through enhance_labels per source: bit for bit
    utts = [ld._mixture(ld.seed + b, ld.n_samples) for b in range(4)]
    assert all(len(u) == 1 + S for u in utts)
    wav = torch.from_numpy(np.stack([np.stack(u) for u in utts])).to(dev)
    logmag, ri = stft_logmag(wav.view(4 * (1 + S), -1), 256, 64)
    T = logmag.shape[1]
    ri = ri.view(4, 1 + S, T, 129, 2)
    start = int(np.random.default_rng(ld.seed).integers(0, T - 50))
    assert torch.equal(feat, logmag.view(4, 1 + S, T, 129)[:, 0, start:start + 50])
    mix = ri[:, 0, start:start + 50].contiguous()
    for k in range(S):
        mm, ms, cs = enhance_labels(mix, ri[:, 1 + k, start:start + 50].contiguous())
        assert torch.equal(label[0], mm) and torch.equal(label[1 + k], ms)
        if psa:
            assert torch.equal(label[1 + S + k], cs)


# ---- training --------------------------------------------------------------------------------------------------------------
def _train_batch(dev, seed):
    from onssen_amd.data.synthetic_wsj0_2mix import SyntheticWsj02mix
    ld = SyntheticWsj02mix("upit-psa", dict(FO, num_speaker=3), "tr", dev, num_batches=1, seed=seed)
    return next(iter(ld))


def test_training_step_through_the_hip_loss(dev, monkeypatch):
    """One step of uPIT_LSTM(129, 129, 32, num_layers=1, dropout=0, num_speaker=3) on a synthetic (4, 50, 129) batch through
    loss_upit_psa on the HIP kernels against the same step with ONSSEN_LOSS_HIP=0.  The two routes sum in different precisions, so
    they are compared only where they chose the same assignment in every row, and the seed is one where that choice is not close:
    the float64 margin between the best two assignments is >= 100 value bounds (asserted)."""
    input, label = _train_batch(dev, seed=0)
    assert tuple(input[0].shape) == (4, 50, 129) and len(label) == 7
    model = _model(dev, 3, 129, 32, 1, seed=3).train()
    res = {}
    for how in ("1", "0"):
        monkeypatch.setenv("ONSSEN_LOSS_HIP", how)
        model.zero_grad(set_to_none=True)
        out = model(input)
        loss, perm = L.loss_upit_psa(out, label, return_perm=True)
        assert L.last_upit_path == ("grad" if how == "1" else "aten")
        loss.mean().backward()
        res[how] = (float(loss.mean().detach()), perm.cpu().numpy(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                    [o.detach().cpu().numpy() for o in out])
    assert (res["1"][1] == res["0"][1]).all()                   # first: both routes chose the same assignment in every row
    lab = [t.cpu().numpy().reshape(4, -1) for t in label]
    masks = np.stack([o.reshape(4, -1) for o in res["1"][3]])
    x, src, cos = lab[0], np.stack(lab[1:4]), np.stack(lab[4:7])
    pair = R.pair_matrix(masks, x, src, cos)
    ob = R.out_bound(x, src, cos, None)
    print("float64 margin / value bound", R.margin(pair) / ob)
    assert (R.margin(pair) >= 100 * ob).all()
    assert (R.best(pair)[1] == res["1"][1]).all()
    assert abs(res["1"][0] - res["0"][0]) <= 1e-5 * abs(res["0"][0])
    assert res["1"][2].keys() == res["0"][2].keys() and len(res["1"][2]) >= 8
    for k, g in res["0"][2].items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        assert float((res["1"][2][k] - g).abs().max()) <= 1e-4 * float(g.abs().max()), k


def test_twenty_training_steps_lower_the_loss(dev, monkeypatch):
    from onssen_amd import dist as odist
    monkeypatch.setenv("ONSSEN_LOSS_HIP", "1")
    input, label = _train_batch(dev, seed=0)
    model = _model(dev, 3, 129, 32, 1, seed=3).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = [odist.train_step(model, opt, L.loss_upit_psa, input, label) for _ in range(20)]
    assert L.last_upit_path == "grad"
    print("loss, first and last of 20 steps", losses[0], losses[-1])
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
