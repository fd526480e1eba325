"""Deep clustering for three and four speakers on the GPU: ``onssen_dc_cluster_k_f32`` against the float64 restatement
(tests/dc_kmeans_ref.py) on planted clusters -- exact masks, see tests/test_emu_dc_kmeans.py for why --, ragged batches, the
untouched two-speaker route, and the public surface (``dc_masks``, ``separate_dc``, ``tester_dc``) end to end.

The random-weight network's embeddings are NOT well separated: nothing here compares them with a float64 reference (a bin on a
boundary may legitimately flip); those calls are compared bit for bit with compositions of the same device kernels."""
import numpy as np
import pytest
import torch

from onssen_amd.synthetic import make_state_dict, synth_mixture
from tests.dc_kmeans_ref import planted, ref_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    from onssen_amd import nn as onn
    sd = make_state_dict("deep_clustering", 129, 32, 2, 20, 2, seed=4, gain=1.0)
    m = onn.deep_clustering(129, 32, 2, 20)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(dev).eval()


def run_k(dev, emb, feat, K, frames=None, iters=20, tol=1e-4):
    """The C ABI entry on buffers of its own -> masks, iterations, converged (NumPy)."""
    from onssen_amd.hip import get_lib
    lib = get_lib()
    B, T, F, D = emb.shape
    e, f = torch.from_numpy(emb).to(dev), torch.from_numpy(feat).to(dev)
    nb = int(lib.dll.onssen_dc_cluster_k_workspace_bytes(B, T, F, D, K))
    ws = torch.full((nb // 4 + 64,), float("nan"), device=dev)
    masks = torch.full((B, T, F, K), float("nan"), device=dev)
    fr = torch.tensor(frames, dtype=torch.int32, device=dev) if frames is not None else None
    lib.dc_cluster_k(e.data_ptr(), f.data_ptr(), B, T, F, D, K, 40.0, iters, masks.data_ptr(), ws.data_ptr(), nb,
                     torch.cuda.current_stream().cuda_stream, frames=fr.data_ptr() if fr is not None else None, tol=tol)
    torch.cuda.synchronize()
    info = ws.view(torch.int32)[:4 * B].view(B, 4).cpu().numpy()
    return masks.cpu().numpy(), info[:, 0], info[:, 1]


# the emulation's cases, then a shape that spans several workgroups per utterance (40 x 129 bins = 21 tiles of 256 bins, one per
# workgroup; test_many_tiles_per_workgroup has the workgroups walk several tiles each)
@pytest.mark.parametrize("B,T,F,D,K", [(2, 7, 33, 20, 3), (1, 5, 17, 8, 4), (3, 40, 129, 20, 3), (3, 40, 129, 20, 4)])
def test_masks_equal_the_reference(dev, B, T, F, D, K):
    emb, feat, _ = planted(B + D + K, B, T, F, D, K)
    masks, its, conv = run_k(dev, emb, feat, K)
    ref, rits, rconv = ref_batch(emb, feat, K)
    np.testing.assert_array_equal(masks, ref)
    np.testing.assert_array_equal(its, rits)
    np.testing.assert_array_equal(conv, rconv.astype(np.int32))
    for b in range(B):
        act = feat[b] >= feat[b].max() - np.float32(2.0)
        assert np.all(masks[b][~act] == 0) and np.all(masks[b][act].sum(-1) == 1)


def test_many_tiles_per_workgroup(dev):
    """T = 600: 303 tiles over 64 workgroups -- every workgroup walks four or five tiles."""
    emb, feat, _ = planted(2, 1, 600, 129, 20, 3)
    masks, its, _ = run_k(dev, emb, feat, 3)
    ref, rits, _ = ref_batch(emb, feat, 3)
    np.testing.assert_array_equal(masks, ref)
    assert its[0] == rits[0]


def test_ragged_rows_equal_the_one_utterance_call(dev):
    B, T, F, D, K = 2, 14, 33, 20, 3
    frames = [14, 9]
    emb0, feat0, _ = planted(7, B, T, F, D, K)
    emb, feat = emb0.copy(), feat0.copy()
    for b in range(B):
        emb[b, frames[b]:] = np.nan
        feat[b, frames[b]:] = 50.0
    masks, its, _ = run_k(dev, emb, feat, K, frames=frames)
    for b in range(B):
        Tb = frames[b]
        m1, it1, _ = run_k(dev, np.ascontiguousarray(emb0[b:b + 1, :Tb]), np.ascontiguousarray(feat0[b:b + 1, :Tb]), K)
        np.testing.assert_array_equal(masks[b, :Tb], m1[0])
        assert its[b] == it1[0] and np.all(masks[b, Tb:] == 0) and masks[b, :Tb].sum() > 0


def test_dc_masks_three_speakers_and_the_untouched_two_speaker_route(dev):
    from onssen_amd.separation import dc_masks
    B, T, F, D = 2, 20, 33, 20
    emb, feat, _ = planted(3, B, T, F, D, 3)
    e, f = torch.from_numpy(emb).to(dev), torch.from_numpy(feat).to(dev)
    m3 = dc_masks(e, f, num_speaker=3)
    assert m3.shape == (B, T, F, 3)
    np.testing.assert_array_equal(m3.cpu().numpy(), ref_batch(emb, feat, 3)[0])
    # num_speaker = 2 is the call as it stands without the argument: same route, same bits, same channel convention
    emb2, feat2, _ = planted(4, B, T, F, D, 2)
    e2, f2 = torch.from_numpy(emb2).to(dev), torch.from_numpy(feat2).to(dev)
    m2d, m2 = dc_masks(e2, f2), dc_masks(e2, f2, num_speaker=2)
    assert m2.shape == (B, T, F, 2) and torch.equal(m2, m2d)
    assert torch.equal(m2[..., 0] + m2[..., 1], (f2 >= f2.amax((1, 2), keepdim=True) - 2.0).float()) and m2[..., 0].sum() > 0
    with pytest.raises(ValueError, match="num_speaker"):
        dc_masks(e, f, num_speaker=5)


def test_separate_dc_three_speakers_is_the_composition_of_its_stages(dev, model):
    from onssen_amd.features import mask_istft, stft_logmag
    from onssen_amd.separation import dc_masks, separate_dc
    ns = [64 * 38 + 5, 64 * 30]                               # about 0.3 s at 8 kHz
    n = max(ns)
    wav = torch.zeros(2, n)
    for b, nb in enumerate(ns):
        wav[b, :nb] = torch.from_numpy(synth_mixture(50 + b, nb))
    wav = wav.to(dev)
    out = separate_dc(model, wav, num_speaker=3, lengths=ns)
    assert out.shape == (2, 3, n) and torch.isfinite(out).all()
    with torch.no_grad():
        lengths = torch.tensor(ns, dtype=torch.int32, device=dev)
        frames = (1 + lengths // 64).to(torch.int32)
        logmag, ri = stft_logmag(wav, 256, 64, lengths=lengths)
        emb, = model([logmag], frames=frames)
        masks = dc_masks(emb, logmag, 40.0, frames=frames, num_speaker=3)
        want = mask_istft(ri, masks, 64, n, frames=frames, lengths=lengths)
    assert masks.shape[-1] == 3 and torch.equal(out, want)
    assert all((out[b, :, ns[b]:] == 0).all() for b in range(2))


def test_tester_dc_evaluates_three_source_references(dev, model):
    from onssen_amd.evaluate import tester_dc
    from onssen_amd.features import stft_logmag
    loader = []
    for k, nb in enumerate([64 * 40, 64 * 33, 64 * 36]):
        src = torch.stack([torch.from_numpy(synth_mixture(90 + 3 * k + c, nb)) for c in range(3)]).to(dev)      # (3, n)
        logmag, ri = stft_logmag(src.sum(0, keepdim=True), 256, 64)
        loader.append(([logmag], [ri[..., 0].contiguous(), ri[..., 1].contiguous(), src.unsqueeze(0)]))
    t = tester_dc(dict(model=model, test_loader=loader, device=str(dev), model_name="dc"))
    one_by_one = t.eval()
    assert np.isfinite(one_by_one)
    # batch = 2 of a two-layer network is the pipelined route for two speakers: three-source items take the plain loop
    got = t.eval(batch=2)
    assert abs(got - one_by_one) <= 1e-9 * max(1.0, abs(one_by_one))
