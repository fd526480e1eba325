"""The Python surface of deep clustering for three and four speakers, as far as it can be checked without a device:
argument checks, where the speaker count comes from, and the binding of the two new C ABI entries."""
import pytest
import torch


def test_dc_masks_refuses_other_speaker_counts_before_touching_the_library(monkeypatch):
    import onssen_amd.hip
    from onssen_amd import separation

    def no_lib():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(onssen_amd.hip, "get_lib", no_lib)
    emb, logmag = torch.zeros(1, 3, 5, 4), torch.zeros(1, 3, 5)
    for k in (5, 1, 0):
        with pytest.raises(ValueError, match="num_speaker"):
            separation.dc_masks(emb, logmag, num_speaker=k)
    with pytest.raises(ValueError, match="num_speaker"):
        separation.separate_dc(None, torch.zeros(1, 640), num_speaker=5)


@pytest.mark.parametrize("C", [2, 3, 4])
def test_get_est_sig_takes_the_speaker_count_from_sig_ref(monkeypatch, C):
    """evaluate.py:33: ``num_spk = sig_ref.shape[1]`` -- not a setting of the tester."""
    from onssen_amd import evaluate, features, separation
    B, T, F, D, n = 2, 6, 9, 4, 320
    seen = {}

    def fake_dc_masks(emb, logmag, db_threshold=40.0, iters=20, frames=None, tol=1e-4, num_speaker=2):
        seen["num_speaker"], seen["frames"] = num_speaker, frames
        return torch.zeros(B, T, F, num_speaker)

    def fake_mask_istft(ri, masks, hop, length, frames=None, lengths=None):
        seen["masks"] = tuple(masks.shape)
        return torch.zeros(B, masks.shape[-1], length)
    monkeypatch.setattr(separation, "dc_masks", fake_dc_masks)
    monkeypatch.setattr(features, "mask_istft", fake_mask_istft)
    t = object.__new__(evaluate.tester_dc)
    t.hop_size, t.host_kmeans = 64, False
    label = [torch.zeros(B, T, F), torch.zeros(B, T, F), torch.zeros(B, C, n)]
    est, ref = t.get_est_sig([torch.zeros(B, T, F)], label, [torch.zeros(B, T, F, D)])
    assert seen == {"num_speaker": C, "frames": None, "masks": (B, T, F, C)}
    assert est.shape == ref.shape == (B, C, n)


def test_host_kmeans_builds_one_hot_masks_for_the_references_speaker_count(monkeypatch):
    """The sklearn branch of get_est_sig: ``KMeans(n_clusters=num_spk)`` and ``mask[i, labels == i] = 1`` (evaluate.py:38-41)."""
    from onssen_amd import evaluate, features
    from tests.dc_kmeans_ref import planted
    B, T, F, D, C, n = 1, 5, 17, 8, 3, 320
    emb, feat, _ = planted(1, B, T, F, D, C)
    seen = {}

    def fake_mask_istft(ri, masks, hop, length, frames=None, lengths=None):
        seen["masks"] = masks
        return torch.zeros(B, masks.shape[-1], length)
    monkeypatch.setattr(features, "mask_istft", fake_mask_istft)
    t = object.__new__(evaluate.tester_dc)
    t.hop_size, t.host_kmeans = 64, True
    feat_t = torch.from_numpy(feat)
    t.get_est_sig([feat_t], [torch.zeros(B, T, F), torch.zeros(B, T, F), torch.zeros(B, C, n)], [torch.from_numpy(emb)])
    m = seen["masks"]
    act = feat_t >= feat_t.max() - 2.0
    assert m.shape == (B, T, F, C)
    assert torch.all(m[act].sum(-1) == 1) and torch.all(m[~act] == 0) and torch.all(m[act].sum(0) > 0)


def test_binding_holds_both_new_entries():
    from onssen_amd import _abi
    assert len(_abi.SIGNATURES["onssen_dc_cluster_k_workspace_bytes"][1]) == 5
    assert len(_abi.SIGNATURES["onssen_dc_cluster_k_f32"][1]) == 15
    assert _abi.ABI_VERSION == 14
