"""The enhancement recipe's Python surface without a GPU: loss.loss_mask_msa / loss_mask_psa on their PyTorch route (CPU tensors,
no library) against the float64 restatement (tests/enhance_ref.py) and against the reference's own values
(tests/golden/g8_loss_mask.npz, tools/gen_golden_loss_mask.py); the restatement against float64 autograd of the literal
upstream expressions; the routing rule; the loader's selection rules up to the point where a device is needed."""
import os

import numpy as np
import pytest
import torch

from tests import enhance_ref as R


def _case(B=3, shape=(7, 9), seed=4):
    c = R.loss_case(B, int(np.prod(shape)), seed)
    return {k: torch.from_numpy(v.reshape((B,) + shape)) for k, v in c.items()}


def test_restatement_matches_float64_autograd_of_the_upstream_expressions():
    """loss_mask.py:21 and :39 written out with torch ops in float64: values to 1e-12 relative, gradients exactly (they are
    products of the same float64 factors) -- the planted zero residual, relu clamp and min clamp included."""
    import torch.nn.functional as F
    t = {k: v.double() for k, v in _case().items()}
    est = t["est"].clone().requires_grad_(True)
    msa = torch.nn.MSELoss()(est, t["s"])
    g_msa, = torch.autograd.grad(msa * -1.7, [est])
    ref_utt, ref_total = R.msa(t["est"].numpy(), t["s"].numpy())
    np.testing.assert_allclose(ref_total, float(msa.detach()), rtol=1e-12)
    np.testing.assert_allclose(R.msa_grad(t["est"].numpy(), t["s"].numpy(), -1.7), g_msa.numpy(), rtol=1e-12, atol=0)
    mask = t["est"].clone().requires_grad_(True)
    r = mask * t["x"] - torch.min(t["x"], F.relu(t["s"] * t["c"]))
    psa = torch.sum(torch.abs(r.reshape(r.size()[0], -1)), dim=1)               # loss_util.norm_1d
    g = torch.tensor([0.7, -1.3, 0.4]).double()
    g_psa, = torch.autograd.grad((psa * g).sum(), [mask])
    args = [t[k].numpy() for k in ("est", "x", "s", "c")]
    np.testing.assert_allclose(R.psa(*args), psa.detach().numpy(), rtol=1e-12)
    ref_g = R.psa_grad(*args, g.numpy())
    np.testing.assert_array_equal(ref_g, g_psa.numpy())
    assert (ref_g[:, 0, 0] == 0).all() and (ref_g[:, 0, 1] != 0).all()          # sign(0) = 0 at the planted zero residual


def test_cpu_paths_match_the_restatement():
    from onssen_amd import loss as L
    t = _case()
    msa = L.loss_mask_msa([t["est"]], [t["s"], t["c"]])
    assert L.last_enhance_path == "aten" and msa.dim() == 0 and msa.dtype == torch.float32
    ref_utt, ref_total = R.msa(t["est"].numpy(), t["s"].numpy())
    assert abs(float(msa) - ref_total) <= 1e-5 * ref_total                     # a float32 mean of non-negative float32 terms
    psa = L.loss_mask_psa([t["est"]], [t["x"], t["s"], t["c"]])
    assert L.last_enhance_path == "aten" and tuple(psa.shape) == (3,)
    ref = R.psa(*(t[k].numpy() for k in ("est", "x", "s", "c")))
    assert (np.abs(psa.numpy() - ref) <= 1e-5 * 2.0 * t["x"].double().flatten(1).sum(1).numpy()).all()
    # gradients flow to the estimate on this route, and only to it
    est = t["est"].clone().requires_grad_(True)
    lab = t["s"].clone().requires_grad_(True)
    L.loss_mask_msa([est], [lab.detach(), t["c"]]).backward()
    np.testing.assert_allclose(est.grad.numpy(), R.msa_grad(t["est"].numpy(), t["s"].numpy()), rtol=1e-5, atol=1e-9)


def test_reference_values(golden_dir):
    """What the reference's own loss_mask module returned for these arrays: the CPU route and the restatement both hold it."""
    from onssen_amd import loss as L
    gold = np.load(os.path.join(golden_dir, "g8_loss_mask.npz"))
    assert gold["clean_est"].shape == (3, 7, 129) and gold["msa"].shape == () and gold["psa"].shape == (3,)
    t = {k: torch.from_numpy(gold[k]) for k in ("clean_est", "mask", "mag_noisy", "mag_clean", "cos_diff")}
    msa = L.loss_mask_msa([t["clean_est"]], [t["mag_clean"], t["cos_diff"]])
    psa = L.loss_mask_psa([t["mask"]], [t["mag_noisy"], t["mag_clean"], t["cos_diff"]])
    np.testing.assert_allclose(msa.numpy(), gold["msa"], rtol=1e-6)             # the same float32 ops, up to the order of a sum
    np.testing.assert_allclose(psa.numpy(), gold["psa"], rtol=1e-6)
    _, ref_total = R.msa(gold["clean_est"], gold["mag_clean"])
    np.testing.assert_allclose(ref_total, gold["msa"], rtol=1e-5)               # float32 sums of ~2700 terms against float64
    np.testing.assert_allclose(R.psa(gold["mask"], gold["mag_noisy"], gold["mag_clean"], gold["cos_diff"]), gold["psa"], rtol=1e-5)


def test_routing(monkeypatch):
    from onssen_amd import loss as L
    for env, with_grad in (("1", "grad"), ("0", "aten")):
        monkeypatch.setenv("ONSSEN_LOSS_HIP", env)
        assert L._enhance_route(False, False) == "aten" and L._enhance_route(False, True) == "aten"      # always on the CPU
        assert L._enhance_route(True, False) == "value"                                                   # no gradient wanted
        assert L._enhance_route(True, True) == with_grad
    # a gradient is wanted only with autograd on and an estimate that requires one
    t = _case()
    est = t["est"].clone().requires_grad_(True)
    assert not L._no_grad_needed(est)
    with torch.no_grad():
        assert L._no_grad_needed(est)
    assert L._no_grad_needed(t["est"])


def test_wrong_counts_raise():
    from onssen_amd import loss as L
    t = _case()
    with pytest.raises(AssertionError, match="1 tensor"):
        L.loss_mask_msa([t["est"], t["est"]], [t["s"], t["c"]])
    with pytest.raises(AssertionError, match="2 tensors"):
        L.loss_mask_msa([t["est"]], [t["x"], t["s"], t["c"]])
    with pytest.raises(AssertionError, match="1 tensor"):
        L.loss_mask_psa([], [t["x"], t["s"], t["c"]])
    with pytest.raises(AssertionError, match="3 tensors"):
        L.loss_mask_psa([t["est"]], [t["s"], t["c"]])


def test_public_names():
    from onssen_amd import data, evaluate, features, loss, separation
    from onssen_amd.nn.enhancement import enhance
    assert callable(loss.loss_mask_msa) and callable(loss.loss_mask_psa)
    assert callable(features.mag_istft) and callable(features.enhance_labels) and callable(separation.separate_enhance)
    assert issubclass(evaluate.tester_enhance, evaluate.tester) and callable(data.daps_enhance_dataloader)
    import inspect
    assert list(inspect.signature(data.daps_enhance_dataloader).parameters) == ["num_batch", "feature_options", "partition", "device"]
    assert list(inspect.signature(enhance.forward).parameters) == ["self", "input", "frames"]
    with pytest.raises(RuntimeError, match="ROCm device"):
        features.mag_istft(torch.zeros(1, 3, 129, 2), torch.zeros(1, 3, 129, 1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        features.enhance_labels(torch.zeros(3, 129, 2), torch.zeros(3, 129, 2))
    # frames= is an inference-path extension: the autograd path (here: a model in train mode) refuses it
    model = enhance(9, 4, 1)
    with pytest.raises(RuntimeError, match="inference-path"):
        model([torch.zeros(2, 5, 9), torch.zeros(2, 5, 9)], frames=[5, 3])


FO = dict(batch_size=2, frame_length=10, sampling_rate=8000, window_size=256, hop_size=64)


def test_loader_selection(tmp_path, monkeypatch):
    from onssen_amd import data
    monkeypatch.delenv("ONSSEN_SYNTHETIC_DATA", raising=False)
    for path in ("", "synthetic", None):
        ld = data.daps_enhance_dataloader(5, dict(FO, data_path=path), "train")
        assert isinstance(ld, data.SyntheticDapsEnhance) and len(ld) == 5 and ld.voices is None      # nothing on a device yet
    assert isinstance(data.daps_enhance_dataloader(5, FO, "train"), data.SyntheticDapsEnhance)       # no data_path at all
    # a data_path that is given but holds no list file for the partition: never synthetic by accident
    with pytest.raises(FileNotFoundError, match="no list file"):
        data.daps_enhance_dataloader(5, dict(FO, data_path=str(tmp_path)), "train")
    monkeypatch.setenv("ONSSEN_SYNTHETIC_DATA", "1")
    assert isinstance(data.daps_enhance_dataloader(5, dict(FO, data_path=str(tmp_path)), "train"), data.SyntheticDapsEnhance)
    monkeypatch.delenv("ONSSEN_SYNTHETIC_DATA")
    # a tree: the list file names the noisy recordings, the clean one is <data_path>/clean/<a>_<b>_clean.wav
    (tmp_path / "train").write_text("noisy/f1_script2_ipad_office1.wav\n\n" + str(tmp_path / "noisy" / "m3_script1_iphone_balcony1.wav") + "\n")
    ld = data.daps_enhance_dataloader(4, dict(FO, data_path=str(tmp_path)), "train")
    assert isinstance(ld, data.DapsEnhanceFiles) and len(ld) == 4 and len(ld.files) == 2 and ld.shuffle and not ld.evaluation
    assert ld.paths(ld.files[0]) == (str(tmp_path / "noisy" / "f1_script2_ipad_office1.wav"), str(tmp_path / "clean" / "f1_script2_clean.wav"))
    assert ld.paths(ld.files[1])[1] == str(tmp_path / "clean" / "m3_script1_clean.wav")
    with pytest.raises(FileNotFoundError, match="no list file"):
        data.daps_enhance_dataloader(4, dict(FO, data_path=str(tmp_path)), "validation")
    (tmp_path / "tt").write_text("noisy/f1_script2_ipad_office1.wav\n")
    ev = data.daps_enhance_dataloader(4, dict(FO, data_path=str(tmp_path)), "tt")
    assert ev.evaluation and not ev.shuffle and len(ev) == 1
    (tmp_path / "validation").write_text("\n")
    with pytest.raises(FileNotFoundError, match="names no recordings"):
        data.daps_enhance_dataloader(4, dict(FO, data_path=str(tmp_path)), "validation")
