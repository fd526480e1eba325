"""The Edinburgh recipe's surface without a GPU: exports, list-file and path resolution, the missing-tree rule, option validation,
the CPU refusal of features.resample and the resampler's host entries (through the host-side build, tests/emu)."""
import os

import numpy as np
import pytest
import torch

FO = dict(batch_size=2, frame_length=50, sampling_rate=16000, window_size=256, hop_size=64, db_threshold=40)


@pytest.fixture
def clean_options(monkeypatch):
    from onssen_amd import options
    for env, *_ in options.TABLE.values():
        monkeypatch.delenv(env, raising=False)
    saved = dict(options._configured)
    options._configured.clear()
    yield options
    options._configured.clear()
    options._configured.update(saved)


def make_tree(root, names, rate=48000, n=4800):
    from onssen_amd.data import write_wav
    from onssen_amd.data.edinburgh_tts import CLEAN_DIR, NOISY_DIR
    rng = np.random.default_rng(1)
    for d in (NOISY_DIR, CLEAN_DIR):
        os.makedirs(os.path.join(root, d), exist_ok=True)
        for name in names:
            write_wav(os.path.join(root, d, name), rng.uniform(-0.5, 0.5, n), rate)
    with open(os.path.join(root, "train"), "w") as f:
        f.write("\n".join(names) + "\n\n")


def test_exports():
    import onssen_amd.data as d
    for name in ("edinburgh_tts_dataloader", "EdinburghTtsFiles", "SyntheticEdinburghTts", "get_stft_from_subtraction"):
        assert name in d.__all__ and hasattr(d, name)
    assert d.get_stft_from_subtraction is d.feature_utils.get_stft_from_subtraction
    assert "get_stft_from_subtraction" in d.feature_utils.__all__
    from onssen_amd import features
    assert callable(features.resample)


def test_list_file_and_path_resolution(tmp_path):
    from onssen_amd.data import EdinburghTtsFiles, edinburgh_tts_dataloader
    names = ["p226_001.wav", "p226_002.wav", "p287_010.wav"]
    make_tree(str(tmp_path), names)
    fo = dict(FO, data_path=str(tmp_path))
    dl = edinburgh_tts_dataloader("chimera++", fo, "train")
    assert isinstance(dl, EdinburghTtsFiles) and len(dl) == 2                     # 3 recordings, batches of 2
    assert [os.path.basename(f) for f in dl.file_list] == names                   # list order; the blank line is no recording
    noisy, clean = dl._sources(dl.file_list[2])
    assert noisy == os.path.join(str(tmp_path), "noisy_trainset_28spk_wav", "p287_010.wav")
    assert clean == os.path.join(str(tmp_path), "clean_trainset_28spk_wav", "p287_010.wav")
    assert os.path.isfile(noisy) and os.path.isfile(clean)
    assert dl.shuffle and not dl.evaluation
    os.replace(os.path.join(str(tmp_path), "train"), os.path.join(str(tmp_path), "tt"))
    ev = edinburgh_tts_dataloader("chimera", fo, "tt")
    assert ev.evaluation and not ev.shuffle and len(ev) == 3                      # whole recordings, one per item


def test_missing_tree_and_synthetic_only_when_asked(tmp_path, clean_options, monkeypatch):
    from onssen_amd.data import SyntheticEdinburghTts, edinburgh_tts_dataloader
    with pytest.raises(FileNotFoundError, match="no list file"):
        edinburgh_tts_dataloader("dc", dict(FO, data_path=str(tmp_path)), "train")
    (tmp_path / "train").write_text("\n")
    with pytest.raises(FileNotFoundError, match="names no recordings"):
        edinburgh_tts_dataloader("dc", dict(FO, data_path=str(tmp_path)), "train")
    for path in ("", "synthetic", None):
        assert isinstance(edinburgh_tts_dataloader("dc", dict(FO, data_path=path), "train"), SyntheticEdinburghTts)
    monkeypatch.setenv("ONSSEN_SYNTHETIC_DATA", "1")
    dl = edinburgh_tts_dataloader("dc", dict(FO, data_path=str(tmp_path / "nowhere")), "validation")
    assert isinstance(dl, SyntheticEdinburghTts) and len(dl) == 8


def test_unknown_model_name(tmp_path):
    from onssen_amd.data import edinburgh_tts_dataloader
    make_tree(str(tmp_path), ["a.wav"])
    for name in ("upit", "enhance", "tasnet", ""):
        with pytest.raises(ValueError, match="unknown model_name"):
            edinburgh_tts_dataloader(name, dict(FO, data_path=str(tmp_path)), "train")
        with pytest.raises(ValueError, match="unknown model_name"):
            edinburgh_tts_dataloader(name, dict(FO, data_path=""), "train")


def test_loader_resample_option(clean_options, monkeypatch):
    o = clean_options
    env, default, conv, doc = o.TABLE["loader_resample"]
    assert env == "ONSSEN_LOADER_RESAMPLE" and default == "scipy" and o.get("loader_resample") == "scipy"
    o.configure(loader_resample="hip")
    assert o.get("loader_resample") == "hip"
    o.configure(loader_resample="SciPy")
    assert o.get("loader_resample") == "scipy"
    with pytest.raises(ValueError, match="loader_resample"):
        o.configure(loader_resample="librosa")
    o.configure(loader_resample=None)
    monkeypatch.setenv("ONSSEN_LOADER_RESAMPLE", "hip")
    assert o.get("loader_resample") == "hip" and o.describe()["loader_resample"]["source"] == "env"
    monkeypatch.delenv("ONSSEN_LOADER_RESAMPLE")
    kwargs = o.apply_config({"model_options": {"hidden_dim": 8}, "feature_options": {"loader_resample": "hip"}})
    assert kwargs == {"hidden_dim": 8} and o.get("loader_resample") == "hip"


def test_reference_config_loads_unchanged(clean_options):
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_edinburgh_tts.json")) as f:
        args = json.load(f)
    assert clean_options.apply_config(args) == dict(args["model_options"])
    assert all(v["source"] == "default" for v in clean_options.describe().values())
    assert args["dataset"] == "edinburgh_tts" and args["feature_options"]["sampling_rate"] == 16000


def test_resample_refuses_cpu_tensors():
    from onssen_amd.features import resample
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample(torch.zeros(2, 100), 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resample(torch.zeros(100), 44100, 16000, sub=torch.zeros(100))


def test_host_entries_through_the_emulation_library():
    from tests.emu_build import load_emu
    lib = load_emu()
    assert lib.resample_geometry(48000, 16000, 1000) == (1, 3, 30, 334)
    assert lib.resample_geometry(44100, 16000, 2000) == (160, 441, 4410, 726)
    assert lib.resample_geometry(8000, 16000, 5) == (2, 1, 20, 10)
    assert lib.resample_geometry(16000, 16000, 7) == (1, 1, 0, 7)                 # equal rates: the identity, one tap
    assert list(lib.resample_taps(5, 5)) == [1.0]
    assert lib.resample_workspace_bytes(1, 3) == 61 * 8 and lib.resample_workspace_bytes(160, 441) == 160 * 56 * 8
    taps = np.array(lib.resample_taps(160, 441))
    assert taps.shape == (8821,) and abs(taps.sum() - 160.0) < 1e-9 and np.array_equal(taps, taps[::-1])
