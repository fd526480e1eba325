"""The Edinburgh noisy-speech recipe end to end on the device: edinburgh_tts_dataloader over a generated tree (48 kHz and
44.1 kHz PCM16 pairs, 16 kHz features), get_stft_from_subtraction and the DAPS loader's ``loader_resample = "hip"`` route.

The resampler itself is pinned to SciPy in tests/test_gpu_resample.py; here
  composition    the loader's tensors equal, bit for bit, the batch built by hand from read_wav -> features.resample(sub=) ->
                 stft_logmag(lengths=) -> wrap-crop -> training_labels
  anchor         mag_mix against a NumPy float64 STFT (periodic Hann, centred, reflect padding: oracle/np_oracle.py) of the
                 SciPy-float64-resampled signal, per bin within window_size * 2^-23 * max|x|: each resampled sample is within one
                 fp32 rounding (2^-24 max|x|), passed through a window-weighted sum of window_size terms (mean weight 1/2), the
                 spectrum is stored as fp32 (2^-24 |X|, |X| <= window_size / 2 max|x|) and |X| is one more fp32 operation
  DAPS opt-in    the two routes round independently: twice that bound."""
import os

import numpy as np
import pytest
import torch

from oracle import np_oracle as O
from tests import resample_ref as R

pytestmark = pytest.mark.gpu

FO = dict(batch_size=2, frame_length=50, sampling_rate=16000, window_size=256, hop_size=64, db_threshold=40)
# (name, rate, samples): the third is shorter than frame_length frames at 16 kHz (2000 samples, 32 frames); the second is 44.1 kHz
FILES = [("p226_001.wav", 48000, 30011), ("p226_002.wav", 44100, 21013), ("p226_003.wav", 48000, 6000),
         ("p227_001.wav", 48000, 17777), ("p227_002.wav", 48000, 24000), ("p228_001.wav", 48000, 12345)]
MODELS = ("dc", "chimera", "chimera++", "phase")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()   # fail loudly if libonssen_hip.so is missing
    return torch.device("cuda:0")


def pair(seed, rate, n):
    """(noisy, clean): a few decaying partials plus white noise at ~10 dB."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    clean = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.3, 0.2, 0.1), rng.uniform(100, 3000, 3), rng.uniform(0, 6, 3)))
    clean = clean * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    return (clean + 0.1 * rng.standard_normal(n)).astype(np.float32), clean.astype(np.float32)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from onssen_amd.data import write_wav
    from onssen_amd.data.edinburgh_tts import CLEAN_DIR, NOISY_DIR
    root = str(tmp_path_factory.mktemp("edinburgh"))
    for d in (NOISY_DIR, CLEAN_DIR):
        os.makedirs(os.path.join(root, d))
    for k, (name, rate, n) in enumerate(FILES):
        noisy, clean = pair(100 + k, rate, n)
        write_wav(os.path.join(root, NOISY_DIR, name), noisy, rate)
        write_wav(os.path.join(root, CLEAN_DIR, name), clean, rate)
    for part in ("train", "tt"):
        with open(os.path.join(root, part), "w") as f:
            f.write("".join(name + "\n" for name, _, _ in FILES))
    return root


def signals(tree, k):
    """(noisy, clean, rate) of recording k as read_wav gives them."""
    from onssen_amd.data import read_wav
    from onssen_amd.data.edinburgh_tts import CLEAN_DIR, NOISY_DIR
    noisy, rate = read_wav(os.path.join(tree, NOISY_DIR, FILES[k][0]))
    clean, rate_c = read_wav(os.path.join(tree, CLEAN_DIR, FILES[k][0]))
    assert rate == rate_c == FILES[k][1] and len(noisy) == len(clean) == FILES[k][2]
    return noisy, clean, rate


def triple(tree, k, dev):
    """Rows (noisy, clean, noise) of recording k at 16 kHz, by three batch-1 resample calls: (3, n) device tensor."""
    from onssen_amd.features import resample
    noisy, clean, rate = signals(tree, k)
    nd, cd = torch.from_numpy(noisy).to(dev), torch.from_numpy(clean).to(dev)
    return torch.cat([resample(nd, rate, 16000)[0], resample(cd, rate, 16000)[0], resample(nd, rate, 16000, sub=cd)[0]])


@pytest.fixture(scope="module")
def by_hand(tree, dev):
    """Per batch of two recordings in list order: (logmag (B, 3, L, F), ri (B, 3, L, F, 2)), built stage by stage."""
    from onssen_amd.features import stft_logmag
    L, hop, out = FO["frame_length"], FO["hop_size"], []
    for k0 in range(0, len(FILES), 2):
        rows = [triple(tree, k, dev) for k in range(k0, min(k0 + 2, len(FILES)))]
        n = [r.shape[1] for r in rows]
        wav = torch.zeros(len(rows), 3, max(n), device=dev)
        for b, r in enumerate(rows):
            wav[b, :, :n[b]] = r
        logmag, ri = stft_logmag(wav.view(-1, max(n)), FO["window_size"], hop, lengths=np.repeat(n, 3))
        lm, sp = [], []
        for b in range(len(rows)):
            idx = torch.arange(L, device=dev) % (1 + n[b] // hop)            # the first L frames, a short utterance repeated
            lm.append(logmag[3 * b:3 * b + 3][:, idx])
            sp.append(ri[3 * b:3 * b + 3][:, idx])
        out.append((torch.stack(lm), torch.stack(sp)))
    return out


@pytest.mark.parametrize("model_name", MODELS)
def test_loader_composes_the_pinned_stages(tree, dev, by_hand, model_name):
    from onssen_amd.data import EdinburghTtsFiles
    from onssen_amd.features import training_labels
    dl = EdinburghTtsFiles(model_name, dict(FO, data_path=tree), "train", dev, shuffle=False)
    assert len(dl) == 3
    batches = list(dl)
    assert len(batches) == 3
    assert 1 + R.n_out(FILES[2][2], 1, 3) // FO["hop_size"] < FO["frame_length"]          # the double-copy wrap is exercised
    for (inp, lab), (logmag, ri) in zip(batches, by_hand):
        feat = logmag[:, 0].contiguous()
        mix, s1, s2 = (ri[:, i].contiguous() for i in range(3))
        one_hot, mm, m1, m2, c1, c2 = training_labels(mix, s1, s2, feat, 40.0, with_cos=True)
        want_in = [feat, mix] if model_name == "phase" else [feat]
        want_lab = {"dc": [one_hot.double(), mm], "chimera": [one_hot.double(), mm, m1, m2],
                    "chimera++": [one_hot.double(), mm, m1, m2, c1, c2], "phase": [one_hot.double(), mm, m1, m2, s1, s2]}[model_name]
        assert len(inp) == len(want_in) and len(lab) == len(want_lab)
        for got, want in zip(list(inp) + list(lab), want_in + want_lab):
            assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
        assert inp[0].shape == (2, 50, 129) and float(lab[1].abs().max()) > 0


def stft64(x, n_fft, hop):
    y = np.pad(np.asarray(x, np.float64), n_fft // 2, mode="reflect")
    idx = np.arange(n_fft)[None, :] + hop * np.arange(1 + (len(y) - n_fft) // hop)[:, None]
    return np.fft.rfft(y[idx] * O.hann_periodic(n_fft)[None, :].astype(np.float64), axis=1)


def test_mag_mix_against_numpy_stft_of_the_scipy_resampled_signal(tree, dev):
    from onssen_amd.data import EdinburghTtsFiles
    dl = EdinburghTtsFiles("chimera", dict(FO, data_path=tree), "train", dev, shuffle=False)
    (feat,), (one_hot, mag_mix, mag_s1, mag_s2) = next(iter(dl))
    worst = 0.0
    for b in range(2):                                                   # one 48 kHz and one 44.1 kHz recording
        noisy, clean, rate = signals(tree, b)
        up, down = R.reduced(16000, rate)
        for got, x in ((mag_mix[b], R.reference(noisy, up, down)), (mag_s1[b], R.reference(clean, up, down)),
                       (mag_s2[b], R.reference(noisy, up, down, sub=clean))):
            ref = np.abs(stft64(x, 256, 64))[:50]
            bound = 256 * 2.0 ** -23 * np.abs(x).max()
            worst = max(worst, float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / bound))
    print(f"largest | |X| - ref | / bound = {worst:.3f}")
    assert worst <= 1.0


def test_reference_config(tree, dev):
    """The reference's own egs/edinburgh_tts/config.json drives the loader: its feature_options with only the corpus path, the
    batch size and the chunk length overridden."""
    import json
    from onssen_amd import options
    from onssen_amd.data import edinburgh_tts_dataloader
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_edinburgh_tts.json")) as f:
        args = json.load(f)
    assert options.apply_config(args) == dict(args["model_options"])
    fo = dict(args["feature_options"], data_path=tree, batch_size=2, frame_length=20)
    assert fo["window_size"] == 1024 and fo["hop_size"] == 256 and fo["sampling_rate"] == 16000
    inp, lab = next(iter(edinburgh_tts_dataloader(args["model_name"], fo, "train", dev)))
    assert args["model_name"] == "chimera++" and len(inp) == 1 and len(lab) == 6
    for t in list(inp) + lab[1:]:
        assert tuple(t.shape) == (2, 20, 513) and torch.isfinite(t).all()
    assert tuple(lab[0].shape) == (2, 20, 513, 2)


def test_evaluation_partition_through_tester_chimera(tree, dev):
    """Partition "tt": whole recordings in tester_chimera's contract.  The mean SI-SDR of eval() equals the one computed by hand from
    the files: resample -> STFT -> the network's masks -> inverse transform at the reference's padded length -> batch_SDR_torch
    (the stages of separate_chimera, whose own output stops at the unpadded length: the tester scores the padded one)."""
    from onssen_amd import nn as onn
    from onssen_amd.data import edinburgh_tts_dataloader
    from onssen_amd.evaluate import batch_SDR_torch, tester_chimera
    from onssen_amd.features import mask_istft, stft_logmag
    from onssen_amd.synthetic import make_state_dict
    sd = make_state_dict("chimera", 129, 48, 2, 20, 2, seed=4, gain=1.5)         # tests/test_gpu_parity.py: the smallest chimera
    m = onn.chimera(129, 48, 2, 20)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    loader = list(edinburgh_tts_dataloader("chimera", dict(FO, data_path=tree), "tt", dev))
    assert len(loader) == len(FILES)
    got = tester_chimera(dict(model=m, test_loader=loader, device=str(dev), model_name="chimera")).eval()
    assert np.isfinite(got)
    total = 0.0
    for k, ((feat,), (sr, si, sig_ref)) in enumerate(loader):
        rows = triple(tree, k, dev)
        n = rows.shape[1]
        assert feat.shape == sr.shape == si.shape == (1, 1 + n // 64, 129)
        assert sig_ref.shape == (1, 2, n + 32 - n % 32) and torch.equal(sig_ref[0, :, :n], rows[1:]) and (sig_ref[0, :, n:] == 0).all()
        with torch.no_grad():
            logmag, ri = stft_logmag(rows[:1], 256, 64)
            _, mask_a, mask_b = m([logmag])
            est = mask_istft(ri, torch.stack([mask_a, mask_b], -1), 64, sig_ref.shape[-1])
        total += float(batch_SDR_torch(est, sig_ref).double().sum())
    want = total / len(FILES)
    print(f"mean SI-SDR: eval() {got:.6f}, by hand {want:.6f}")
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want))


def test_get_stft_from_subtraction_on_the_device(tmp_path, dev, monkeypatch):
    from onssen_amd.data import get_stft, get_stft_from_subtraction, write_wav
    monkeypatch.setenv("ONSSEN_LOADER_RESAMPLE", "hip")
    noisy, clean = pair(7, 48000, 20011)
    f_mix, f_clean = str(tmp_path / "mix.wav"), str(tmp_path / "clean.wav")
    write_wav(f_mix, noisy, 48000, subtype="FLOAT")
    write_wav(f_clean, clean, 48000, subtype="FLOAT")
    worst = 0.0
    for got, x in ((get_stft_from_subtraction(f_mix, f_clean, 16000, 256, 64), R.reference(noisy, 1, 3, sub=clean)),
                   (get_stft(f_mix, 16000, 256, 64), R.reference(noisy, 1, 3))):
        ref = stft64(x, 256, 64)
        assert got.dtype == np.complex64 and got.shape == ref.shape == (1 + 6671 // 64, 129)
        worst = max(worst, float(np.abs(got.astype(np.complex128) - ref).max() / (256 * 2.0 ** -23 * np.abs(x).max())))
    print(f"largest |X - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_daps_loader_resamples_on_the_device_when_asked(tmp_path, dev, monkeypatch):
    from onssen_amd.data import DapsEnhanceFiles, write_wav
    os.makedirs(tmp_path / "clean")
    names, sigs = ["f1_script1_ipad.wav", "m2_script3_ipad.wav"], []
    for k, name in enumerate(names):
        noisy, clean = pair(50 + k, 44100, 20000 + 1000 * k)
        write_wav(str(tmp_path / name), noisy, 44100)
        write_wav(str(tmp_path / "clean" / ("_".join(name.split("_")[:2]) + "_clean.wav")), clean, 44100)
    (tmp_path / "train").write_text("\n".join(names) + "\n")
    (tmp_path / "tt").write_text("\n".join(names) + "\n")
    fo = dict(FO, data_path=str(tmp_path), frame_length=20)
    monkeypatch.delenv("ONSSEN_LOADER_RESAMPLE", raising=False)
    host = next(iter(DapsEnhanceFiles(1, fo, "train", dev, shuffle=False)))
    host_eval = list(DapsEnhanceFiles(1, fo, "tt", dev))
    monkeypatch.setenv("ONSSEN_LOADER_RESAMPLE", "hip")
    device = next(iter(DapsEnhanceFiles(1, fo, "train", dev, shuffle=False)))
    device_eval = list(DapsEnhanceFiles(1, fo, "tt", dev))
    for a, b in zip(host[0] + host[1] + [t for item in host_eval for part in item for t in part],
                    device[0] + device[1] + [t for item in device_eval for part in item for t in part]):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.isfinite(b).all()
    from onssen_amd.data import read_wav                       # both chunks of the batch come from the first recording
    x_noisy = R.reference(read_wav(str(tmp_path / names[0]))[0], 160, 441)
    x_clean = R.reference(read_wav(str(tmp_path / "clean" / "f1_script1_clean.wav"))[0], 160, 441)
    worst = 0.0
    for a, b, x in ((host[0][1], device[0][1], x_noisy), (host[1][0], device[1][0], x_clean)):
        worst = max(worst, float((a.double() - b.double()).abs().max() / (2 * 256 * 2.0 ** -23 * np.abs(x).max())))
    print(f"largest |mag(host route) - mag(device route)| / bound = {worst:.3f}")
    assert worst <= 1.0
