"""Speech-enhancement loader with the reference's call signature and yield contract (onssen/data/daps_enhance.py:30-126).

``daps_enhance_dataloader(num_batch, feature_options, partition, device)`` of the reference wraps a stateful dataset in a
``DataLoader(batch_size, shuffle=True)``: the list file ``<data_path>/<partition>`` names the noisy recordings, the clean one of
``.../<a>_<b>_<...>.wav`` is ``<data_path>/clean/<a>_<b>_clean.wav``, a file whose rate differs from ``sampling_rate`` is
resampled, and every ``__getitem__`` hands out the NEXT ``frame_length`` frames of the current recording until fewer than
``frame_length`` remain, then opens another one -- so a batch is ``batch_size`` consecutive chunks of that stream and an epoch
is ``num_batch`` batches.  Each item is ``[feature, mag_noisy], [mag_clean, cos_diff]``.

Here the batch is built at once and on the device: per recording ONE ``stft_logmag`` launch transforms the noisy and the clean
signal together, the chunks of a batch are gathered, and ONE ``enhance_labels`` launch gives the three label maps; every tensor
is ``(batch_size, frame_length, F)``.  Files are taken in shuffled order (``shuffle=False``: list order), a list that is used
up is read again, and the position in the stream carries over from one epoch to the next, as the reference's dataset keeps it.
A recording shorter than ``frame_length`` frames gives no chunk (the reference would hand out a short one and fail to collate).

An evaluation partition (``"tt"`` or ``"test"``, the wsj0-2mix loader's convention) yields whole recordings, batch 1, in list
order, in the contract of ``evaluate.tester_enhance``: ``[feature_noisy (1,T,F), mag_noisy (1,T,F)]``,
``[stft_r (1,T,F), stft_i (1,T,F), sig_ref (1,1,n)]`` with the clean signal zero-padded by ``32 - n % 32`` samples.

Without a tree the rule of ``onssen_amd.data`` applies: the synthetic corpus (``SyntheticDapsEnhance``) is used only when
``data_path`` is absent / ``""`` / ``"synthetic"`` or ``ONSSEN_SYNTHETIC_DATA=1`` is set; a ``data_path`` that is given but holds
no list file for the partition raises ``FileNotFoundError``.

A file whose rate differs from ``sampling_rate`` (DAPS is a 44.1 kHz corpus) is resampled by ``scipy.signal.resample_poly`` on
the host (see data/wsj0_2mix.py), or -- option ``loader_resample = "hip"`` -- the noisy / clean pair goes to the device at its own
rate in one transfer and through ONE ``features.resample`` launch (the same filter, csrc/resample.inc) before the STFT.

Not here: log-mel features (``get_log_mel_spectrogram``: no recipe of the reference calls it).  ``edinburgh_tts_dataloader`` and
``get_stft_from_subtraction`` are in data/edinburgh_tts.py and data/feature_utils.py."""
import os

import numpy as np
import torch

from .. import options

EVAL_PARTITIONS = ("tt", "test")


def _getter(fo):
    return (lambda k, d=None: fo.get(k, d)) if isinstance(fo, dict) else (lambda k, d=None: getattr(fo, k, d))


def _geometry(self, num_batch, feature_options, partition, device):
    g = _getter(feature_options)
    self.num_batch, self.partition = int(num_batch), partition
    self.batch_size, self.frame_length = int(g("batch_size")), int(g("frame_length"))
    self.sampling_rate, self.window_size, self.hop_size = int(g("sampling_rate")), int(g("window_size")), int(g("hop_size"))
    self.device = torch.device(device if device is not None else "cuda:0")
    self.evaluation = partition in EVAL_PARTITIONS


def _eval_item(noisy, clean, window_size, hop_size, device):
    """One whole recording in the evaluation contract (the STFT of the file as it is; only the reference is padded).
    ``noisy`` / ``clean``: host arrays, or 1-D tensors on the device."""
    from ..features import enhance_labels, stft_logmag
    n = min(len(noisy), len(clean))
    if torch.is_tensor(noisy):
        wav = noisy[None, :n]
        sig_ref = torch.nn.functional.pad(clean[:n], (0, 32 - n % 32))[None, None]
    else:
        wav = torch.from_numpy(np.ascontiguousarray(noisy[:n])[None]).to(device)
        sig_ref = torch.from_numpy(np.pad(clean[:n], (0, 32 - n % 32))[None, None]).to(device)
    logmag, ri = stft_logmag(wav, window_size, hop_size)
    mag_noisy = enhance_labels(ri, None)[0]
    return [logmag, mag_noisy], [ri[..., 0].contiguous(), ri[..., 1].contiguous(), sig_ref]


def resampled_pair(f_a, f_b, sampling_rate, device):
    """Two files' signals at ``sampling_rate`` as the rows of ONE device tensor, cut to the shorter one: (wav (2, n), n).  The
    pair is uploaded as it is read, in one transfer, and converted by ONE ``features.resample`` launch (two when the files'
    rates differ)."""
    from ..features import resample
    from .wsj0_2mix import read_wav
    (a, rate_a), (b, rate_b) = read_wav(f_a), read_wav(f_b)
    host = np.zeros((2, max(len(a), len(b))), np.float32)
    host[0, :len(a)], host[1, :len(b)] = a, b
    wav = torch.from_numpy(host).to(device)
    if rate_a == rate_b:
        y, _ = resample(wav, rate_a, sampling_rate, lengths=[len(a), len(b)])
    else:
        ya, yb = resample(wav[:1, :len(a)], rate_a, sampling_rate)[0], resample(wav[1:, :len(b)], rate_b, sampling_rate)[0]
        n = min(ya.shape[1], yb.shape[1])
        y = torch.cat([ya[:, :n], yb[:, :n]])
    n = min(-(-len(a) * sampling_rate // rate_a), -(-len(b) * sampling_rate // rate_b))
    return y[:, :n], n


class DapsEnhanceFiles:
    """Iterable over ``(input_list, label_list)`` batches of one partition of a DAPS-style tree; ``len()`` = batches per epoch
    (``num_batch``; the number of recordings for an evaluation partition)."""

    def __init__(self, num_batch, feature_options, partition="train", device=None, shuffle=None, seed=None):
        _geometry(self, num_batch, feature_options, partition, device)
        self.base_path = _getter(feature_options)("data_path")
        self.list_file = os.path.join(self.base_path, partition)
        with open(self.list_file) as f:
            self.files = [line.strip() for line in f if line.strip()]
        if not self.files:
            raise FileNotFoundError(f"daps_enhance_dataloader: the list file {self.list_file!r} names no recordings")
        self.shuffle = (not self.evaluation) if shuffle is None else bool(shuffle)
        self.rng = np.random.default_rng(seed)
        self.pending = []            # recordings of the current pass over the list that have not been opened yet
        self.opened = []             # every recording opened so far, in order (what the stream has consumed)
        self.cur = None              # (feature (T,F), stft_noisy (T,F,2), stft_clean (T,F,2)) of the current recording
        self.at = 0                  # its next frame

    def __len__(self):
        return len(self.files) if self.evaluation else self.num_batch

    def paths(self, f_noisy):
        """(noisy, clean) paths of one line of the list file (daps_enhance.py:95-97); a relative line that does not exist as it
        stands is taken relative to ``data_path``."""
        names = os.path.basename(f_noisy).split("_")
        if not os.path.isabs(f_noisy) and not os.path.exists(f_noisy):
            f_noisy = os.path.join(self.base_path, f_noisy)
        return f_noisy, os.path.join(self.base_path, "clean", names[0] + "_" + names[1] + "_clean.wav")

    def _signals(self, f_noisy):
        from .wsj0_2mix import _load
        return tuple(_load(p, self.sampling_rate) for p in self.paths(f_noisy))

    def _open_next(self):
        """The next recording with at least one chunk in it: both signals through ONE STFT launch."""
        from ..features import stft_logmag
        hip = options.get("loader_resample") == "hip"
        skipped = 0
        while True:
            if not self.pending:
                order = self.rng.permutation(len(self.files)) if self.shuffle else np.arange(len(self.files))
                self.pending = [self.files[i] for i in order]
            fn = self.pending.pop(0)
            if hip:                    # the pair at its own rate in one transfer, one resample launch
                wav, n = resampled_pair(*self.paths(fn), self.sampling_rate, self.device)
            else:
                noisy, clean = self._signals(fn)
                n = min(len(noisy), len(clean))
            if 1 + n // self.hop_size >= self.frame_length and n > self.window_size // 2:
                break
            skipped += 1
            if skipped >= len(self.files):
                raise ValueError(f"daps_enhance_dataloader: no recording of {self.list_file!r} holds frame_length = "
                                 f"{self.frame_length} frames")
        self.opened.append(fn)
        if not hip:
            wav = torch.from_numpy(np.stack([noisy[:n], clean[:n]])).to(self.device)
        logmag, ri = stft_logmag(wav, self.window_size, self.hop_size)
        self.cur, self.at = (logmag[0], ri[0], ri[1]), 0

    def _next_chunk(self):
        L = self.frame_length
        if self.cur is None or self.cur[0].shape[0] - self.at < L:
            self._open_next()
        out = tuple(t[self.at:self.at + L] for t in self.cur)
        self.at += L
        return out

    def _iter_eval(self):
        for fn in self.files:
            if options.get("loader_resample") == "hip":
                wav, _ = resampled_pair(*self.paths(fn), self.sampling_rate, self.device)
                yield _eval_item(wav[0], wav[1], self.window_size, self.hop_size, self.device)
            else:
                yield _eval_item(*self._signals(fn), self.window_size, self.hop_size, self.device)

    def __iter__(self):
        from ..features import enhance_labels
        if self.evaluation:
            yield from self._iter_eval()
            return
        for _ in range(self.num_batch):
            chunks = [self._next_chunk() for _ in range(self.batch_size)]
            feature, noisy, clean = (torch.stack([c[k] for c in chunks]) for k in range(3))
            mag_noisy, mag_clean, cos_diff = enhance_labels(noisy, clean)
            yield [feature, mag_noisy], [mag_clean, cos_diff]


class SyntheticDapsEnhance:
    """The same contract without a corpus: ``voices`` synthetic voices (``synthetic.synth_voice``, as ``SyntheticVoicePairs``)
    are generated once and kept on the device; every row of a batch is one voice plus white noise drawn on the device from a
    seeded generator, at a signal-to-noise ratio drawn from U(0, 20) dB by the same generator, peak-normalised.  The noisy and
    the clean signals of a batch go through one STFT launch, a random ``frame_length`` crop and ``enhance_labels``.  An
    evaluation partition yields ``num_batch`` whole utterances of different lengths, the same ones on every pass.  Nothing touches the device before the
    first batch is asked for."""

    def __init__(self, num_batch, feature_options, partition="train", device=None, voices=32, seed=0):
        _geometry(self, num_batch, feature_options, partition, device)
        self.n_voices = int(voices)
        self.seed = seed + {"train": 0, "validation": 10_000}.get(partition, 20_000)
        self.n_samples = self.hop_size * (self.frame_length + 40)     # a little longer than one chunk: crops differ
        self.voices = self.gen = None

    def __len__(self):
        return self.num_batch

    def _setup(self):
        from ..synthetic import synth_voice
        if self.voices is None:
            host = np.stack([synth_voice(700_000 + self.seed + v, self.n_samples, self.sampling_rate) for v in range(self.n_voices)])
            self.voices = torch.from_numpy(host).to(self.device)
            self.gen = torch.Generator(device=self.device).manual_seed(self.seed)

    def _pairs(self, B, g=None):
        """(noisy, clean), (B, n_samples) each, on the device, drawn from ``g`` (default: the loader's running generator)."""
        dev, g = self.device, (g or self.gen)
        clean = self.voices[torch.randint(0, self.n_voices, (B,), device=dev, generator=g)]
        snr_db = torch.rand(B, device=dev, generator=g) * 20.0
        noise = torch.randn(B, self.n_samples, device=dev, generator=g)
        noisy = clean + noise * (clean.std(dim=1, keepdim=True) * 10.0 ** (-snr_db / 20.0)[:, None])
        scale = 0.9 / noisy.abs().amax(dim=1, keepdim=True)
        return noisy * scale, clean * scale

    def __iter__(self):
        from ..features import enhance_labels, stft_logmag
        self._setup()
        B, L = self.batch_size, self.frame_length
        if self.evaluation:          # the same utterances on every pass: a generator of their own
            g = torch.Generator(device=self.device).manual_seed(self.seed + 1)
            for it in range(self.num_batch):
                noisy, clean = self._pairs(1, g)
                n = min(self.n_samples, self.hop_size * (L + 17 * (it % 3)) + 37 * it)        # utterances differ in length
                yield _eval_item(noisy[0, :n].cpu().numpy(), clean[0, :n].cpu().numpy(), self.window_size, self.hop_size, self.device)
            return
        for _ in range(self.num_batch):
            noisy, clean = self._pairs(B)
            logmag, ri = stft_logmag(torch.stack([noisy, clean], 1).view(2 * B, -1), self.window_size, self.hop_size)
            T, F = logmag.shape[1], logmag.shape[2]
            logmag, ri = logmag.view(B, 2, T, F), ri.view(B, 2, T, F, 2)
            start = int(torch.randint(0, T - L, (1,), device="cpu"))
            feature = logmag[:, 0, start:start + L].contiguous()
            mag_noisy, mag_clean, cos_diff = enhance_labels(ri[:, 0, start:start + L], ri[:, 1, start:start + L])
            yield [feature, mag_noisy], [mag_clean, cos_diff]


def daps_enhance_dataloader(num_batch, feature_options, partition, device=None):
    path = _getter(feature_options)("data_path")
    if not path or path == "synthetic":
        return SyntheticDapsEnhance(num_batch, feature_options, partition, device)
    list_file = os.path.join(path, partition)
    if os.path.isfile(list_file):
        return DapsEnhanceFiles(num_batch, feature_options, partition, device)
    if options.get("synthetic_data") not in ("", "0"):
        return SyntheticDapsEnhance(num_batch, feature_options, partition, device)
    raise FileNotFoundError(f"daps_enhance_dataloader: no list file {list_file!r} (data_path is set but holds nothing for partition "
                            f"{partition!r}); pass data_path='' / 'synthetic' or set ONSSEN_SYNTHETIC_DATA=1 for the synthetic corpus")
