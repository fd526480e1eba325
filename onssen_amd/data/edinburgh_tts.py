"""Edinburgh noisy-speech loader with the reference's call signature and yield contract (onssen/data/edinburgh_tts.py:10-120).

``edinburgh_tts_dataloader(model_name, feature_options, partition, device)`` of the reference trains the separation networks
as enhancers: source 1 is the clean recording, source 2 the noise = noisy - clean (``get_stft_from_subtraction``).  The list
file ``<data_path>/<partition>`` names the recordings; the noisy one is ``<data_path>/noisy_trainset_28spk_wav/<name>``, the
clean one ``<data_path>/clean_trainset_28spk_wav/<name>`` (``:61-71``).  The corpus is 48 kHz and the recipe 16 kHz: upstream
every file is resampled on every read, three STFTs per sample on the host.  Here, per batch:

    the library's batch reader fills ONE pinned slot with the batch's 2 x batch_size files at their own rate (``_Slot`` and
    ``onssen_wav_read_batch_f32``, as the wsj0-2mix loader; ``loader_prefetch`` batches ahead on a producer thread),
    ONE host-to-device transfer,
    ONE ``features.resample`` launch giving three rows per utterance -- noisy, clean, and noisy - clean by the kernel's ``sub``
    operand: subtracted at the files' rate, before the filter, as upstream -- (one launch per distinct rate in the batch),
    ONE ragged ``stft_logmag`` launch,
    the FIRST ``frame_length`` frames of every utterance, a shorter one repeated "in a double-copy fashion" (``:73-82``:
    frame t of the chunk is frame t mod T of the utterance; upstream takes no random crop here),
    ONE ``training_labels`` launch.

This loader always resamples on the device: it is new code and has no host route (option ``loader_resample`` does not apply).
Layouts per ``model_name`` are the wsj0-2mix loader's ("dc", "chimera", "chimera++", "phase"; other names raise).  Batches of
``batch_size`` in shuffled order (the reference's ``DataLoader(shuffle=True)``); ``len()`` is the number of batches.

Extension (upstream has no evaluation for this recipe): partitions ``"tt"`` / ``"test"`` yield whole recordings, batch 1, in
list order, in ``tester_chimera``'s contract: ``[feature (1,T,F)], [stft_r (1,T,F), stft_i (1,T,F), sig_ref (1,2,n)]`` with
sig_ref = (clean, noise) at ``sampling_rate``, zero-padded by ``32 - n % 32`` samples.

Without a tree the rule of ``onssen_amd.data`` applies: the synthetic corpus (``SyntheticEdinburghTts``) only when ``data_path``
is absent / ``""`` / ``"synthetic"`` or ``ONSSEN_SYNTHETIC_DATA=1`` is set; otherwise a missing list file raises
``FileNotFoundError``."""
import os

import numpy as np
import torch

from .. import options
from ..features import resample, stft_logmag, training_labels
from .daps_enhance import SyntheticDapsEnhance, _getter
from .wsj0_2mix import Wsj02mixFiles, _Slot

MODELS = ("dc", "chimera", "chimera++", "phase")
EVAL_PARTITIONS = ("tt", "test")
NOISY_DIR, CLEAN_DIR = "noisy_trainset_28spk_wav", "clean_trainset_28spk_wav"


def _layout(model_name, feat, mix, s1, s2, db_threshold):
    """(input_list, label_list) of one batch from the cropped log-magnitude (B, L, F) and the three spectra (B, L, F, 2)."""
    out = training_labels(mix, s1, s2, feat, db_threshold, with_cos=model_name == "chimera++")
    one_hot, mm, m1, m2 = out[:4]
    one_hot = one_hot.double()                             # np.zeros default dtype upstream (feature_utils.py:86)
    if model_name == "dc":
        return [feat], [one_hot, mm]
    if model_name == "chimera":
        return [feat], [one_hot, mm, m1, m2]
    if model_name == "chimera++":
        return [feat], [one_hot, mm, m1, m2, out[4], out[5]]
    return [feat, mix], [one_hot, mm, m1, m2, s1, s2]


def resample_triples(pairs, lengths, rate, sampling_rate):
    """pairs (B, 2, S) device tensor of (noisy, clean) rows at ``rate``, lengths (B,) host ints -> (y (3 B, n_out), lengths_out
    (3 B,) int32 on the device): rows (noisy, clean, noisy - clean) per utterance at ``sampling_rate``, ONE launch."""
    B, _, S = pairs.shape
    x = pairs[:, [0, 1, 0]]                                # the launch's rows; its `sub` rows: (0, 0, clean)
    sub = torch.zeros_like(x)
    sub[:, 2] = pairs[:, 1]
    n = int(max(lengths))
    return resample(x.view(3 * B, S)[:, :n], rate, sampling_rate, lengths=np.repeat(np.asarray(lengths, np.int64), 3),
                    sub=sub.view(3 * B, S)[:, :n])


class EdinburghTtsFiles(Wsj02mixFiles):
    """Iterable over ``(input_list, label_list)`` batches of one partition of an Edinburgh-style tree.  The host side of a batch
    (reader, pinned ring, producer thread) is the wsj0-2mix loader's; the rows of a slot are (noisy, clean) per utterance."""

    def __init__(self, model_name, feature_options, partition="train", device=None, shuffle=None, seed=None):
        if model_name not in MODELS:
            raise ValueError(f"unknown model_name {model_name!r} (edinburgh_tts_dataloader: one of {MODELS})")
        g = _getter(feature_options)
        self.model_name, self.partition = model_name, partition
        self.batch_size, self.frame_length = int(g("batch_size")), int(g("frame_length"))
        self.sampling_rate, self.window_size, self.hop_size = int(g("sampling_rate")), int(g("window_size")), int(g("hop_size"))
        self.db_threshold = float(g("db_threshold"))
        self.device = torch.device(device if device is not None else "cuda:0")
        self.base_path = g("data_path")
        self.list_file = os.path.join(self.base_path, partition)
        with open(self.list_file) as f:
            names = [line.strip() for line in f if line.strip()]
        if not names:
            raise FileNotFoundError(f"edinburgh_tts_dataloader: the list file {self.list_file!r} names no recordings")
        self.file_list = [os.path.join(self.base_path, NOISY_DIR, n) for n in names]      # edinburgh_tts.py:61-64
        self.evaluation = partition in EVAL_PARTITIONS
        self.shuffle = (not self.evaluation) if shuffle is None else bool(shuffle)
        self.rng = np.random.default_rng(seed)
        self._headers = {}

    def __len__(self):
        n = len(self.file_list)
        return n if self.evaluation else -(-n // self.batch_size)

    def _sources(self, fn):
        """(noisy, clean) paths of one recording (edinburgh_tts.py:69-71)."""
        return fn, os.path.join(self.base_path, CLEAN_DIR, os.path.basename(fn))

    def _read_batch(self, files, slot, rng=None):
        """Host side of one batch: the 2 x len(files) files into the rows of ``slot`` at their own rate.
        Returns (slot, samples per utterance (B,) int64, rate per utterance (B,) int64)."""
        from ..hip import get_lib
        lib = get_lib()
        paths = [p for fn in files for p in self._sources(fn)]
        stride = -(-max(self._frames_of(p)[0] for p in paths) // 64) * 64
        wav = slot.shape(len(paths), stride)
        rc = lib.wav_read_batch(paths, wav.data_ptr(), stride, slot.frames.data_ptr(), slot.rates.data_ptr(), slot.status.data_ptr(),
                                max(1, int(options.get("loader_workers"))))
        status = slot.status[:len(paths)].numpy()
        if rc != 0 or status.any():
            bad = int(np.argmax(status != 0))
            raise OSError(f"{paths[bad]}: {lib.dll.onssen_error_string(int(status[bad])).decode()} (status {int(status[bad])})")
        rates = slot.rates[:len(paths)].numpy().astype(np.int64).reshape(-1, 2)
        if (rates[:, 0] != rates[:, 1]).any():
            bad = int(np.argmax(rates[:, 0] != rates[:, 1]))
            raise ValueError(f"{paths[2 * bad]} ({rates[bad, 0]} Hz) and {paths[2 * bad + 1]} ({rates[bad, 1]} Hz) differ in sample rate")
        return slot, slot.frames[:len(paths)].numpy().astype(np.int64).reshape(-1, 2).min(axis=1), rates[:, 0].copy()

    def _resampled(self, pairs, n_nat, rates):
        """(B, 2, S) device rows at the files' rates -> (wav (3 B, n) at sampling_rate, samples per utterance (B,) host):
        one resample launch per distinct rate of the batch."""
        sr = self.sampling_rate
        n_utt = np.array([-(-int(n) * sr // int(r)) for n, r in zip(n_nat, rates)], np.int64)
        kinds = np.unique(rates)
        if len(kinds) == 1:
            return resample_triples(pairs, n_nat, int(kinds[0]), sr)[0], n_utt
        B = len(n_nat)
        wav = torch.zeros(B, 3, int(n_utt.max()), device=pairs.device, dtype=torch.float32)
        for r in kinds:
            sel = np.nonzero(rates == r)[0]
            y, _ = resample_triples(pairs[torch.from_numpy(sel).to(pairs.device)], n_nat[sel], int(r), sr)
            wav[torch.from_numpy(sel).to(pairs.device), :, :y.shape[1]] = y.view(len(sel), 3, -1)
        return wav.view(3 * B, -1), n_utt

    def _device_batch(self, item):
        """Device side of one batch: (B, 3, L, F) log-magnitude and (B, 3, L, F, 2) spectrum of (noisy, clean, noise), the first
        ``frame_length`` frames of every utterance, wrapping."""
        slot, n_nat, rates = item
        B, L, hop = len(n_nat), self.frame_length, self.hop_size
        pairs = slot.wav.to(self.device, non_blocking=True)             # ONE contiguous transfer from the pinned buffer
        slot.release()
        wav, n_utt = self._resampled(pairs.view(B, 2, -1), n_nat, rates)
        logmag, ri = stft_logmag(wav, self.window_size, hop, lengths=torch.from_numpy(np.repeat(n_utt, 3)))
        T, F = logmag.shape[1], logmag.shape[2]
        Tb = 1 + n_utt // hop
        idx = torch.from_numpy(np.arange(L)[None, :] % Tb[:, None]).to(self.device)       # frame t of the chunk = frame t mod T
        rows = torch.arange(B, device=self.device)[:, None, None]
        trip = torch.arange(3, device=self.device)[None, :, None]
        return logmag.view(B, 3, T, F)[rows, trip, idx[:, None, :]], ri.view(B, 3, T, F, 2)[rows, trip, idx[:, None, :]]

    def _iter_eval(self):
        for fn in self.file_list:
            slot, n_nat, rates = self._read_batch([fn], _Slot(False, numel=1))
            wav, n_utt = self._resampled(slot.wav.to(self.device).view(1, 2, -1), n_nat, rates)
            n = int(n_utt[0])
            logmag, ri = stft_logmag(wav[:1, :n], self.window_size, self.hop_size)
            sig_ref = torch.nn.functional.pad(wav[1:3, :n], (0, 32 - n % 32))[None]
            yield [logmag], [ri[..., 0].contiguous(), ri[..., 1].contiguous(), sig_ref]

    def __iter__(self):
        if self.evaluation:
            yield from self._iter_eval()
            return
        order = self.rng.permutation(len(self.file_list)) if self.shuffle else np.arange(len(self.file_list))
        for item in self._prefetched(order):
            logmag, ri = self._device_batch(item)
            yield _layout(self.model_name, logmag[:, 0].contiguous(), *(ri[:, i].contiguous() for i in range(3)), self.db_threshold)


class SyntheticEdinburghTts:
    """The same contract without a corpus: the noisy / clean pairs of ``SyntheticDapsEnhance`` (synthetic voices plus white noise
    at 0 .. 20 dB, generated at ``sampling_rate``: nothing to resample), noise = noisy - clean; ``num_batches`` batches per
    epoch, or as many whole utterances for an evaluation partition."""

    def __init__(self, model_name, feature_options, partition="train", device=None, num_batches=8, seed=0):
        if model_name not in MODELS:
            raise ValueError(f"unknown model_name {model_name!r} (edinburgh_tts_dataloader: one of {MODELS})")
        self.model_name, self.num_batches = model_name, int(num_batches)
        self.db_threshold = float(_getter(feature_options)("db_threshold"))
        self.pairs = SyntheticDapsEnhance(num_batches, feature_options, partition, device, seed=seed)

    def __len__(self):
        return self.num_batches

    def __iter__(self):
        p = self.pairs
        p._setup()
        B, L = p.batch_size, p.frame_length
        if p.evaluation:                                    # the same utterances on every pass: a generator of their own
            g = torch.Generator(device=p.device).manual_seed(p.seed + 1)
            for it in range(self.num_batches):
                noisy, clean = p._pairs(1, g)
                n = min(p.n_samples, p.hop_size * (L + 17 * (it % 3)) + 37 * it)
                logmag, ri = stft_logmag(noisy[:, :n], p.window_size, p.hop_size)
                sig_ref = torch.nn.functional.pad(torch.cat([clean, noisy - clean])[:, :n], (0, 32 - n % 32))[None]
                yield [logmag], [ri[..., 0].contiguous(), ri[..., 1].contiguous(), sig_ref]
            return
        for _ in range(self.num_batches):
            noisy, clean = p._pairs(B)
            logmag, ri = stft_logmag(torch.stack([noisy, clean, noisy - clean], 1).view(3 * B, -1), p.window_size, p.hop_size)
            T, F = logmag.shape[1], logmag.shape[2]
            logmag, ri = logmag.view(B, 3, T, F)[:, :, :L], ri.view(B, 3, T, F, 2)[:, :, :L]
            yield _layout(self.model_name, logmag[:, 0].contiguous(), *(ri[:, i].contiguous() for i in range(3)), self.db_threshold)


def edinburgh_tts_dataloader(model_name, feature_options, partition, device=None):
    path = _getter(feature_options)("data_path")
    if not path or path == "synthetic":
        return SyntheticEdinburghTts(model_name, feature_options, partition, device)
    list_file = os.path.join(path, partition)
    if os.path.isfile(list_file):
        return EdinburghTtsFiles(model_name, feature_options, partition, device)
    if options.get("synthetic_data") not in ("", "0"):
        return SyntheticEdinburghTts(model_name, feature_options, partition, device)
    raise FileNotFoundError(f"edinburgh_tts_dataloader: no list file {list_file!r} (data_path is set but holds nothing for partition "
                            f"{partition!r}); pass data_path='' / 'synthetic' or set ONSSEN_SYNTHETIC_DATA=1 for the synthetic corpus")
