"""Time-domain batches of the "conv-tasnet" / "lstm-tasnet" recipes (onssen/data/wsj0_2mix.py:86-113, 216-245), shared by
the synthetic and the file loaders.  Their feature_options need only ``batch_size``, ``sampling_rate``, ``chunk_size`` and
``data_path``.

    tr / cv   [mix (B, chunk_size)] , [s1 (B, chunk_size), s2 (B, chunk_size)]: each utterance cropped at a random start, or
              zero-padded at the end when it is shorter than chunk_size
    tt        [mix (1, S')] , [sig_ref (1, 2, S')]: whole utterances padded by 32 - S % 32 samples (a full 32 when S is
              already a multiple of 32)
"""
import numpy as np
import torch

MODELS = ("conv-tasnet", "lstm-tasnet")


def options_of(model_name, feature_options):
    """(batch_size, sampling_rate, chunk_size); ValueError without chunk_size."""
    fo = feature_options
    g = (lambda k: fo.get(k)) if isinstance(fo, dict) else (lambda k: getattr(fo, k, None))
    if g("chunk_size") is None:
        raise ValueError(f"{model_name}: feature_options needs 'chunk_size' (samples per training chunk)")
    return int(g("batch_size")), int(g("sampling_rate")), int(g("chunk_size"))


def crop_or_pad(sigs, chunk, rng):
    """Same crop (one random start for mix, s1, s2) or end padding for every signal of one utterance."""
    n = len(sigs[0])
    if n < chunk:
        return [np.pad(s, (0, chunk - n)) for s in sigs]
    start = int(rng.integers(0, n - chunk + 1))
    return [s[start:start + chunk] for s in sigs]


def training_batch(utterances, chunk, rng, device):
    """utterances: list of (mix, s1, s2) -> [mix (B, chunk)], [s1 (B, chunk), s2 (B, chunk)] float32 on ``device``."""
    rows = [crop_or_pad(u, chunk, rng) for u in utterances]
    mix, s1, s2 = (torch.from_numpy(np.stack([r[k] for r in rows]).astype(np.float32)).to(device) for k in range(3))
    return [mix], [s1, s2]


def eval_item(mix, s1, s2, device):
    gap = 32 - len(mix) % 32
    pad = lambda a: np.pad(np.asarray(a, np.float32), (0, gap))           # noqa: E731
    sig_ref = torch.from_numpy(np.stack([pad(s1), pad(s2)])[None]).to(device)
    return [torch.from_numpy(pad(mix)[None]).to(device)], [sig_ref]
