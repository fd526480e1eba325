#!/usr/bin/env python
"""sha256 of what the deep-clustering separation routes return on fixed synthetic inputs, one line per result -- run it at two
commits and diff the output to show that a change of the host side computes what it computed (MI355X):
  python tools/dc_stream_digests.py [ROOT]        ROOT: the checkout to import onssen_amd from (default: this one)
separate_dc at B = 5, n = 64 * 24, uniform and ragged; separate_dc_stream over four such batches with the graph on and off;
separate_dc_ragged_stream over four ragged batches at H = 32, B = 5; and, for the 2-means of more utterances than one Lloyd launch
takes (32), separate_dc and dc_masks at B = 34."""
import hashlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                   # noqa: E402
import torch                                                         # noqa: E402
from onssen_amd import nn as onn                                     # noqa: E402
from onssen_amd.nn import _core                                      # noqa: E402
from onssen_amd.features import stft_logmag                          # noqa: E402
from onssen_amd.separation import dc_masks, separate_dc, separate_dc_ragged_stream, separate_dc_stream     # noqa: E402
from onssen_amd.synthetic import make_state_dict, synth_mixture      # noqa: E402


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def main():
    dev = torch.device("cuda:0")
    F, H, D, B, n = 129, 32, 20, 5, 64 * 24
    sd = make_state_dict("deep_clustering", F, H, 2, D, 2, seed=3)
    m = onn.deep_clustering(F, H, 2, D)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(dev).eval()
    xs = [torch.from_numpy(np.stack([synth_mixture(100 + 97 * k + b, n) for b in range(B)])).to(dev) for k in range(4)]
    rng = np.random.default_rng(7)
    rag = []
    for k in range(4):                         # every batch padded to its own longest utterance, one of them longer than the first
        lens = rng.integers(64 * 6, 64 * (20 + 6 * k), B)
        wav = np.zeros((B, int(lens.max())), np.float32)
        for b, ln in enumerate(lens):
            wav[b, :ln] = synth_mixture(500 + 31 * k + b, int(ln))
        rag.append((torch.from_numpy(wav).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)))
    a0 = _core._XcdPolicy.aborts
    print("separate_dc uniform", sha(separate_dc(m, xs[0])))
    print("separate_dc ragged", sha(separate_dc(m, rag[0][0], lengths=rag[0][1])))
    for graph in (True, False):
        for k, out in enumerate(separate_dc_stream(m, xs, graph=graph)):
            print(f"separate_dc_stream graph={graph} batch {k}", sha(out))
    for k, out in enumerate(separate_dc_ragged_stream(m, rag)):
        print(f"separate_dc_ragged_stream batch {k} {tuple(out.shape)}", sha(out))
    big = torch.cat(xs + xs)[:34]              # two Lloyd launches: the compacted route, then the clustering of a materialised embedding
    print("separate_dc B=34", sha(separate_dc(m, big)))
    logmag, _ = stft_logmag(big)
    emb = torch.nn.functional.normalize(torch.randn(34, logmag.shape[1], F, D, generator=torch.Generator().manual_seed(5)), dim=-1).to(dev)
    print("dc_masks B=34", sha(dc_masks(emb, logmag)))
    print("dc_masks B=34 iters=0", sha(dc_masks(emb, logmag, iters=0)))
    _core._XcdStatus.flush()
    print("aborted launches", _core._XcdPolicy.aborts - a0)


if __name__ == "__main__":
    main()
