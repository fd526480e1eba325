#!/usr/bin/env python
"""Golden values of the reference's loss_mask_msa / loss_mask_psa (onssen/loss/loss_mask.py) on random outputs / labels, computed
on the CPU; writes tests/golden/g8_loss_mask.npz (arrays only)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.gen_golden import OUT, load_ref_pkg   # noqa: E402


def main():
    ref = load_ref_pkg("ref_loss", "loss")
    rng = np.random.default_rng(8)
    B, T, F = 3, 7, 129
    mag_noisy = (np.abs(rng.standard_normal((B, T, F))) + 1e-3).astype(np.float32)
    mag_clean = (mag_noisy * rng.random((B, T, F)) * 1.5).astype(np.float32)
    cos_diff = np.cos(rng.uniform(-np.pi, np.pi, (B, T, F))).astype(np.float32)
    clean_est = (mag_noisy * rng.random((B, T, F))).astype(np.float32)
    mask = rng.random((B, T, F)).astype(np.float32)
    tt = torch.from_numpy
    msa = ref.loss_mask_msa([tt(clean_est)], [tt(mag_clean), tt(cos_diff)]).numpy()
    psa = ref.loss_mask_psa([tt(mask)], [tt(mag_noisy), tt(mag_clean), tt(cos_diff)]).numpy()
    np.savez_compressed(f"{OUT}/g8_loss_mask.npz", clean_est=clean_est, mask=mask, mag_noisy=mag_noisy, mag_clean=mag_clean,
                        cos_diff=cos_diff, msa=msa, psa=psa)
    print("msa", msa.shape, float(msa), "psa", psa.shape, psa)


if __name__ == "__main__":
    main()
