#!/usr/bin/env python
"""tests/golden/g9_mask_istft_bits.npz: what onssen_mask_istft_f32 of the host-side build (tests/emu) returns for the inputs of
tests/phase_istft_cases.py, recorded BEFORE mask_istft_kernel gained its phase flag.  tests/test_emu_phase_istft.py asks the
current build for the same bits.  Usage: python tools/gen_golden_mask_istft.py [path/to/libonssen_emu.so]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def outputs(lib):
    from tests.phase_istft_cases import SHAPES, case
    out = {}
    for n_fft, hop, n in SHAPES:
        for C in (2, 3) if n_fft == 256 and hop == 64 else (2,):
            _, ri, masks, _ = case(n_fft, hop, n, C)
            B, T, F, _ = masks.shape
            y = np.full((B, C, n), np.nan, np.float32)
            lib.mask_istft(ri.ctypes.data, masks.ctypes.data, T * F * C, 1, F * C, C, B, C, T, n_fft, hop, n, y.ctypes.data, None)
            out[f"n{n_fft}_h{hop}_c{C}"] = y
    return out


if __name__ == "__main__":
    from onssen_amd._abi import Lib
    from tests.emu_build import build_emu
    lib = Lib(sys.argv[1] if len(sys.argv) > 1 else build_emu())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g9_mask_istft_bits.npz"), **outputs(lib))
