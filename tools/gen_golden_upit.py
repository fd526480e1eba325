#!/usr/bin/env python
"""Generate the uPIT fixtures under tests/golden/ by running the REFERENCE's uPIT_LSTM (modelled on tools/gen_golden.py).

The reference's file is ``nn/uPIT-LSTM.py``: its name has a hyphen, so it is loaded by file path with importlib (it imports
torch only).  Runs on torch-CPU, where the reference exists, with this repo's deterministic weights (``make_state_dict("upit",
...)``, gain 2.0) and the log-magnitude input of ``gen_golden.logmag_input``.  Only the weight RECIPE, the input and the outputs
(data) are written; no reference source travels.  Upstream returns the first two of the S masks whatever ``num_speaker`` is.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_upit.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, logmag_input, run_ref  # noqa: E402
from onssen_amd.synthetic import make_state_dict  # noqa: E402


def main():
    torch.manual_seed(0)
    spec = importlib.util.spec_from_file_location("ref_upit_lstm", os.path.join(REF, "nn", "uPIT-LSTM.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    F, H, L, B, T = 129, 16, 2, 2, 12
    for S in (2, 3):
        seed = 40 + S
        sd = make_state_dict("upit", F, H, L, 20, S, seed=seed, gain=2.0)
        x = logmag_input(seed, B, T, F, 256, 64)
        model = ref.uPIT_LSTM(F, F, H, 20, L, num_speaker=S)
        mask_A, mask_B = run_ref(model, sd, [x])
        fn = os.path.join(OUT, f"g10_upit_H{H}_L{L}_S{S}.npz")
        np.savez_compressed(fn, kind="upit", F=F, H=H, L=L, C=S, seed=seed, gain=2.0, x=x, mask_A=mask_A, mask_B=mask_B)
        print("wrote", fn, mask_A.shape, mask_B.shape, os.path.getsize(fn), "bytes")


if __name__ == "__main__":
    main()
