"""The ragged Conv-TasNet forward (onssen_tasnet_forward_ragged_f32) on the host-side emulation build: every utterance of a
batch of different lengths comes out bit for bit as the rectangular forward of that utterance alone, for every norm, causal
setting, activation and precision; input padding is never read (it is NaN here) and the output padding is exactly zero."""
import ctypes as C

import numpy as np
import pytest

from tests import tasnet_ref
from tests.emu_build import load_emu
from tests.tasnet_ragged_emu import Packed
from tests.test_emu_tasnet import BASE, CASES, TOL

# frames per utterance: the 64-frame statistics chunk, the 32-frame depthwise tile and the 16-block decoder tile (T + 1 blocks)
# exactly, one over and one under; unsorted.  L = 4, hop = 2: S = 2 T + 2, and + 1 where the last sample belongs to no frame.
FRAMES = [1, 63, 64, 65, 74, 129, 33]
ODD = {63, 74}
LENS = [2 * t + 2 + (1 if t in ODD else 0) for t in FRAMES]
E_ARG, E_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _waves(lens, seed=3):
    rng = np.random.default_rng(seed)
    return [(0.5 * rng.standard_normal(s)).astype(np.float32) for s in lens]


def test_lengths_are_what_the_docstring_says():
    assert [tasnet_ref.frames(s, BASE["L"]) for s in LENS] == FRAMES
    assert any((s - BASE["L"]) % (BASE["L"] // 2) for s in LENS)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_rows_equal_the_one_utterance_forward(lib, case, prec):
    cfg = dict(BASE, **case)
    sd = tasnet_ref.make_state(cfg, seed=5)
    pk = Packed(lib, sd, cfg, prec)
    xs = _waves(LENS)
    out = pk.ragged(xs)
    worst = 0.0
    for b, v in enumerate(xs):
        so = pk.s_out(len(v))
        alone = pk.one(v)[:, 0]
        assert alone.shape == (cfg["num_spks"], so)
        assert np.isfinite(out[:, b, :so]).all(), f"utterance {b}"
        assert np.array_equal(out[:, b, :so], alone), f"utterance {b} (T = {FRAMES[b]})"
        assert np.all(out[:, b, so:] == 0.0) and out[:, b, so:].size > 0, f"utterance {b}: tail"
        ref = np.stack([np.atleast_1d(r) for r in tasnet_ref.forward(sd, v, cfg)])
        err = np.abs(out[:, b, :so] - ref).max() / max(1.0, np.abs(ref).max())
        worst = max(worst, err)
        assert err <= TOL[prec], f"utterance {b}: {err:.2e}"
    print(f"{case} {prec}: worst max |err| / max(1, max |ref|) over the utterances = {worst:.2e}")


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("norm", ["gln", "cln", "bn"])
def test_equal_lengths_equal_the_rectangular_batch(lib, norm, prec):
    cfg = dict(BASE, norm=norm, activate="relu", causal=False)
    pk = Packed(lib, tasnet_ref.make_state(cfg, seed=6), cfg, prec)
    xs = _waves([151] * 3, seed=4)
    rect = pk.one(np.stack(xs))
    out = pk.ragged(xs, out_extra=0)
    assert out.shape == rect.shape and np.array_equal(out, rect)


def test_order_independent_and_repeatable(lib):
    cfg = dict(BASE, norm="gln", activate="sigmoid", causal=False)
    pk = Packed(lib, tasnet_ref.make_state(cfg, seed=9), cfg, "f32")
    xs = _waves(LENS, seed=8)
    a = pk.ragged(xs)
    assert np.array_equal(a, pk.ragged(xs))
    perm = [4, 0, 6, 2, 5, 1, 3]
    p = pk.ragged([xs[i] for i in perm])
    for k, i in enumerate(perm):
        assert np.array_equal(p[:, k], a[:, i])


def test_refusals_and_workspace_size(lib):
    cfg = dict(BASE, norm="gln", activate="relu", causal=False)
    pk = Packed(lib, tasnet_ref.make_state(cfg, seed=1), cfg, "f32")
    L = cfg["L"]
    assert pk.raw(2, [40, 30], 40, 40) == 0
    assert pk.raw(0, [], 40, 40) == E_ARG
    assert pk.raw(65, [10] * 65, 40, 40) == E_ARG
    assert pk.raw(64, [10] * 64, 40, 40) == 0
    assert pk.raw(2, [40, L - 1], 40, 40) == E_ARG               # shorter than one frame
    assert pk.raw(2, [41, 30], 40, 48) == E_ARG                  # S_b > x_stride
    assert pk.raw(2, [40, 30], 40, 39) == E_ARG                  # out_stride < max S_out_b
    assert pk.raw(2, [41, 30], 41, 40) == 0                      # S_out of 41 samples is 40
    assert pk.raw(2, [40, 30], 40, 40, ws_bytes=256) == E_WORKSPACE
    big = (C.c_int32 * 2)(2 ** 31 - 1, 2 ** 31 - 1)             # sum T_b over 2^31 / 4
    assert lib.dll.onssen_tasnet_ragged_workspace_bytes(pk.cf, 2, big) == 0
    assert lib.dll.onssen_tasnet_ragged_workspace_bytes(pk.cf, 65, (C.c_int32 * 65)(*[10] * 65)) == 0
    assert lib.dll.onssen_tasnet_ragged_workspace_bytes(pk.cf, 1, (C.c_int32 * 1)(L - 1)) == 0
    # the table is a kernel argument, not workspace: one utterance needs exactly the rectangular forward's bytes
    for S in (L, 150, 2 * 129 + 2):
        assert lib.tasnet_ragged_workspace_bytes(pk.cf, 1, lib.tasnet_lengths([S])) == lib.tasnet_workspace_bytes(pk.cf, 1, S)
    # and a batch needs what a rectangular batch of as many rows and statistics chunks needs
    assert lib.tasnet_ragged_workspace_bytes(pk.cf, 3, lib.tasnet_lengths([150] * 3)) == lib.tasnet_workspace_bytes(pk.cf, 3, 150)
