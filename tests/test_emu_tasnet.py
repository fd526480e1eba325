"""The Conv-TasNet kernels (csrc/tasnet.inc) through the C ABI on the host-side emulation build (tests/emu): the whole forward
against the fp64 restatement tests/tasnet_ref.py at tiny sizes with ragged tile edges -- T = 74 frames (not a multiple of the
64-frame statistics chunk, the 32-frame depthwise tile, the 16-block decoder tile or any GEMM tile height) and channel counts
20 / 12 / 24 (not multiples of 64 or 32) -- for every norm, causal setting, activation and precision; two runs give the same
bits."""
import numpy as np
import pytest

from tests import tasnet_emu, tasnet_ref
from tests.emu_build import load_emu

BASE = dict(N=20, L=4, B=12, H=24, P=3, X=2, R=1, num_spks=2)
CASES = [
    dict(norm="gln", activate="relu", causal=False),
    dict(norm="gln", activate="softmax", causal=True),
    dict(norm="cln", activate="sigmoid", causal=False),
    dict(norm="cln", activate="relu", causal=True, P=5),
    dict(norm="bn", activate="softmax", causal=False, num_spks=3),
    dict(norm="bn", activate="sigmoid", causal=True, P=4),
]
# bf16x3: three bf16 products per fp32 product (~1e-5 relative per dot product); bf16: plain bf16 products
TOL = {"f32": 2e-6, "bf16x3": 3e-5, "bf16": 3e-2}


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _x(n=2, S=150, seed=0):
    return (0.5 * np.random.default_rng(seed).standard_normal((n, S))).astype(np.float32)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_forward_matches_ref(lib, case, prec):
    cfg = dict(BASE, **case)
    sd = tasnet_ref.make_state(cfg, seed=5)
    x = _x()
    out = tasnet_emu.forward(lib, sd, cfg, x, prec)
    ref = np.stack(tasnet_ref.forward(sd, x, cfg))
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{case} {prec}: max |err| / max(1, max |ref|) = {err:.2e}")
    assert err <= TOL[prec]


def test_fixture_through_the_abi(lib):
    """A reference fixture (its own weights and an S where (S - L) is not a multiple of L/2) through pack + forward."""
    import glob
    import os
    path = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_tasnet_gln_relu.npz")))[0]
    cfg, sd, x, out64, _ = tasnet_ref.load_fixture(path)
    out = tasnet_emu.forward(lib, sd, cfg, x, "f32")
    assert np.abs(out - out64).max() <= 2e-6 * max(1.0, np.abs(out64).max())


def test_two_runs_same_bits(lib):
    cfg = dict(BASE, norm="gln", activate="sigmoid", causal=False)
    sd = tasnet_ref.make_state(cfg, seed=9)
    x = _x(3, 141, seed=2)
    for prec in ("f32", "bf16x3"):
        a = tasnet_emu.forward(lib, sd, cfg, x, prec)
        b = tasnet_emu.forward(lib, sd, cfg, x, prec)
        assert np.array_equal(a, b)


def test_abi_rejects_unsupported_shapes(lib):
    ok = dict(BASE, norm="gln", activate="relu", causal=False)
    assert lib.tasnet_param_floats(tasnet_emu.lib_cfg(lib, ok, "f32")) > 0
    for bad in (dict(L=5), dict(L=66), dict(P=4), dict(N=1025), dict(num_spks=9)):
        cfg = tasnet_emu.lib_cfg(lib, dict(ok, **bad), "f32")
        assert lib.dll.onssen_tasnet_param_floats(cfg) == -1
        assert lib.dll.onssen_tasnet_image_bytes(cfg) == 0
