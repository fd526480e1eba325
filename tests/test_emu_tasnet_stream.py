"""Streaming Conv-TasNet (onssen_tasnet_stream_*, csrc/tasnet_stream.inc) on the host-side emulation build: a stream that is
reset, fed chunks of any sizes and flushed gives, after its one hop of delay, bit for bit the offline forward of the whole
signal -- at every precision, for chunks below, at and above every block's history, the 32-frame depthwise tile and the
64-frame statistics chunk; slots are independent; refusals launch nothing.

Cost: the emulation runs every lane as an OS thread and every MFMA as two barrier waits, so ONE emulated GEMM launch takes about
0.08 s whatever its M, and a streamed step of this configuration (6 blocks, 14 GEMMs) about 1.3 s (f32) to 1.9 s (bf16x3).  The
9-step schedule and the single 129-hop step run for every configuration and precision (about 30 s each); the run of 129
one-hop steps costs 3 to 4 minutes, so here it runs for ONE configuration (cln, P = 5: histories 4, 8, 16) at f32, and for every
configuration and precision on the device, where a step takes milliseconds (tests/test_gpu_tasnet_stream.py).  Offline
references, packed images and undisturbed runs are computed once and shared."""
import numpy as np
import pytest

from tests import tasnet_emu, tasnet_ref
from tests.emu_build import load_emu
from tests.tasnet_ragged_emu import Packed
from tests.tasnet_stream_emu import Stream, stitched
from tests.test_emu_tasnet import BASE

SBASE = dict(BASE, X=3, R=2, L=4, causal=True)
CASES = [
    dict(norm="cln", activate="relu", P=5),                 # histories of 4, 8 and 16 frames
    dict(norm="bn", activate="sigmoid", P=4),
    dict(norm="cln", activate="softmax", num_spks=3, P=3),
]
SCHEDULE = [1, 1, 3, 16, 33, 2, 65, 7, 1]                   # hops per step: 129 in all, S = 258
HOPS = sum(SCHEDULE)
HOP = SBASE["L"] // 2
E_ARG, E_WORKSPACE = -1, -2
_ids = lambda c: "-".join(f"{k}={v}" for k, v in c.items())


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def _x(n=3, hops=HOPS, seed=0):
    return (0.5 * np.random.default_rng(seed).standard_normal((n, hops * HOP))).astype(np.float32)


def _packed(lib, case, prec, seed=5):
    cfg = dict(SBASE, **case)
    return Packed(lib, tasnet_ref.make_state(cfg, seed=seed), cfg, prec)


_SHARED = {}


def _ctx(lib, i, prec):
    """(packed image, signal, offline forward) of configuration i at `prec`: made once, never modified."""
    key = ("ctx", i, prec)
    if key not in _SHARED:
        pk, x = _packed(lib, CASES[i], prec), _x()
        ref = pk.one(x)
        for a in (x, ref):
            a.setflags(write=False)
        _SHARED[key] = (pk, x, ref)
    return _SHARED[key]


def _scheduled(lib, i, prec):
    """(step outputs, flush) of the undisturbed SCHEDULE run of _ctx's signal: made once, never modified."""
    key = ("run", i, prec)
    if key not in _SHARED:
        pk, x, _ = _ctx(lib, i, prec)
        steps, tail = Stream(pk, 3).run(x, SCHEDULE)
        for a in (steps, tail):
            a.setflags(write=False)
        _SHARED[key] = (steps, tail)
    return _SHARED[key]


def _check(steps, tail, ref, what):
    assert steps.shape == ref.shape and tail.shape == ref.shape[:2] + (HOP,)
    assert np.isfinite(steps).all() and np.isfinite(tail).all()
    assert np.all(steps[..., :HOP] == 0.0), f"{what}: the first hop after a reset is exactly zero"
    got = stitched(steps, tail, HOP)
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), f"{what}: {len(bad)} values differ, first at {bad[:1].tolist()}"


def test_schedule_is_what_the_docstring_says():
    assert HOPS == 129 and HOPS * HOP == 258
    hist = {(5 - 1) << x for x in range(3)} | {(4 - 1) << x for x in range(3)} | {(3 - 1) << x for x in range(3)}
    assert hist >= {4, 8, 16}
    for h in hist:
        assert any(f < h for f in SCHEDULE) and any(f > h for f in SCHEDULE)
    assert {4, 8, 16} & set(SCHEDULE) == {16} and 3 in SCHEDULE     # F equal to a history: 16 (P = 5, x = 2) and 3 (P = 4, x = 0)
    assert max(SCHEDULE) > 64 and any(32 < f <= 64 for f in SCHEDULE)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[_ids(c) for c in CASES])
def test_stream_equals_offline_bit_for_bit(lib, i, prec):
    pk, x, ref = _ctx(lib, i, prec)
    assert ref.shape == (pk.c["num_spks"], 3, HOPS * HOP) and np.isfinite(ref).all()
    _check(*_scheduled(lib, i, prec), ref, "the schedule")
    _check(*Stream(pk, 3).run(x, [HOPS]), ref, "one step of 129 hops")


def test_single_hop_steps_equal_offline_bit_for_bit(lib):
    """129 steps of one hop (see the module docstring for why one configuration here and all of them on the device)."""
    pk, x, ref = _ctx(lib, 0, "f32")
    _check(*Stream(pk, 3).run(x, [1] * HOPS), ref, "129 steps of one hop")


def test_history_of_four_eight_sixteen_frames(lib):
    pk = _ctx(lib, 0, "f32")[0]
    assert [(pk.c["P"] - 1) << x for x in range(pk.c["X"])] == [4, 8, 16]
    # the ring and its statistics: n * sum(history) * R rows of H + 2 floats, each region rounded up to 256 bytes
    n, H, R = 3, pk.c["H"], pk.c["R"]
    rows = n * (4 + 8 + 16) * R
    small = n * 8 + n * HOP * 4 * (1 + pk.c["num_spks"])      # counters and the two carries; 3 + 2 R X regions in all
    assert 0 <= pk.lib.tasnet_stream_state_bytes(pk.cf, n) - rows * (H + 2) * 4 - small < (3 + 2 * R * 3) * 256


def test_reset_of_one_slot_leaves_the_others_alone(lib):
    pk, x, _ = _ctx(lib, 0, "f32")
    y = _x(n=1, hops=HOPS - 21, seed=2)[0]
    steps_ref, tail_ref = _scheduled(lib, 0, "f32")
    st = Stream(pk, 3)                                     # the state buffer was 0xFF bytes before its reset
    outs, at = [], 0
    for i, F in enumerate(SCHEDULE):
        if i == 4:                                         # 21 hops in: slot 1 starts over on another signal
            assert at == 21 * HOP
            st.reset([1])
        chunk = x[:, at:at + F * HOP].copy()
        if i >= 4:
            chunk[1] = y[at - 21 * HOP:at - 21 * HOP + F * HOP]
        outs.append(st.push(chunk))
        at += F * HOP
    steps, tail = np.concatenate(outs, axis=-1), st.flush()
    for b in (0, 2):
        assert np.array_equal(steps[:, b], steps_ref[:, b]) and np.array_equal(tail[:, b], tail_ref[:, b])
    assert np.array_equal(steps[:, 1, :21 * HOP], steps_ref[:, 1, :21 * HOP])
    new = np.concatenate([steps[:, 1, 21 * HOP:][:, HOP:], tail[:, 1]], axis=-1)
    assert np.all(steps[:, 1, 21 * HOP:22 * HOP] == 0.0)
    assert np.array_equal(new, pk.one(y)[:, 0])


def test_two_runs_same_bits(lib):
    pk, x, _ = _ctx(lib, 2, "bf16x3")
    a, b = _scheduled(lib, 2, "bf16x3"), Stream(pk, 3).run(x, SCHEDULE)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_flush_before_any_frame_is_zero_and_changes_nothing(lib):
    pk = _ctx(lib, 1, "f32")[0]
    st = Stream(pk, 2)
    assert np.all(st.flush() == 0.0)
    x = _x(n=2, hops=9, seed=6)
    first = st.push(x[:, :HOP])                            # one hop: still no complete frame
    assert np.all(first == 0.0) and np.all(st.flush() == 0.0)
    before = st.state.copy()
    st.flush()
    assert np.array_equal(before, st.state)
    rest = st.push(x[:, HOP:])
    assert np.array_equal(stitched(np.concatenate([first, rest], axis=-1), st.flush(), HOP), pk.one(x))


def _raw_step(pk, cf, n, F, state_cut=0, ws_cut=0, n_buf=2, f_buf=4):
    """The return code of a step on generous scratch buffers, and whether `out` and the state stayed as they were."""
    lib = pk.lib
    good = _ctx(lib, 0, "f32")[0]
    sb = lib.tasnet_stream_state_bytes(good.cf, n_buf)
    wsb = lib.tasnet_stream_workspace_bytes(good.cf, n_buf, f_buf)
    if state_cut or ws_cut:                                # exact sizes of this very call, one byte short
        sb, wsb = lib.tasnet_stream_state_bytes(cf, n) - state_cut, lib.tasnet_stream_workspace_bytes(cf, n, F) - ws_cut
    state, ws = tasnet_emu.aligned(sb + 1), tasnet_emu.aligned(wsb + 1)
    state[:] = 0x5A
    x = np.zeros((n_buf, f_buf * HOP), np.float32)
    out = np.full((pk.c["num_spks"], n_buf, f_buf * HOP), np.nan, dtype=np.float32)
    rc = lib.dll.onssen_tasnet_stream_step_f32(cf, pk.image.ctypes.data, x.ctypes.data, n, F, f_buf * HOP, out.ctypes.data,
                                               state.ctypes.data, sb, ws.ctypes.data, wsb, None)
    return rc, bool(np.isnan(out).all() and np.all(state == 0x5A))


def test_refusals_launch_nothing(lib):
    ok = _ctx(lib, 0, "f32")[0]
    assert _raw_step(ok, ok.cf, 2, 4)[0] == 0              # the scratch call itself is sound
    for bad in (dict(causal=False), dict(norm="gln")):
        cfg = dict(dict(SBASE, **CASES[0]), **bad)
        pk = Packed(lib, tasnet_ref.make_state(cfg, seed=5), cfg, "f32")
        assert _raw_step(pk, pk.cf, 2, 4) == (E_ARG, True), bad
        assert lib.dll.onssen_tasnet_stream_state_bytes(pk.cf, 2) == 0
        assert lib.dll.onssen_tasnet_stream_workspace_bytes(pk.cf, 2, 4) == 0
        buf = tasnet_emu.aligned(4096)
        buf[:] = 0x5A
        assert lib.dll.onssen_tasnet_stream_reset(pk.cf, buf.ctypes.data, 4096, 2, None, 0, None) == E_ARG
        out = np.full((2, 2, HOP), np.nan, np.float32)
        assert lib.dll.onssen_tasnet_stream_flush_f32(pk.cf, pk.image.ctypes.data, buf.ctypes.data, 4096, 2, out.ctypes.data,
                                                      None) == E_ARG
        assert np.all(buf == 0x5A) and np.isnan(out).all()
    assert _raw_step(ok, ok.cf, 2, 0) == (E_ARG, True)     # frames = 0
    assert _raw_step(ok, ok.cf, 0, 4) == (E_ARG, True)     # n = 0
    assert _raw_step(ok, ok.cf, 2, 4, state_cut=1) == (E_WORKSPACE, True)
    assert _raw_step(ok, ok.cf, 2, 4, ws_cut=1) == (E_WORKSPACE, True)
    assert lib.dll.onssen_tasnet_stream_state_bytes(ok.cf, 0) == 0
    assert lib.dll.onssen_tasnet_stream_workspace_bytes(ok.cf, 2, 0) == 0
    # reset: a slot index = n, and a state one byte short
    import ctypes as C
    sb = lib.tasnet_stream_state_bytes(ok.cf, 3)
    state = tasnet_emu.aligned(sb)
    state[:] = 0x5A
    assert lib.dll.onssen_tasnet_stream_reset(ok.cf, state.ctypes.data, sb, 3, (C.c_int32 * 2)(0, 3), 2, None) == E_ARG
    assert lib.dll.onssen_tasnet_stream_reset(ok.cf, state.ctypes.data, sb, 3, (C.c_int32 * 1)(-1), 1, None) == E_ARG
    assert lib.dll.onssen_tasnet_stream_reset(ok.cf, state.ctypes.data, sb - 1, 3, None, 0, None) == E_WORKSPACE
    out = np.full((2, 3, HOP), np.nan, np.float32)
    assert lib.dll.onssen_tasnet_stream_flush_f32(ok.cf, ok.image.ctypes.data, state.ctypes.data, sb - 1, 3, out.ctypes.data,
                                                  None) == E_WORKSPACE
    assert np.all(state == 0x5A) and np.isnan(out).all()
    assert lib.dll.onssen_tasnet_stream_reset(ok.cf, state.ctypes.data, sb, 3, (C.c_int32 * 1)(2), 1, None) == 0
    assert not np.all(state == 0x5A)


def test_state_size_overflow_is_zero(lib):
    big = tasnet_emu.lib_cfg(lib, dict(SBASE, norm="cln", activate="relu", P=2, X=25, H=2 ** 30), "f32")
    assert lib.dll.onssen_tasnet_stream_state_bytes(big, 65535) == 0    # 2^16 streams x 2^24 frames x 2^32 bytes
    assert lib.dll.onssen_tasnet_stream_state_bytes(big, 65536) == 0
    deep = tasnet_emu.lib_cfg(lib, dict(SBASE, norm="cln", activate="relu", P=3, X=25), "f32")
    assert lib.dll.onssen_tasnet_stream_state_bytes(deep, 1) == 0       # history 2^25 > ONSSEN_TASNET_STREAM_MAX_HISTORY
