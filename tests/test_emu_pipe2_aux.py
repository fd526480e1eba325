"""Host-side kernel test of onssen_blstm_pipe2_map_forward_f32: the pair launch whose trailing workgroups build the deep-clustering
target map.  It must leave, byte for byte, what onssen_blstm_pipe2_forward_f32 + onssen_dc_index_f32 leave: the same pair workspace
and the same clustering workspace (header, int words, status word, target map), and nothing in the compacted-rows region."""
import numpy as np
import pytest

from onssen_amd import _abi
from onssen_amd.synthetic import make_state_dict
from tests.emu_build import load_emu

F, D, DB = 9, 4, 40.0


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def P(a):
    return a.ctypes.data


def _shm(shape, fill=0.0, dtype=np.float32):
    """'Device' buffer in MAP_SHARED memory, 256-byte aligned: visible to forked workgroup processes."""
    import mmap
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    a = np.frombuffer(mmap.mmap(-1, max(n, 4096)), dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    a[...] = fill
    return a


def _packed_weights(lib, H, ug):
    """The two layers' x3 projection images, split-bf16 recurrent images and packed biases (as the pair launch's own test packs them)."""
    sd = make_state_dict("chimera", F, H, 2, 4, 2, seed=H + ug, gain=2.0)
    Hp, NP, _, we = lib.lstm_geometry(H, ug)
    _, _, we3 = lib.lstm_geometry_x3(H, ug)
    wih3, whh3, bias = [], [], []
    for l in range(2):
        K = F if l == 0 else 2 * Hp
        Kp = (F + 3) // 4 * 4 if l == 0 else 2 * Hp
        a, c, b3 = _shm((2, NP, Kp)), _shm((2, NP)), _shm((2, we3), dtype=np.uint16)
        scratch = _shm((we,))
        for d, sfx in enumerate(("", "_reverse")):
            srcs = []
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                v = sd[f"rnn.{n}_l{l}{sfx}"]
                sv = _shm(v.shape); sv[...] = v
                srcs.append(sv)
            lib.lstm_pack(P(srcs[0]), P(srcs[1]), P(srcs[2]), P(srcs[3]), srcs[0].shape[1], 0 if l == 0 else 1, H, ug,
                          P(a[d]), P(scratch), P(c[d]), None)
            lib.lstm_pack_whh_bf16x3(P(srcs[1]), H, ug, P(b3[d]), None)
        pl = _shm((2 * NP, (K + 31) // 32, 2, 32), dtype=np.uint16)
        lib.x3_image(P(a), Kp, 0, 1, 2 * NP, K, P(pl), None)
        wih3.append(pl), whh3.append(b3), bias.append(c)
    return [P(a) for a in wih3], [P(a) for a in whh3], [P(a) for a in bias], (wih3, whh3, bias)


def _utterance(rng, kind, T):
    """One utterance's (T, F) features.  0: random.  1: all equal -- every bin active, the loudest bin is index 0.  2: the maximum
    occurs twice (the loudest bin is the first), bins exactly AT max - db/20 (active: the test is inclusive) and one ulp below (silent)."""
    f = rng.standard_normal((T, F)).astype(np.float32)
    if kind == 1:
        f[...] = np.float32(-0.75)
    elif kind == 2:
        f = f.clip(-3.0, 1.0).reshape(-1)
        top, thr = np.float32(1.5), np.float32(1.5) - np.float32(DB) / np.float32(20.0)
        f[[7, 19]] = top
        f[[3, 11, 20]] = thr
        f[[4, 12, 21]] = np.nextafter(thr, np.float32(-np.inf))
        f = f.reshape(T, F)
    return f


@pytest.mark.parametrize("H,ug,B,T,kinds", [
    (8, 4, 3, 4, [(0, 1, 2)]),                    # stacked 8-row groups; the three kinds of utterance side by side
    (24, 8, 17, 3, [(0, 1, 2)]),                  # the smallest batch on 16-row unstacked groups, second group part-filled; 16 aux workgroups
    (8, 4, 1, 4, [(0,), (1,), (2,)]),             # n_aux = 1
    (8, 4, 32, 4, [(2, 0, 1)]),                   # n_aux = 16: every aux workgroup owns two utterances
])
def test_pair_launch_with_aux_map_leaves_the_old_bytes(lib, monkeypatch, H, ug, B, T, kinds):
    monkeypatch.setenv("ONSSEN_EMU_SCRAMBLE_XCC", "0")
    lib.dll.onssen_xcd_spin_limit(40000000)
    wih, whh, bias, _keep = _packed_weights(lib, H, ug)
    flags = _abi.BLSTM_BF16X3 | _abi.BLSTM_XCD
    nb = lib.blstm_pipe2_workspace_bytes(B, T, F, H, ug)
    cnb, comp_off, dest_off = lib.dc_compact_layout(B, T, F, D)
    stat = int(lib.dll.onssen_dc_cluster_status_offset(B, D))
    assert T * F < 64 and stat < comp_off < dest_off < cnb         # chunks of one bin, and chunks without any
    ws_new, ws_old = _shm((nb // 4,)), _shm((nb // 4,))            # zeroed once (ABI)
    fill = (np.arange(cnb // 4, dtype=np.uint64) * 2654435761 % 0xfffffffb).astype(np.uint32) | 1      # non-zero, position-dependent
    cw_new, cw_old = _shm((cnb // 4,), dtype=np.uint32), _shm((cnb // 4,), dtype=np.uint32)
    x = _shm((B, T, F))
    rng = np.random.default_rng(100 * H + B)
    for call, ks in enumerate(kinds):
        for b in range(B):
            x[b] = _utterance(rng, ks[b % len(ks)], T)
        cw_new[...] = fill; cw_old[...] = fill
        # the pair launch's workgroups talk to each other: one forked process each; dc_index's do not (and there are 64 per utterance)
        monkeypatch.setenv("ONSSEN_EMU_FORK", "1")
        lib.blstm_pipe2_map_forward(P(x), T * F, F, B, T, F, H, ug, wih, whh, bias, P(ws_new), nb, flags, DB, D, P(cw_new), cnb, None)
        lib.blstm_pipe2_forward(P(x), T * F, F, B, T, F, H, ug, wih, whh, bias, P(ws_old), nb, flags, None)
        monkeypatch.setenv("ONSSEN_EMU_FORK", "0")
        lib.dc_index(P(x), B, T, F, D, DB, P(cw_old), cnb, None)
        for w in (ws_new, ws_old):
            assert w.view(np.uint32)[280] == 0, f"launch aborted (code {w.view(np.uint32)[280]})"
        assert ws_new.tobytes() == ws_old.tobytes(), call
        new, old = np.array(cw_new), np.array(cw_old)
        np.testing.assert_array_equal(new[:comp_off // 4], old[:comp_off // 4])          # header, int words, status word
        np.testing.assert_array_equal(new[dest_off // 4:], old[dest_off // 4:])          # the target map
        np.testing.assert_array_equal(new[comp_off // 4:dest_off // 4], fill[comp_off // 4:dest_off // 4])      # nobody's yet
        assert new[stat // 4] == fill[stat // 4]                                         # the status word is the clustering's to write
        # and the old bytes are the right ones: the map against NumPy, the loudest bin, the count
        dest = new.view(np.int32)[dest_off // 4:dest_off // 4 + B * T * F].reshape(B, T * F)
        stride = 1 + 2 * D + 64 * 2 * (D + 1) + 1
        iw = new.view(np.int32)[-(-B * stride * 4 // 256) * 64:][:B * 72].reshape(B, 72)
        for b in range(B):
            f = np.array(x[b]).reshape(-1)
            act = f >= f.max() - np.float32(DB) / np.float32(20.0)
            np.testing.assert_array_equal(dest[b], np.where(act, np.cumsum(act) - 1, -1))
            assert new.view(np.float32)[b * stride] == f.max() and new[b * stride + stride - 1] == int(np.argmax(f))
            assert iw[b, 64] == act.sum() and iw[b, :64].sum() == act.sum() and not iw[b, 65:].any()
            if ks[b % len(ks)] == 1:
                assert act.all() and np.argmax(f) == 0
            if ks[b % len(ks)] == 2:
                assert np.argmax(f) == 7 and act[[3, 11, 20]].all() and not act[[4, 12, 21]].any()


def test_map_workspace_is_validated_like_dc_index(lib, monkeypatch):
    monkeypatch.setenv("ONSSEN_EMU_FORK", "1")
    H, ug, B, T = 8, 4, 2, 3
    wih, whh, bias, _keep = _packed_weights(lib, H, ug)
    arr = lambda ptrs: (_abi.C.c_void_p * 2)(*ptrs)
    flags = _abi.BLSTM_BF16X3 | _abi.BLSTM_XCD
    nb = lib.blstm_pipe2_workspace_bytes(B, T, F, H, ug)
    cnb, _, _ = lib.dc_compact_layout(B, T, F, D)
    cluster_nb = int(lib.dll.onssen_dc_cluster_workspace_bytes(B, T, F, D))
    ws, cw, x = _shm((nb // 4,)), _shm((cnb // 4 + 64,)), _shm((B, T, F))
    before = ws.tobytes()

    def call(xs_b=T * F, xs_t=F, d=D, map_ws=P(cw), map_nb=cnb):
        return lib.dll.onssen_blstm_pipe2_map_forward_f32(P(x), xs_b, xs_t, B, T, F, H, ug, arr(wih), arr(whh), arr(bias), P(ws), nb, flags,
                                                          DB, d, map_ws, map_nb, None)
    assert call(map_nb=cluster_nb) == -2          # ONSSEN_E_WORKSPACE: the clustering's size lacks the map
    assert call(map_ws=P(cw) + 64) == -3          # ONSSEN_E_ALIGN
    assert call(d=33) == -1 and call(d=0) == -1 and call(map_ws=None) == -1      # ONSSEN_E_ARG
    assert call(xs_b=T * F + 1) == -1 and call(xs_t=F + 1) == -1                 # the features are the dense input
    assert ws.tobytes() == before                 # nothing was launched
