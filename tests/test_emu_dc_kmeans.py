"""The deep-clustering back end for 2 .. 4 speakers (onssen_amd/csrc/kmeans_k.inc, ``onssen_dc_cluster_k_f32``) through the
host-side emulation of the product's HIP source, against the float64 restatement in tests/dc_kmeans_ref.py.

The planted clusters are separated so widely (orthonormal directions, noise 0.15) that the float64 reference agrees with the
planted labels and with sklearn on every active bin in 2-3 iterations; with that margin a float32 rounding cannot move a bin
across a boundary, so the masks must EQUAL the reference's -- channel order included, since the numbering is deterministic."""
import numpy as np
import pytest

from onssen_amd import _abi
from tests.dc_kmeans_ref import kmeans_masks_ref, planted, ref_batch
from tests.emu_build import load_emu
from tests.test_emu_kernels import P, _shm, _two_cluster_embeddings, aligned_f32


@pytest.fixture(scope="module")
def lib():
    return load_emu()


def shm_of(a):
    s = _shm(a.shape, dtype=a.dtype)
    s[...] = a
    return s


def run_k(lib, emb, feat, K, iters=20, tol=1e-4, db=40.0, frames=None, scribble=None):
    """-> masks (B,T,F,K), iterations (B,), converged (B,) of one call on buffers of its own."""
    B, T, F, D = emb.shape
    e, f = shm_of(emb), shm_of(feat)
    nb = lib.dll.onssen_dc_cluster_k_workspace_bytes(B, T, F, D, K)
    assert nb > 0
    ws = _shm((nb // 4 + 64,), fill=np.nan if scribble is None else scribble)
    masks = _shm((B, T, F, K), fill=np.nan)
    fr = None
    if frames is not None:
        fr = _shm((B,), dtype=np.int32)
        fr[...] = frames
    lib.dc_cluster_k(P(e), P(f), B, T, F, D, K, db, iters, P(masks), P(ws), nb, None, frames=P(fr), tol=tol)
    info = np.array(ws.view(np.int32)[:4 * B]).reshape(B, 4)
    return np.array(masks), info[:, 0], info[:, 1]


@pytest.mark.parametrize("B,T,F,D,K", [(2, 7, 33, 20, 3), (1, 5, 17, 8, 4), (1, 9, 17, 6, 3)])     # D = 6: rows that are no 16-byte multiples
def test_masks_equal_the_reference(lib, B, T, F, D, K):
    emb, feat, lab = planted(B + D + K, B, T, F, D, K)
    masks, its, conv = run_k(lib, emb, feat, K)
    ref, rits, rconv = ref_batch(emb, feat, K)
    np.testing.assert_array_equal(masks, ref)
    np.testing.assert_array_equal(its, rits)
    np.testing.assert_array_equal(conv, rconv.astype(np.int32))
    for b in range(B):
        act = feat[b] >= feat[b].max() - np.float32(2.0)
        assert np.all(masks[b][~act] == 0) and np.all(masks[b][act].sum(-1) == 1)
        # the reference itself recovers the planted partition (up to the numbering)
        got = masks[b][act].argmax(-1)
        assert len({(g, l) for g, l in zip(got, lab[b][act])}) == K


def test_ragged_rows_equal_the_one_utterance_call(lib):
    """Each row of a ragged batch equals, bit for bit, the uniform call on that utterance alone; the padding -- NaN
    embeddings and a feature louder than anything real -- is never active, never moves the threshold and gets zero masks."""
    B, T, F, D, K = 2, 14, 33, 20, 3
    frames = [14, 9]
    emb0, feat0, _ = planted(7, B, T, F, D, K)
    emb, feat = emb0.copy(), feat0.copy()
    for b in range(B):
        emb[b, frames[b]:] = np.nan
        feat[b, frames[b]:] = 50.0
    masks, its, _ = run_k(lib, emb, feat, K, frames=frames)
    for b in range(B):
        Tb = frames[b]
        m1, it1, _ = run_k(lib, np.ascontiguousarray(emb0[b:b + 1, :Tb]), np.ascontiguousarray(feat0[b:b + 1, :Tb]), K)
        np.testing.assert_array_equal(masks[b, :Tb], m1[0])
        assert its[b] == it1[0]
        assert np.all(masks[b, Tb:] == 0)
        assert masks[b, :Tb].sum() > 0


def test_fewer_bins_than_clusters(lib):
    """T = 1, F = 2, K = 3: the third centroid duplicates the first (a tie, to the smaller bin index), its cluster stays empty
    and keeps its centroid.  (Rows with exact unit norms and exact dot products: the ties are ties in every precision.)"""
    emb = np.array([[[[0.5, 0.5, 0.5, 0.5], [0.5, -0.5, 0.5, -0.5]]]], np.float32)
    feat = np.array([[[-0.5, -1.0]]], np.float32)
    masks, its, conv = run_k(lib, emb, feat, 3)
    ref, rits, rconv = ref_batch(emb, feat, 3)
    np.testing.assert_array_equal(masks, ref)
    np.testing.assert_array_equal(masks[0, 0], [[1, 0, 0], [0, 1, 0]])
    assert its[0] == rits[0] == 1 and conv[0] == 1 and rconv[0]


def test_identical_active_embeddings(lib):
    rng = np.random.default_rng(3)
    T, F, D, K = 3, 5, 4, 4
    feat = rng.uniform(-3.0, 0.0, (1, T, F)).astype(np.float32)
    act = feat >= feat.max() - np.float32(2.0)
    emb = rng.standard_normal((1, T, F, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=-1, keepdims=True)
    emb[act] = 0.5
    assert 0 < act.sum() < act.size
    masks, its, conv = run_k(lib, emb, feat, K)
    ref, rits, _ = ref_batch(emb, feat, K)
    np.testing.assert_array_equal(masks, ref)
    assert np.all(masks[act] == [1, 0, 0, 0]) and np.all(masks[~act] == 0)
    assert its[0] == rits[0] == 1 and conv[0] == 1


@pytest.mark.parametrize("iters,tol", [(0, 1e-4), (20, 0.0)])
def test_no_iterations_and_the_fixed_point(lib, iters, tol):
    """iters = 0: the masks of the initial centroids; tol = 0: the iterations run to the bitwise fixed point."""
    B, T, F, D, K = 1, 7, 33, 20, 3
    emb, feat, _ = planted(5, B, T, F, D, K)
    masks, its, conv = run_k(lib, emb, feat, K, iters=iters, tol=tol)
    ref, rits, rconv = ref_batch(emb, feat, K, iters=iters, tol=tol)
    np.testing.assert_array_equal(masks, ref)
    assert its[0] == rits[0] and bool(conv[0]) == bool(rconv[0]) == (iters > 0)
    if iters == 0:
        assert its[0] == 0


def test_two_clusters_equal_the_two_means(lib):
    """K = 2 through the general entry against onssen_dc_cluster_f32 in its launch-per-iteration form: the same partition with
    the channels swapped -- the 2-means writes mask[0] = label (1 for the cluster grown from the farthest point)."""
    rng = np.random.default_rng(11)
    B, T, F, D = 2, 20, 33, 20
    emb, feat, _ = _two_cluster_embeddings(rng, B, T, F, D)
    masks, _, _ = run_k(lib, emb, feat, 2, iters=10)
    nb = lib.dll.onssen_dc_cluster_workspace_bytes(B, T, F, D)
    ws = aligned_f32(nb // 4 + 4)
    m2 = np.full((B, T, F, 2), np.nan, np.float32)
    lib.dc_cluster(P(emb), P(feat), B, T, F, D, 40.0, 10, P(m2), P(ws), nb, None, flags=_abi.DC_CLUSTER_LAUNCH_PER_ITERATION)
    np.testing.assert_array_equal(masks, m2[..., ::-1])
    assert masks[..., 0].sum() > 0 and masks[..., 1].sum() > 0


def test_two_calls_give_the_same_bits(lib):
    emb, feat, _ = planted(9, 2, 7, 33, 20, 4)
    a = run_k(lib, emb, feat, 4, scribble=np.nan)
    b = run_k(lib, emb, feat, 4, scribble=12345.0)          # whatever the workspace held before
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("K,D,short", [(1, 20, 0), (5, 20, 0), (3, 33, 0), (3, 20, 16)])
def test_argument_errors_write_nothing(lib, K, D, short):
    B, T, F = 1, 3, 5
    emb, feat = _shm((B, T, F, D), fill=0.5), _shm((B, T, F), fill=-1.0)
    nb = lib.dll.onssen_dc_cluster_k_workspace_bytes(B, T, F, D, K)
    assert (nb == 0) == (short == 0)
    ws = _shm((4096,), fill=7.0)
    masks = _shm((B, T, F, max(K, 1)), fill=np.nan)
    rc = lib.dll.onssen_dc_cluster_k_f32(P(emb), P(feat), B, T, None, F, D, K, 40.0, 5, 1e-4, P(masks), P(ws), nb - short if short else 16384, None)
    assert rc == -1
    assert np.all(np.isnan(np.array(masks))) and np.all(np.array(ws) == 7.0)
    if short:       # ... and a NULL pointer, with everything else in order
        assert lib.dll.onssen_dc_cluster_k_f32(P(emb), None, B, T, None, F, D, K, 40.0, 5, 1e-4, P(masks), P(ws), nb, None) == -1
        assert np.all(np.isnan(np.array(masks)))


def test_reference_agrees_with_sklearn():
    """The restatement the device is held to is itself k-means: the partition of sklearn's KMeans on the planted inputs."""
    from sklearn.cluster import KMeans
    for K, D, T, F in [(3, 20, 7, 33), (4, 8, 5, 17), (3, 6, 9, 17)]:
        emb, feat, lab = planted(K + D, 1, T, F, D, K)
        m, n_iter, conv = kmeans_masks_ref(emb[0].reshape(-1, D), feat[0].reshape(-1), K)
        act = m.sum(-1) == 1
        sk = KMeans(n_clusters=K, n_init=10, random_state=0).fit_predict(emb[0].reshape(-1, D)[act])
        pairs = {(a, b) for a, b in zip(m[act].argmax(-1), sk)}
        assert len(pairs) == K and conv and n_iter <= 3
        assert len({(a, b) for a, b in zip(m[act].argmax(-1), lab[0].reshape(-1)[act])}) == K
