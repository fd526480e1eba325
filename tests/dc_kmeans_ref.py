"""Test support (not a test): a float64 NumPy restatement of the K-cluster deep-clustering back end
(onssen_amd/csrc/kmeans_k.inc, ``onssen_dc_cluster_k_f32``) for ONE utterance, and the planted-cluster inputs its tests share.

The algorithm, as include/onssen_hip.h states it:
  threshold       a bin is active iff feature >= max(feature) - db / 20 (a float32 comparison, as on the device: the features ARE
                  float32 and so is the threshold they are compared with); the first maximum is the loudest bin
  initialisation  c_0 = the loudest bin's embedding; c_k = the active bin minimising max_{j<k} e.c_j, ties to the smallest bin
                  index; c_0 when nothing is active
  iteration       label = argmin_k |c_k|^2 - 2 e.c_k, ties to the smallest k; new centroid = mean of its bins, an empty cluster
                  keeps its centroid; stop at the bitwise fixed point, when the summed squared shift is
                  <= tol x (1 - |mean|^2) / D, or after ``iters`` iterations
  masks           (N, K) one-hot under the final centroids on the active bins, zero elsewhere
Everything after the threshold is float64."""
import numpy as np


def kmeans_masks_ref(emb, feat, K, db=40.0, iters=20, tol=1e-4):
    """emb (N, D) float32, feat (N,) float32 -> (masks (N, K) float32, iterations run, converged)."""
    emb, feat = np.asarray(emb), np.asarray(feat, np.float32)
    N, D = emb.shape
    i0 = int(np.argmax(feat))                                           # the first maximum
    act = feat >= np.float32(feat[i0] - np.float32(db) / np.float32(20.0))
    e = emb.astype(np.float64)
    ea = e[act]
    idx = np.flatnonzero(act)
    c = [e[i0]]
    for k in range(1, K):
        if len(idx) == 0:
            c.append(c[0])
            continue
        score = np.max(np.stack([ea @ cj for cj in c], 0), 0)
        c.append(e[idx[int(np.argmin(score))]])                         # np.argmin: the first minimum = the smallest bin index
    c = np.stack(c)

    def labels(c):
        return np.argmin((c * c).sum(1)[None] - 2.0 * (ea @ c.T), 1)    # the first minimum = the smallest k

    n_iter, converged = 0, False
    for _ in range(iters):
        lab = labels(c)
        new = c.copy()
        for k in range(K):
            if np.any(lab == k):
                new[k] = ea[lab == k].mean(0)
        n_iter += 1
        shift, changed = ((new - c) ** 2).sum(), bool(np.any(new != c))
        c = new
        mean = ea.mean(0) if len(ea) else np.zeros(D)
        var = max(1.0 - (mean * mean).sum(), 0.0) / D
        if not changed or (tol > 0 and shift <= tol * var):
            converged = True
            break
    masks = np.zeros((N, K), np.float32)
    if len(idx):
        masks[idx, labels(c)] = 1.0
    return masks, n_iter, converged


def planted(seed, B, T, F, D, K, noise=0.15):
    """Embeddings with K planted, well separated clusters: per utterance K orthonormal directions (QR of a seeded Gaussian
    matrix), every bin one of them plus isotropic noise, renormalised; speaker shares .5/.3/.2 at K = 3, equal otherwise;
    features uniform in [-3, 0], so that about two thirds of the bins are active at db = 40.
    -> emb (B, T, F, D) float32, feat (B, T, F) float32, lab (B, T, F)."""
    rng = np.random.default_rng(seed)
    share = [0.5, 0.3, 0.2] if K == 3 else [1.0 / K] * K
    emb = np.empty((B, T, F, D), np.float32)
    lab = np.empty((B, T, F), np.int64)
    for b in range(B):
        q, _ = np.linalg.qr(rng.standard_normal((D, K)))
        lab[b] = rng.choice(K, size=(T, F), p=share)
        x = q.T[lab[b]] + noise * rng.standard_normal((T, F, D))
        emb[b] = (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)
    feat = rng.uniform(-3.0, 0.0, (B, T, F)).astype(np.float32)
    return emb, feat, lab


def ref_batch(emb, feat, K, frames=None, **kw):
    """The reference over a batch -> masks (B, T, F, K) (zero on the padding), iterations (B,), converged (B,)."""
    B, T, F, D = emb.shape
    masks = np.zeros((B, T, F, K), np.float32)
    its, conv = np.zeros(B, np.int64), np.zeros(B, bool)
    for b in range(B):
        Tb = T if frames is None else int(frames[b])
        m, its[b], conv[b] = kmeans_masks_ref(emb[b, :Tb].reshape(-1, D), feat[b, :Tb].reshape(-1), K, **kw)
        masks[b, :Tb] = m.reshape(Tb, F, K)
    return masks, its, conv
