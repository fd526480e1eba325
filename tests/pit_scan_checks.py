"""Every assignment can win: the check shared by tests/test_emu_pit_scan.py (host-side build) and tests/test_gpu_pit_scan.py
(device) for the three entries whose final kernels step through the speaker assignments with csrc/pit.inc's enumerator:
onssen_batch_sdr_f32, onssen_sisnr_pit_f32 and onssen_wa_pit_f32.

One call per (entry, K) whose K! rows are the K! permutations: row r holds K independent random references, its estimates are
those references rearranged by permutation number r of itertools.permutations(range(K)), plus 5 % noise.  The expected index
comes from the float64 restatements (oracle/np_oracle.py, tests/sisnr_pit_ref.py, tests/wa_pit_cases.py), and
two conditions are asserted on them alone before the library is looked at: every row's best total is at least GAP (relative)
from its runner-up, and the K! winning indices of a call are pairwise distinct -- a scan that skipped, repeated or misnumbered
an assignment cannot pass.  A ``backend`` is tests/wa_checks.py's."""
import itertools

import numpy as np

N_SAMPLES = 64          # per signal
GAP = 1e-3
NOISE = 0.05
ENTRIES = ("batch_sdr", "sisnr_pit", "wa_pit")
CASES = [(e, K) for e in ENTRIES for K in (1, 2, 3, 4)]


def waveforms(K, seed):
    """est, ref (K!, K, N_SAMPLES) float32: est[r, i] = ref[r, p_r[i]] + noise."""
    rng = np.random.default_rng(seed)
    perms = list(itertools.permutations(range(K)))
    ref = rng.standard_normal((len(perms), K, N_SAMPLES)).astype(np.float32)
    est = np.empty_like(ref)
    for r, p in enumerate(perms):
        for i in range(K):
            est[r, i] = ref[r, p[i]] + (NOISE * rng.standard_normal(N_SAMPLES)).astype(np.float32)
    return est, ref


def rel_gap(totals, best):
    """(rows,): |best - runner-up| / |best| of a (rows, K!) table of totals; inf where there is one assignment."""
    if totals.shape[1] == 1:
        return np.full(len(totals), np.inf)
    rest = np.sort(np.abs(totals - best[:, None]), 1)[:, 1]
    return rest / np.abs(best)


def sdr_case(be, K):
    from oracle import np_oracle as O
    est, ref = waveforms(K, 11 + K)
    B = len(est)
    _, want = O.batch_sdr(est, ref)
    # the oracle's pair table through its one-speaker form (the centring is per signal), for the runner-up
    tab = np.stack([np.stack([O.batch_sdr(est[:, i:i + 1], ref[:, j:j + 1])[0] for j in range(K)], 1) for i in range(K)], 1)
    tot = np.stack([sum(tab[:, i, p[i]] for i in range(K)) for p in itertools.permutations(range(K))], 1)
    assert (tot.argmax(1) == want).all()

    def run():
        d_est, d_ref = be.dev(est), be.dev(ref)
        nb = be.lib.batch_sdr_workspace_bytes(B)
        ws = be.dev(np.zeros(nb // 8 + 1, np.float64))
        out, perm = be.dev(np.full(B, np.nan, np.float32)), be.dev(np.full(B, -1, np.int32))
        be.lib.batch_sdr(be.ptr(d_est), be.ptr(d_ref), None, B, K, N_SAMPLES, be.ptr(out), be.ptr(perm), be.ptr(ws), nb, None)
        return be.host(perm)
    return want, rel_gap(tot, tot.max(1)), run


def sisnr_case(be, K):
    from tests import sisnr_pit_ref as R
    est, ref = waveforms(K, 21 + K)
    B = len(est)
    ests, refs = np.ascontiguousarray(est.transpose(1, 0, 2)), np.ascontiguousarray(ref.transpose(1, 0, 2))      # (K, B, n)
    want = R.reference(list(ests), list(refs))

    def run():
        d_est, d_ref = be.dev(ests), be.dev(refs)
        sig = lambda d: be.lib.sisnr_signals([be.ptr(d) + 4 * i * B * N_SAMPLES for i in range(K)], [N_SAMPLES] * K)
        nb = be.lib.sisnr_pit_workspace_bytes(B, K)
        ws = be.dev(np.full(nb // 8 + 1, np.nan, np.float64))
        value, perm = be.dev(np.full(B, np.nan, np.float32)), be.dev(np.full(B, -1, np.int32))
        be.lib.sisnr_pit(sig(d_est), sig(d_ref), K, B, N_SAMPLES, None, be.ptr(value), be.ptr(perm), None, be.ptr(ws), nb, None)
        return be.host(perm)
    return want["perm"], want["margin"] / np.abs(want["value"]), run


def wa_case(be, K):
    from tests import wa_pit_cases as W
    est, ref = waveforms(K, 31 + K)
    B = len(est)
    _, want, _, _, gap = W.reference(est, ref, None, np.ones(B))

    def run():
        d_est, d_ref = be.dev(est), be.dev(ref)
        nb = be.lib.wa_pit_workspace_bytes(B, K)
        ws = be.dev(np.full(nb // 8 + 1, np.nan, np.float64))
        value, perm = be.dev(np.full(B, np.nan, np.float32)), be.dev(np.full(B, -1, np.int32))
        be.lib.wa_pit(be.ptr(d_est), be.ptr(d_ref), K * N_SAMPLES, N_SAMPLES, B, K, N_SAMPLES, None, be.ptr(value), be.ptr(perm), None,
                      be.ptr(ws), nb, None)
        return be.host(perm)
    return np.asarray(want), gap, run


_BUILD = dict(batch_sdr=sdr_case, sisnr_pit=sisnr_case, wa_pit=wa_case)


def check_every_assignment_wins(be, entry, K):
    want, gap, run = _BUILD[entry](be, K)
    want = [int(v) for v in want]
    print(f"{entry} K={K}: expected indices {want}, smallest relative gap to the runner-up {float(np.min(gap)):.3e} (at least {GAP})")
    assert (np.asarray(gap) >= GAP).all(), gap
    assert len(want) == len(set(want)) == len(list(itertools.permutations(range(K)))), want
    got = run()
    assert [int(v) for v in got] == want, (got.tolist(), want)
