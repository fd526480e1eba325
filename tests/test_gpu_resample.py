"""features.resample on the device against scipy.signal.resample_poly in float64: the cases of tests/test_emu_resample.py through
the Python surface, with the same bound (tests/resample_ref.py: |y - ref| <= 2^-24 |ref| + 1e-13 absum), plus a graph capture."""
import numpy as np
import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

RATES = {(1, 3): (48000, 16000), (160, 441): (44100, 16000), (2, 1): (8000, 16000), (320, 441): (22050, 16000),
         (1, 500): (8000, 16)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from onssen_amd.hip import get_lib
    get_lib()   # fail loudly if libonssen_hip.so is missing
    return torch.device("cuda:0")


def make(lengths, seed, with_sub, dev):
    """Rows of ``lengths`` samples; whatever lies beyond a row's length is NaN."""
    rng = np.random.default_rng(seed)
    x = np.full((len(lengths), max(lengths)), np.nan, np.float32)
    sub = np.full_like(x, np.nan) if with_sub else None
    for b, n in enumerate(lengths):
        x[b, :n] = rng.uniform(-1, 1, n)
        if with_sub:
            sub[b, :n] = rng.uniform(-1, 1, n)
    return x, sub, torch.from_numpy(x).to(dev), (torch.from_numpy(sub).to(dev) if with_sub else None)


def check_rows(x, sub, y, lo, key, lengths, what):
    up, down = key
    y, lo = y.cpu().numpy(), lo.cpu().numpy()
    assert y.shape == (len(lengths), R.n_out(max(lengths), up, down))
    worst = 0.0
    for b, n in enumerate(lengths):
        no = R.n_out(n, up, down)
        assert lo[b] == no
        s = None if sub is None else sub[b, :n]
        ref = R.reference(x[b, :n], up, down, s)
        worst = max(worst, R.ratio(y[b, :no], ref, R.absum(x[b, :n], up, down, np.arange(no), s), up, down))
        assert np.all(y[b, no:] == 0.0) and not np.signbit(y[b, no:]).any()
    print(f"{what}: largest |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


CASES = [((1, 3), (1000, 1, 61, 999), False), ((160, 441), (2000, 5, 441), False), ((2, 1), (333, 1), False),
         ((320, 441), (700,), False), ((1, 3), (20011, 3000), False), ((160, 441), (20011,), False),
         ((1, 3), (1000, 61, 2500), True), ((160, 441), (2000, 441), True), ((1, 500), (30011, 700), True)]


@pytest.mark.parametrize("key,lengths,with_sub", CASES)
def test_values_padding_and_lengths(dev, key, lengths, with_sub):
    from onssen_amd.features import resample
    x, sub, xd, sd = make(lengths, 3, with_sub, dev)
    y, lo = resample(xd, *RATES[key], lengths=list(lengths), sub=sd)
    check_rows(x, sub, y, lo, key, lengths, f"{key} {lengths} sub={with_sub}")


@pytest.mark.parametrize("key,lengths", [((1, 3), (1000, 1, 61, 3100)), ((160, 441), (2000, 5, 441))])
def test_rows_equal_their_batch_1_result_and_runs_repeat(dev, key, lengths):
    from onssen_amd.features import resample
    x, sub, xd, sd = make(lengths, 13, True, dev)
    y, lo = resample(xd, *RATES[key], lengths=list(lengths), sub=sd)
    y2, lo2 = resample(xd, *RATES[key], lengths=torch.tensor(lengths, dtype=torch.int32, device=dev), sub=sd)
    assert torch.equal(y, y2) and torch.equal(lo, lo2)
    for b, n in enumerate(lengths):
        one, lo1 = resample(xd[b, :n].clone(), *RATES[key], sub=sd[b, :n].clone())
        assert int(lo1[0]) == one.shape[1] == R.n_out(n, *key)
        assert torch.equal(one[0], y[b, :one.shape[1]]), f"row {b}"


def test_equal_rates_copy(dev):
    from onssen_amd.features import resample
    x, sub, xd, sd = make((300, 1), 17, True, dev)
    y, lo = resample(xd, 16000, 16000, lengths=[300, 1])
    assert lo.tolist() == [300, 1] and torch.equal(y[0], xd[0]) and float(y[1, 0]) == float(xd[1, 0]) and (y[1, 1:] == 0).all()
    y, _ = resample(xd, 44100, 44100, lengths=[300, 1], sub=sd)
    want = (x[0].astype(np.float64) - sub[0].astype(np.float64)).astype(np.float32)
    assert y[0].cpu().numpy().tobytes() == want.tobytes()


def test_64_bit_indexing(dev):
    """44.1 -> 16 kHz over 13 500 000 samples (five minutes): 4 897 960 outputs, the last m down = 2 159 999 919 > 2^31; checked
    at both ends and in the stripe in which m 441 crosses 2^31."""
    from onssen_amd.features import resample
    up, down, n = 160, 441, 13_500_000
    x = np.random.default_rng(23).uniform(-1, 1, n).astype(np.float32)
    y, lo = resample(torch.from_numpy(x).to(dev), 44100, 16000)
    y = y[0].cpu().numpy()
    no = R.n_out(n, up, down)
    assert no == 4_897_960 == len(y) == int(lo[0]) and (no - 1) * down > 2 ** 31
    ref = R.reference(x, up, down)
    assert np.isfinite(y).all()
    worst = 0.0
    for a, b in ((0, 4096), (no - 4096, no), (4_868_000, 4_871_000)):
        worst = max(worst, R.ratio(y[a:b], ref[a:b], R.absum(x, up, down, np.arange(a, b)), up, down))
    print(f"2^31 case: largest |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_graph_capture_replays_on_fresh_inputs(dev):
    """One call captured into a graph (the launch allocates nothing on its own and does not synchronise) and replayed twice on
    new inputs equals the eager result bit for bit."""
    from onssen_amd.features import resample
    lengths = (5000, 3333, 17)
    x0, s0, xd, sd = make(lengths, 31, True, dev)
    xd, sd = torch.nan_to_num(xd), torch.nan_to_num(sd)            # (static buffers that are refilled below)
    ld = torch.tensor(lengths, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm up off the default stream: the ratio's tap image exists
        resample(xd, 44100, 16000, lengths=ld, sub=sd)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y, lo = resample(xd, 44100, 16000, lengths=ld, sub=sd)
    for seed in (41, 43):
        _, _, xn, sn = make(lengths, seed, True, dev)
        xd.copy_(torch.nan_to_num(xn))
        sd.copy_(torch.nan_to_num(sn))
        g.replay()
        torch.cuda.synchronize()
        ye, le = resample(xd, 44100, 16000, lengths=ld, sub=sd)
        assert torch.equal(y, ye) and torch.equal(lo, le) and float(ye.abs().max()) > 0
