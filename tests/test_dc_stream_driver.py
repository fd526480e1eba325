"""``separation.dc_stream`` -- the loop behind ``separate_dc_stream``, ``separate_dc_ragged_stream`` and ``tester_dc.eval`` --
against a fake pipeline that records its calls and raises ``XcdAborted`` where it is told to.  No GPU, no library."""
import warnings

import pytest

from onssen_amd.nn import _core
from onssen_amd.separation import dc_stream


class FakePipe:
    """``push(k)`` returns the estimate of the item before k (None for the first); ``flush()`` that of the last."""

    def __init__(self, log, abort_push=(), abort_flush=False):
        self.log, self.abort_push, self.abort_flush = log, set(abort_push), abort_flush
        self.inflight = None

    def push(self, item):
        self.log.append(("push", item))
        if item in self.abort_push:
            raise _core.XcdAborted(f"push {item} gave up")
        prev, self.inflight = self.inflight, item
        return None if prev is None else ("est", prev)

    def flush(self):
        self.log.append(("flush", self.inflight))
        if self.abort_flush:
            raise _core.XcdAborted("flush gave up")
        prev, self.inflight = self.inflight, None
        return ("est", prev)

    def reset(self):
        self.log.append(("reset",))
        self.inflight = None


def run(monkeypatch, items, abort_push=(), abort_flush=False, bad_status_after_push=None, fit=None):
    """The driver over ``items`` on one FakePipe -> (results, log).  Results: ("res", k) released from the pipeline's estimate of k,
    ("rerun", k) from the re-run callable, ("fallback", k) from the fallback.  ``bad_status_after_push`` = k: the status check that
    follows push k raises (the step that produced the estimate of k - 1 gave up a wait)."""
    log = []
    pipe = FakePipe(log, abort_push, abort_flush)

    def status(policy=True):
        log.append(("status",))
        if bad_status_after_push is not None and log[-3][0] == "push" and log[-3][1] == bad_status_after_push:
            raise _core.XcdAborted("status word set")

    def release(est, item):
        assert est == ("est", item)                  # the estimate handed back belongs to the oldest held item
        log.append(("release", item))
        return ("res", item)

    def rerun(held, e):
        assert isinstance(e, _core.XcdAborted)
        log.append(("rerun", list(held)))
        return [("rerun", k) for k in held]

    def fallback(item):
        log.append(("fallback", item))
        return ("fallback", item)

    monkeypatch.setattr(_core._XcdStatus, "flush", staticmethod(status))
    got = list(dc_stream(items, fit or (lambda item, p: pipe), lambda p, item: p.push(item), release, rerun, fallback, "by the fake"))
    return got, log


def reruns(log):
    return [e[1] for e in log if e[0] == "rerun"]


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_one_result_per_item_in_order(monkeypatch, n):
    r0 = _core._XcdPolicy.recovered
    got, log = run(monkeypatch, range(n))
    assert got == [("res", k) for k in range(n)]
    assert [e[1] for e in log if e[0] == "push"] == list(range(n))
    assert [e for e in log if e[0] == "flush"] == ([("flush", n - 1)] if n else [])
    assert not reruns(log) and ("reset",) not in log and _core._XcdPolicy.recovered == r0


def test_abort_at_a_push_reruns_the_two_held_items_and_the_stream_continues(monkeypatch):
    r0 = _core._XcdPolicy.recovered
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got, log = run(monkeypatch, range(5), abort_push=[2])
    assert got == [("res", 0), ("rerun", 1), ("rerun", 2), ("res", 3), ("res", 4)]
    assert reruns(log) == [[1, 2]] and log.count(("reset",)) == 1 and log.index(("reset",)) < log.index(("rerun", [1, 2]))
    assert _core._XcdPolicy.recovered == r0 + 1
    assert len(w) == 1 and "push 2 gave up" in str(w[0].message) and "by the fake" in str(w[0].message)


def test_abort_at_the_first_push_reruns_it_alone(monkeypatch):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, log = run(monkeypatch, range(3), abort_push=[0])
    assert got == [("rerun", 0), ("res", 1), ("res", 2)] and reruns(log) == [[0]]


def test_abort_at_the_final_flush_reruns_the_last_item_only(monkeypatch):
    r0 = _core._XcdPolicy.recovered
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, log = run(monkeypatch, range(5), abort_flush=True)
    assert got == [("res", k) for k in range(4)] + [("rerun", 4)]
    assert reruns(log) == [[4]] and _core._XcdPolicy.recovered == r0 + 1


def test_a_result_is_released_only_after_a_clean_status_check(monkeypatch):
    """Push 3 hands back the estimate of 2, then the status check fails: that estimate is not released, 2 and 3 are re-run."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, log = run(monkeypatch, range(5), bad_status_after_push=3)
    assert ("release", 2) in log                    # (it was computed: the status is examined after it ...)
    assert ("res", 2) not in got                    # (... and never handed out)
    assert got == [("res", 0), ("res", 1), ("rerun", 2), ("rerun", 3), ("res", 4)] and reruns(log) == [[2, 3]]
    # every release on the clean path is followed by the status check before anything else happens
    for i, e in enumerate(log):
        if e[0] == "release" and e[1] != 4:         # (the last one comes from flush(), which examines the status itself)
            assert log[i + 1] == ("status",)


def test_an_item_the_pipeline_cannot_take_drains_first_then_takes_the_fallback(monkeypatch):
    log_ref = []
    one = FakePipe(log_ref)
    got = list(dc_stream([0, 1, "odd", 3], lambda item, pipe: None if item == "odd" else one, lambda p, item: p.push(item),
                         lambda est, item: ("res", item),
                         lambda held, e: pytest.fail("no abort here"), lambda item: log_ref.append(("fallback", item)) or ("fallback", item),
                         "by the fake"))
    assert got == [("res", 0), ("res", 1), ("fallback", "odd"), ("res", 3)]
    assert log_ref == [("push", 0), ("push", 1), ("flush", 1), ("fallback", "odd"), ("push", 3), ("flush", 3)]


def test_another_pipeline_drains_the_old_one_first(monkeypatch):
    """``fit`` answers with a new pipeline (a longer batch, another B): what the old one holds leaves through its flush()."""
    log = []
    a, b = FakePipe(log), FakePipe(log)
    got = list(dc_stream(range(4), lambda item, pipe: a if item < 2 else b, lambda p, item: p.push(item), lambda est, item: ("res", item),
                         lambda held, e: pytest.fail("no abort here"), lambda item: pytest.fail("no fallback here"), "by the fake"))
    assert got == [("res", k) for k in range(4)]
    assert log == [("push", 0), ("push", 1), ("flush", 1), ("push", 2), ("push", 3), ("flush", 3)]


def test_recovered_rises_by_one_per_recovery(monkeypatch):
    r0 = _core._XcdPolicy.recovered
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, log = run(monkeypatch, range(6), abort_push=[1, 4], abort_flush=True)
    assert sorted(k for _, k in got) == list(range(6)) and [k for _, k in got] == list(range(6))
    assert reruns(log) == [[0, 1], [3, 4], [5]] and _core._XcdPolicy.recovered == r0 + 3
