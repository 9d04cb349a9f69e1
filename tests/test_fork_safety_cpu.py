"""Finalisers that call the HIP runtime run only in the process that owns the object: a forked DataLoader worker inherits copies of the
trainer's garbage, and collecting it there must not reach the runtime."""
import gc
import os

from kurosiwo_amd import distributed as D
from kurosiwo_amd import launch


class _Lib:
    def __init__(self):
        self.destroyed = []

    def ksmi_runner_destroy(self, r):
        self.destroyed.append(r)
        return 0


def _streams(monkeypatch, pid):
    lib = _Lib()
    monkeypatch.setattr(launch._lib, "load", lambda: lib)
    s = object.__new__(launch.StepStreams)
    s._runner, s._runner_pid = 1234, pid
    return s, lib


def test_runner_is_destroyed_by_its_own_process(monkeypatch):
    s, lib = _streams(monkeypatch, os.getpid())
    del s
    gc.collect()
    assert lib.destroyed == [1234]


def test_runner_is_left_alone_in_a_forked_child(monkeypatch):
    s, lib = _streams(monkeypatch, os.getpid() + 1)         # as seen from a child: created under another pid
    del s
    gc.collect()
    assert lib.destroyed == []


def test_before_fork_collects_garbage_only_for_loaders_with_workers(monkeypatch):
    calls = []
    monkeypatch.setattr(D.gc, "collect", lambda: calls.append(1))

    class L:
        num_workers = 0
    ld = L()
    assert D.before_fork(ld) is ld and not calls
    ld.num_workers = 2
    assert D.before_fork(ld) is ld and calls == [1]
    assert D.before_fork([1, 2]) == [1, 2] and calls == [1]
