"""lib.capturing: a graph capture runs with Python's cyclic garbage collector off.  A collection inside a capture runs the destructors of
dead cycles on whatever thread allocates next; the ROCm build's CUDAGraph destructor synchronises the device, which a capturing stream
forbids, and an error raised in a destructor aborts the process.  No GPU is needed to see the guard work: the capture itself is replaced
by a recording context manager."""
import contextlib
import gc
import threading

import pytest
import torch

from mtn_amd import lib


@pytest.fixture
def fake_graph(monkeypatch):
    seen = []

    @contextlib.contextmanager
    def graph(g, **kw):
        seen.append(("enter", g, kw, gc.isenabled()))
        yield
        seen.append(("exit", g, gc.isenabled()))

    monkeypatch.setattr(torch.cuda, "graph", graph)
    return seen


def test_collector_is_off_inside_and_back_on_after(fake_graph):
    assert gc.isenabled()
    with lib.capturing("g", pool="p", capture_error_mode="thread_local"):
        assert not gc.isenabled()
    assert gc.isenabled()
    assert fake_graph == [("enter", "g", dict(pool="p", capture_error_mode="thread_local"), False), ("exit", "g", False)]


def test_collector_comes_back_after_an_error_and_stays_off_if_it_was(fake_graph):
    with pytest.raises(RuntimeError):
        with lib.capturing("g"):
            raise RuntimeError("a capture that fails")
    assert gc.isenabled()
    gc.disable()
    try:
        with lib.capturing("g"):
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_the_last_open_capture_switches_the_collector_back_on(fake_graph):
    """Nested, and in two threads at once: the collector stays off until the last capture has ended."""
    with lib.capturing("outer"):
        with lib.capturing("inner"):
            assert not gc.isenabled()
        assert not gc.isenabled()
    assert gc.isenabled()
    inside, release, states = threading.Event(), threading.Event(), []

    def other():
        with lib.capturing("other"):
            inside.set()
            release.wait(10)
        states.append(gc.isenabled())

    t = threading.Thread(target=other)
    with lib.capturing("main"):
        t.start()
        assert inside.wait(10)
    states.append(gc.isenabled())                                    # this thread's capture is over, the other's is not
    release.set()
    t.join(10)
    assert states == [False, True] and gc.isenabled()
