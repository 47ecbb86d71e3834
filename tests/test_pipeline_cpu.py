"""CPU: pipeline.EpochLoader, the one-ahead epoch iterator RirSynthLoader and RealMixLoader share, under a stub loader on device="cpu" -
plain Python ``host_batch`` and ``render`` that log their calls; neither the library nor a GPU is touched.  Order and sizes of an epoch,
the render of batch k + 1 before batch k is handed out, the error paths and the teardown of the producer thread.  (The real loaders' draws
are pinned by test_plan_reproduces_every_draw and test_mix_loader_plan_reproduces_the_dataset_and_instance_sequence.)"""
import threading

import numpy as np
import pytest


def _stub(dataset_sz, batch_size, fail_host=None, fail_render=None, signal_at=None, **kw):
    from sar_ssl_amd.pipeline import EpochLoader

    class Stub(EpochLoader):
        def __init__(self):
            super().__init__(dataset_sz, batch_size, "cpu", **kw)
            self.log, self.nhost, self.reached = [], 0, threading.Event()

        def plan_item(self, rs):
            return int(rs.randint(0, 1 << 30))

        def host_batch(self, plans):                          # (producer thread; list.append is atomic)
            k, self.nhost = self.nhost, self.nhost + 1
            if k == fail_host:
                raise KeyError("host_batch %d" % k)
            self.log.append(("host", k))
            if k == signal_at:
                self.reached.set()
            return {"k": k, "plans": plans}

        def render(self, h, item0=0):
            if h["k"] == fail_render:
                raise ZeroDivisionError("render %d" % h["k"])
            self.log.append(("render", h["k"], item0))
            return h

        def handout(self, h):
            return (h["k"], h["plans"]), []

    return Stub()


def _renders(ld):
    return [e[1:] for e in ld.log if e[0] == "render"]


@pytest.mark.parametrize("drop_last,sizes", [(False, [4, 4, 3]), (True, [4, 4])])
def test_batches_arrive_in_plan_order_with_the_ragged_last_batch(drop_last, sizes):
    ld = _stub(11, 4, drop_last=drop_last)
    assert ld.side is None and ld.device.type == "cpu"
    np.random.seed(5)
    want = list(ld.plan_batches())
    np.random.seed(5)
    got = list(ld)
    assert len(ld) == len(got) == len(sizes) and [len(p) for _, p in got] == sizes
    assert [k for k, _ in got] == list(range(len(sizes))) and [p for _, p in got] == want
    assert len({x for p in want for x in p}) == sum(sizes)                                   # one stream through the epoch, not one per batch
    assert len(_stub(12, 4)) == len(_stub(12, 4, drop_last=True)) == 3 and len(_stub(3, 4)) == 1 and len(_stub(3, 4, drop_last=True)) == 0
    assert list(_stub(3, 4, drop_last=True)) == []


def test_the_render_of_the_next_batch_is_enqueued_before_a_batch_is_handed_out():
    ld = _stub(19, 4)
    n = len(ld)
    assert n == 5
    for k, _ in ld:
        ahead = min(k + 1, n - 1)                              # exactly one ahead: batch k + 1 is rendered, batch k + 2 is not
        assert _renders(ld) == [(j, j * 4) for j in range(ahead + 1)], (k, ld.log)
    assert _renders(ld) == [(j, j * 4) for j in range(n)]


def test_a_host_batch_error_reaches_the_consumer_in_order_and_the_producer_ends():
    before = set(threading.enumerate())
    ld = _stub(24, 4, fail_host=2)
    got = []
    with pytest.raises(KeyError, match="host_batch 2"):
        for k, _ in ld:
            got.append(k)
    assert got in ([0], [0, 1])                               # after batch 0, before batch 2 (batch 1 was rendered, not handed out)
    assert ld.nhost == 3 and set(threading.enumerate()) == before


def test_a_render_error_leaves_no_thread():
    before = set(threading.enumerate())
    ld = _stub(400, 4, fail_render=1, prefetch=1)
    with pytest.raises(ZeroDivisionError, match="render 1"):
        list(ld)
    assert _renders(ld) == [(0, 0)] and ld.nhost < 100 and set(threading.enumerate()) == before


def test_close_with_the_producer_blocked_on_a_full_queue_joins_it():
    before = set(threading.enumerate())
    ld = _stub(400, 4, prefetch=1, signal_at=3)
    it = iter(ld)
    assert next(it)[0] == 0                                   # the consumer took batches 0 and 1; batch 2 fills the queue
    assert ld.reached.wait(10)                                # batch 3 is read: the producer's next step is a put on the full queue
    assert len(set(threading.enumerate()) - before) == 1
    it.close()
    assert set(threading.enumerate()) == before and ld.nhost < 100
    with pytest.raises(StopIteration):
        next(it)


def test_plan_batches_continues_numpys_global_state_and_leaves_it_alone():
    ld = _stub(11, 4)
    np.random.seed(7)
    state = np.random.get_state()
    a = list(ld.plan_batches())
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    assert list(ld.plan_batches()) == a
    rs = np.random.RandomState(7)                             # the stream is numpy's own, from where the global state stood
    assert a[0] == [int(rs.randint(0, 1 << 30)) for _ in range(4)]
    np.random.seed(8)
    assert list(ld.plan_batches()) != a
