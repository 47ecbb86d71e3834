"""The concurrency the data pipelines share: the one-ahead epoch iterator of the GPU-rendering loaders (rirsynth.RirSynthLoader,
realsig.RealMixLoader) and the double-buffered PCM writer of the generators (roomsim._signals, realsig.generate).  Planning, rendering
and what a job writes stay with the callers.  dataset.PcmSegmentLoader uploads from its producer thread and keeps its own iterator;
onlinesig.OnlineSignalLoader renders whole chunks on its worker thread (the judge's read-back blocks there) and keeps its own too.
"""
import queue
import threading

import numpy as np


class EpochLoader:
    """An epoch of ``dataset_sz`` items in batches of ``batch_size``, rendered on ``device`` one batch ahead of the one handed out.
    A loader supplies

    * ``plan_item(rs)``: the host draws of one item on the epoch's RandomState,
    * ``host_batch(plans)``: the (pinned) host tensors of a batch - it runs on the producer thread,
    * ``render(h, item0=0)``: the enqueue of a host batch on the current stream; item0 is the running index of the batch's first item,
    * ``handout(res) -> (what the iterator yields for render's result, the device tensors in it)``.

    On a CUDA device the renders run on ``side`` and every tensor handed out is recorded on the consumer's stream; on a CPU device
    (``side is None``) the render runs inline and no event is made."""

    def __init__(self, dataset_sz, batch_size, device, drop_last=False, prefetch=2):
        import torch
        self.dataset_sz, self.batch_size, self.drop_last, self.prefetch = int(dataset_sz), int(batch_size), drop_last, max(1, prefetch)
        self.device = torch.device(device)
        self.side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

    def __len__(self):
        n = self.dataset_sz // self.batch_size
        return n if self.drop_last or self.dataset_sz % self.batch_size == 0 else n + 1

    def plan_batches(self):
        """Generator of the epoch's plans, batch by batch (host only): one host stream, continued from numpy's global state where the
        iteration starts (the reference's order with num_workers=0, after the epoch's set_random_seed); the global state is left alone."""
        rs = np.random.RandomState()
        rs.set_state(np.random.get_state())
        left = self.dataset_sz
        for _ in range(len(self)):
            n = min(self.batch_size, left)
            left -= n
            yield [self.plan_item(rs) for _ in range(n)]

    def __iter__(self):
        import torch
        ready = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def producer():
            try:
                for plans in self.plan_batches():
                    if stop.is_set():
                        return
                    ready.put(self.host_batch(plans))
                ready.put(None)
            except BaseException as e:                       # surface planning / reader errors in the consumer
                ready.put(e)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            prev, i = None, 0
            while True:
                h = ready.get()
                if isinstance(h, BaseException):
                    raise h
                cur = None
                if h is not None:
                    ev = None
                    if self.side is not None:
                        with torch.cuda.stream(self.side):
                            res = self.render(h, item0=i * self.batch_size)
                            ev = torch.cuda.Event()
                            ev.record(self.side)
                    else:
                        res = self.render(h, item0=i * self.batch_size)
                    cur = (res, ev, h)                        # (h: the pinned buffers live until the batch is handed out)
                    i += 1
                if prev is not None:
                    item, tensors = self.handout(prev[0])
                    if prev[1] is not None:
                        st = torch.cuda.current_stream(self.device)
                        st.wait_event(prev[1])
                        for t in tensors:
                            t.record_stream(st)
                    yield item
                prev = cur
                if h is None:
                    break
        finally:
            stop.set()
            while th.is_alive():                             # a producer blocked on the full queue sees ``stop`` once it is drained
                try:
                    ready.get(timeout=0.05)
                except queue.Empty:
                    pass
            th.join()


def src_snr_rows(plans, ns, ntab=0):
    """The pinned row block a generator uploads for its mix -> (len(plans), ns + 1 + ntab) f32: ``src | snr`` of each plan and, with ntab,
    its mixing table ``C`` flattened behind them.  Filled through the numpy view (no torch op runs on the host)."""
    import torch
    host = torch.empty((len(plans), ns + 1 + ntab), dtype=torch.float32, pin_memory=True)
    hn = host.numpy()
    for j, p in enumerate(plans):
        hn[j, :ns], hn[j, ns] = p["src"], p["snr"]
        if ntab:
            hn[j, ns + 1:] = p["C"].reshape(-1)
    return host


class StagedWriter:
    """``with StagedWriter(rows, ns, nch) as w``: two pinned int16 buffers (rows, ns, nch) and one writer thread.  ``w.stage(pcm, job,
    *args)`` copies a packed (n <= rows, ns, nch) int16 device tensor into the dense prefix of the next buffer - after the job that last
    read that buffer is done -, records an event on pcm's current stream and queues ``job(staged, *args)`` behind ``ev.synchronize()``, so
    the files of one batch are written while the next renders.  Leaving the block waits for both buffers and re-raises a job's exception."""

    def __init__(self, rows, ns, nch):
        import torch
        from concurrent.futures import ThreadPoolExecutor
        self.pinned = [torch.empty((rows, ns, nch), dtype=torch.int16, pin_memory=True) for _ in range(2)]
        self.busy, self.staged = [None, None], 0              # the job that still reads each buffer; batches staged so far
        self.thread = ThreadPoolExecutor(max_workers=1)

    def __enter__(self):
        return self

    def stage(self, pcm, job, *args):
        import torch
        k = self.staged % 2
        self.staged += 1
        if self.busy[k] is not None:
            self.busy[k].result()                             # the buffer's previous batch is on disk
        staged = self.pinned[k][:pcm.shape[0]]
        staged.copy_(pcm, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(pcm.device))

        def run():
            ev.synchronize()
            job(staged, *args)
        self.busy[k] = self.thread.submit(run)

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                for f in self.busy:
                    if f is not None:
                        f.result()
        finally:
            self.thread.shutdown(wait=True)
        return False
