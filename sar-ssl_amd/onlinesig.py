"""Online simulated pretraining: every training batch is drawn, rendered and packed on the GPU while the previous step runs.

``run_pretrain.py --pretrain --simu-exp`` reads a corpus that ``gen_simu.py --mode sig`` wrote first (512 000 items, 134 GB, the same rooms
in every epoch).  ``--simu-online`` replaces the training loader by ``OnlineSignalLoader``: the generator's own stages (roomsim:
``render_items``, ``judge_on_device``, the retry of rejected items, rirsynth.mix_simulated, hip.pcm16_pack - one loop, ``roomsim._generate``
with ``roomsim._signal_sink``) run chunk by chunk on a worker thread under a side stream and hand int16 (B, Ns, nch) device batches to a
bounded queue - what dataset.PcmSegmentLoader yields and Learner.pretrain_epoch takes.  Nothing is written to disk and no room repeats.

Two things make the host keep up: the source corpus lives on the device and is cropped there (rirsynth.DeviceSourceBank, hip.src_gather),
and the room draw solves Sabine's equation in closed form instead of calling a numerical optimiser (roomsim.random_room's
beta_solver="closed").

AN ITEM IS A PURE FUNCTION OF ITS GLOBAL INDEX g = epoch dataset_sz + (step world + rank) B + j - not of the batch size, the chunk, the
rank layout or what was rendered before:

* room stream    RandomState([ROOM_TAG, seed, g // reuse]): random_spatial_acoustics' draws (``room_cfg``),
* signal stream  RandomState([SIG_TAG, seed, g]): speaker index, DeviceSourceBank.plan (utterance, crop start), SNR - rirsynth.draw_item's
                 order without its white draw (``item_plan``),
* white noise    noise="device": sarssl_gauss_fill keyed by (seed, g); "numpy": RandomState([WHITE_TAG, seed, g]), uploaded,
* RIR tail       keyed by (seed, g // reuse, attempt), on the device or with noise="numpy" roomsim.numpy_noise.

The array seeds keep every online stream apart from the disk stages' ``seed + idx``.  With reuse = K > 1 a rendered RIR / direct-path pair
serves the K consecutive items of its room, which differ in source, noise and SNR: the image-source render is the dearest stage.
"""
import queue
import sys
import threading

import numpy as np

from . import roomsim

ROOM_TAG, SIG_TAG, WHITE_TAG = 0x6f6e726d, 0x6f6e7367, 0x6f6e7768          # first word of the streams' array seeds
CHUNK = 1024


class OnlineSignalLoader:
    """``for [pcm] in loader``: pcm int16 (B, Ns, nch) on ``device``, B accepted items each (the last batch of an epoch is ragged where
    dataset_sz is no multiple of batch_size; with world > 1 an epoch is the full batches every rank can take in equal number, as the disk
    loader's drop_last).  bank: a rirsynth.DeviceSourceBank on ``device``.  chunk: items rendered per ``roomsim._generate`` run (rounded
    to whole batches); render_batch: rooms per render / judge round inside it.  ranges: roomsim.DEFAULTS' keys.
    An item that fails the accept test MAX_ATTEMPTS times is logged and replaced by the next accepted item of its chunk.
    ``attempts`` records the renders every room took (the accepted attempt's tail noise is what a restatement needs)."""

    def __init__(self, bank, dataset_sz, batch_size, T, seed, device, reuse=1, noise="device", rank=0, world=1, mic_array_cfg=None,
                 snr_range=(15, 30), chunk=CHUNK, render_batch=128, log=None, **ranges):
        import torch
        self.args = roomsim._generator_args(ranges, noise)
        self.fs = self.args["fs"]
        self.nsample = roomsim.sig_samples(T, self.fs)
        self.bank, self.dataset_sz, self.batch_size, self.T = bank, int(dataset_sz), int(batch_size), T
        self.seed, self.reuse, self.noise, self.rank, self.world = int(seed), int(reuse), noise, int(rank), int(world)
        if self.reuse < 1 or self.batch_size % self.reuse != 0:
            raise ValueError("reuse = %d does not divide the batch size %d: the items of a room share one batch" % (self.reuse, self.batch_size))
        if self.dataset_sz < 1 or self.batch_size < 1 or not 0 <= self.rank < self.world:
            raise ValueError("dataset_sz %d, batch_size %d, rank %d of %d" % (self.dataset_sz, self.batch_size, self.rank, self.world))
        if bank.fs != self.fs:
            raise ValueError("the source bank is sampled at %d Hz, fs = %d" % (bank.fs, self.fs))
        self.mic_array_cfg = roomsim.MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
        self.nmic = self.mic_array_cfg["mic_pos_relative"].shape[0]
        self.snr_range = tuple(snr_range)
        self.device = torch.device(device)
        self.side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.steps_per_chunk = max(1, int(chunk) // self.batch_size)
        self.render_batch, self.log = max(1, int(render_batch)), log or (lambda s: print(s, file=sys.stderr, flush=True))
        self.lmax = roomsim.sig_lmax(self.args["T60_range"], self.fs)
        self.epoch, self.attempts, self._tls = 0, {}, threading.local()

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        if self.world > 1:
            return (self.dataset_sz // self.batch_size) // self.world
        return (self.dataset_sz + self.batch_size - 1) // self.batch_size

    # ------------------------------------------------------------------------------------------------------------ host: pure functions of g
    def indices(self, epoch, step):
        """The global indices of this rank's batch ``step`` of ``epoch``."""
        first = (step * self.world + self.rank) * self.batch_size
        g0 = epoch * self.dataset_sz + first
        assert 0 <= first < self.dataset_sz and g0 + self.batch_size < (1 << 31)
        return list(range(g0, g0 + min(self.batch_size, self.dataset_sz - first)))

    def _stream(self, tag, k):
        """RandomState([tag, seed, k]): this thread's one generator, seeded again (constructing one gathers OS entropy first, 50 us)."""
        rs = getattr(self._tls, "rs", None)
        if rs is None:
            rs = self._tls.rs = np.random.RandomState(0)
        rs.seed([tag, self.seed & 0xffffffff, int(k)])
        return rs

    def room_cfg(self, room):
        """The configuration of room ``room`` = g // reuse: random_spatial_acoustics' draws with the closed-form Sabine solve."""
        rs = self._stream(ROOM_TAG, room)
        draw = {k: self.args[k] for k in roomsim.DEFAULTS if k != "fs"}
        return roomsim.random_spatial_acoustics(rs, 0, 0, mic_array_cfg=self.mic_array_cfg, beta_solver="closed", reseed=False, **draw)

    def item_cfg(self, g):
        return self.room_cfg(int(g) // self.reuse)

    def item_plan(self, g):
        """The signal plan of item g: DeviceSourceBank.plan's record with src_idx, snr, idx and (noise="numpy") white (Ns, nmic) f64."""
        g = int(g)
        rs = self._stream(SIG_TAG, g)
        src_idx = int(rs.randint(0, len(self.bank)))
        rec = self.bank.plan(rs, src_idx, self.nsample)
        snr = float(rs.uniform(*self.snr_range))
        white = None
        if self.noise == "numpy":
            white = self._stream(WHITE_TAG, g).standard_normal((self.nsample, self.nmic))
        return dict(rec, src_idx=src_idx, snr=snr, idx=g, white=white)

    def restate_plan(self, g):
        """What roomsim.restate_sig takes for item g: ``item_plan`` with the configuration and the source crop (f64, gathered in numpy)."""
        p = self.item_plan(g)
        return dict(p, cfg=self.item_cfg(g), src=self.bank.host_crop(p, self.nsample))

    # ------------------------------------------------------------------------------------------------------------ device: one chunk
    def render_chunk(self, G):
        """Render the items ``G`` (global indices, a room's items adjacent) on the current stream -> int16 (len(G), Ns, nmic) on the device,
        row k item G[k].  Blocks on the judge's small read-backs; the result is complete once the stream reaches this point."""
        import torch
        dev, K, ns = self.device, self.reuse, self.nsample
        by_room, pos = {}, {g: k for k, g in enumerate(G)}
        for g in G:
            by_room.setdefault(g // K, []).append(g)
        rooms = list(by_room)
        at = {r: k for k, r in enumerate(rooms)}

        class Rooms(dict):                                   # a room is drawn when the loop first asks for it
            def __missing__(cfgs, r):
                cfgs[r] = self.room_cfg(r)
                return cfgs[r]
        cfgs = Rooms()
        buf = torch.empty((len(G), ns, self.nmic), dtype=torch.int16, device=dev)
        done = set()

        def emit(pcm, aids, rows, lab, plans):
            buf.index_copy_(0, torch.tensor([pos[g] for g in aids], device=dev), pcm)
            done.update(aids)

        prepare, sink = roomsim._signal_sink(cfgs, self.seed, self.args, dev, self.noise, self.T, self.nmic, self.item_plan, emit,
                                             load=lambda plans: self.bank.gather(plans, ns), items=by_room.__getitem__, table="device")

        def prepare_ahead(ids):                              # (host work while the GPU renders: this batch's plans, the next one's rooms)
            prepare(ids)
            k = at[ids[0]] + self.render_batch
            for r in rooms[k:k + self.render_batch]:
                cfgs[r]

        res = roomsim._generate("OnlineSignalLoader", None, "online", cfgs, self.seed, self.args, dev, self.noise, self.render_batch, "device",
                                sink, self.log, prepare_ahead, self.lmax, ids=rooms)
        self.attempts.update(res["attempts"])
        if len(done) < len(G):
            if not done:
                raise RuntimeError("OnlineSignalLoader: no item of a chunk of %d passed the accept test" % len(G))
            for k, g in enumerate(G):
                if g not in done:
                    other = next(G[(k + d) % len(G)] for d in range(1, len(G)) if G[(k + d) % len(G)] in done)
                    self.log("OnlineSignalLoader: item %d is replaced by item %d" % (g, other))
                    buf[k].copy_(buf[pos[other]])
        return buf

    def __iter__(self):
        import torch
        if self.side is None:
            raise RuntimeError("OnlineSignalLoader renders on the GPU only (device %s); there is no CPU fallback" % self.device)
        epoch, steps, spc = self.epoch, len(self), self.steps_per_chunk
        ready = queue.Queue(maxsize=spc)                     # one chunk is handed out while the next one renders
        stop = threading.Event()

        def worker():
            try:
                torch.cuda.set_device(self.device)
                with torch.cuda.stream(self.side):
                    for s0 in range(0, steps, spc):
                        groups = [self.indices(epoch, s) for s in range(s0, min(steps, s0 + spc))]
                        buf = self.render_chunk([g for grp in groups for g in grp])
                        a = 0
                        for grp in groups:
                            if stop.is_set():
                                return
                            ev = torch.cuda.Event()
                            ev.record(self.side)
                            ready.put((buf[a:a + len(grp)], ev))
                            a += len(grp)
                ready.put(None)
            except BaseException as e:                       # surface render errors in the consumer
                ready.put(e)

        th = threading.Thread(target=worker, daemon=True)
        th.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                pcm, ev = item
                st = torch.cuda.current_stream(self.device)
                st.wait_event(ev)                            # (the training stream waits on the device; the host never does)
                pcm.record_stream(st)
                yield [pcm]
        finally:
            stop.set()
            while th.is_alive():                             # a worker blocked on the full queue sees ``stop`` once it is drained
                try:
                    ready.get(timeout=0.05)
                except queue.Empty:
                    pass
            th.join()
