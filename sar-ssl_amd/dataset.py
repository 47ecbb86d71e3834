"""``FixMicSigDataset`` (code/dataset.py:107-178) for pre-generated simulated microphone signals: ``{idx}.wav`` files
(16 kHz, nch channels, 16-bit PCM as written by code/data_generation/utils_simu_rir_sig.py:855-856), minus ``*_dp.wav``.

``soundfile`` is not available here, so RIFF/WAVE PCM-16 is parsed directly with numpy.  ``raw_pcm=True`` returns the
int16 samples untouched (half the PCIe bytes); the STFT kernel converts on the fly.
"""
import ctypes
import queue
import struct
import threading
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

from .pipeline import EpochLoader


def read_wav_pcm16(path):
    """-> (int16 array (nsample, nch), fs).  Supports plain PCM-16 and WAVE_FORMAT_EXTENSIBLE PCM-16."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file" % path)
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            tag, nch, fs, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and len(body) >= 26:
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, nch, fs, bits)
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError("%s: missing fmt/data chunk" % path)
    tag, nch, fs, bits = fmt
    if tag != 1 or bits != 16:
        raise ValueError("%s: only 16-bit PCM is supported (format tag %d, %d bits)" % (path, tag, bits))
    x = np.frombuffer(pcm, dtype="<i2")
    return x[: (x.size // nch) * nch].reshape(-1, nch), fs


_WAV_TAGS = {1: "PCM", 3: "IEEE float"}


def read_wav(path, raw_pcm16=False):
    """-> (float64 array (nsample, nch), fs) of a measured corpus's file, what soundfile.read returns: PCM-16 / 24 / 32 scaled by
    2^-(bits-1) as libsndfile's float read does, IEEE float-32 widened; plain or WAVE_FORMAT_EXTENSIBLE.  raw_pcm16: a PCM-16 file
    comes back as its int16 samples (half the upload; the kernels scale by 1 / 32768 themselves).  Any other format tag or width is
    refused by name."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file" % path)
    pos, fmt, raw = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            if len(body) < 16:
                raise ValueError("%s: fmt chunk of %d bytes, 16 at least" % (path, len(body)))
            tag, nch, fs, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and len(body) >= 26:
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, nch, fs, bits)
        elif cid == b"data":
            raw = body
        pos += 8 + size + (size & 1)
    if fmt is None or raw is None:
        raise ValueError("%s: missing fmt/data chunk" % path)
    tag, nch, fs, bits = fmt
    if (tag, bits) not in ((1, 16), (1, 24), (1, 32), (3, 32)):
        names = {6: "A-law", 7: "mu-law", 2: "MS ADPCM", 17: "IMA ADPCM", 0x55: "MPEG layer 3"}
        raise ValueError("%s: %s, %d bits (format tag 0x%04x) is not read: PCM-16 / 24 / 32 and IEEE float-32 are"
                         % (path, _WAV_TAGS.get(tag) or names.get(tag, "unknown format"), bits, tag))
    nframe = len(raw) // (nch * (bits // 8))
    raw = raw[:nframe * nch * (bits // 8)]
    if tag == 3:
        x = np.frombuffer(raw, dtype="<f4").astype(np.float64)
    elif bits == 16:
        x = np.frombuffer(raw, dtype="<i2")
        x = x if raw_pcm16 else x.astype(np.float64) / 32768.0
    elif bits == 32:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0
    else:
        b = np.zeros((len(raw) // 3, 4), np.uint8)                # the three bytes as the upper ones of an int32: sample * 256, sign kept
        b[:, 1:] = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3)
        x = b.view("<i4")[:, 0].astype(np.float64) / 2147483648.0
    return x.reshape(-1, nch), fs


def write_wav_pcm16(path, pcm, fs=16000):
    """pcm: int16 (nsample, nch)."""
    pcm = np.ascontiguousarray(pcm.astype("<i2"))
    nch = pcm.shape[1]
    body = pcm.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, nch, fs, fs * nch * 2, nch * 2, 16)
    with open(path, "wb") as f:
        f.write(hdr + b"data" + struct.pack("<I", len(body)) + body)


class Selecting(object):
    """Keep samples [select_range[0], select_range[1]) of a (nsample, nch) signal (code/dataset.py:386-395)."""

    def __init__(self, select_range):
        self.select_range = select_range

    def __call__(self, mic_sig):
        nsample = mic_sig.shape[0]
        assert self.select_range[-1] <= nsample, f"Selecting range ({self.select_range[-1]}) is larger than signal length ({nsample})~"
        return mic_sig[self.select_range[0]:self.select_range[1], ...]


TASKS = ("TDOA", "T60", "DRR", "C50", "ABS")


def simulated_annos(info):
    """The labels FixMicSigDataset forms from a simulated segment's ``_info.npz`` (code/dataset.py:153-170); ABS by Sabine's formula."""
    vol = info["room_sz"][0] * info["room_sz"][1] * info["room_sz"][2]
    sur = info["room_sz"][0] * info["room_sz"][1] + info["room_sz"][0] * info["room_sz"][2] + info["room_sz"][1] * info["room_sz"][2]
    return {"TDOA": info["TDOA"].astype(np.float32), "T60": info["T60_edc"].astype(np.float32),
            "DRR": info["DRR"].astype(np.float32), "C50": info["C50"].astype(np.float32),
            "ABS": np.array(0.161 * vol / sur / info["T60_edc"]).astype(np.float32)}


def locata_annos(info):
    """The labels of a LOCATA segment (code/dataset.py:221-227): its TDOA, NaN for the room-acoustics tasks."""
    return {"TDOA": info["TDOA"].astype(np.float32), "T60": np.array(np.nan), "DRR": np.array(np.nan), "C50": np.array(np.nan),
            "ABS": np.array(np.nan)}


class FixMicSigDataset(Dataset):
    def __init__(self, data_dir, fs, load_anno, dataset_sz, load_dp=False, transforms=None, raw_pcm=False):
        dirs = data_dir if isinstance(data_dir, list) else [data_dir]
        files, dp_files = [], []
        for d in dirs:
            files += list(Path(d).rglob("*.wav"))
            dp_files += list(Path(d).rglob("*_dp.wav"))
        if isinstance(data_dir, list):
            np.random.shuffle(files)
        dp = set(dp_files)
        self.files = [f for f in files if f not in dp]
        self.dataset_sz = len(self.files) if dataset_sz is None else int(np.min([len(self.files), dataset_sz]))
        self.fs, self.load_anno, self.load_dp, self.transforms, self.raw_pcm = fs, load_anno, load_dp, transforms, raw_pcm

    def __len__(self):
        return self.dataset_sz

    def __getitem__(self, idx):
        file_name = str(self.files[idx])
        pcm, fs = read_wav_pcm16(file_name)
        if self.fs != fs:
            import scipy.signal
            mic_sig = scipy.signal.resample_poly(pcm.astype(np.float64) / 32768.0, self.fs, fs)
        elif self.raw_pcm and self.transforms is None:
            return [np.ascontiguousarray(pcm)]
        else:
            mic_sig = pcm.astype(np.float32) / 32768.0            # soundfile's float conversion of PCM-16
        if self.transforms is not None:
            for t in self.transforms:
                mic_sig = t(mic_sig)
        return_data = [mic_sig.astype(np.float32)]
        if self.load_anno:
            return_data += [simulated_annos(dict(np.load(file_name.replace(".wav", "_info.npz"))))]
        if self.load_dp:
            dp, fs_dp = read_wav_pcm16(file_name.replace(".wav", "_dp.wav"))
            dp_sig = dp.astype(np.float32) / 32768.0
            if self.fs != fs_dp:
                import scipy.signal
                dp_sig = scipy.signal.resample_poly(dp_sig, self.fs, fs_dp)
            if self.transforms is not None:
                for t in self.transforms:
                    dp_sig = t(dp_sig)
            return_data += [dp_sig]
        return return_data


def read_wav_batch(paths, nsample, nch, fs=0, offset=0, out=None, nthreads=0):
    """Raw int16 PCM of samples [offset, offset+nsample) of every file -> int16 tensor (len(paths), nsample, nch), filled by the
    threaded reader of the C-ABI library (csrc/wavio.hip, ``sarssl_wav_read_batch``; the GIL is released during the call)."""
    from . import _lib
    n = len(paths)
    if out is None:
        out = torch.empty((n, nsample, nch), dtype=torch.int16)
    assert out.dtype == torch.int16 and out.is_contiguous() and not out.is_cuda and out.numel() >= n * nsample * nch
    arr = (ctypes.c_char_p * n)(*[str(p).encode() for p in paths])
    _lib.call("sarssl_wav_read_batch", arr, ctypes.c_int(n), ctypes.c_long(nsample), ctypes.c_int(nch), ctypes.c_int(fs),
              ctypes.c_long(offset), ctypes.c_void_p(out.data_ptr()), ctypes.c_int(nthreads))
    return out[:n] if out.shape[0] != n else out


def write_wav_batch(paths, pcm, fs=16000, nthreads=0):
    """pcm: int16 host tensor or array (len(paths), nsample, nch) -> one 44-byte-header PCM-16 file per path, byte for byte what
    ``write_wav_pcm16`` writes, by the threaded writer of the C-ABI library (csrc/wavio.hip, ``sarssl_wav_write_batch``; the GIL is
    released during the call).  Files appear under their names only when complete (written as ``<path>.tmp``, then renamed)."""
    from . import _lib
    if isinstance(pcm, np.ndarray):
        pcm = torch.from_numpy(np.ascontiguousarray(pcm))
    n = len(paths)
    assert pcm.dtype == torch.int16 and pcm.is_contiguous() and not pcm.is_cuda and pcm.dim() == 3 and pcm.shape[0] >= n
    arr = (ctypes.c_char_p * n)(*[str(p).encode() for p in paths])
    _lib.call("sarssl_wav_write_batch", arr, ctypes.c_int(n), ctypes.c_long(pcm.shape[1]), ctypes.c_int(pcm.shape[2]), ctypes.c_int(fs),
              ctypes.c_void_p(pcm.data_ptr()), ctypes.c_int(nthreads))


def wav_probe(path):
    """-> (nch, fs, nsample) of a PCM-16 WAV file."""
    from . import _lib
    nch, fs, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    _lib.call("sarssl_wav_probe", str(path).encode(), ctypes.byref(nch), ctypes.byref(fs), ctypes.byref(ns))
    return nch.value, fs.value, ns.value


class PcmSegmentLoader:
    """Batch iterator over a FixMicSigDataset-style directory of equal-length PCM-16 segments that replaces
    ``DataLoader(FixMicSigDataset(...), num_workers=N)`` on the pretraining path (code/run_pretrain.py:160-186): a background
    thread fills (pinned) int16 batch buffers with the native reader and, when ``device`` is a GPU, uploads them on a copy stream
    while the previous step computes.  Yields ``[pcm]`` with pcm int16 (B, nsample, nch) - the STFT kernel converts on the fly.
    Without a device the yielded host tensor is a view of a recycled buffer: valid until the next batch is requested.

    shuffle / rank / world / seed reproduce ``DistributedSampler`` semantics (rank-strided slice of one global permutation per
    epoch, padded by wrap-around); ``set_epoch`` changes the permutation."""

    def __init__(self, files, batch_size, nsample=None, nch=None, fs=16000, shuffle=False, seed=0, rank=0, world=1, drop_last=False,
                 device=None, nthreads=8, prefetch=2):
        self.files = [str(f) for f in files]
        assert self.files, "no segments"
        if nsample is None or nch is None:
            c, _, ns = wav_probe(self.files[0])
            nch, nsample = nch or c, nsample or ns
        self.batch_size, self.nsample, self.nch, self.fs = int(batch_size), int(nsample), int(nch), fs
        self.shuffle, self.seed, self.rank, self.world, self.drop_last = shuffle, seed, rank, world, drop_last
        self.device = torch.device(device) if device is not None else None
        self.nthreads, self.prefetch, self.epoch = nthreads, max(1, prefetch), 0
        self.per_rank = (len(self.files) + world - 1) // world

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.per_rank // self.batch_size if self.drop_last else (self.per_rank + self.batch_size - 1) // self.batch_size

    def _order_all(self, epoch):
        n = len(self.files)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + epoch)
            idx = torch.randperm(n, generator=g).tolist()
        else:
            idx = list(range(n))
        total = self.per_rank * self.world
        return idx + idx[: total - n]

    def _order_for(self, epoch):
        return self._order_all(epoch)[self.rank::self.world]

    def _order(self):
        return self._order_for(self.epoch)

    def __iter__(self):
        order = self._order()
        nb = len(self)
        cuda = self.device is not None and self.device.type == "cuda"
        pin = cuda and torch.cuda.is_available()
        bufs = [torch.empty((self.batch_size, self.nsample, self.nch), dtype=torch.int16, pin_memory=pin) for _ in range(self.prefetch + 1)]
        free, ready = queue.Queue(), queue.Queue(maxsize=self.prefetch)
        for b in bufs:
            free.put(b)
        copy_stream = torch.cuda.Stream(self.device) if cuda else None
        stop = threading.Event()

        def producer():
            try:
                for i in range(nb):
                    if stop.is_set():
                        return
                    ids = order[i * self.batch_size:(i + 1) * self.batch_size]
                    buf = free.get()
                    host = read_wav_batch([self.files[j] for j in ids], self.nsample, self.nch, self.fs, 0, out=buf, nthreads=self.nthreads)
                    if cuda:
                        with torch.cuda.stream(copy_stream):
                            dev = host.to(self.device, non_blocking=True)
                            ev = torch.cuda.Event()
                            ev.record(copy_stream)
                        ready.put((dev, ev, buf))
                    else:
                        ready.put((host, None, buf))                            # valid until the consumer asks for the next batch
                ready.put(None)
            except BaseException as e:                                              # surface reader errors in the consumer
                ready.put(e)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                t, ev, buf = item
                if ev is not None:
                    torch.cuda.current_stream(self.device).wait_event(ev)
                    ev.synchronize()                                                 # the pinned buffer is reusable once the copy is done
                    t.record_stream(torch.cuda.current_stream(self.device))
                    free.put(buf)
                    yield [t]
                else:
                    yield [t]
                    free.put(buf)
        finally:
            stop.set()
            while th.is_alive():
                try:
                    ready.get(timeout=0.05)
                except queue.Empty:
                    pass
                free.put(bufs[0])
            th.join()


def segment_files(data_dir):
    """The ``*.wav`` files FixMicSigDataset would list (code/dataset.py:113-126): recursive, minus ``*_dp.wav``."""
    dirs = data_dir if isinstance(data_dir, list) else [data_dir]
    files, dp = [], set()
    for d in dirs:
        files += list(Path(d).rglob("*.wav"))
        dp |= set(Path(d).rglob("*_dp.wav"))
    return [f for f in files if f not in dp]


# ---------------------------------------------------------------------------------------------------------------- LOCATA TDOA corpus
class FixMicSigDatasetLOCATA(Dataset):
    """FixMicSigDatasetLOCATA (code/dataset.py:180-230): the ``{idx}.wav`` segments gen_LOCATA.py wrote (16 kHz PCM-16) with their
    ``{idx}_info.npz`` - TDOA, and NaN for T60 / DRR / C50 / ABS.  The files are at ``fs`` already: one at another rate raises (the
    reference would resample it per item)."""

    def __init__(self, data_dir, fs, load_anno, dataset_sz, transforms=None):
        if isinstance(data_dir, list):
            self.files = []
            for d in data_dir:
                self.files += list(Path(d).rglob("*.wav"))
            np.random.shuffle(self.files)
        else:
            self.files = list(Path(data_dir).rglob("*.wav"))
        self.dataset_sz = len(self.files) if dataset_sz is None else int(np.min([len(self.files), dataset_sz]))
        self.fs, self.load_anno, self.transforms = fs, load_anno, transforms

    def __len__(self):
        return self.dataset_sz

    def __getitem__(self, idx):
        file_name = str(self.files[idx])
        pcm, fs = read_wav_pcm16(file_name)
        if self.fs != fs:
            raise ValueError("%s: sampled at %d Hz, the LOCATA TDOA corpus is read at %d Hz and not resampled (gen_LOCATA.py writes %d Hz)"
                             % (file_name, fs, self.fs, self.fs))
        mic_sig = pcm.astype(np.float32) / 32768.0
        if self.transforms is not None:
            for t in self.transforms:
                mic_sig = t(mic_sig)
        return_data = [mic_sig.astype(np.float32)]
        if self.load_anno:
            return_data += [locata_annos(dict(np.load(file_name.replace(".wav", "_info.npz"))))]
        return return_data


def _select_range(transforms, what):
    """(first sample, one past the last) of ``transforms`` for a batch reader, or None for the whole file: nothing or one ``Selecting``."""
    if not transforms:
        return None
    if len(transforms) != 1 or not isinstance(transforms[0], Selecting):
        raise ValueError("%s reads a batch straight into one buffer: its transforms are None or [Selecting(...)]" % what)
    a, b = transforms[0].select_range
    return int(a), int(b)


class RandomMicSigDataset(EpochLoader):
    """RandomMicSigDataset (code/dataset.py:232-285) as a batch loader: yields ``(mic_sig (B, Ns, 2) f32 on the device, {task: (B,) f32
    tensor})`` in the shape Learner.train_epoch / test_epoch iterate.  The reference's constructor arguments, then the loader's.

    Per item the host draws the dataset - ``randint(0, len(dataset_list))`` over [simulated, LOCATA] by ``real_sim_ratio`` - and the
    instance ``randint(0, len(dataset))`` on the epoch's one host stream (pipeline.EpochLoader.plan_batches: continued from numpy's
    global state, the reference's order with num_workers=0).  The producer thread reads the batch's PCM-16 through the native reader into
    ONE pinned buffer - Selecting's range only - and the labels from the ``_info.npz`` files; the consumer uploads and scales by
    1 / 32768 (exact; what soundfile's float read gives).  A file at another rate than ``fs`` raises."""

    def __init__(self, real_sig_dir, sim_sig_dir, real_sim_ratio, fs, stage, load_anno, dataset_sz, transforms=None, batch_size=16,
                 device="cuda", drop_last=False, prefetch=2, nthreads=4):
        import os
        super().__init__(dataset_sz, batch_size, device, drop_last, prefetch)
        realdataset = FixMicSigDatasetLOCATA(data_dir=os.path.join(real_sig_dir, stage), load_anno=load_anno, dataset_sz=None, fs=fs,
                                             transforms=transforms)
        simdataset = FixMicSigDataset(data_dir=sim_sig_dir, load_anno=load_anno, dataset_sz=None, fs=fs, transforms=transforms)
        real_sim_ratio = list(real_sim_ratio)
        assert real_sim_ratio in [[0, 1], [1, 0], [1, 1]], real_sim_ratio
        self.dataset_list = {(0, 1): [simdataset], (1, 0): [realdataset], (1, 1): [simdataset, realdataset]}[tuple(real_sim_ratio)]
        for d in self.dataset_list:
            if len(d) == 0:
                raise ValueError("RandomMicSigDataset: no segments below %s" % (sim_sig_dir if d is simdataset else os.path.join(real_sig_dir, stage),))
        self.fs, self.load_anno, self.nthreads = fs, load_anno, nthreads
        self.range = _select_range(transforms, "RandomMicSigDataset")
        if self.range is None:
            self.range = (0, wav_probe(str(self.dataset_list[0].files[0]))[2])

    def plan_item(self, rs):
        d = int(rs.randint(0, len(self.dataset_list)))
        dataset = self.dataset_list[d]
        idx = int(rs.randint(0, len(dataset)))
        return dict(dataset=d, idx=idx, path=str(dataset.files[idx]), real=isinstance(dataset, FixMicSigDatasetLOCATA))

    def handout(self, res):
        if not self.load_anno:
            return res, [res]
        return res, [res[0]] + list(res[1].values())

    def host_batch(self, plans):
        pin = self.device.type == "cuda"
        a, b = self.range
        buf = torch.empty((len(plans), b - a, 2), dtype=torch.int16, pin_memory=pin)
        read_wav_batch([p["path"] for p in plans], b - a, 2, self.fs, a, out=buf, nthreads=self.nthreads)
        h = {"plans": plans, "pcm": buf}
        if self.load_anno:
            lab = torch.empty((len(TASKS), len(plans)), dtype=torch.float32, pin_memory=pin)
            ln = lab.numpy()
            for j, p in enumerate(plans):
                info = dict(np.load(p["path"].replace(".wav", "_info.npz")))
                annos = locata_annos(info) if p["real"] else simulated_annos(info)
                for k, task in enumerate(TASKS):
                    ln[k, j] = np.asarray(annos[task], np.float32).reshape(())
            h["labels"] = lab
        return h

    def render(self, h, item0=0):
        sig = h["pcm"].to(self.device, non_blocking=True).to(torch.float32).mul_(1.0 / 32768.0)
        if not self.load_anno:
            return sig
        lab = h["labels"].to(self.device, non_blocking=True)
        return sig, {task: lab[k] for k, task in enumerate(TASKS)}
