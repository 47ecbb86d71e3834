"""The LOCATA TDOA corpus of the downstream task: ``gen_LOCATA.py`` on the GPU.

The reference cuts labelled 1.04 s microphone-pair segments out of the LOCATA recordings (LOCATADataset,
code/data_generation/utils_LOCATA.py:31-390, as code/data_generation/gen_LOCATA.py builds it: tasks 1 / 3 / 5, arrays dicit / benchmark2 /
eigenmike, microphone distance 0.03 - 0.20 m, pairs, prob_mode [''], src_single_static) and writes 80 000 / 1 000 / 4 000 of them as
``{idx}.wav`` + ``{idx}_info.npz`` (key TDOA, float32, 0-d).  It builds one item at a time in DataLoader workers; here the host plans a
batch and reads its crops, and the device resamples (hip.resample_poly_batch), normalises (hip.peak_scale), packs PCM-16 and forms the
labels (hip.interp_mean) a batch per launch.

``TdoaCorpus`` restates the item list, the probabilities and the draws; ``restate_item`` is the f64 statement of one item and the
authority for the tests.  This differs from realsig.RecordingCorpus (the pretraining corpus of utils_real_micsig.py) in the splits, in
the weights (every recording 1, divided by its pair count - not its duration), in the silence at the head of a recording that is
skipped, in the crop window by stage and in the labels.

Draw order.  One global stream seeded {'train': 6000, 'val': 6100, 'test': 6200}[stage], items in sequence: the reference's order with
num_workers=0.  The reference's own command runs 32 forked workers which all inherit the same numpy state, so what it writes is neither
reproducible nor free of duplicates (every worker starts on the same draws); this generator is both.

Not built, refused by name: moving-source labels (src_single_static=False), the VAD files, the other arrays.  The task of an item is
read from its ``task<k>`` directory (the reference searches the whole path string for 'task1' .. 'task6').
"""
import os
import sys

import numpy as np

from .pipeline import EpochLoader, StagedWriter
from .realsig import LOCATA_ARRAYS, LOCATA_MIC_POS, LOCATA_TASKS, probs_cumsum, select_pairs, wav_header
from .rirsynth import _listing

FS = 16000
T = 1.04
SEEDS = {"train": 6000, "val": 6100, "test": 6200}                              # gen_LOCATA.py:34
DATA_NUM = {"train": 80000, "val": 1000, "test": 4000}                          # :33
SPLIT = {"train": ("eval",), "val": ("eval",), "test": ("dev",)}                # utils_LOCATA.py:133-135
ST_ED_RATIO = {"train": (0, 0.8), "val": (0.8, 1), "test": (0, 1)}              # :136-138
SOUND_SPEED = 343.0
MIN_DURA = 1.1                                                                  # __getitem__'s min_dura: 2.2 s of signal at least
SIL_WINDOW = 4                                                                  # seconds searched for the first loud sample
FIXED_ARRAY_TASKS, MOVING_ARRAY_TASKS = (1, 2, 3, 4), (5, 6)


def _read_rows(path, a, b):
    """Rows [a, b) of ALL channels as soundfile's float32: PCM-16 through the native reader, the other formats through dataset.read_wav."""
    from .dataset import read_wav, read_wav_batch
    nch, wfs, _, pcm = wav_header(path)
    if pcm:
        return read_wav_batch([path], b - a, nch, wfs, a, nthreads=1)[0].numpy()
    return read_wav(path)[0][a:b].astype(np.float32)


def _as_f32(x):
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x


def silence_beginning(path, max_dura=SIL_WINDOW):
    """_calculate_silence_beginning (utils_LOCATA.py:191-195): the first sample of channel 0, within the first ``max_dura`` seconds, above
    0.15 of that window's maximum, in seconds."""
    _, wfs, frames, _ = wav_header(path)
    x = _as_f32(_read_rows(path, 0, min(int(wfs * max_dura), frames)))
    return np.argmax(x[:, 0] > x[:, 0].max() * 0.15) / wfs


def _table(path):
    """A tab-separated annotation file -> {column: f64 array}: pandas where it imports (the reference's parser), else a reader of our own."""
    try:
        import pandas as pd
    except ImportError:
        with open(path) as f:
            names = f.readline().rstrip("\r\n").split("\t")
            rows = [line.rstrip("\r\n").split("\t") for line in f if line.strip()]
        return {n: np.array([float(r[i]) for r in rows], np.float64) for i, n in enumerate(names)}
    df = pd.read_csv(path, sep="\t")
    return {n: df[n].values for n in df.columns}


class TdoaCorpus:
    """LOCATADataset for the arguments of gen_LOCATA.py.  ``items``: (wav, directory, task, array, source names, pair, pair positions,
    silence) per (recording, microphone pair); ``cumsum``: float32, last entry 1.  ``plan(rs)`` makes the draws of one item on the
    caller's RandomState from headers only, ``read(plan)`` returns its crop, ``tables(plan)`` its annotation table (cached per recording
    and pair).  Listings are in os.listdir order; sort=True makes the order (and the draws) portable.  A task directory that a split
    lacks is passed over."""

    def __init__(self, data_dir, stage, T=T, fs=FS, tasks=LOCATA_TASKS, arrays=LOCATA_ARRAYS, mic_dist_range=(0.03, 0.20), sort=False,
                 src_single_static=True, load_vad=False):
        if stage not in SPLIT:
            raise ValueError("stage %r: train, val and test" % (stage,))
        if not src_single_static:
            raise ValueError("src_single_static=False (a label per sample of a moving source) is not built: the corpus holds one TDOA "
                             "per segment, as gen_LOCATA.py writes it")
        if load_vad:
            raise ValueError("the VAD files are not read: the reference's own VAD branch does not run (utils_LOCATA.py:263-291)")
        for a in arrays:
            if a not in LOCATA_MIC_POS:
                raise ValueError("array %r: dicit, benchmark2 and eigenmike are built (gen_LOCATA.py uses no other)" % (a,))
        self.T, self.fs, self.stage = T, fs, stage
        # select_micpairs of this class keeps, next to the indices realsig.select_pairs returns, the positions mic_poss[idx, :] - in the
        # same ``permutations`` order and by the same distance test
        self.pairs = {a: select_pairs(LOCATA_MIC_POS[a], 2, mic_dist_range) for a in arrays}
        self.items, self._hdr, self._tab = [], {}, {}
        probs = []
        for ds in SPLIT[stage]:
            for task in tasks:
                task_path = data_dir + "/" + ds + "/task" + str(task)
                if not os.path.isdir(task_path):
                    continue
                for recording in _listing(os.listdir(task_path), sort):
                    have = os.listdir(os.path.join(task_path, recording))
                    for array in arrays:
                        if array not in have:
                            continue
                        file_dir = os.path.join(task_path, recording, array)
                        wav = os.path.join(file_dir, "audio_array_" + array + ".wav")
                        nch, wfs, frames, _ = self.header(wav)
                        if nch != LOCATA_MIC_POS[array].shape[0]:
                            raise ValueError("%s: %d channels, the %s array has %d" % (wav, nch, array, LOCATA_MIC_POS[array].shape[0]))
                        sil = silence_beginning(wav)
                        sources = [f[13:-4] for f in _listing(os.listdir(file_dir), sort) if f.startswith("audio_source") and f.endswith(".wav")]
                        if frames / wfs >= T:
                            npair = len(self.pairs[array])
                            for pair in self.pairs[array]:
                                self.items.append((wav, file_dir, task, array, tuple(sources), tuple(pair),
                                                   LOCATA_MIC_POS[array][pair, :], sil))
                                probs.append(1 / npair)
        self.cumsum = probs_cumsum(probs) if probs else np.zeros(0, np.float32)

    def __len__(self):
        return len(self.items)

    def header(self, path):
        h = self._hdr.get(path)
        if h is None:
            h = self._hdr[path] = wav_header(path)
        return h

    def plan(self, rs, min_dura=MIN_DURA):
        """The draws of LOCATADataset.__getitem__ on ``rs``: one uniform() for the item, one randint() for the crop start inside the
        stage's window behind the leading silence - the lower or the upper half of the recording where it is shorter than 10 s.  The
        reference's asserts are a ValueError that names the file."""
        u = rs.uniform()
        idx = int(np.searchsorted(self.cumsum, u))
        if idx >= len(self.items):
            raise ValueError("LOCATA %s: the draw %r selects item %d of %d (an empty corpus?)" % (self.stage, u, idx, len(self.items)))
        wav, _, _, _, _, pair, _, sil = self.items[idx]
        _, wfs, frames, _ = self.header(wav)
        duration = frames / wfs - sil
        nsample = int(duration * wfs)
        want = int(self.T * wfs)
        if not ((nsample >= want) & (duration >= 2 * min_dura)):
            raise ValueError("%s: Signal length is too short (LOCATA): %s s behind %s s of silence, %s s and %d samples are needed"
                             % (wav, nsample / wfs, sil, 2 * min_dura, want))
        r = ST_ED_RATIO[self.stage]
        if duration < 10:
            r = (0, 0.5) if (r[0] + r[1]) / 2 < 0.5 else (0.5, 1)
        lo, hi = round(nsample * r[0] + wfs * sil), round(nsample * r[1] + wfs * sil) - want
        if hi <= lo or hi + want > frames + 1:
            raise ValueError("%s: no crop of %d samples inside [%d, %d) of %d" % (wav, want, lo, hi + want, frames))
        st = int(rs.randint(lo, hi))
        return dict(idx=idx, path=wav, pair=pair, fs=wfs, want=want, start=st, uniform=u)

    def read(self, p):
        """The crop of a plan on the host: rows of ALL channels, the pair's two columns picked -> (want, 2) int16 for a PCM-16 file, else
        float32 (what RecordingCorpus.read does for the pretraining corpus)."""
        x = _read_rows(p["path"], p["start"], p["start"] + p["want"])
        return np.ascontiguousarray(x[:, list(p["pair"])])

    def tables(self, p):
        """load_annotation up to the interpolation (utils_LOCATA.py:209-256) -> (timestamps (npoint,), TDOA (npoint, nsource)) in f64:
        the pair's positions turned by the FIRST rotation matrix, at the array's first position (tasks 1 - 4) or at its position per time
        stamp (tasks 5, 6); TDOA = (|source - mic 1| - |source - mic 0|) / c per time stamp and source."""
        key = (p["path"], p["pair"])
        got = self._tab.get(key)
        if got is not None:
            return got
        _, file_dir, task, array, sources, _, mic_pos, _ = self.items[p["idx"]]
        rec = self._tab.get(file_dir)
        if rec is None:
            tm = _table(os.path.join(file_dir, "required_time.txt"))
            required_time = tm["hour"] * 3600 + tm["minute"] * 60 + tm["second"]
            ar = _table(os.path.join(file_dir, "position_array_" + array + ".txt"))
            array_pos = np.stack((ar["x"], ar["y"], ar["z"]), axis=-1)
            rot0 = np.zeros((3, 3))
            for i in range(3):
                for j in range(3):
                    rot0[i, j] = ar["rotation_" + str(i + 1) + str(j + 1)][0]
            traj = []
            for name in sources:
                sp = _table(os.path.join(file_dir, "position_source_" + name + ".txt"))
                traj.append(np.stack((sp["x"], sp["y"], sp["z"]), axis=-1))
            if not traj:
                raise ValueError("%s: no audio_source_*.wav names a source" % file_dir)
            rec = self._tab[file_dir] = (required_time - required_time[0], array_pos, rot0, np.stack(traj).transpose(1, 2, 0))
        timestamps, array_pos, rot0, traj_pts = rec                                             # traj_pts (npoint, 3, nsource)
        rel = np.matmul(rot0, np.expand_dims(mic_pos, axis=-1)).squeeze()                      # (2, 3)
        if task in FIXED_ARRAY_TASKS:
            mic = np.tile((rel + array_pos[0, :])[np.newaxis, :, :], (traj_pts.shape[0], 1, 1))
        elif task in MOVING_ARRAY_TASKS:
            mic = rel[np.newaxis, :, :] + array_pos[:, np.newaxis, :]                           # (npoint, 2, 3)
        else:
            raise ValueError("%s: task %s has no rule for the array position" % (file_dir, task))
        nsource = traj_pts.shape[-1]
        diff = np.tile(traj_pts[:, np.newaxis, :, :], (1, 2, 1, 1)) - np.tile(mic[:, :, :, np.newaxis], (1, 1, 1, nsource))
        dist = np.sqrt(np.sum(diff ** 2, axis=2))                                               # (npoint, 2, nsource)
        tdoa = (dist[:, 1, :] - dist[:, 0, :]) / SOUND_SPEED
        got = self._tab[key] = (np.ascontiguousarray(timestamps, np.float64), np.ascontiguousarray(tdoa, np.float64))
        return got

    def restate_item(self, p):
        """What the reference returns for the plan, in f64 -> (signal (Ns, 2), TDOA): the crop as soundfile's float32, resampled
        (realrir.restate_resample), x / (max|x| + 1e-8) * 0.9; the label the mean over the crop's sample times
        ``t = n / fs + start / fs_rec`` and over all sources of np.interp(t, timestamps, TDOA)."""
        from .realrir import restate_resample
        x = _as_f32(self.read(p))
        x = restate_resample(x, self.fs, p["fs"]) if p["fs"] != self.fs else x.astype(np.float64)
        t = np.arange(x.shape[0]) / self.fs + p["start"] / p["fs"]
        ts, tdoa = self.tables(p)
        per_sample = np.stack([np.interp(t, ts, tdoa[:, s]) for s in range(tdoa.shape[1])], axis=-1)
        x = x / (np.max(np.abs(x)) + 1e-8) * 0.9
        return x, np.mean(per_sample)


# ---------------------------------------------------------------------------------------------------------------- the generator
class _TdoaLoader(EpochLoader):
    """Batches of TdoaCorpus items for ``generate``: pipeline.EpochLoader's producer thread plans the items, reads their crops and
    annotation tables; the render uploads them, resamples the crops in ONE launch per (sampling rate, sample format), normalises and packs
    PCM-16 on its stream and forms the labels on a stream of their own.  Hands out (plans, pcm int16 (B, Ns, 2), stats (B, 1 + ncol)
    f64: the peak and the per-source label means)."""

    def __init__(self, corpus, dataset_sz, batch_size, device="cuda", nthreads=4):
        import torch
        super().__init__(dataset_sz, batch_size, device)
        self.corpus, self.nthreads = corpus, nthreads
        self.nsample = int(corpus.T * corpus.fs)
        self.label_stream = torch.cuda.Stream(self.device)
        self._pool = None

    def plan_item(self, rs):
        return self.corpus.plan(rs)

    def handout(self, res):
        _, pcm, (stats, _) = res
        return res, [pcm, stats]

    def host_batch(self, plans):
        import torch
        from concurrent.futures import ThreadPoolExecutor
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=max(1, self.nthreads))
        h = {"plans": plans, "groups": []}
        groups = {}
        # a crop is rows of ALL the recording's channels: the reads run side by side, the native reader releases the GIL
        for i, crop in enumerate(self._pool.map(self.corpus.read, plans)):
            groups.setdefault((plans[i]["fs"], crop.dtype.str), []).append((i, crop))
        for (wfs, _), members in groups.items():
            n_max = max(c.shape[0] for _, c in members)
            buf = torch.empty((len(members), n_max, 2), dtype=torch.from_numpy(members[0][1]).dtype, pin_memory=True)
            for j, (_, c) in enumerate(members):
                buf[j, :c.shape[0]] = torch.from_numpy(c)
            n_in = torch.tensor([c.shape[0] for _, c in members], dtype=torch.int32).pin_memory()
            h["groups"].append(([i for i, _ in members], wfs, buf, n_in))
        tabs = [self.corpus.tables(p) for p in plans]
        ncol = max(t[1].shape[1] for t in tabs)
        if ncol > 8:
            raise ValueError("%s: %d sources, the label kernel takes 8" % (plans[0]["path"], ncol))
        off = np.zeros(len(plans) + 1, np.int32)
        off[1:] = np.cumsum([t[0].shape[0] for t in tabs])
        tv = torch.zeros((int(off[-1]), 1 + ncol), dtype=torch.float64, pin_memory=True)          # ts | TDOA per source, 0 past an item's sources
        tn = tv.numpy()
        for b, (ts, td) in enumerate(tabs):
            tn[off[b]:off[b + 1], 0] = ts
            tn[off[b]:off[b + 1], 1:1 + td.shape[1]] = td
        h.update(off=off, tv=tv, nsrc=[t[1].shape[1] for t in tabs], t0=[p["start"] / p["fs"] for p in plans])
        return h

    def render(self, h, item0=0):
        import torch
        from . import hip
        dev, B, fs = self.device, len(h["plans"]), self.corpus.fs
        out = torch.empty((B, self.nsample, 2), dtype=torch.float32, device=dev)
        cur = torch.cuda.current_stream(dev)
        # the labels first, on their own stream: they depend on nothing the signal path makes, and the wait inside hip.interp_mean (for
        # the upload of its per-item rows) then waits for the tables' upload only
        with torch.cuda.stream(self.label_stream):
            tv = h["tv"].to(dev, non_blocking=True)
            means = hip.interp_mean(h["off"], tv[:, 0].contiguous(), tv[:, 1:].contiguous(), h["t0"], [1.0 / fs] * B, [self.nsample] * B)
        for ids, wfs, buf, n_in in h["groups"]:
            x, n = buf.to(dev, non_blocking=True), n_in.to(dev, non_blocking=True)
            if wfs == fs:
                t = x.to(torch.float32).mul_(1.0 / 32768.0) if x.dtype == torch.int16 else x
            else:
                t = hip.resample_poly_batch(x, n, fs, wfs)
            if t.shape[1] != self.nsample:
                raise ValueError("crops of %d samples at %d Hz give %d samples at %d Hz, an item has %d"
                                 % (x.shape[1], wfs, t.shape[1], fs, self.nsample))
            if len(ids) == B:
                out = t.contiguous()
            else:
                out.index_copy_(0, torch.tensor(ids, dtype=torch.int64).to(dev, non_blocking=True), t)
        peak = hip.peak_scale(out)
        pcm = hip.pcm16_pack(out)
        cur.wait_stream(self.label_stream)
        means.record_stream(cur)
        stats = torch.cat((peak.to(torch.float64)[:, None], means), dim=1)                      # one tensor, one read-back
        return h["plans"], pcm, (stats, h["nsrc"])


def _write_info(path, tdoa):
    """``np.savez(path, TDOA=<0-d float32>)`` with the archive's time stamp fixed, so that a second run writes the same bytes."""
    import zipfile
    zi = zipfile.ZipInfo("TDOA.npy", date_time=(1980, 1, 1, 0, 0, 0))
    with zipfile.ZipFile(path + ".tmp", "w", zipfile.ZIP_STORED) as z, z.open(zi, "w") as f:
        np.lib.format.write_array(f, np.asarray(tdoa, np.float32).reshape(()), allow_pickle=False)
    os.replace(path + ".tmp", path)


def check_save_dir(out_dir, overwrite):
    """The reference asks on stdin before it writes into an existing directory; here a non-empty one is refused unless overwrite."""
    if os.path.isdir(out_dir) and os.listdir(out_dir) and not overwrite:
        raise FileExistsError("%s exists and is not empty: give --overwrite to regenerate its signals (the reference asks on stdin)" % out_dir)


def generate(data_dir, save_to, stage, data_num=None, fs=FS, batch=16, device="cuda", sort=False, overwrite=False, nthreads=0, log=None,
             corpus=None):
    """gen_LOCATA.py for one stage -> ``<save_to>/<stage>/{idx}.wav`` (PCM-16, 16 640 x 2) and ``{idx}_info.npz`` for idx < data_num, the
    item plans in order.  Per batch: the loader's render (see _TdoaLoader), ONE read-back of the peaks and label means - a peak that is
    not finite raises, naming the recording, before anything of the batch is written -, the pinned copy and the writer thread
    (pipeline.StagedWriter), and the labels' files."""
    import torch
    from .dataset import write_wav_batch
    data_num = DATA_NUM[stage] if data_num is None else int(data_num)
    out_dir = os.path.join(save_to, stage)
    check_save_dir(out_dir, overwrite)
    corpus = TdoaCorpus(data_dir, stage, T, fs, sort=sort) if corpus is None else corpus
    if len(corpus) == 0:
        raise ValueError("LOCATA %s: no recording of tasks %s and arrays %s under %s/%s" % (stage, LOCATA_TASKS, LOCATA_ARRAYS, data_dir, SPLIT[stage][0]))
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device(device)
    loader = _TdoaLoader(corpus, data_num, batch, dev)
    np.random.seed(seed=SEEDS[stage])                          # the loader's plans continue from numpy's global state (EpochLoader.plan_batches)

    def write(buf, ids):
        write_wav_batch([os.path.join(out_dir, "%d.wav" % i) for i in ids], buf, fs, nthreads)

    done, plans_out, labels = 0, [], []
    with torch.cuda.device(dev), StagedWriter(batch, loader.nsample, 2) as writer:
        for plans, pcm, (stats, nsrc) in loader:
            ids = list(range(done, done + len(plans)))
            host = stats.cpu().numpy()
            for j, p in enumerate(plans):
                if not np.isfinite(host[j, 0]):
                    raise ValueError("%s: samples [%d, %d) hold a value that is not finite" % (p["path"], p["start"], p["start"] + p["want"]))
            writer.stage(pcm, write, ids)
            for j, i in enumerate(ids):
                tdoa = np.float32(host[j, 1:1 + nsrc[j]].sum() / nsrc[j])
                _write_info(os.path.join(out_dir, "%d_info.npz" % i), tdoa)
                labels.append(tdoa)
            plans_out += plans
            done += len(plans)
            if log and (done % (100 * batch) < batch or done == data_num):
                log("%s: %d / %d items" % (stage, done, data_num))
    return plans_out, np.array(labels, np.float32)


def main(argv=None):
    """``gen_LOCATA.py`` with the reference's flag names (--stage takes several values, --fs, --save-to; --workers is accepted and unused)
    and this project's --data-dir, --gpus, --batch, --data-num, --sort, --overwrite."""
    import argparse
    from .roomsim import _literal
    ap = argparse.ArgumentParser(description="Generate the LOCATA TDOA corpus (labelled 1.04 s microphone-pair segments) on the GPU")
    ap.add_argument("--stage", type=str, nargs="+", default=["train"])
    ap.add_argument("--workers", type=int, default=32, help="accepted for the reference's command line; the producer is one thread")
    ap.add_argument("--fs", type=int, default=FS)
    ap.add_argument("--save-to", type=str, default="../../data/MicSig/real_ds_locata")
    ap.add_argument("--data-dir", type=str, default="../../../data/MicSig/LOCATA")
    ap.add_argument("--gpus", type=_literal, default=[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--data-num", type=int, default=None, help="items per stage (default: 80000 / 1000 / 4000)")
    ap.add_argument("--sort", action="store_true", default=False, help="sorted directory listings: the same items on every file system")
    ap.add_argument("--overwrite", action="store_true", default=False, help="write into a stage directory that holds files already")
    a = ap.parse_args(argv)
    for stage in a.stage:
        if stage not in SEEDS:
            ap.error("--stage %s: train, val and test" % stage)
    if a.fs != FS:
        ap.error("--fs %d: %d only; the downstream loader reads 16 kHz segments" % (a.fs, FS))
    if a.batch < 1 or (a.data_num is not None and a.data_num < 1):
        ap.error("--batch and --data-num are positive")
    if not os.path.isdir(a.data_dir):
        ap.error("--data-dir: %s is not a directory (the LOCATA corpus with eval/ and dev/)" % a.data_dir)
    for stage in a.stage:
        try:
            check_save_dir(os.path.join(a.save_to, stage), a.overwrite)
        except FileExistsError as e:
            ap.error(str(e))
    import torch
    gpus = a.gpus if isinstance(a.gpus, (list, tuple)) else [a.gpus]
    torch.cuda.set_device(int(gpus[0]))
    for stage in a.stage:
        plans, _ = generate(a.data_dir, a.save_to, stage, a.data_num, a.fs, a.batch, "cuda:%d" % int(gpus[0]), a.sort, a.overwrite, log=print)
        print("%d segments written to %s" % (len(plans), os.path.join(a.save_to, stage)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
