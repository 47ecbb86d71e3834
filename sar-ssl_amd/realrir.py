"""Measured RIR banks: the ACE corpus cut into microphone pairs and resampled on the GPU.

The reference writes ``data/RIR/real/ACE/<room>/<array>/SP1_MP<pos>-<i>-<j>.npy`` + ``_info.npz`` and the noise cuts
``data/RIR/real/ACE_noise/<room>/<array>/_MP<pos>-<i>-<j>_<type>.wav`` with ``gen_real_rir.py --dataset ACE --data_type rir noise``
(ACERIRDataset.gen_rir / gen_noise, code/data_generation/gen_real_rir.py:873-1169) - the tree rirsynth.MeasuredBank and the real-data
branch of ``run_downstream.py --ds-train`` read.  This module is that producer.  ``gen_rir`` and ``gen_noise`` restate the two methods
call for call; what they hand to scipy.signal.resample_poly per selected PAIR (several hundred times per recording for the 32-capsule
array, the same channels each time) is one launch per file here - hip.resample_poly over all channels (csrc/resample.hip), chunked for
the minutes-long noise recordings - and a pair is a column pick afterwards.  ``restate_resample`` is the f64 numpy statement the kernel
is tested against, and ``HostResampler`` runs the generators on it without a GPU (fixture F25, tools/make_golden_realrir.py).

Kept as the reference has them, (sic): capsule 8 of the EM32 table repeats capsule 6, so the pairs (6, 8) at distance 0 and every pair
with 8 are judged on that position - the pair list on disk must match; labels DRR / C50 are those of the pair's FIRST channel, T60 the
pair's mean, DRRfromDataset the first channel's.  Not kept: the reference leaves ``rir`` unbound when the corpus is already at --fs
(:1052-1054) and dies on ``None`` when a channel has no direct-path peak; here equal rates pass through and a missing peak is an error
that names the file.  There is no ``input()`` prompt: an existing output directory is overwritten file by file.
The float -> PCM-16 rule of the noise cuts is roomsim.pcm16, this project's reading of libsndfile's, UNPINNED.
"""
import os
import sys
from itertools import combinations

import numpy as np

FS = 16000
ROOMS = ("Building_Lobby", "Lecture_Room_1", "Lecture_Room_2", "Meeting_Room_1", "Meeting_Room_2", "Office_1", "Office_2")
ARRAYS = ("Chromebook", "Mobile", "Lin8Ch", "EM32")             # the corpus's Single and Crucif arrays are not used (:884)
POSITIONS = ("1", "2")
ANNOTATION_CSV = "20150814T154139_Corpus_Mean_DRRs_and_T60s.csv"
UNBUILT = ("DCASE", "Mesh", "MIR", "dEchorate", "BUTReverb")
NOISE_MISMATCH_SECONDS = 5                                       # a recording with the wrong channel count becomes 5 s of zeros (:1153-1156)

# Microphone positions in millimetres, relative to the array's origin (facts of the corpus; gen_real_rir.py:888-901 by value).
_EM32_MM = (
    (0, 39, 15), (-22, 36, 0), (0, 39, -15), (22, 36, 0), (0, 22, 36), (-24, 24, 24), (-39, 15, 0),
    (-24, 24, 24),                  # (sic) capsule 8 repeats capsule 6; the Eigenmike's geometry has (-24, 24, -24) here
    (0, 22, -36), (24, 24, -24), (39, 15, 0), (24, 24, 24), (-15, 0, 39), (-36, 0, 22), (-36, 0, -22), (-15, 0, -39),
    (0, -39, 15), (22, -36, 0), (0, -39, -15), (-22, -36, 0), (0, -22, 36), (24, -24, 24), (39, -15, 0), (24, -24, -24),
    (0, -22, -36), (-24, -24, -24), (-39, -15, 0), (-24, -24, 24), (15, 0, 39), (36, 0, 22), (36, 0, -22), (15, 0, -39))
MIC_POS = {
    "Chromebook": np.array(((0, 0, 0), (0, 62, 0))) / 1000.0,
    "Mobile": np.array(((0.045, 0, 0), (0, 0, 0), (0, 0.0893029, 0))),
    "Lin8Ch": np.array([(60 * k, 0, 0) for k in range(8)]) / 1000.0,
    "EM32": np.array(_EM32_MM) / 1000.0,
}
ROOM_SZ = {"Building_Lobby": (4.47, 5.13, 3.18), "Lecture_Room_1": (6.93, 9.73, 3), "Lecture_Room_2": (13.6, 9.29, 2.94),
           "Meeting_Room_1": (6.61, 5.11, 2.95), "Meeting_Room_2": (10.3, 9.07, 2.63), "Office_1": (3.32, 4.83, 2.95),
           "Office_2": (3.22, 5.1, 2.94)}                        # metres (:904-910)
INFO_KEYS = ("room_sz", "mic_pos", "T60fromDataset", "DRRfromDataset", "DRR", "C50", "ABS", "fs")


# ---------------------------------------------------------------------------------------------------------------- the resampler
def restate_resample(x, up, down):
    """scipy.signal.resample_poly(x, up, down, axis=0) at its defaults, written out in f64: with up / down reduced, half = 10 max(up, down),
    h = up firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) and n_out = ceil(n_in up / down),
        y[m, c] = sum over n in [0, n_in) with |m down - n up| <= half of x[n, c] h[m down - n up + half],
    the terms taken in ascending n.  x: (n_in,) or (n_in, nch)."""
    from .hip import resample_ratio, resample_taps             # (the tap table the device is given; importing hip touches no GPU)
    up, down = resample_ratio(up, down)
    x = np.asarray(x, np.float64)
    flat = x.ndim == 1
    x2 = x[:, None] if flat else x
    n_in = x2.shape[0]
    half = 10 * max(up, down)
    h = resample_taps(up, down)
    n_out = -(-n_in * up // down)
    m = np.arange(n_out, dtype=np.int64)
    first = -((half - m * down) // up)                              # ceil((m down - half) / up)
    y = np.zeros((n_out, x2.shape[1]))
    for j in range(2 * half // up + 1):
        n = first + j
        idx = m * down - n * up + half
        ok = (n >= 0) & (n < n_in) & (idx >= 0)
        if ok.any():
            y[ok] += x2[n[ok]] * h[idx[ok]][:, None]
    return y[:, 0] if flat else y


def _chunk_rows(m0, m1, n_in, up, down):
    """Input rows [lo, hi) that outputs [m0, m1) read: the rows they fall on and a halo of ceil(half / up) on either side, clipped."""
    half = 10 * max(up, down)
    lo = max(0, -((half - m0 * down) // up))
    hi = min(n_in - 1, ((m1 - 1) * down + half) // up) + 1
    return lo, hi


class DeviceResampler:
    """hip.resample_poly over whole files: every channel in one launch, the outputs in chunks of ``chunk`` rows so that a minutes-long
    recording needs neither its f32 copy nor its result resident on the device at once (the pieces are bit-equal to the one-shot call)."""

    def __init__(self, device, chunk=1 << 20):
        self.device, self.chunk = device, int(chunk)

    def _run(self, x, fs_to, fs_from, out_dtype):
        import torch
        from . import hip
        up, down = hip.resample_ratio(fs_to, fs_from)
        n_in, nch = x.shape
        n_out = -(-n_in * up // down)
        out = torch.empty((n_out, nch), dtype=out_dtype)
        for m0 in range(0, n_out, self.chunk):
            m1 = min(n_out, m0 + self.chunk)
            lo, hi = _chunk_rows(m0, m1, n_in, up, down)
            part = x[lo:hi]
            part = np.ascontiguousarray(part if part.dtype == np.int16 else part.astype(np.float32))
            dev = torch.from_numpy(part).to(self.device)
            out[m0:m1] = hip.resample_poly(dev, up, down, out_dtype=out_dtype, n_in=n_in, row0=lo, m0=m0, m1=m1).cpu()
        return out.numpy()

    def f32(self, x, fs_to, fs_from):
        import torch
        return self._run(x, fs_to, fs_from, torch.float32)

    def pcm16(self, x, fs_to, fs_from):
        import torch
        return self._run(x, fs_to, fs_from, torch.int16)


class HostResampler:
    """The generators on the f64 restatement (no GPU): what fixture F25 pins against the reference, and what the device is held to."""

    def f32(self, x, fs_to, fs_from):
        return restate_resample(_as_float(x), fs_to, fs_from)

    def pcm16(self, x, fs_to, fs_from):
        from .roomsim import pcm16
        return pcm16(restate_resample(_as_float(x), fs_to, fs_from))


def _as_float(x):
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else np.asarray(x, np.float64)


# ---------------------------------------------------------------------------------------------------------------- the corpus
def pair_in_range(mic_pos, mic_dist_range):
    """micpair_dist_in_range (:32-38): the pair's distance lies inside the closed range."""
    dist = np.sqrt(np.sum((mic_pos[0, :] - mic_pos[1, :]) ** 2))
    return bool((dist >= mic_dist_range[0]) & (dist <= mic_dist_range[1]))


def selected_pairs(array_name, mic_dist_range=(0.03, 0.20), nmic=2):
    """Index lists of the array's microphone combinations inside the distance range, in ``combinations`` order."""
    pos = MIC_POS[array_name]
    return [list(c) for c in combinations(range(pos.shape[0]), nmic) if pair_in_range(pos[list(c), :], mic_dist_range)]


def read_annotations(path):
    """{'<room>/<array>/<pos>': f64 (2, nmic) = full-band T60 and DRR per channel} from the corpus CSV (separator ', ', :1015-1029)."""
    with open(path) as f:
        rows = [line.split(", ") for line in f.read().splitlines() if line.strip()]
    col = {name: i for i, name in enumerate(rows[0])}
    annos = {}
    for r in rows[1:]:
        array_name, room_name, pos = r[col["Mic config:"]], r[col["Room decode:"]], str(int(float(r[col["Room config:"]])))
        ch = int(float(r[col["Chan:"]])) - 1
        if array_name not in MIC_POS:
            continue                                               # Single, Crucif: the reference's table has the latter, nothing reads it
        key = room_name + "/" + array_name + "/" + pos
        if ch == 0:
            annos[key] = np.zeros((2, MIC_POS[array_name].shape[0]))
        annos[key][:, ch] = [float(r[col["FB T60:"]]), float(r[col["FB DRR:"]])]
    return annos


def find_direct_path(rir, th_ratio=0.5, num_largest=5):
    """_find_dp_from_rir (:931-959): of the five largest local maxima those at least half the maximum, the earliest; None if there is none."""
    from scipy.signal import find_peaks
    peaks, _ = find_peaks(rir)
    largest = peaks[np.argsort(rir[peaks])[-num_largest:]]
    kept = largest[rir[largest] >= th_ratio * np.max(rir)]
    return int(kept[np.argmin(kept)]) if len(kept) > 0 else None


def channel_labels(rir, fs, where=""):
    """Per channel of rir (nsample, nch), in f64: direct-path index over the first fs / 160 samples, DRR over +-2.5 ms around it and C50
    up to +50 ms, eps = 1e-8 placed as the reference places it (:1062-1093) -> (dp int (nch,), DRR (nch,), C50 (nch,))."""
    rir = np.asarray(rir, np.float64)
    nsample, nch = rir.shape
    eps = 1e-8
    dp, drr, c50 = np.zeros(nch, np.int64), np.zeros(nch), np.zeros(nch)
    n = np.arange(nsample)
    for c in range(nch):
        d = find_direct_path(rir[:int(fs / 160), c])
        if d is None:
            raise ValueError("%s: channel %d has no direct-path peak in its first %d samples" % (where, c + 1, int(fs / 160)))
        p = rir[:, c] ** 2
        near = ((n >= d - int(fs * 2.5 / 1000)) & (n <= d + int(fs * 2.5 / 1000))).astype(np.float64)
        early = (n <= d + int(fs * 50 / 1000)).astype(np.float64)
        dp[c] = d
        drr[c] = 10 * np.log10(np.sum(p * near) / (np.sum(p * (1.0 - near)) + eps) + eps)
        c50[c] = 10 * np.log10(np.sum(p * early) / (np.sum(p * (1.0 - early)) + eps) + eps)
    return dp, drr, c50


def _recordings(read_dir, array_name, room_name, pos, word):
    """Files of one array position whose name contains ``word``, in os.listdir order (:1038-1042, 1135-1142)."""
    d = os.path.join(read_dir, "RIRN", array_name, room_name, pos)
    return d, [w for w in os.listdir(d) if word in w]


def _each_position():
    for room_name in ROOMS:
        for array_name in ARRAYS:
            for pos in POSITIONS:
                yield room_name, array_name, pos


def gen_rir(read_dir, save_dir, resampler, fs=FS, mic_dist_range=(0.03, 0.20), nmic=2, log=None):
    """ACERIRDataset.gen_rir: -> the list of written .npy paths.  One resampling per file; the labels per channel from the f32 result."""
    from .dataset import read_wav
    annos = read_annotations(os.path.join(read_dir, "Data", ANNOTATION_CSV))
    written = []
    for room_name, array_name, pos in _each_position():
        d, names = _recordings(read_dir, array_name, room_name, pos, "RIR")
        if not names:
            raise ValueError("%s: no file with RIR in its name" % d)
        path = os.path.join(d, names[-1])                       # the reference keeps the last match of its listing
        pairs = selected_pairs(array_name, mic_dist_range, nmic)
        if log:
            log("rir %s/%s/%s: %d pairs" % (room_name, array_name, pos, len(pairs)))
        if not pairs:
            continue
        rirs, rir_fs = read_wav(path, raw_pcm16=True)
        mic_pos_all = MIC_POS[array_name]
        if rirs.shape[1] != mic_pos_all.shape[0]:
            raise ValueError("%s: %d channels, the %s array has %d" % (path, rirs.shape[1], array_name, mic_pos_all.shape[0]))
        rir = resampler.f32(rirs, fs, rir_fs) if rir_fs != fs else _as_float(rirs)
        stored = np.asarray(rir, np.float32)
        _, drr, c50 = channel_labels(rir, fs, path)
        room_sz = np.array(ROOM_SZ[room_name], np.float64)
        vol = room_sz[0] * room_sz[1] * room_sz[2]
        sur = (room_sz[0] * room_sz[1] + room_sz[1] * room_sz[2] + room_sz[0] * room_sz[2]) * 2
        key = room_name + "/" + array_name + "/" + pos
        out_dir = os.path.join(save_dir, room_name, array_name)
        os.makedirs(out_dir, exist_ok=True)
        for idx in pairs:
            t60 = np.mean(annos[key][0][idx])
            stem = os.path.join(out_dir, "SP1_MP%s-%d-%d" % (pos, idx[0] + 1, idx[1] + 1))
            np.save(stem + ".npy", np.ascontiguousarray(stored[:, idx].T)[None, :, :, None])      # (npoint 1, nmic, nsample, nsource 1)
            np.savez(stem + "_info.npz", room_sz=room_sz, mic_pos=mic_pos_all[idx, :], T60fromDataset=t60,
                     DRRfromDataset=annos[key][1][idx][0], DRR=drr[idx[0]], C50=c50[idx[0]], ABS=0.161 * vol / t60 / sur, fs=fs)
            written.append(stem + ".npy")
    return written


def noise_cuts(path, array_name, pairs, stem, resampler, fs=FS, nmic=2, log=None, batch=16, nthreads=0):
    """One noise recording -> its cut for every pair, written as ``stem % (i, j)`` (1-based): read, resample ONCE to PCM-16, pick columns,
    write ``batch`` files at a time -> the written paths.  A recording whose channel count is not the array's becomes 5 s of zeros."""
    from .dataset import read_wav, write_wav_batch
    from .roomsim import pcm16
    x, noise_fs = read_wav(path, raw_pcm16=True)
    nch = MIC_POS[array_name].shape[0]
    if x.shape[1] != nch:
        if log:
            log("%s: %d channels, the %s array has %d: %d s of zeros" % (path, x.shape[1], array_name, nch, NOISE_MISMATCH_SECONDS))
        pcm = None
    else:
        pcm = resampler.pcm16(x, fs, noise_fs) if noise_fs != fs else pcm16(_as_float(x))
    written = []
    for k in range(0, len(pairs), batch):
        part = pairs[k:k + batch]
        paths = [stem % (i[0] + 1, i[1] + 1) for i in part]
        if pcm is None:
            cut = np.zeros((len(part), int(NOISE_MISMATCH_SECONDS * fs), nmic), np.int16)
        else:
            cut = np.stack([pcm[:, i] for i in part])
        write_wav_batch(paths, cut, fs, nthreads)
        written += paths
    return written


def gen_noise(read_dir, save_dir, resampler, fs=FS, mic_dist_range=(0.03, 0.20), nmic=2, log=None, batch=16, nthreads=0):
    """ACERIRDataset.gen_noise: -> the list of written .wav paths (``noise_cuts`` of every recording whose name contains Noise; its type
    is the last _ field of the name)."""
    written = []
    for room_name, array_name, pos in _each_position():
        d, names = _recordings(read_dir, array_name, room_name, pos, "Noise")
        types = {}
        for w in names:
            types[w.split("_")[-1].split(".")[0]] = w            # a later file of the same type replaces an earlier one
        pairs = selected_pairs(array_name, mic_dist_range, nmic)
        if log:
            log("noise %s/%s/%s: %d pairs x %d types" % (room_name, array_name, pos, len(pairs), len(types)))
        if not pairs:
            continue
        out_dir = os.path.join(save_dir, room_name, array_name)
        os.makedirs(out_dir, exist_ok=True)
        for noise_type, w in types.items():
            stem = os.path.join(out_dir, "_MP" + pos + "-%d-%d_" + noise_type + ".wav")
            written += noise_cuts(os.path.join(d, w), array_name, pairs, stem, resampler, fs, nmic, log, batch, nthreads)
    return written


# ---------------------------------------------------------------------------------------------------------------- command line
def main(argv=None):
    """``gen_real_rir.py`` with the reference's flag names, and this project's --gpus."""
    import argparse
    from .roomsim import _literal
    ap = argparse.ArgumentParser(description="Cut the ACE corpus into microphone pairs: RIRs with labels and noise recordings, resampled on the GPU")
    ap.add_argument("--dataset", type=str, nargs="+", default=["ACE"])
    ap.add_argument("--data_type", type=str, nargs="+", default=["rir", "noise"])
    ap.add_argument("--fs", type=int, default=FS)
    ap.add_argument("--nmic", type=int, default=2)
    ap.add_argument("--mic_dist_range", type=float, nargs=2, default=[0.03, 0.20])
    ap.add_argument("--read_dir", type=str, default="")
    ap.add_argument("--save_dir", type=str, default="")
    ap.add_argument("--gpus", type=_literal, default=[0])
    a = ap.parse_args(argv)
    for name in a.dataset:
        if name in UNBUILT:
            ap.error("--dataset %s: only ACE is built; the banks of DCASE, Mesh, MIR, dEchorate and BUTReverb that gen_sig_from_real_rir.py reads come from the reference's gen_real_rir.py" % name)
        if name != "ACE":
            ap.error("--dataset %s: dataset not found" % name)
    for t in a.data_type:
        if t not in ("rir", "noise"):
            ap.error("--data_type %s: rir and noise" % t)
    if a.nmic != 2:
        ap.error("--nmic %d: microphone pairs only, as the bank's readers expect" % a.nmic)
    if not a.read_dir or not a.save_dir:
        ap.error("--read_dir and --save_dir are required")
    import torch
    gpus = a.gpus if isinstance(a.gpus, (list, tuple)) else [a.gpus]
    torch.cuda.set_device(int(gpus[0]))
    resampler = DeviceResampler("cuda:%d" % int(gpus[0]))
    read_dir = os.path.join(a.read_dir, "ACE")
    for t in a.data_type:
        if t == "rir":
            out = gen_rir(read_dir, os.path.join(a.save_dir, "ACE"), resampler, a.fs, a.mic_dist_range, a.nmic, log=print)
            print("%d RIR pairs written to %s" % (len(out), os.path.join(a.save_dir, "ACE")))
        else:
            out = gen_noise(read_dir, os.path.join(a.save_dir, "ACE_noise"), resampler, a.fs, a.mic_dist_range, a.nmic, log=print)
            print("%d noise cuts written to %s" % (len(out), os.path.join(a.save_dir, "ACE_noise")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
