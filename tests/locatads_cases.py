"""The synthetic LOCATA tree of the TDOA-corpus tests (fixture F27, tools/make_golden_locata_ds.py): 48 kHz PCM-16 recordings with their
annotation files, drawn from seeded numpy RandomStates, so the tool and the tests write the same bytes; nothing here needs the reference.

    <root>/{eval,dev}/task{1,3,5}/<recording>/<array>/audio_array_<array>.wav      see FILES
                                                     /required_time.txt            120 stamps a second, from 10:15:30
                                                     /position_array_<array>.txt   a rotation about z and x; the array drifts in task 5
                                                     /audio_source_<name>.wav, position_source_<name>.txt   one or two slow trajectories

Recordings of about 3 s and 6 s take the half-window rule (the lower half for train and test, the upper for val), the 12 s ones the
stage's own window; every one keeps 2.2 s behind its quiet lead-in.  The ``dummy`` array is not in the generator's list and must be
passed over.
"""
import os

import numpy as np

FS, FS_REC, T, NS = 16000, 48000, 1.04, 16640
SEED = 27
RATE = 120                                                    # annotation stamps per second
# (split, task, recording, array, channels, seconds, quiet lead-in in seconds, source names)
FILES = (("eval", 1, "recording1", "dicit", 15, 3.0, 0.25, ("talker1",)),
         ("eval", 1, "recording1", "dummy", 4, 3.0, 0.25, ("talker1",)),
         ("eval", 1, "recording2", "eigenmike", 32, 3.1, 0.10, ("loudspeaker2",)),
         ("eval", 3, "recording1", "benchmark2", 12, 6.0, 0.40, ("talker2",)),
         ("eval", 5, "recording1", "benchmark2", 12, 12.0, 0.30, ("talker1", "talker3")),
         ("dev", 1, "recording1", "benchmark2", 12, 3.0, 0.20, ("loudspeaker1",)),
         ("dev", 3, "recording1", "dicit", 15, 6.0, 0.35, ("talker4",)),
         ("dev", 5, "recording1", "benchmark2", 12, 12.0, 0.15, ("talker2", "talker5")))
ITEMS = 8                                                     # items per stage whose draws and labels F27 holds
SIGNALS = {"train": (0,), "val": (0,), "test": (0,)}          # items whose signal F27 holds
STAGES = ("train", "val", "test")


def _write_wav(path, v, fs):
    from sar_ssl_amd.dataset import write_wav_pcm16
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_wav_pcm16(path, v, fs)


def _write_table(path, names, cols):
    with open(path, "w") as f:
        f.write("\t".join(names) + "\n")
        for row in zip(*cols):
            f.write("\t".join(("%d" % v) if isinstance(v, (int, np.integer)) else ("%.6f" % v) for v in row) + "\n")


def _rotation(az, el):
    ca, sa, ce, se = np.cos(az), np.sin(az), np.cos(el), np.sin(el)
    return np.array(((ca, -sa, 0.0), (sa, ca, 0.0), (0.0, 0.0, 1.0))) @ np.array(((1.0, 0.0, 0.0), (0.0, ce, -se), (0.0, se, ce)))


def build_recording(root, k, split, task, rec, array, nch, seconds, lead, sources):
    rs = np.random.RandomState(SEED + k)
    d = os.path.join(root, split, "task%d" % task, rec, array)
    frames = int(round(seconds * FS_REC))
    t = np.arange(frames)[:, None] / FS_REC
    x = 6000 * np.sin(2 * np.pi * (300 + 40 * np.arange(nch)[None, :]) * t) + 1500 * rs.standard_normal((frames, nch))
    x[:int(round(lead * FS_REC))] *= 0.02
    _write_wav(os.path.join(d, "audio_array_%s.wav" % array), x.astype(np.int16), FS_REC)
    npoint = int(seconds * RATE) + 1
    sec = 30.0 + np.arange(npoint) / RATE
    time_cols = ([2017] * npoint, [3] * npoint, [9] * npoint, [10] * npoint, [15 + int(s // 60) for s in sec], [s % 60 for s in sec])
    time_names = ["year", "month", "day", "hour", "minute", "second"]
    _write_table(os.path.join(d, "required_time.txt"), time_names, time_cols)
    u = np.arange(npoint) / RATE
    pos = np.stack((3.0 + 0.02 * k + (0.05 * u if task == 5 else 0 * u), 4.0 + (0.03 * np.sin(0.4 * u) if task == 5 else 0 * u), 1.2 + 0 * u), -1)
    R = _rotation(np.pi / 6 + 0.1 * k, 0.2)
    names = time_names + ["x", "y", "z", "ref_vec_x", "ref_vec_y", "ref_vec_z"] + ["rotation_%d%d" % (i + 1, j + 1) for i in range(3) for j in range(3)]
    cols = list(time_cols) + [pos[:, 0], pos[:, 1], pos[:, 2], [R[0, 0]] * npoint, [R[1, 0]] * npoint, [R[2, 0]] * npoint]
    cols += [[R[i, j]] * npoint for i in range(3) for j in range(3)]
    _write_table(os.path.join(d, "position_array_%s.txt" % array), names, cols)
    for s, name in enumerate(sources):
        _write_wav(os.path.join(d, "audio_source_%s.wav" % name), (rs.standard_normal((480, 1)) * 1000).astype(np.int16), FS_REC)
        sp = np.stack((1.5 + 1.1 * s + 0.08 * u, 6.0 - 0.9 * s + 0.05 * np.cos(0.3 * u + s), 1.6 + 0.01 * u), -1)
        I = np.eye(3)
        cols = list(time_cols) + [sp[:, 0], sp[:, 1], sp[:, 2], [1.0] * npoint, [0.0] * npoint, [0.0] * npoint]
        cols += [[I[i, j]] * npoint for i in range(3) for j in range(3)]
        _write_table(os.path.join(d, "position_source_%s.txt" % name), names, cols)
        with open(os.path.join(d, "VAD_%s_%s.txt" % (array, name)), "w") as f:          # present in the corpus, never read
            f.write("VAD\n0\n")
    return d


def build_tree(root, files=FILES):
    """-> root: every task directory of both splits exists."""
    for split in ("eval", "dev"):
        for task in (1, 3, 5):
            os.makedirs(os.path.join(root, split, "task%d" % task), exist_ok=True)
    for k, f in enumerate(files):
        build_recording(root, k, *f)
    return root


def write_segments(root, stage, n, fs=FS, ns=NS, seed=0):
    """``n`` segments as gen_LOCATA.py writes them under root/<stage>: {idx}.wav (PCM-16, two channels), {idx}_info.npz -> (pcm, tdoa)."""
    from sar_ssl_amd import locatads
    rs = np.random.RandomState(seed)
    pcm = rs.randint(-20000, 20000, (n, ns, 2)).astype(np.int16)
    tdoa = rs.uniform(-5e-4, 5e-4, n).astype(np.float32)
    for i in range(n):
        _write_wav(os.path.join(root, stage, "%d.wav" % i), pcm[i], fs)
        locatads._write_info(os.path.join(root, stage, "%d_info.npz" % i), tdoa[i])
    return pcm, tdoa


def write_simulated(root, n, ns=20000, seed=1):
    """``n`` simulated segments in the layout FixMicSigDataset reads (longer than an item: Selecting cuts them) -> (pcm, infos)."""
    rs = np.random.RandomState(seed)
    pcm = rs.randint(-20000, 20000, (n, ns, 2)).astype(np.int16)
    infos = []
    for i in range(n):
        info = dict(room_sz=rs.uniform(3, 8, 3), TDOA=np.float32(rs.uniform(-5e-4, 5e-4)), T60_edc=np.float64(rs.uniform(0.2, 1.0)),
                    DRR=np.float16(rs.uniform(-5, 10)), C50=np.float16(rs.uniform(0, 20)))
        _write_wav(os.path.join(root, "%d.wav" % i), pcm[i], FS)
        _write_wav(os.path.join(root, "%d_dp.wav" % i), pcm[i], FS)                              # never listed
        np.savez(os.path.join(root, "%d_info.npz" % i), **info)
        infos.append(info)
    return pcm, infos


def build_short(root):
    """A tree whose one recording is listed (longer than T) and refused when drawn: 2.0 s, less than the 2.2 s the reference asserts."""
    return build_tree(root, (("eval", 1, "recording1", "benchmark2", 12, 2.0, 0.1, ("talker1",)),))
