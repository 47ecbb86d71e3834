"""A synthetic tree in the ACE corpus's layout, generated from a seed: what tools/make_golden_realrir.py runs the reference over (fixture
F25) and what the tests run sar_ssl_amd.realrir over.  The inputs are not stored - both sides call ``build_tree`` - so this file and the
seed ARE the fixture's inputs: change neither without regenerating f25_realrir_ace.npz.

    <root>/ACE/Data/20150814T154139_Corpus_Mean_DRRs_and_T60s.csv
    <root>/ACE/RIRN/<array>/<room>/<pos>/<array>_<room>_<pos>_RIR.wav               0.1 s at 48 kHz, one channel per microphone
    <root>/ACE/RIRN/<array>/<room>/<pos>/<array>_<room>_<pos>_Noise_<type>.wav      0.25 s at 48 kHz, types Ambient and Fan

All 7 rooms x 4 arrays x 2 positions exist (the reference lists every directory).  An RIR channel is a positive 7-sample Hann pulse inside
the first 2 ms and an exponentially decaying noise tail behind it.  The sample format goes by array, so every format the reader takes
is on the path: Chromebook PCM-16, Mobile and Lin8Ch PCM-24, EM32 IEEE float-32 (its noise in WAVE_FORMAT_EXTENSIBLE).  One recording has
the wrong channel count (``MISMATCH``): the reference, and this project, write 5 s of zeros for it.
"""
import os
import struct

import numpy as np

SEED = 20250
FS_IN, FS = 48000, 16000
ROOMS = ("Building_Lobby", "Lecture_Room_1", "Lecture_Room_2", "Meeting_Room_1", "Meeting_Room_2", "Office_1", "Office_2")
ARRAYS = {"Chromebook": 2, "Mobile": 3, "Lin8Ch": 8, "EM32": 32}
POSITIONS = ("1", "2")
NOISE_TYPES = ("Ambient", "Fan")
N_RIR, N_NOISE = 4800, 12000
FORMATS = {"Chromebook": "pcm16", "Mobile": "pcm24", "Lin8Ch": "pcm24", "EM32": "float32"}
MISMATCH = ("Office_1", "Mobile", "2", "Fan")                   # this recording has one channel instead of three
CSV_NAME = "20150814T154139_Corpus_Mean_DRRs_and_T60s.csv"
STORED_PAIRS = {"Chromebook": (1, 2), "Mobile": (1, 3), "Lin8Ch": (2, 5), "EM32": (6, 9)}     # 1-based, room Office_2, position 2: arrays in F25


def write_wav(path, x, fs, fmt, extensible=False):
    """x: float (nsample, nch) in [-1, 1) -> a WAV file of sample format pcm16 | pcm24 | pcm32 | float32 (integers: rint(x 2^(bits-1)),
    clipped).  -> the values a reader that scales by 2^-(bits-1) gets back, as f64."""
    x = np.asarray(x, np.float64)
    nch = x.shape[1]
    if fmt == "float32":
        tag, bits, q = 3, 32, x.astype("<f4")
        body, back = q.tobytes(), q.astype(np.float64)
    else:
        tag, bits = 1, int(fmt[3:])
        full = float(1 << (bits - 1))
        q = np.clip(np.rint(x * full), -full, full - 1).astype(np.int64)
        back = q / full
        if bits == 16:
            body = q.astype("<i2").tobytes()
        elif bits == 32:
            body = q.astype("<i4").tobytes()
        else:
            body = (q & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    block = nch * bits // 8
    if extensible:
        sub = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt_body = struct.pack("<HHIIHH", 0xFFFE, nch, fs, fs * block, block, bits) + struct.pack("<HHI", 22, bits, 0) + sub
    else:
        fmt_body = struct.pack("<HHIIHH", tag, nch, fs, fs * block, block, bits)
    chunks = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body + b"data" + struct.pack("<I", len(body)) + body
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(chunks)) + chunks + (b"\x00" if len(body) & 1 else b""))
    return back


def synthetic_rir(rs, nch):
    """(N_RIR, nch): a Hann pulse of 7 samples and height 0.8 centred 0.6 .. 1.7 ms in, then noise decaying with 15 ms."""
    x = np.zeros((N_RIR, nch))
    t = np.arange(N_RIR) / FS_IN
    pulse = 0.8 * np.hanning(9)[1:-1]
    for c in range(nch):
        d = int(rs.randint(30, 80))
        x[d - 3:d + 4, c] = pulse
        tail = 0.12 * rs.randn(N_RIR) * np.exp(-(t - t[d]) / 0.015)
        tail[:d + 6] = 0.0
        x[:, c] += tail
    return x


def build_tree(root):
    """Writes the tree below ``root`` -> {'rir': {(room, array, pos): path}, 'noise': {(room, array, pos, type): path}}."""
    rs = np.random.RandomState(SEED)
    ace = os.path.join(root, "ACE")
    os.makedirs(os.path.join(ace, "Data"), exist_ok=True)
    lines = ["Room:, Room decode:, Room config:, Mic config:, Chan:, FB DRR:, FB T60:"]
    files = {"rir": {}, "noise": {}}
    for ri, room in enumerate(ROOMS):
        for array, nch in ARRAYS.items():
            for pos in POSITIONS:
                d = os.path.join(ace, "RIRN", array, room, pos)
                os.makedirs(d, exist_ok=True)
                for ch in range(nch):
                    lines.append("%d, %s, %s, %s, %d, %.4f, %.4f" % (ri + 1, room, pos, array, ch + 1, rs.uniform(-2, 12), rs.uniform(0.3, 1.3)))
                stem = "%s_%s_%s" % (array, room, pos)
                p = os.path.join(d, stem + "_RIR.wav")
                write_wav(p, synthetic_rir(rs, nch), FS_IN, FORMATS[array])
                files["rir"][(room, array, pos)] = p
                for typ in NOISE_TYPES:
                    n = 1 if (room, array, pos, typ) == MISMATCH else nch
                    p = os.path.join(d, stem + "_Noise_" + typ + ".wav")
                    write_wav(p, np.clip(0.2 * rs.randn(N_NOISE, n), -0.99, 0.99), FS_IN, FORMATS[array], extensible=(array == "EM32"))
                    files["noise"][(room, array, pos, typ)] = p
    with open(os.path.join(ace, "Data", CSV_NAME), "w") as f:
        f.write("\n".join(lines) + "\n")
    return files


def tree_listing(save_dir):
    """Sorted relative paths of every file below ``save_dir``."""
    out = []
    for d, _, names in os.walk(save_dir):
        out += [os.path.relpath(os.path.join(d, n), save_dir) for n in names]
    return sorted(out)
