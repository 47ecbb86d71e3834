"""The synthetic trees of the real-data pretraining tests (fixture F26, tools/make_golden_realpretrain.py): a tiny measured-RIR bank in the
bank format for DCASE and ACE, a WSJ0-shaped source tree, a LOCATA-shaped tree of 48 kHz recordings and two corpora of fixed files.
Everything is drawn from seeded numpy RandomStates, so the tool and the tests write the same bytes; nothing here needs the reference.

    rir/DCASE/<room>/foa/rir_<mic>.npy + _info.npz        rooms gym (pretrain split), tb103 (preval split); no noise cuts
    rir/ACE/<room>/<array>/SP1_<mic>.npy + _info.npz       rooms Office_1, Lobby; rir/ACE_noise/Office_1/... holds cuts for one room
    src/{tr,dt}/<set>/<speaker>/<utterance>.wav            16 kHz, one channel, utterances shorter than an item
    locata/{eval,dev}/task{1,3,5}/<recording>/<array>/audio_array_<array>.wav      48 kHz; see LOCATA_FILES
    micsig/<stage>/<dataset>/<i>.wav                       fixed files of a measured-RIR corpus, (NS, 2) PCM-16
"""
import os

import numpy as np

FS, FS_REC, T, NS, NMIC = 16000, 48000, 0.272, 4352, 2
T_LONG = 0.5                       # an item length no recording reaches: RealMicSigDataset's shorter-than-T branch
SNR_RANGE = (15, 30)
SEED = 26
BANK_ROOMS = {"DCASE": ("gym", "tb103"), "ACE": ("Office_1", "Lobby")}
NOISE_ROOM = ("ACE", "Office_1")
COMBOS = (("pretrain", "DCASE"), ("preval", "DCASE"), ("pretrain", "ACE"))      # every (stage, dataset) the generator accepts here
GEN_ITEMS = 3                     # items 0 .. GEN_ITEMS - 1 of each combination are held by F26
# (split, task, recording, array, channels, frames): a 15-channel recording longer than T, a 4-channel one of an array that is not in the
# list (never an item), a 12-channel one shorter than T (dropped) and a 12-channel one of exactly T
LOCATA_FILES = (("eval", 1, "recording1", "dicit", 15, 20000), ("eval", 1, "recording1", "dummy", 4, 20000),
                ("eval", 1, "recording2", "benchmark2", 12, 9000), ("dev", 1, "recording1", "benchmark2", 12, 13056))
LOCATA_ITEMS, LOCATA_SEED = 4, 5
LOCATA_OUTPUTS = {("train", ""): 4, ("train", "long/"): 2, ("test", ""): 1, ("test", "long/"): 0}      # items whose output F26 holds
FIXED = {("pretrain", "DCASE"): 5, ("pretrain", "ACE"): 3, ("preval", "DCASE"): 4}
MIX_LIST, MIX_PROBS, MIX_SEED, MIX_ITEMS = ("LOCATA", "DCASE", "ACE"), (1, 5, 5), 9, 32


def _write(path, v, fs=FS):
    from sar_ssl_amd.dataset import write_wav_pcm16
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if path.endswith(".wav"):
        write_wav_pcm16(path, v, fs)
    elif path.endswith(".npz"):
        np.savez(path, **v)
    else:
        np.save(path, v)


def build_bank(root):
    """-> root/rir: two rooms per dataset, two RIRs of different lengths per room, noise cuts for one room of ACE."""
    rs = np.random.RandomState(SEED)
    for ds, rooms in BANK_ROOMS.items():
        for r, room in enumerate(rooms):
            for k in range(2):
                L = int(rs.randint(300, 1101))
                h = rs.standard_normal((1, NMIC, L, 1)) * np.exp(-np.arange(L) / (L / 5.0))[None, None, :, None] * 0.2
                for c in range(NMIC):
                    h[0, c, 20 + 7 * k + 3 * c, 0] = 1.0 - 0.1 * c
                mic = "MP%d-1-2" % (k + 1)
                stem = os.path.join(root, "rir", ds, room, "foa" if ds == "DCASE" else "Lin8Ch", ("rir_" if ds == "DCASE" else "SP1_") + mic)
                _write(stem + ".npy", h.astype(np.float32))
                _write(stem + "_info.npz", {"fs": np.array(FS), "T60fromDataset": np.array(0.3 + 0.1 * r + 0.01 * k), "DRR": np.array(2.0 * r - k),
                                            "C50": np.array(10.0 + r + 0.5 * k), "ABS": np.array(0.2 + 0.05 * r)})
    ds, room = NOISE_ROOM
    for k, (typ, n) in enumerate((("Fan", NS + 1500), ("Babble", NS + 700))):
        _write(os.path.join(root, "rir", ds + "_noise", room, "Lin8Ch", "_MP1-1-2_%s.wav" % typ),
               (rs.standard_normal((n, NMIC)) * (2000 + 1000 * k)).astype(np.int16))
    _write(os.path.join(root, "rir", ds + "_noise", room, "Lin8Ch", "_MP2-1-2_Fan.wav"), (rs.standard_normal((NS + 300, NMIC)) * 1500).astype(np.int16))
    return os.path.join(root, "rir")


def build_sources(root):
    """-> root/src: tr and dt, two speakers with two utterances each, every utterance shorter than NS (same-speaker padding runs)."""
    rs = np.random.RandomState(SEED + 1)
    for sub, sset in (("tr", "si_tr_s"), ("dt", "si_dt_05")):
        for s in range(2):
            for u in range(2):
                n = int(rs.randint(1800, 3000))
                x = np.cumsum(rs.standard_normal(n)) * 300 + rs.standard_normal(n) * 2000
                _write(os.path.join(root, "src", sub, sset, "%s%d" % (sub, s), "utt%d%d.wav" % (s, u)), np.clip(x, -30000, 30000).astype(np.int16)[:, None])
    return os.path.join(root, "src")


def build_locata(root, files=LOCATA_FILES):
    """-> root/locata: ``files`` at 48 kHz; every task directory of both splits exists, task 3 and 5 hold nothing."""
    rs = np.random.RandomState(SEED + 2)
    for split in ("eval", "dev"):
        for task in (1, 3, 5):
            os.makedirs(os.path.join(root, "locata", split, "task%d" % task), exist_ok=True)
    for split, task, rec, array, nch, frames in files:
        t = np.arange(frames)[:, None] / FS_REC
        x = 6000 * np.sin(2 * np.pi * (300 + 40 * np.arange(nch)[None, :]) * t) + 1500 * rs.standard_normal((frames, nch))
        _write(os.path.join(root, "locata", split, "task%d" % task, rec, array, "audio_array_%s.wav" % array), x.astype(np.int16), FS_REC)
    return os.path.join(root, "locata")


def build_fixed(root):
    """-> root/micsig/<stage>/<dataset>/<i>.wav (and one <i>_dp.wav that the listing leaves out)."""
    rs = np.random.RandomState(SEED + 3)
    for (stage, ds), n in FIXED.items():
        for i in range(n):
            _write(os.path.join(root, "micsig", stage, ds, "%d.wav" % i), (rs.standard_normal((NS, NMIC)) * 4000).astype(np.int16))
    _write(os.path.join(root, "micsig", "pretrain", "DCASE", "0_dp.wav"), np.zeros((NS, NMIC), np.int16))
    return os.path.join(root, "micsig")


def build_all(root):
    return dict(rir=build_bank(root), src=build_sources(root), locata=build_locata(root), micsig=build_fixed(root))


def mix_dirs(d):
    return {"LOCATA": d["locata"], "DCASE": os.path.join(d["micsig"], "pretrain", "DCASE"), "ACE": os.path.join(d["micsig"], "pretrain", "ACE")}
