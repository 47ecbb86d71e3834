"""Fixture F20 of the real-data downstream branch (RIR renderer), from the REAL reference (build container only):

    python tools/make_golden_rirmix.py        ->  tests/golden/f20_rirmix.npz

Imports the reference through oracle/ref_shim.py with in-process stand-ins for ``soundfile`` (served by the project's own PCM reader),
``webrtcvad`` and ``gpuRIR``, writes a tiny synthetic tree to a temporary directory (``write_tree``: 3 rooms x 2 measured RIRs, one room
with a noise recording; 2 simulated RIRs with direct-path files; 2 speakers x 2 short utterances; T = 0.272 s, Ns = 4352), and calls the
reference's two ``MicSigFromRIRDataset.__getitem__`` and ``RandomMicSigFromRIRDataset.__getitem__`` on it.  Nothing of the reference's
source travels: the file holds the tree's arrays and, per item, what was drawn (file names relative to the tree, crop starts, SNR, the head
and the sums of the white noise), the labels and the output as f32.  ``write_tree`` / ``restore_tree`` need no reference: the tests rebuild the tree from the fixture.
"""
import os
import random
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sarssl_boot  # noqa: E402,F401

GOLD = os.path.join(ROOT, "tests", "golden")
FS, T, NS, NMIC, C = 16000, 0.272, 4352, 2, 343.0
SEED = 7
SNR_RANGE = [15, 30]
ROOMS = ["Office_1", "Lecture_2", "Lobby_3"]
NOISE_ROOM = "Lecture_2"
ITEMS = 2                         # indices 0..ITEMS-1 of each MicSigFromRIRDataset
WHITE_HEAD = 32                   # rows of a white-noise draw that are stored, with the draw's sum and sum of squares
OUTER_SEED, OUTER_ITEMS = 11, 6


def tree_arrays(seed=20, ns=NS):
    """{relative path: array} of the synthetic tree.  ``.wav`` entries are int16 (nsample, nch) PCM at FS; ``ns``: the item length the noise
    recordings must cover."""
    rs = np.random.RandomState(seed)
    files = {}

    def rir(L, nch, delay):
        h = rs.standard_normal((1, nch, L, 1)) * np.exp(-np.arange(L) / (L / 5.0))[None, None, :, None] * 0.2
        for c in range(nch):
            h[0, c, delay + 3 * c, 0] = 1.0 - 0.1 * c
        return h

    for r, room in enumerate(ROOMS):
        for k in range(2):
            L = int(rs.randint(300, 1101))
            stem = "real/ACE/%s/conf%d/rir_mic%d" % (room, k, k)
            files[stem + ".npy"] = rir(L, NMIC, 20 + 7 * k).astype(np.float32)
            files[stem + "_info.npz"] = {"fs": np.array(FS), "T60fromDataset": np.array(0.3 + 0.1 * r + 0.01 * k), "DRR": np.array(2.0 * r - k),
                                         "C50": np.array(10.0 + r + 0.5 * k), "ABS": np.array(0.2 + 0.05 * r)}
    files["real/ACE_noise/%s/conf0/ambient_mic0_fan.wav" % NOISE_ROOM] = (rs.standard_normal((ns + 1500, NMIC)) * 2000).astype(np.int16)
    files["real/ACE_noise/%s/conf0/ambient_mic0_babble.wav" % NOISE_ROOM] = (rs.standard_normal((ns + 700, NMIC)) * 3000).astype(np.int16)
    for k in range(2):
        L = int(rs.randint(300, 1101))
        stem = "simu/train/R%d/%d" % (k + 1, k)
        h = rir(L, NMIC, 30 + 5 * k)
        dp = np.zeros((1, NMIC, 64 + 16 * k, 1))
        for c in range(NMIC):
            dp[0, c, 30 + 5 * k + 3 * c, 0] = 1.0 - 0.1 * c
        files[stem + ".npy"] = h.astype(np.float32)
        files[stem + "_dp.npy"] = dp.astype(np.float32)
        files[stem + "_info.npz"] = {"fs": np.array(FS), "T60_edc": np.array(0.4 + 0.2 * k), "DRR": np.array(1.5 - k), "C50": np.array(8.0 + k),
                                     "room_sz": np.array([5.0 + k, 4.0, 3.0]),
                                     "mic_pos": np.array([[2.0, 2.0, 1.5], [2.0 + 0.05 * (k + 1), 2.0, 1.5]])}
    for s in range(2):
        for u in range(2):
            n = int(rs.randint(1800, 3000))                       # shorter than Ns: same-speaker padding runs
            x = np.cumsum(rs.standard_normal(n)) * 300 + rs.standard_normal(n) * 2000
            files["src/tr/si_tr_s/spk%d/utt%d%d.wav" % (s, s, u)] = np.clip(x, -30000, 30000).astype(np.int16)[:, None]
    return files


def write_tree(root, files):
    from sar_ssl_amd.dataset import write_wav_pcm16
    for rel in files:                                            # (insertion order: directory entries are created in a fixed order)
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        v = files[rel]
        if rel.endswith(".wav"):
            write_wav_pcm16(path, v, FS)
        elif rel.endswith(".npz"):
            np.savez(path, **v)
        else:
            np.save(path, v)
    return root


def pack_tree(files):
    """Flat npz keys of the tree: 'tree/<rel>' arrays, info entries as 'tree/<rel>/<key>'."""
    out = {}
    for rel, v in files.items():
        if isinstance(v, dict):
            for k, a in v.items():
                out["tree/%s/%s" % (rel, k)] = a
        else:
            out["tree/" + rel] = v
    out["tree_order"] = np.array(list(files.keys()))
    return out


def restore_tree(root, fixture):
    """Write the tree stored in a loaded F20 to ``root`` (tests; no reference needed)."""
    files = {}
    for rel in [str(r) for r in fixture["tree_order"]]:
        if rel.endswith(".npz"):
            pre = "tree/%s/" % rel
            files[rel] = {k[len(pre):]: fixture[k] for k in fixture if k.startswith(pre)}
        else:
            files[rel] = fixture["tree/" + rel]
    return write_tree(root, files)


def dirs_of(root):
    real = os.path.join(root, "real", "ACE")
    return dict(rir_real=real, real_rooms=[os.path.join(real, r) for r in ROOMS], rir_train_simu=os.path.join(root, "simu", "train"),
                src=os.path.join(root, "src", "tr"))


READS = []                        # (file, start) of every soundfile.read the reference makes


def _install_stubs():
    from sar_ssl_amd.dataset import read_wav_pcm16

    def read(file, start=0, stop=None, dtype="float64", **kw):
        READS.append((str(file), start))
        pcm, fs = read_wav_pcm16(str(file))
        x = pcm[start:stop].astype(dtype) / np.dtype(dtype).type(32768.0)
        return (x[:, 0] if x.shape[1] == 1 else x), fs

    def info(file):
        pcm, fs = read_wav_pcm16(str(file))
        return types.SimpleNamespace(samplerate=fs, duration=pcm.shape[0] / fs, frames=pcm.shape[0], channels=pcm.shape[1])

    sf = types.ModuleType("soundfile")
    sf.read, sf.info, sf.write = read, info, None
    sys.modules["soundfile"] = sf
    for name in ("webrtcvad", "gpuRIR", "librosa", "textgrid"):             # imported by the data_generation modules, unused here
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)


def _rel(root, path):
    return "" if path is None else os.path.relpath(str(path), root)


def main():
    import ref_shim
    _install_stubs()
    ref_shim.load()
    import dataset as ref_dataset                                           # noqa: E402  (the reference's code/dataset.py)
    import common.utils as ref_utils                                        # noqa: E402

    # directory listings in sorted order, in this process only: the fixture then does not depend on the file system it was made on
    # (the banks of sar_ssl_amd.rirsynth and cross_validation_datadir take sort=True for the same order)
    import pathlib
    listdir, rglob = os.listdir, pathlib.Path.rglob
    os.listdir = lambda p: sorted(listdir(p))
    pathlib.Path.rglob = lambda self, pattern: sorted(rglob(self, pattern))

    files = tree_arrays()
    store = pack_tree(files)
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, files)
        d = dirs_of(root)

        def make(ratio, seed=SEED):
            return ref_dataset.RandomMicSigFromRIRDataset(real_rir_dir_list=d["real_rooms"], sim_rir_dir_list=[d["rir_train_simu"]], src_dir=d["src"],
                                                          dataset_sz=100, T=T, fs=FS, c=C, nmic=NMIC, snr_range=SNR_RANGE, real_sim_ratio=ratio,
                                                          transforms=None, seed=seed)

        both = make([1, 1])
        real_ds, sim_ds = both.dataset_list
        # the white noise of the simulated variant, recorded as drawn
        drawn = {}
        noi = sim_ds.noidataset
        orig = noi.generate_diffuse_noise

        def spy(noise, mic_pos, **kw):
            drawn["white"] = np.array(noise)
            return orig(noise, mic_pos, **kw)

        noi.generate_diffuse_noise = spy
        store["rir_files_measured"] = np.array([_rel(root, f) for f in real_ds.rirdataset.rir_files])
        store["rir_files_simulated"] = np.array([_rel(root, f) for f in sim_ds.rirdataset.rir_files])
        store["speakers"] = np.array(real_ds.srcdataset.spkIDs)

        # what an item draws, recorded as drawn: RIR file, noise file and start, utterance files and crop start, SNR
        log = {}
        import data_generation.utils_src as ref_src                          # noqa: E402
        pad_orig = ref_src.pad_cut_sig_samespk

        def pad_spy(utt_path_list, current_utt_idx, nsample_desired, fs_desired):
            n0 = len(READS)
            out_sig = pad_orig(utt_path_list, current_utt_idx, nsample_desired, fs_desired)
            used = [f for f, _ in READS[n0:]]
            sig = np.concatenate([sys.modules["soundfile"].read(f)[0] for f in used])
            del READS[n0 + len(used):]
            st = [i for i in np.flatnonzero(sig[:sig.shape[0] - nsample_desired + 1] == out_sig[0]) if np.array_equal(sig[i:i + nsample_desired], out_sig)]
            assert len(st) == 1
            log.update(utt_idx=current_utt_idx, utt_files=used, crop_start=st[0])
            return out_sig

        ref_src.pad_cut_sig_samespk = pad_spy
        for ds in (real_ds, sim_ds):
            cls = type(ds.rirdataset)

            def get_spy(self, i, _orig=cls.__getitem__):
                log["rir_file"] = str(self.rir_files[i])
                return _orig(self, i)

            cls.__getitem__ = get_spy
        for owner in (real_ds, noi):
            def snr_spy(clean, noise, snr, mic_sig_dp=None, _orig=owner.add_noise, **kw):
                log["snr"] = snr
                return _orig(clean, noise, snr, mic_sig_dp=mic_sig_dp, **kw)

            owner.add_noise = snr_spy

        def record(prefix, ds, idx):
            log.clear()
            drawn.clear()
            del READS[:]
            mic, annos = ds[idx]
            store[prefix + "out"] = np.asarray(mic, np.float32)          # (the type RandomMicSigFromRIRDataset hands on)
            for k, v in annos.items():
                store[prefix + "label_" + k] = np.asarray(v)
            noise_reads = [(f, st) for f, st in READS if "_noise" in f]
            assert len(noise_reads) <= 1
            store[prefix + "rir_file"] = np.array(_rel(root, log["rir_file"]))
            store[prefix + "noise_file"] = np.array(_rel(root, noise_reads[0][0]) if noise_reads else "")
            store[prefix + "noise_start"] = np.array(noise_reads[0][1] if noise_reads else 0)
            store[prefix + "utt_idx"], store[prefix + "crop_start"] = np.array(log["utt_idx"]), np.array(log["crop_start"])
            store[prefix + "utt_files"] = np.array([_rel(root, f) for f in log["utt_files"]])
            store[prefix + "snr"] = np.array(log["snr"])
            store[prefix + "simulated"] = np.array("white" in drawn)
            if "white" in drawn:
                w = drawn["white"]
                store[prefix + "white_head"], store[prefix + "white_sums"] = w[:WHITE_HEAD].copy(), np.array([w.sum(), (w ** 2).sum()])

        # ITEMS indices per variant, the smallest that between them cover a noise recording and none / both simulated RIRs
        def pick(ds, prefix, key):
            ids, seen = [], set()
            for i in range(64):
                record("probe/", ds, i)
                v = str(store["probe/" + key])
                if v not in seen and len(ids) < ITEMS:
                    seen.add(v)
                    ids.append(i)
            for k in [k for k in store if k.startswith("probe/")]:
                del store[k]
            assert len(ids) == ITEMS
            for j, i in enumerate(ids):
                record("%s/%d/" % (prefix, j), ds, i)
            store[prefix + "_ids"] = np.array(ids)

        pick(real_ds, "measured", "noise_file")
        pick(sim_ds, "simulated", "rir_file")
        np.random.seed(OUTER_SEED)
        for i in range(OUTER_ITEMS):
            record("outer/%d/" % i, both, None)

        # cross_validation_datadir under a seeded `random`
        random.seed(3)
        cv = ref_utils.cross_validation_datadir(d["rir_real"])
        store["cv_seed"] = np.array(3)
        for t, tr in enumerate(cv):
            for k in ("train", "val", "test"):
                store["cv/%d/%s" % (t, k)] = np.array([_rel(root, p) for p in tr[k]])
    store["consts"] = np.array([FS, NS, NMIC, SEED, OUTER_SEED, ITEMS, OUTER_ITEMS])
    store["T"], store["snr_range"], store["c"] = np.array(T), np.array(SNR_RANGE), np.array(C)
    out = os.path.join(GOLD, "f20_rirmix.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
