"""Fixture F25 of the measured-RIR generator (gen_real_rir.py --dataset ACE --data_type rir noise), from the REAL reference (build
container only):

    python tools/make_golden_realrir.py        ->  tests/golden/f25_realrir_ace.npz

Writes the synthetic ACE tree of tests/realrir_cases.py to a temporary directory and runs the reference's own ``ACERIRDataset.gen_rir``
and ``gen_noise`` (code/data_generation/gen_real_rir.py) over it, with in-process stand-ins for the modules that are not installed:
``soundfile.read`` is this project's dataset.read_wav, ``soundfile.write`` records the float array it is handed, ``mat73`` and ``h5py``
(other corpora) are empty.  The file holds data only, nothing of the reference's source:

    pairs             the relative stems '<room>/<array>/SP1_MP<pos>-<i>-<j>' of every written pair, in the reference's order
    labels            f64 (npair, 5): T60fromDataset, DRRfromDataset, DRR, C50, ABS of each pair's _info.npz
    mic_idx           int (npair, 2): the pair's 0-based microphones; each _info.npz's mic_pos was checked to be mic_pos/<array>[mic_idx]
    mic_pos/<array>   the reference's microphone table, room_sz/<room> its room sizes (each _info.npz's room_sz checked against it)
    info_keys, fs     the keys of an _info.npz, its fs
    dp                int (n, 32): the reference rule's direct-path index of every channel of every RIR file (-1 beyond nch), rows in
                      rooms x arrays x positions order
    rir/<array>       f32 (1, 2, 1600, 1): the stored .npy of the pair realrir_cases.STORED_PAIRS[array] of Office_2, position 2
    noise_files       the relative names of every noise cut written, sorted
    noise/<array>/<type>  int16 (4000, 2): roomsim.pcm16 of the f64 array the reference handed to soundfile.write for that pair
    noise_zero        the relative names whose array was all zero, with their common shape

Input condition, asserted here: the direct-path index of every channel is the same when the f64 resampled RIR is moved by +-1e-5 of its
peak (all samples up, all down, and 16 random sign patterns), so an f32 resampler cannot legitimately flip the window of a label.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sarssl_boot  # noqa: E402,F401
import realrir_cases as cases  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LABELS = ("T60fromDataset", "DRRfromDataset", "DRR", "C50", "ABS")


def load_reference(written):
    import ref_shim
    from sar_ssl_amd.dataset import read_wav
    sf = types.ModuleType("soundfile")
    sf.read = lambda path, **kw: read_wav(str(path))
    sf.write = lambda path, data, fs, **kw: written.update({str(path): (np.array(data), fs)})
    sys.modules["soundfile"] = sf
    for name in ("mat73", "h5py"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("ref_gen_real_rir", os.path.join(ref_shim.REF_CODE, "data_generation", "gen_real_rir.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_dp_stability(ref, files):
    """-> dp (n, 32) of every RIR file's channels; asserts the input condition of the module docstring."""
    import scipy.signal
    from sar_ssl_amd.dataset import read_wav
    rs = np.random.RandomState(cases.SEED + 1)
    rows = []
    for room in cases.ROOMS:
        for array in cases.ARRAYS:
            for pos in cases.POSITIONS:
                x, fs_in = read_wav(files["rir"][(room, array, pos)])
                y = scipy.signal.resample_poly(x, cases.FS, fs_in)
                row = -np.ones(32, np.int64)
                for c in range(y.shape[1]):
                    h = y[:cases.FS // 160, c]
                    d, _ = ref._find_dp_from_rir(h)
                    assert d is not None, (room, array, pos, c)
                    e = 1e-5 * np.abs(y[:, c]).max()
                    moves = [np.full(h.shape, e), np.full(h.shape, -e)] + [e * rs.choice((-1.0, 1.0), h.shape) for _ in range(16)]
                    for mv in moves:
                        assert ref._find_dp_from_rir(h + mv)[0] == d, (room, array, pos, c)
                    row[c] = d
                rows.append(row)
    return np.stack(rows)


def main():
    from sar_ssl_amd.roomsim import pcm16
    written = {}
    gen = load_reference(written)
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        files = cases.build_tree(os.path.join(tmp, "in"))
        rir_dir, noise_dir = os.path.join(tmp, "out", "ACE"), os.path.join(tmp, "out", "ACE_noise")
        ds = gen.ACERIRDataset(data_dir=os.path.join(tmp, "in", "ACE"), fs=cases.FS, nmic_selected=2, mic_dist_range=[0.03, 0.20], save_dir=rir_dir)
        store["dp"] = check_dp_stability(ds, files)
        nrir = ds.gen_rir()
        ds.save_dir = noise_dir
        nnoise = ds.gen_noise()
        for a in cases.ARRAYS:
            store["mic_pos/" + a] = np.asarray(ds.mic_poss[a], np.float64)
        for r in cases.ROOMS:
            store["room_sz/" + r] = np.asarray(ds.room_szs[r], np.float64)
        # the pairs in the reference's order: rooms x arrays x positions x combinations
        from itertools import combinations
        stems, labels, mic_idx = [], [], []
        for room in cases.ROOMS:
            for array, nch in cases.ARRAYS.items():
                for pos in cases.POSITIONS:
                    for i, j in combinations(range(nch), 2):
                        stem = "%s/%s/SP1_MP%s-%d-%d" % (room, array, pos, i + 1, j + 1)
                        f = os.path.join(rir_dir, stem + "_info.npz")
                        if not os.path.exists(f):
                            continue
                        info = dict(np.load(f))
                        assert sorted(info) == sorted(store.setdefault("info_keys", np.array(sorted(info))).tolist())
                        assert np.array_equal(info["mic_pos"], store["mic_pos/" + array][[i, j]]) and np.array_equal(info["room_sz"], store["room_sz/" + room])
                        assert int(info["fs"]) == cases.FS
                        stems.append(stem); labels.append([float(info[k]) for k in LABELS]); mic_idx.append((i, j))
                        if room == "Office_2" and pos == "2" and (i + 1, j + 1) == cases.STORED_PAIRS[array]:
                            store["rir/" + array] = np.load(os.path.join(rir_dir, stem + ".npy"))
                            assert store["rir/" + array].dtype == np.float32 and store["rir/" + array].shape == (1, 2, 1600, 1)
        assert len(stems) == nrir == len(cases.tree_listing(rir_dir)) // 2, (len(stems), nrir)
        store["pairs"], store["labels"], store["mic_idx"] = np.array(stems), np.array(labels, np.float64), np.array(mic_idx, np.int16)
        store["fs"] = np.array(cases.FS)
        assert len(written) == nnoise, (len(written), nnoise)
        names, zero, zshape = [], [], None
        for path, (data, fs) in written.items():
            rel = os.path.relpath(path, noise_dir)
            assert fs == cases.FS
            names.append(rel)
            if not data.any():
                zero.append(rel)
                assert zshape in (None, data.shape)
                zshape = data.shape
            room, array, name = rel.split(os.sep)
            _, mp, typ = name[:-4].split("_")
            if room == "Office_2" and mp == "MP2-%d-%d" % cases.STORED_PAIRS[array]:
                assert data.dtype == np.float64 and data.shape == (4000, 2)
                store["noise/%s/%s" % (array, typ)] = pcm16(data)
        store["noise_files"], store["noise_zero"], store["noise_zero_shape"] = np.array(sorted(names)), np.array(sorted(zero)), np.array(zshape)
    assert all("rir/" + a in store and "noise/%s/%s" % (a, t) in store for a in cases.ARRAYS for t in cases.NOISE_TYPES)
    out = os.path.join(GOLD, "f25_realrir_ace.npz")
    np.savez_compressed(out, **store)
    print("%d pairs, %d noise cuts (%d of zeros, shape %s)" % (len(stems), len(names), len(zero), zshape))
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main()
