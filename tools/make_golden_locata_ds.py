"""Fixture F27 of the LOCATA TDOA corpus, from the REAL reference (build container only):

    python tools/make_golden_locata_ds.py        ->  tests/golden/f27_locata_ds.npz

Writes the synthetic tree of tests/locatads_cases.py to a temporary directory and runs the reference's own LOCATADataset
(code/data_generation/utils_LOCATA.py) over it with the arguments of its gen_LOCATA.py, imported through oracle/ref_shim.py with an
in-process stand-in for ``soundfile`` served by the project's own PCM reader.  It seeds as gen_LOCATA.py does and calls ``__getitem__``
in sequence, with no workers.  Directory listings are sorted in this process, so the fixture does not depend on the file system it was
made on (the project's class takes sort=True for the same order).  The file holds data only, nothing of the reference's source:

    <stage>/items, pairs, cumsum, sil     the item list (wav path relative to the tree), the pair of each item, the cumulative sum
                                          (float32 as computed) and the silence at the head of each item's recording
    <stage>/uniform, idx, start, tdoa     per drawn item: the uniform draw, the item index, the crop start drawn, the float32 label
    <stage>/sig/<i>                       the float32 signal of a few items
"""
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
import locatads_cases as cases  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DRAWS = []


def _install_soundfile():
    from sar_ssl_amd.dataset import read_wav_pcm16
    cache = {}

    def load(file):
        if str(file) not in cache:
            cache.clear()
            cache[str(file)] = read_wav_pcm16(str(file))
        return cache[str(file)]

    def read(file, start=0, stop=None, dtype="float64", **kw):
        pcm, fs = load(file)
        x = pcm[start:stop].astype(dtype) / np.dtype(dtype).type(32768.0)
        return (x[:, 0] if x.shape[1] == 1 else x), fs

    def info(file):
        pcm, fs = load(file)
        return types.SimpleNamespace(samplerate=fs, duration=pcm.shape[0] / fs, frames=pcm.shape[0], channels=pcm.shape[1])

    sf = types.ModuleType("soundfile")
    sf.read, sf.info, sf.write = read, info, None
    sys.modules["soundfile"] = sf


class spy_draws:
    """np.random.uniform / randint as they are, every call noted in DRAWS."""

    def __enter__(self):
        self.saved = (np.random.uniform, np.random.randint)
        u, r = self.saved

        def uniform(*a, **k):
            v = u(*a, **k)
            DRAWS.append(("uniform", float(v)))
            return v

        def randint(*a, **k):
            v = r(*a, **k)
            DRAWS.append(("randint", int(v)))
            return v

        np.random.uniform, np.random.randint = uniform, randint
        del DRAWS[:]
        return self

    def __exit__(self, *exc):
        np.random.uniform, np.random.randint = self.saved


def record(store, root, ref):
    from sar_ssl_amd import locatads
    seeds = {"train": 6000, "val": 6100, "test": 6200}                     # gen_LOCATA.py's
    for stage in cases.STAGES:
        np.random.seed(seed=seeds[stage])
        ds = ref.LOCATADataset(data_dir=root, T=1.04, fs=16000, stage=stage, tasks=[1, 3, 5], arrays=["dicit", "benchmark2", "eigenmike"],
                               mic_dist_range=[0.03, 0.20], nmic_selected=2, prob_mode=[""], load_anno=True, dataset_sz=cases.ITEMS,
                               sound_speed=343.0, src_single_static=True, transforms=None)
        # the project's tables are the reference's (realsig.LOCATA_MIC_POS by value, the pairs in the same order): checked here, not stored
        for a in ds.mic_idxes_selected:
            mine = locatads.select_pairs(locatads.LOCATA_MIC_POS[a], 2, (0.03, 0.20))
            assert [tuple(i) for i in ds.mic_idxes_selected[a]] == [tuple(i) for i in mine]
            assert all(np.array_equal(p, locatads.LOCATA_MIC_POS[a][i, :]) for p, i in zip(ds.mic_pos_selected[a], mine))
        pre = stage + "/"
        store[pre + "items"] = np.array([os.path.relpath(it[0], root) for it in ds.data_items])
        store[pre + "pairs"] = np.array([list(it[5]) for it in ds.data_items], np.int16).reshape(-1, 2)
        store[pre + "sil"] = np.array([it[8] for it in ds.data_items], np.float64)
        assert ds.data_probs_cumsum.dtype == np.float32
        store[pre + "cumsum"] = np.asarray(ds.data_probs_cumsum, np.float32)
        rows = []
        for i in range(cases.ITEMS):
            with spy_draws():
                sig, anno = ds.__getitem__()
                draws = list(DRAWS)
            assert [d[0] for d in draws] == ["uniform", "randint"], draws
            assert sig.dtype == np.float32 and sig.shape == (cases.NS, 2) and anno["TDOA"].dtype == np.float32 and anno["TDOA"].shape == ()
            rows.append((draws[0][1], int(np.searchsorted(ds.data_probs_cumsum, draws[0][1])), draws[1][1], anno["TDOA"]))
            if i in cases.SIGNALS[stage]:
                store[pre + "sig/%d" % i] = sig
        store[pre + "uniform"] = np.array([r[0] for r in rows], np.float64)
        store[pre + "idx"] = np.array([r[1] for r in rows], np.int64)
        store[pre + "start"] = np.array([r[2] for r in rows], np.int64)
        store[pre + "tdoa"] = np.array([r[3] for r in rows], np.float32)


def main():
    import ref_shim
    _install_soundfile()
    ref_shim.load()
    import data_generation.utils_LOCATA as ref                             # noqa: E402  (the reference's class)
    listdir = os.listdir
    os.listdir = lambda p: sorted(listdir(p))
    store = {}
    with tempfile.TemporaryDirectory() as root:
        record(store, cases.build_tree(root), ref)
    out = os.path.join(GOLD, "f27_locata_ds.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 600000


if __name__ == "__main__":
    main()
