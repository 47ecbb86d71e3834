"""Fixture F26 of real-data pretraining, from the REAL reference (build container only):

    python tools/make_golden_realpretrain.py        ->  tests/golden/f26_realpretrain.npz

Writes the synthetic trees of tests/realsig_cases.py to a temporary directory and runs the reference's own classes over them, imported
through oracle/ref_shim.py with in-process stand-ins for ``soundfile`` (served by the project's own PCM reader), ``webrtcvad``, ``gpuRIR``,
``librosa`` and ``textgrid``.  Directory listings are sorted in this process, so the fixture does not depend on the file system it was made
on (the project's classes take sort=True for the same order).  The file holds data only, nothing of the reference's source:

    gen/<stage>/<dataset>/...    MicSigFromRIRDataset (gen_sig_from_real_rir.py) as its command line builds it - rir_files: its RIR listing;
                                 seed; per item i: rir_file, noise_file, noise_start, src_idx, utt_idx, utt_files, crop_start, snr and the
                                 float output as f32
    locata/<stage>/...           LOCATADataset: items (relative path), pairs, cumsum (float32 as computed); per drawn item its uniform draw,
                                 idx, the crop start drawn (-1: none drawn), the first row read and, for the first few, the output as f32;
                                 'long/' the same with T = T_LONG, which no recording reaches (pad_cut_sig_sameutt's doubling and draw)
    mix/...                      RandomRealDataset over LOCATA and two fixed corpora: dataset and instance index of 32 items, and for its
                                 LOCATA items their idx and start
    dirs/...                     opt_pretrain().dir()'s three real-data dictionaries as JSON, relative to the work directory
"""
import json
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
import realsig_cases as cases  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
READS = []                        # (file, start) of every soundfile.read the reference makes
DRAWS = []                        # (name, value) of every np.random.uniform / randint call while recording


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
    for name in ("webrtcvad", "gpuRIR", "librosa", "textgrid"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)


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


def _rel(root, path):
    return "" if path is None else os.path.relpath(str(path), root)


def record_generator(store, root, d, ref_dataset, ref_src):
    from sar_ssl_amd import realsig
    gen = ref_dataset.real_dataset
    log = {}
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
    rir_get, src_get = gen.RIRDataset.__getitem__, ref_src.WSJ0Dataset.__getitem__

    def rir_spy(self, i):
        log["rir_file"] = str(self.rir_files[i])
        return rir_get(self, i)

    def src_spy(self, i):
        log["src_idx"] = int(i)
        return src_get(self, i)

    gen.RIRDataset.__getitem__, ref_src.WSJ0Dataset.__getitem__ = rir_spy, src_spy
    try:
        for stage, name in cases.COMBOS:
            # what the reference's command line builds (gen_sig_from_real_rir.py:332-425); the directories and the seed by its rules
            dirs = realsig.rir_dirs(d["rir"], stage, name)
            seed = int({"pretrain": 1, "preval": 2e6}[stage] + ["DCASE", "MIR", "Mesh", "dEchorate", "BUTReverb", "ACE"].index(name) * 10e6)
            src = ref_src.WSJ0Dataset(path=d["src"] + "/" + {"pretrain": "tr", "preval": "dt"}[stage], T=cases.T, fs=cases.FS, num_source=1)
            rirs = gen.RIRDataset(fs=cases.FS, rir_dir_list=dirs, dataset_sz=None, load_info=False, load_noise=True, load_noise_duration=cases.T)
            ds = gen.MicSigFromRIRDataset(rirs, src, snr_range=list(cases.SNR_RANGE), fs=cases.FS, dataset_sz=cases.GEN_ITEMS, seed=seed,
                                          load_info=False, save_anno=False, save_to=None)
            add_orig = ds.add_noise

            def snr_spy(clean, noise, snr, mic_sig_dp=None, _orig=add_orig, **kw):
                log["snr"] = snr
                return _orig(clean, noise, snr, mic_sig_dp=mic_sig_dp, **kw)

            ds.add_noise = snr_spy
            pre = "gen/%s/%s/" % (stage, name)
            store[pre + "rir_files"] = np.array([_rel(root, f) for f in rirs.rir_files])
            store[pre + "seed"] = np.array(seed)
            store[pre + "speakers"] = np.array(src.spkIDs)
            for i in range(cases.GEN_ITEMS):
                log.clear()
                del READS[:]
                mic = ds[i]
                noise_reads = [(f, st) for f, st in READS if "_noise" in f]
                assert len(noise_reads) <= 1
                p = pre + "%d/" % i
                store[p + "out"] = np.asarray(mic, np.float32)
                store[p + "rir_file"] = np.array(_rel(root, log["rir_file"]))
                store[p + "noise_file"] = np.array(_rel(root, noise_reads[0][0]) if noise_reads else "")
                store[p + "noise_start"] = np.array(noise_reads[0][1] if noise_reads else 0)
                store[p + "src_idx"], store[p + "utt_idx"], store[p + "crop_start"] = np.array(log["src_idx"]), np.array(log["utt_idx"]), np.array(log["crop_start"])
                store[p + "utt_files"] = np.array([_rel(root, f) for f in log["utt_files"]])
                store[p + "snr"] = np.array(log["snr"])
    finally:
        ref_src.pad_cut_sig_samespk = pad_orig
        gen.RIRDataset.__getitem__, ref_src.WSJ0Dataset.__getitem__ = rir_get, src_get


def _locata_item(ds):
    """One LOCATADataset item under the spies -> (uniform, idx, start drawn or -1, first row read (0: also the whole file), output)."""
    del READS[:]
    with spy_draws():
        out, = ds.__getitem__()
        draws = list(DRAWS)
    assert draws[0][0] == "uniform" and len(draws) <= 2 and len(READS) == 1
    u = draws[0][1]
    idx = int(np.searchsorted(ds.data_probs_cumsum, u))
    start = draws[1][1] if len(draws) == 2 else -1
    return u, idx, start, READS[0][1], np.asarray(out, np.float32)


def record_locata(store, root, d, ref_dataset):
    for stage in ("train", "test", "val"):
        ds = ref_dataset.LOCATADataset(data_dir=d["locata"], T=cases.T, fs=cases.FS, stage=stage, tasks=[1, 3, 5])
        pre = "locata/%s/" % stage
        store[pre + "items"] = np.array([_rel(root, p) for p, _ in ds.data_items])
        store[pre + "pairs"] = np.array([list(pair) for _, pair in ds.data_items], np.int16).reshape(-1, 2)
        store[pre + "cumsum"] = np.asarray(ds.data_probs_cumsum, np.float32)
        if stage == "val":
            assert len(ds.data_items) == 0
            continue
        assert ds.data_probs_cumsum.dtype == np.float32
        for tag, T, seed in (("", cases.T, cases.LOCATA_SEED), ("long/", cases.T_LONG, cases.LOCATA_SEED + 1)):
            ds.T = T
            np.random.seed(seed)
            for i in range(cases.LOCATA_ITEMS):
                u, idx, start, row0, out = _locata_item(ds)
                p = pre + tag + "%d/" % i
                store[p + "uniform"], store[p + "idx"], store[p + "start"], store[p + "row0"] = np.array(u), np.array(idx), np.array(start), np.array(row0)
                if i < cases.LOCATA_OUTPUTS[stage, tag]:
                    store[p + "out"] = out
            ds.T = cases.T


def record_mix(store, root, d, ref_dataset):
    dirs = cases.mix_dirs(d)
    ds = ref_dataset.RandomRealDataset(data_dirs=dirs, T=cases.T, fs=cases.FS, mic_dist_range=[0.03, 0.20], nmic_selected=2, stage="train", seed=1,
                                       dataset_sz=cases.MIX_ITEMS, dataset_list=list(cases.MIX_LIST), dataset_probs=list(cases.MIX_PROBS))
    store["mix/cumsum"] = np.asarray(ds.ds_probs_cumsum, np.float32)
    store["mix/len"] = np.array([len(x) for x in ds.dataset_list])
    np.random.seed(cases.MIX_SEED)
    seq = []
    for i in range(cases.MIX_ITEMS):
        del READS[:]
        with spy_draws():
            out = ds[i]
            draws = list(DRAWS)
        assert draws[0][0] == "uniform" and draws[1][0] == "randint"
        dsi = int(np.searchsorted(ds.ds_probs_cumsum, draws[0][1]))
        row = [dsi, draws[1][1], -1, -1]
        if cases.MIX_LIST[dsi] == "LOCATA":
            assert draws[2][0] == "uniform" and len(draws) <= 4
            row[2] = int(np.searchsorted(ds.dataset_list[dsi].data_probs_cumsum, draws[2][1]))
            row[3] = draws[3][1] if len(draws) == 4 else -1
        else:
            assert len(draws) == 2 and np.asarray(out[0]).dtype == np.float32
        seq.append(row)
    store["mix/sequence"] = np.array(seq, np.int64)                         # dataset, instance, LOCATA idx, LOCATA start drawn
    assert len(set(r[0] for r in seq)) == len(cases.MIX_LIST), "the 32 items do not reach every corpus"


def record_dirs(store):
    import importlib.util
    import ref_shim
    spec = importlib.util.spec_from_file_location("ref_opt", os.path.join(ref_shim.REF_CODE, "opt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    o = mod.opt_pretrain()
    o.work_dir = o.work_dir_local = "/W"
    dirs = o.dir()
    for k in ("micsig_real_pretrain", "micsig_real_preval", "micsig_real_pretest"):
        store["dirs/" + k] = np.array(json.dumps({n: os.path.relpath(v, "/W") for n, v in dirs[k].items()}, sort_keys=True))


def main():
    import ref_shim
    _install_stubs()
    ref_shim.load()
    import dataset as ref_dataset                                           # noqa: E402  (the reference's code/dataset.py)
    import data_generation.utils_src as ref_src                              # noqa: E402
    import pathlib
    listdir, rglob = os.listdir, pathlib.Path.rglob
    os.listdir = lambda p: sorted(listdir(p))
    pathlib.Path.rglob = lambda self, pattern: sorted(rglob(self, pattern))
    store = {}
    with tempfile.TemporaryDirectory() as root:
        d = cases.build_all(root)
        record_generator(store, root, d, ref_dataset, ref_src)
        record_locata(store, root, d, ref_dataset)
        record_mix(store, root, d, ref_dataset)
    record_dirs(store)
    out = os.path.join(GOLD, "f26_realpretrain.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1000000


if __name__ == "__main__":
    main()
