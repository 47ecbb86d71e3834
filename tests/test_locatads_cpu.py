"""CPU: the host side of the LOCATA TDOA corpus (sar_ssl_amd/locatads.py) against fixture F27 - the reference's own LOCATADataset with
the arguments of its gen_LOCATA.py over the synthetic tree of tests/locatads_cases.py (tools/make_golden_locata_ds.py): the item list and
cumulative sums, the silence at the head of a recording, every draw, restate_item's label and signal, and the refusals.  Listings are
sorted on both sides (sort=True)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401
import locatads_cases as cases  # noqa: E402

F27 = os.path.join(ROOT, "tests", "golden", "f27_locata_ds.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(F27)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return cases.build_tree(str(tmp_path_factory.mktemp("locata_ds")))


@pytest.fixture(scope="module")
def corpora(tree):
    from sar_ssl_amd import locatads
    return {stage: locatads.TdoaCorpus(tree, stage, sort=True) for stage in cases.STAGES}


def test_constants_are_the_command_lines():
    from sar_ssl_amd import locatads
    assert locatads.SEEDS == {"train": 6000, "val": 6100, "test": 6200} and locatads.DATA_NUM == {"train": 80000, "val": 1000, "test": 4000}
    assert locatads.SPLIT == {"train": ("eval",), "val": ("eval",), "test": ("dev",)}
    assert locatads.ST_ED_RATIO == {"train": (0, 0.8), "val": (0.8, 1), "test": (0, 1)}
    assert int(locatads.T * locatads.FS) == cases.NS


@pytest.mark.parametrize("stage", cases.STAGES)
def test_item_list_pairs_cumsum_and_silence(fx, tree, corpora, stage):
    c = corpora[stage]
    assert [os.path.relpath(it[0], tree) for it in c.items] == list(fx[stage + "/items"])
    assert np.array_equal(np.array([it[5] for it in c.items]), fx[stage + "/pairs"])
    assert c.cumsum.dtype == np.float32 and np.array_equal(c.cumsum, fx[stage + "/cumsum"]) and c.cumsum[-1] == 1
    sil = np.array([it[7] for it in c.items])
    assert np.array_equal(sil, fx[stage + "/sil"]) and sil.min() > 0.05                       # the quiet lead-ins are found
    assert not any("dummy" in it[0] for it in c.items)
    arrays = {it[3] for it in c.items}
    assert arrays == ({"dicit", "benchmark2", "eigenmike"} if stage != "test" else {"dicit", "benchmark2"})
    # every recording weighs the same, whatever its duration and its pair count
    w = np.diff(np.concatenate(([0.0], c.cumsum.astype(np.float64))))
    per_rec = {}
    for it, wi in zip(c.items, w):
        per_rec[it[0]] = per_rec.get(it[0], 0.0) + wi
    assert np.allclose(list(per_rec.values()), 1.0 / len(per_rec), rtol=1e-3)


@pytest.mark.parametrize("stage", cases.STAGES)
def test_every_draw_and_the_restated_item(fx, corpora, stage):
    from sar_ssl_amd import locatads, parity
    c = corpora[stage]
    rs = np.random.RandomState(locatads.SEEDS[stage])
    gl, gs = parity.LOCATADS["label"], parity.LOCATADS["signal"]
    tol_label, tol_sig = min(gl["gate"], gl["cap"]), min(gs["gate"], gs["ceiling"])
    halves, worst_label, worst_sig, seen = set(), 0.0, 0.0, 0
    for i in range(cases.ITEMS):
        p = c.plan(rs)
        assert p["uniform"] == fx[stage + "/uniform"][i] and p["idx"] == fx[stage + "/idx"][i] and p["start"] == fx[stage + "/start"][i], (stage, i)
        _, wfs, frames, _ = c.header(p["path"])
        halves.add((frames / wfs < 10, p["start"] + p["want"] / 2 > frames / 2))
        x, tdoa = c.restate_item(p)
        ref = fx[stage + "/tdoa"][i]
        assert ref.dtype == np.float32 and x.shape == (cases.NS, 2) and x.dtype == np.float64
        d = abs(float(np.float32(tdoa)) - float(ref)) / abs(float(ref))
        worst_label = max(worst_label, d)
        assert d <= tol_label, (stage, i, d)
        key = stage + "/sig/%d" % i
        if key in fx.files:
            seen += 1
            assert abs(np.abs(x).max() - 0.9) < 1e-7
            d = np.abs(x - fx[key].astype(np.float64)).max() / 0.9
            worst_sig = max(worst_sig, d)
            assert d <= tol_sig, (stage, i, d)
    print("%s: label distance %.3g (gate %.3g), signal distance %.3g of the peak (gate %.3g)" % (stage, worst_label, tol_label, worst_sig, tol_sig))
    assert seen == len(cases.SIGNALS[stage])
    # both half-window rules and the stage's own window are drawn from: (short recording, crop in the upper half) - a short recording
    # gives its lower half to train and its upper half to val and, (0 + 1) / 2 being no less than 0.5, to test
    assert halves >= {"train": {(True, False), (False, False)}, "val": {(True, True), (False, True)}, "test": {(True, True), (False, False)}}[stage]
    assert (True, True) not in halves if stage == "train" else (True, False) not in halves


def test_tables_follow_the_array_in_task_5_only(corpora):
    c = corpora["train"]
    by_task = {}
    for idx, it in enumerate(c.items):
        by_task.setdefault(it[2], idx)
    for task, idx in by_task.items():
        it = c.items[idx]
        ts, tdoa = c.tables(dict(idx=idx, path=it[0], pair=it[5]))
        assert ts[0] == 0 and np.all(np.diff(ts) > 0) and tdoa.shape == (ts.shape[0], len(it[4])) and tdoa.dtype == np.float64
        assert np.abs(tdoa).max() <= 0.2 / 343.0 + 1e-12                                      # no pair is wider than the distance range
    assert len(c.items[by_task[5]][4]) == 2 and len(c.items[by_task[1]][4]) == 1
    # the same object on a second request (parsed once per recording and pair)
    it = c.items[0]
    p = dict(idx=0, path=it[0], pair=it[5])
    assert c.tables(p) is c.tables(p)


def test_refusals(tmp_path, tree):
    from sar_ssl_amd import locatads
    short = locatads.TdoaCorpus(cases.build_short(str(tmp_path / "short")), "train", sort=True)
    assert len(short) > 0
    with pytest.raises(ValueError, match="audio_array_benchmark2.wav.*too short"):
        short.plan(np.random.RandomState(0))
    with pytest.raises(ValueError, match="src_single_static"):
        locatads.TdoaCorpus(tree, "train", src_single_static=False)
    with pytest.raises(ValueError, match="VAD"):
        locatads.TdoaCorpus(tree, "train", load_vad=True)
    with pytest.raises(ValueError, match="dummy"):
        locatads.TdoaCorpus(tree, "train", arrays=("dummy",))
    with pytest.raises(ValueError, match="stage"):
        locatads.TdoaCorpus(tree, "pretrain")
    # an existing, non-empty stage directory: refused before anything else is looked at (no GPU is touched), by the function and the command
    out = tmp_path / "out"
    (out / "train").mkdir(parents=True)
    (out / "train" / "0.wav").write_bytes(b"x")
    with pytest.raises(FileExistsError, match="--overwrite"):
        locatads.generate(tree, str(out), "train", data_num=1)
    with pytest.raises(SystemExit):
        locatads.main(["--stage", "train", "--data-dir", tree, "--save-to", str(out)])
    locatads.check_save_dir(str(out / "train"), overwrite=True)
    locatads.check_save_dir(str(out / "val"), overwrite=False)
    for bad in (["--stage", "pretrain"], ["--fs", "8000"], ["--batch", "0"], ["--data-dir", str(tmp_path / "nowhere")]):
        with pytest.raises(SystemExit):
            locatads.main(bad + ([] if "--data-dir" in bad else ["--data-dir", tree]) + ["--save-to", str(tmp_path / "o2")])


def test_info_file_is_what_the_reference_writes_and_repeats_byte_for_byte(tmp_path):
    from sar_ssl_amd import locatads
    a, b = str(tmp_path / "a_info.npz"), str(tmp_path / "b_info.npz")
    locatads._write_info(a, np.float32(1.25e-4))
    locatads._write_info(b, np.float32(1.25e-4))
    info = np.load(a)
    assert info.files == ["TDOA"] and info["TDOA"].dtype == np.float32 and info["TDOA"].shape == () and info["TDOA"] == np.float32(1.25e-4)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_random_micsig_dataset_draws_reads_and_labels(tmp_path):
    """RandomMicSigDataset on a CPU device: the reference's two draws per item on the stream continued from numpy's global state, the
    files' samples scaled by 1 / 32768, Selecting's range of a longer simulated file, NaN labels for the LOCATA items."""
    import torch
    from sar_ssl_amd import dataset
    real, sim = str(tmp_path / "real_ds_locata"), str(tmp_path / "simu_ds" / "train")
    rpcm, rtdoa = cases.write_segments(real, "train", 5)
    spcm, sinfo = cases.write_simulated(os.path.join(sim, "R1"), 4)
    sel = [dataset.Selecting(select_range=[0, cases.NS])]
    for ratio, nlist in (([1, 1], 2), ([1, 0], 1), ([0, 1], 1)):
        dl = dataset.RandomMicSigDataset(real_sig_dir=real, sim_sig_dir=sim, real_sim_ratio=ratio, fs=16000, stage="train", load_anno=True,
                                         dataset_sz=7, transforms=sel, batch_size=3, device="cpu")
        assert len(dl) == 3 and len(dl.dataset_list) == nlist
        np.random.seed(77)
        got = list(dl)
        assert [g[0].shape[0] for g in got] == [3, 3, 1]
        rs = np.random.RandomState(77)
        k = 0
        for sig, lab in got:
            assert sig.dtype == torch.float32 and sig.shape[1:] == (cases.NS, 2) and sorted(lab) == sorted(dataset.TASKS)
            for j in range(sig.shape[0]):
                ds = dl.dataset_list[int(rs.randint(0, len(dl.dataset_list)))]
                idx = int(rs.randint(0, len(ds)))
                i = int(os.path.basename(str(ds.files[idx]))[:-4])
                if isinstance(ds, dataset.FixMicSigDatasetLOCATA):
                    assert np.array_equal(sig[j].numpy(), rpcm[i].astype(np.float32) / 32768.0)
                    assert lab["TDOA"][j] == rtdoa[i] and all(np.isnan(float(lab[t][j])) for t in ("T60", "DRR", "C50", "ABS"))
                    one = ds[idx]
                    assert np.array_equal(one[0], sig[j].numpy()) and one[1]["TDOA"] == rtdoa[i] and np.isnan(one[1]["T60"])
                else:
                    assert np.array_equal(sig[j].numpy(), spcm[i, :cases.NS].astype(np.float32) / 32768.0)
                    want = dataset.simulated_annos(sinfo[i])
                    assert all(float(lab[t][j]) == float(want[t]) for t in dataset.TASKS)
                k += 1
        assert k == 7
    # a 48 kHz file handed to the loader raises, by the batch reader and by the item reader
    bad = str(tmp_path / "bad")
    cases.write_segments(bad, "val", 2, fs=48000)
    dl = dataset.RandomMicSigDataset(real_sig_dir=bad, sim_sig_dir=[], real_sim_ratio=[1, 0], fs=16000, stage="val", load_anno=True,
                                     dataset_sz=2, transforms=sel, batch_size=2, device="cpu")
    with pytest.raises(Exception, match="48000"):
        list(dl)
    with pytest.raises(ValueError, match="48000 Hz"):
        dl.dataset_list[0][0]
    with pytest.raises(ValueError, match="no segments"):
        dataset.RandomMicSigDataset(real_sig_dir=bad, sim_sig_dir=[], real_sim_ratio=[1, 0], fs=16000, stage="test", load_anno=True,
                                    dataset_sz=2, transforms=sel, batch_size=2, device="cpu")
    with pytest.raises(ValueError, match="Selecting"):
        dataset.RandomMicSigDataset(real_sig_dir=real, sim_sig_dir=[], real_sim_ratio=[1, 0], fs=16000, stage="train", load_anno=True,
                                    dataset_sz=2, transforms=[lambda x: x], batch_size=2, device="cpu")


def test_parse_exits_without_the_corpus_and_returns_with_it(tmp_path):
    from sar_ssl_amd.opt import opt_downstream
    work = tmp_path / "work"
    work.mkdir()
    argv = ["--ds-train", "--ds-task", "TDOA", "--ds-real-sim-ratio", "1", "1", "--work-dir", str(work), "--time", "t0"]
    with pytest.raises(SystemExit) as e:
        opt_downstream().parse(argv)
    msg = str(e.value)
    corpus = str(work / "SAR-SSL" / "data" / "MicSig" / "real_ds_locata")
    assert "LOCATA" in msg and "RandomMicSigDataset" in msg and "gen_LOCATA.py --stage train val test" in msg and corpus in msg
    os.makedirs(os.path.join(corpus, "train"))                                                   # the directory alone is not a corpus
    with pytest.raises(SystemExit):
        opt_downstream().parse(argv)
    cases.write_segments(corpus, "train", 1, ns=64)
    opts = opt_downstream()
    a = opts.parse(argv)
    assert a.ds_setting["TDOA"]["num"] == 80000 and a.ds_setting["TDOA"]["bs_set"] == [16] and a.ds_setting["TDOA"]["lr_set"] == [0.001, 0.0001]
    assert a.ds_setting["TDOA"]["ntrial"] == 1 and a.ds_specifics == {"task": ["TDOA"], "data": "real_locata", "real_sim_ratio": [1, 1]}
    dirs = opts.dir()
    assert dirs["micsig_real"] == corpus and dirs["micsig_train_simu"] == str(work / "SAR-SSL" / "data" / "MicSig" / "simu_ds" / "train")
    assert "real_train1real1sim_valreal" in dirs["log_task_finetune"]
    # still refused: the test stage on real data, and TDOA next to a room-acoustics task
    with pytest.raises(SystemExit) as e:
        opt_downstream().parse(["--ds-test", "--ds-task", "TDOA", "--work-dir", str(work)])
    assert "--ds-test" in str(e.value) and "simulated" in str(e.value)
    with pytest.raises(SystemExit) as e:
        opt_downstream().parse(["--ds-train", "--ds-task", "TDOA", "T60", "--work-dir", str(work)])
    assert "T60" in str(e.value) and "one after the other" in str(e.value)
    a = opt_downstream().parse(["--ds-train", "--ds-task", "T60", "--work-dir", str(work)])      # the room-acoustics branch is untouched
    assert a.ds_specifics["data"] == "real_ace"


def test_abi_declares_and_exports_the_two_entries():
    import re
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read()
    names = set(re.findall(r"\b(sarssl_[a-z0-9_]+)\s*\(", hdr))
    assert {"sarssl_peak_scale", "sarssl_interp_mean", "sarssl_interp_mean_workspace_bytes"} <= names
    from sar_ssl_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        fn = lib.sarssl_interp_mean_workspace_bytes
        fn.restype = _lib.c_long
        assert fn(_lib.c_int(16)) == 16 * 32 and fn(_lib.c_int(0)) == -1 and fn(_lib.c_int(65536)) == -1
