"""CPU: the host side of real-data pretraining (sar_ssl_amd/realsig.py) against fixture F26 - the reference's own MicSigFromRIRDataset,
LOCATADataset and RandomRealDataset over the synthetic trees of tests/realsig_cases.py (tools/make_golden_realpretrain.py): the generator's
host plan and its f64 restatement, RecordingCorpus' item list, probabilities, draws and crops, RealMixLoader's item sequence, the
directories of opt_pretrain and the refusals of the two command lines.  Listings are sorted on both sides (sort=True)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401
import realsig_cases as cases  # noqa: E402

F26 = os.path.join(ROOT, "tests", "golden", "f26_realpretrain.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(F26)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("realsig"))
    return dict(cases.build_all(root), root=root)


def _rel(tree, path):
    return "" if path is None else os.path.relpath(str(path), tree["root"])


def _generator_inputs(tree, stage, name):
    from sar_ssl_amd import realsig, rirsynth
    bank = rirsynth.MeasuredBank(realsig.rir_dirs(tree["rir"], stage, name), cases.FS, sort=True)
    sources = rirsynth.SourceBank(tree["src"] + "/" + realsig.SRC_SUBDIR[stage], cases.FS, sort=True)
    return bank, sources


def test_seeds_counts_and_splits():
    from sar_ssl_amd import realsig
    for i, name in enumerate(("DCASE", "MIR", "Mesh", "dEchorate", "BUTReverb", "ACE")):
        assert realsig.dataset_seed("pretrain", name) == int(1 + i * 10e6)
        assert realsig.dataset_seed("preval", name) == int(2e6 + i * 10e6)
    assert realsig.SIG_NUM == {"pretrain": 102400, "preval": 2560}
    assert realsig.rir_dirs("R", "preval", "DCASE") == ["R/DCASE/tb103", "R/DCASE/se203"]
    assert len(realsig.rir_dirs("R", "pretrain", "DCASE")) == 7 and len(realsig.rir_dirs("R", "pretrain", "BUTReverb")) == 8
    assert realsig.rir_dirs("R", "preval", "BUTReverb") == ["R/BUTReverb/VUT_FIT_E112"]
    for name in ("MIR", "Mesh", "dEchorate", "ACE"):
        assert realsig.rir_dirs("R", "pretrain", name) == ["R/" + name]
        with pytest.raises(ValueError, match="args.stage == 'pretrain'"):
            realsig.rir_dirs("R", "preval", name)


@pytest.mark.parametrize("stage,name", cases.COMBOS)
def test_generator_plan_reproduces_every_recorded_draw_and_the_restatement_the_output(fx, tree, stage, name):
    from sar_ssl_amd import parity, realsig
    bank, sources = _generator_inputs(tree, stage, name)
    pre = "gen/%s/%s/" % (stage, name)
    assert [_rel(tree, f) for f in bank.files] == [str(f) for f in fx[pre + "rir_files"]]
    assert sources.spk_ids == [str(s) for s in fx[pre + "speakers"]]
    seed = realsig.dataset_seed(stage, name)
    assert seed == int(fx[pre + "seed"])
    plans = realsig.plan_items(range(cases.GEN_ITEMS), seed, bank, sources, cases.T, cases.FS, cases.SNR_RANGE)
    worst, noisy = 0.0, 0
    for i, p in enumerate(plans):
        k = pre + "%d/" % i
        assert _rel(tree, p["rir_file"]) == str(fx[k + "rir_file"])
        assert _rel(tree, p["noise_file"]) == str(fx[k + "noise_file"]) and p["noise_start"] == int(fx[k + "noise_start"])
        assert p["src_idx"] == int(fx[k + "src_idx"]) and p["utt_idx"] == int(fx[k + "utt_idx"]) and p["crop_start"] == int(fx[k + "crop_start"])
        assert [_rel(tree, f) for f in p["utt_files"]] == [str(f) for f in fx[k + "utt_files"]]
        assert p["snr"] == float(fx[k + "snr"])
        noisy += p["noise_file"] is not None
        got, want = realsig.restate_item(p, bank, pcm=False), fx[k + "out"].astype(np.float64)
        assert got.shape == want.shape == (cases.NS, cases.NMIC)
        err = float(np.abs(got - want).max())                 # outputs are peak-normalised to 0.9: of full scale
        worst = max(worst, err)
        assert np.array_equal(realsig.restate_item(p, bank), np.clip(np.rint(got * 32767.0), -32767, 32767).astype(np.int16))
    print("PARITY realsig/restatement_vs_f26/%s/%s measured=%.3e tol=%.3e" % (stage, name, worst, parity.RIRMIX["restatement_vs_f20"]))
    assert worst <= parity.RIRMIX["restatement_vs_f20"]
    if (stage, name) == ("pretrain", "ACE"):
        assert 0 < noisy < cases.GEN_ITEMS                    # both kinds of item: with a noise cut and without
    if stage == "preval":
        assert all("/tb103/" in _rel(tree, p["rir_file"]) for p in plans)


def test_share_bound_is_a_condition_the_restatement_alone_meets(fx, tree):
    """parity.SIMSIG['share_bound'] caps the share of samples of a generated file that may differ from restate_item at all.  The cap is
    a condition on the inputs: the f64 restatement, moved by the mix gate in either direction, changes no more samples than that."""
    from sar_ssl_amd import parity, realsig
    from sar_ssl_amd.roomsim import pcm16
    gate = parity.RIRMIX["gate"]
    for stage, name in cases.COMBOS:
        bank, sources = _generator_inputs(tree, stage, name)
        for p in realsig.plan_items(range(8), realsig.dataset_seed(stage, name), bank, sources, cases.T, cases.FS, cases.SNR_RANGE):
            y = realsig.restate_item(p, bank, pcm=False)
            for moved in (y + gate, y - gate):
                d = pcm16(moved).astype(np.int64) - pcm16(y)
                assert np.abs(d).max() <= parity.SIMSIG["pcm_step"] and np.mean(d != 0) <= parity.SIMSIG["share_bound"]


def _corpus(tree, stage, T=cases.T):
    from sar_ssl_amd import realsig
    return realsig.RecordingCorpus(tree["locata"], T, cases.FS, stage, sort=True)


@pytest.mark.parametrize("stage", ["train", "test", "val"])
def test_recording_corpus_items_and_probabilities(fx, tree, stage):
    c = _corpus(tree, stage)
    pre = "locata/%s/" % stage
    assert [_rel(tree, p) for p, _ in c.items] == [str(s) for s in fx[pre + "items"]]
    assert np.array_equal(np.array([pair for _, pair in c.items], np.int16).reshape(-1, 2), fx[pre + "pairs"])
    want = fx[pre + "cumsum"]
    assert c.cumsum.dtype == np.float32 and c.cumsum.tobytes() == want.tobytes()
    if stage == "val":
        assert len(c) == 0
    else:
        assert c.cumsum[-1] == 1 and not any("dummy" in p or "recording2" in p for p, _ in c.items)


def test_microphone_pairs_are_permutations_on_the_reference_tables():
    from sar_ssl_amd import realsig
    for array, nch in (("dicit", 15), ("benchmark2", 12), ("eigenmike", 32)):
        assert realsig.LOCATA_MIC_POS[array].shape == (nch, 3)
        pairs = realsig.select_pairs(realsig.LOCATA_MIC_POS[array])
        assert all((j, i) in pairs for i, j in pairs) and len(pairs) % 2 == 0
    em = realsig.LOCATA_MIC_POS["eigenmike"]
    assert np.array_equal(em[7], em[5]) and (5, 7) not in realsig.select_pairs(em)         # (sic) the repeated capsule: distance 0


@pytest.mark.parametrize("stage,tag,T,seed", [("train", "", cases.T, cases.LOCATA_SEED), ("train", "long/", cases.T_LONG, cases.LOCATA_SEED + 1),
                                              ("test", "", cases.T, cases.LOCATA_SEED), ("test", "long/", cases.T_LONG, cases.LOCATA_SEED + 1)])
def test_recording_corpus_draws_and_crops(fx, tree, stage, tag, T, seed):
    from sar_ssl_amd import parity, realrir
    c = _corpus(tree, stage)
    c.T = T                                                   # as the fixture does: the list is T's, the crop T_LONG's
    rs = np.random.RandomState(seed)
    branches = set()
    for i in range(cases.LOCATA_ITEMS):
        k = "locata/%s/%s%d/" % (stage, tag, i)
        p = c.plan(rs)
        assert p["idx"] == int(fx[k + "idx"])
        drawn = int(fx[k + "start"])
        nsample = c.header(p["path"])[2]
        branch = "shorter" if p["repeat"] > 1 else ("equal" if drawn < 0 else "longer")
        branches.add(branch)
        assert p["start"] == (0 if branch == "equal" else drawn) and p["read"][0] == int(fx[k + "row0"])
        crop = c.read(p)
        assert crop.dtype == np.int16 and crop.shape == (int(T * cases.FS_REC), 2)
        if branch == "shorter":
            assert nsample < p["want"] and p["repeat"] == 2
        if k + "out" in fx.files:
            want = fx[k + "out"].astype(np.float64)
            got = realrir.restate_resample(crop.astype(np.float32) / np.float32(32768.0), 1, 3)
            assert np.array_equal(got, c.restate(p)) and got.shape == want.shape == (int(T * cases.FS), 2)
            err = float(np.abs(got - want).max() / np.abs(want).max())
            print("PARITY realsig/crop_vs_f26/%s%s%d measured=%.3e tol=%.3e" % (stage, tag, i, err, parity.RESAMPLE["ceiling"]))
            assert err <= parity.RESAMPLE["ceiling"]
    if tag:
        assert branches == {"shorter"}
    elif stage == "train":
        assert branches == {"longer", "equal"}


@pytest.mark.parametrize("fmt,extensible", [("pcm24", False), ("float32", True)])
def test_a_recording_that_is_not_pcm16_is_probed_from_its_header_and_cropped_as_f32(tmp_path, fmt, extensible):
    import realrir_cases
    from sar_ssl_amd import realsig
    x = np.clip(np.random.RandomState(8).standard_normal((15000, 15)) * 0.2, -0.99, 0.99)
    path = tmp_path / "eval" / "task1" / "recording1" / "dicit" / "audio_array_dicit.wav"
    path.parent.mkdir(parents=True)
    back = realrir_cases.write_wav(str(path), x, cases.FS_REC, fmt, extensible)
    assert realsig.wav_header(str(path)) == (15, cases.FS_REC, 15000, False)
    c = realsig.RecordingCorpus(str(tmp_path), cases.T, cases.FS, "train", sort=True)
    assert len(c) == len(c.pairs["dicit"]) and c.cumsum[-1] == 1
    p = c.plan(np.random.RandomState(1))
    crop = c.read(p)
    assert crop.dtype == np.float32 and crop.shape == (int(cases.T * cases.FS_REC), 2)
    assert np.array_equal(crop, back[p["start"]:p["start"] + p["want"]][:, list(p["pair"])].astype(np.float32))
    assert c.restate(p).shape == (cases.NS, 2)


def test_mix_loader_plan_reproduces_the_dataset_and_instance_sequence(fx, tree):
    from sar_ssl_amd import realsig
    dirs = cases.mix_dirs(tree)
    names, corpora, w, dropped = realsig.build_mix(cases.MIX_LIST, cases.MIX_PROBS, dirs, "train", cases.T, cases.FS, sort=True)
    assert names == list(cases.MIX_LIST) and not dropped and [len(c) for c in corpora] == [int(n) for n in fx["mix/len"]]
    assert not any(f.endswith("_dp.wav") for f in corpora[1].files)
    loader = realsig.RealMixLoader(corpora, w, cases.MIX_ITEMS, 5, cases.T, cases.FS, device="cpu")
    assert loader.cumsum.tobytes() == fx["mix/cumsum"].tobytes() and len(loader) == 7
    np.random.seed(cases.MIX_SEED)
    plans = [p for batch in loader.plan_batches() for p in batch]
    assert len(plans) == cases.MIX_ITEMS
    seq = fx["mix/sequence"]
    for p, (d, ins, idx, start) in zip(plans, seq):
        assert (p["dataset"], p["ins"]) == (d, ins)
        if p["kind"] == "recording":
            assert p["idx"] == idx and (start < 0 or p["start"] == start)
        else:
            assert p["path"] == corpora[d].files[ins]
    assert {p["kind"] for p in plans} == {"fixed", "recording"}
    np.random.seed(cases.MIX_SEED)                            # the plan continues numpy's global state and leaves it alone
    again = [p for batch in loader.plan_batches() for p in batch]
    assert [(p["dataset"], p["ins"]) for p in again] == [(p["dataset"], p["ins"]) for p in plans]


def test_build_mix_reduces_the_reference_lists_and_says_why(tree):
    from sar_ssl_amd import realsig
    from sar_ssl_amd.opt import opt_pretrain
    assert len(realsig.TRAIN_LIST) == len(realsig.TRAIN_PROBS) == 13 and realsig.TRAIN_PROBS == (1, 5, 5, 8, 8, 8, 15, 5, 5, 5, 5, 5, 5)
    assert realsig.VAL_LIST == ("AISHELL4", "M2MeT", "RealMAN", "DCASE", "BUTReverb") and realsig.VAL_PROBS == (1, 2, 5, 2, 1)
    dirs = dict(opt_pretrain().dir()["micsig_real_pretrain"], **cases.mix_dirs(tree))
    lines = []
    names, corpora, w, dropped = realsig.build_mix(realsig.TRAIN_LIST, realsig.TRAIN_PROBS, dirs, "train", cases.T, sort=True, log=lines.append)
    assert names == ["LOCATA", "DCASE", "ACE"] and w == [1, 5, 5]
    d = dict(dropped)
    assert all(d[n] == "not built" for n in ("MCWSJ", "LibriCSS", "AMI", "AISHELL4", "M2MeT", "RealMAN"))
    assert all(d[n] == "not on disk" for n in ("MIR", "Mesh", "dEchorate", "BUTReverb")) and len(d) == 10
    assert len(lines) == 1 and "MCWSJ (not built)" in lines[0] and "Mesh (not on disk)" in lines[0]


def test_opt_pretrain_directories_of_the_real_branch(fx):
    from sar_ssl_amd.opt import opt_pretrain
    o = opt_pretrain()
    o.parse(["--pretrain", "--gpu-id", "0,", "--work-dir", "/tmp/w"])
    d = o.dir()
    for k in ("micsig_real_pretrain", "micsig_real_preval", "micsig_real_pretest"):
        want = json.loads(str(fx["dirs/" + k]))
        assert d[k] == {n: "/tmp/w/" + v for n, v in want.items()}
    assert d["micsig_real_pretrain"]["LOCATA"] == "/tmp/w/data/MicSig/LOCATA"
    assert d["micsig_real_preval"]["DCASE"] == "/tmp/w/SAR-SSL/data/MicSig/real/preval/DCASE"


def _no_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was touched"))


@pytest.mark.parametrize("extra,word", [(["--stage", "preval", "--dataset", "ACE"], "args.stage == 'pretrain'"),
                                        (["--dataset", "Nowhere"], "Dataset not found"),
                                        (["--dataset", "DCASE", "--fs", "8000"], "--fs 8000")])
def test_generator_command_line_refusals(tree, tmp_path, monkeypatch, capsys, extra, word):
    from sar_ssl_amd import realsig
    _no_gpu(monkeypatch)
    save = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        realsig.main(extra + ["--src_dir", tree["src"], "--rir_dir", tree["rir"], "--save_dir", str(save)])
    assert e.value.code != 0 and word in capsys.readouterr().err and not save.exists()


def test_generator_refuses_a_bank_at_another_rate_and_a_moving_source(tree, tmp_path, monkeypatch, capsys):
    import shutil
    from sar_ssl_amd import realsig
    _no_gpu(monkeypatch)
    for what, word in (("fs", "another rate"), ("npoint", "npoint != 1")):
        rir = tmp_path / what / "rir"
        shutil.copytree(tree["rir"], str(rir))
        stem = str(rir / "ACE" / "Lobby" / "Lin8Ch" / "SP1_MP1-1-2")
        if what == "fs":
            info = dict(np.load(stem + "_info.npz"))
            np.savez(stem + "_info.npz", **dict(info, fs=np.array(48000)))
        else:
            np.save(stem + ".npy", np.repeat(np.load(stem + ".npy"), 2, axis=0))
        save = tmp_path / what / "out"
        with pytest.raises(SystemExit) as e:
            realsig.main(["--dataset", "ACE", "--src_dir", tree["src"], "--rir_dir", str(rir), "--save_dir", str(save)])
        assert e.value.code != 0 and word in capsys.readouterr().err and not save.exists()


def test_run_pretrain_real_branch_refusals(tmp_path, monkeypatch):
    import sar_ssl_amd.run_pretrain as rp
    from sar_ssl_amd import launch
    _no_gpu(monkeypatch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(launch, "spawn_ranks", lambda *a, **k: pytest.fail("a rank was spawned"))
    work = tmp_path / "w"
    with pytest.raises(SystemExit) as e:
        rp.main(["--pretrain", "--gpu-id", "0,1", "--work-dir", str(work), "--time", "t0"])
    assert "one GPU" in str(e.value)
    (work / "data" / "MicSig" / "LOCATA").mkdir(parents=True)                               # an empty corpus directory
    with pytest.raises(SystemExit) as e:
        rp.main(["--pretrain", "--gpu-id", "0,", "--work-dir", str(work), "--time", "t0"])
    msg = str(e.value)
    assert str(work / "data" / "MicSig" / "LOCATA") in msg and str(work / "SAR-SSL" / "data" / "MicSig" / "real" / "pretrain" / "ACE") in msg
    assert "gen_sig_from_real_rir.py" in msg and "gen_real_rir.py" in msg and not (work / "SAR-SSL" / "exp").exists()
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)                          # (past the no-GPU exit, to the one that is pinned)
    for stage in ("--test", "--pretrain-frozen-encoder"):                                  # unchanged: these stay simulated-only
        with pytest.raises(SystemExit) as e:
            rp.main([stage, "--gpu-id", "0,", "--work-dir", str(work), "--time", "t0"])
        assert "are implemented on this path" in str(e.value)


def test_abi_declares_the_batch_entries():
    import re
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read()
    names = set(re.findall(r"\b(sarssl_[a-z0-9_]+)\s*\(", hdr))
    assert {"sarssl_resample_poly_batch", "sarssl_resample_poly_batch_supported"} <= names
    from sar_ssl_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        assert hasattr(lib, "sarssl_resample_poly_batch") and hasattr(lib, "sarssl_resample_poly_batch_supported")
        assert lib.sarssl_resample_poly_batch_supported(4, 15, 1, 3) == 1 and lib.sarssl_resample_poly_batch_supported(65535, 32, 160, 441) == 1
        for bad in ((0, 2, 1, 3), (65536, 2, 1, 3), (4, 33, 1, 3), (4, 2, 2, 6), (4, 2, 442, 1)):
            assert lib.sarssl_resample_poly_batch_supported(*bad) == 0
