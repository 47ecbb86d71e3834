"""GPU: real-data pretraining end to end over the synthetic trees of tests/realsig_cases.py - gen_sig_from_real_rir.py's generator against
realsig.restate_item (parity.SIMSIG), realsig.RealMixLoader against its host plan, its files and hip.resample_poly of its crops, and
``run_pretrain.py --pretrain`` without ``--simu-exp`` over corpora the generator wrote.  The generator runs once for the module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import realsig_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu
DATA_NUM, BATCH = 8, 3                                       # a ragged last batch


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("realsig"))
    return dict(cases.build_all(root), root=root)


def _main(tree, save, stage, names, batch=BATCH, data_num=DATA_NUM):
    from sar_ssl_amd import realsig
    return realsig.main(["--stage", stage, "--dataset"] + names + ["--T", str(cases.T), "--src_dir", tree["src"], "--rir_dir", tree["rir"],
                         "--save_dir", save, "--data_num", str(data_num), "--batch", str(batch)])


@pytest.fixture(scope="module")
def generated(tree, tmp_path_factory):
    save = str(tmp_path_factory.mktemp("micsig_real"))
    assert _main(tree, save, "pretrain", ["DCASE", "ACE"]) == 0
    assert _main(tree, save, "preval", ["DCASE"]) == 0
    return save


def _banks(tree, stage, name):
    from sar_ssl_amd import realsig, rirsynth
    bank = rirsynth.MeasuredBank(realsig.rir_dirs(tree["rir"], stage, name), cases.FS)          # (the command's listing order: the file system's)
    return bank, rirsynth.SourceBank(tree["src"] + "/" + realsig.SRC_SUBDIR[stage], cases.FS)


@pytest.mark.parametrize("stage,name", cases.COMBOS)
def test_generated_files_against_the_restatement(tree, generated, stage, name):
    from sar_ssl_amd import parity, realsig
    from sar_ssl_amd.dataset import read_wav_pcm16
    out_dir = os.path.join(generated, stage, name)
    assert sorted(os.listdir(out_dir)) == sorted("%d.wav" % i for i in range(DATA_NUM))          # no info files, no direct-path files
    bank, sources = _banks(tree, stage, name)
    plans = realsig.plan_items(range(DATA_NUM), realsig.dataset_seed(stage, name), bank, sources, cases.T, cases.FS, cases.SNR_RANGE)
    assert len({p["rir_idx"] for p in plans}) > 1 and len({bank.rirs[p["rir_idx"]].shape[1] for p in plans}) > 1     # RIRs of different lengths
    if name == "ACE":
        assert 0 < sum(p["noise_file"] is not None for p in plans) < DATA_NUM
    else:
        assert all(p["noise_file"] is None for p in plans)                                  # a bank without noise cuts
    if stage == "preval":
        assert all(os.sep + "tb103" + os.sep in str(p["rir_file"]) for p in plans)
    step, share = 0, 0.0
    for i, p in enumerate(plans):
        pcm, fs = read_wav_pcm16(os.path.join(out_dir, "%d.wav" % i))
        want = realsig.restate_item(p, bank)
        assert fs == cases.FS and pcm.shape == want.shape == (cases.NS, cases.NMIC)
        d = np.abs(pcm.astype(np.int32) - want)
        step, share = max(step, int(d.max())), max(share, float(np.mean(d != 0)))
    print("SIMSIG realsig/%s/%s: max step %d (bound %d), largest share of differing samples %.3e (bound %.3e)"
          % (stage, name, step, parity.SIMSIG["pcm_step"], share, parity.SIMSIG["share_bound"]))
    assert step <= parity.SIMSIG["pcm_step"] and share <= parity.SIMSIG["share_bound"]


def test_a_second_run_writes_the_same_bytes(tree, generated, tmp_path):
    save = str(tmp_path / "again")
    assert _main(tree, save, "pretrain", ["ACE"]) == 0
    for i in range(DATA_NUM):
        a, b = (open(os.path.join(d, "pretrain", "ACE", "%d.wav" % i), "rb").read() for d in (generated, save))
        assert a == b, i
    assert _main(tree, save, "pretrain", ["ACE"], batch=5) == 0                              # over existing files, without a prompt;
    for i in range(DATA_NUM):                                                                # a file does not depend on the batch it was in
        a, b = (open(os.path.join(d, "pretrain", "ACE", "%d.wav" % i), "rb").read() for d in (generated, save))
        assert a == b, i


def test_the_staged_writer_reuses_both_buffers_and_writes_a_ragged_last_batch(tree, generated, tmp_path):
    """pipeline.StagedWriter under the generator: 7 items in batches of 2 are four batches, so each pinned buffer is staged twice and the
    last batch fills the dense prefix of one row; every file equals, byte for byte, the one the module's run wrote at batch 3."""
    save = str(tmp_path / "staged")
    assert _main(tree, save, "pretrain", ["ACE"], batch=2, data_num=7) == 0
    out_dir = os.path.join(save, "pretrain", "ACE")
    assert sorted(os.listdir(out_dir)) == sorted("%d.wav" % i for i in range(7))              # all seven, and no *.tmp left behind
    assert not [f for _, _, files in os.walk(save) for f in files if f.endswith(".tmp")]
    for i in range(7):
        a, b = (open(os.path.join(d, "pretrain", "ACE", "%d.wav" % i), "rb").read() for d in (generated, save))
        assert a == b, i


def test_loader_items_equal_their_files_their_crops_and_the_host_plan(tree, generated):
    from sar_ssl_amd import hip, realsig
    from sar_ssl_amd.dataset import read_wav_pcm16
    corpora = [realsig.FixedCorpus(os.path.join(generated, "pretrain", "ACE"), "train", sort=True),
               realsig.RecordingCorpus(tree["locata"], cases.T, cases.FS, "train", sort=True)]
    loader = realsig.RealMixLoader(corpora, [1, 1], 12, 4, cases.T, cases.FS, device="cuda")
    np.random.seed(3)
    plans = [p for b in loader.plan_batches() for p in b]
    np.random.seed(3)
    batches = [b for b in loader]
    assert len(batches) == 3 and all(len(b) == 1 and b[0].shape == (4, cases.NS, 2) and b[0].dtype == torch.float32 and b[0].is_cuda for b in batches)
    torch.cuda.synchronize()
    got = torch.cat([b[0] for b in batches]).cpu().numpy()
    kinds = [p["kind"] for p in plans]
    assert kinds.count("fixed") >= 2 and kinds.count("recording") >= 2 and any(len(set(kinds[k:k + 4])) == 2 for k in (0, 4, 8))
    branches = set()
    for i, p in enumerate(plans):
        if p["kind"] == "fixed":
            pcm, _ = read_wav_pcm16(p["path"])
            assert p["path"] == corpora[0].files[p["ins"]] and np.array_equal(got[i], pcm.astype(np.float32) / np.float32(32768.0)), i
        else:
            crop = corpora[1].read(p)
            assert crop.dtype == np.int16 and crop.shape == (p["want"], 2)
            alone = hip.resample_poly(torch.from_numpy(crop).cuda(), cases.FS, p["fs"]).cpu().numpy()
            assert np.array_equal(got[i].view(np.uint8), alone.view(np.uint8)), i
            branches.add(p["read"][0] > 0)
    assert branches                                                                         # (which crops the seed reaches is the plan's business)


T_FULL = 4.112                                               # the command line's item length: 65 792 samples, 197 376 at 48 kHz


def test_run_pretrain_real_branch_entry_point(tree, tmp_path):
    """`run_pretrain.py --pretrain --gpu-id 0,` (no --simu-exp): one epoch of two steps and one validation batch over a LOCATA-shaped
    recording and DCASE corpora the generator wrote at the command line's item length; scalars, a checkpoint, and the lines that say
    which of the reference's 13 + 5 corpora were left out, and why."""
    from sar_ssl_amd import realsig
    work = tmp_path / "work"
    save = str(work / "SAR-SSL" / "data" / "MicSig" / "real")
    for stage, n in (("pretrain", 8), ("preval", 4)):
        assert realsig.main(["--stage", stage, "--dataset", "DCASE", "--T", str(T_FULL), "--src_dir", tree["src"], "--rir_dir", tree["rir"],
                             "--save_dir", save, "--data_num", str(n), "--batch", "4"]) == 0
    os.makedirs(str(work / "data" / "MicSig"))
    os.rename(cases.build_locata(str(tmp_path), (("eval", 1, "recording1", "dicit", 15, 200000),)), str(work / "data" / "MicSig" / "LOCATA"))
    cmd = [sys.executable, os.path.join(ROOT, "run_pretrain.py"), "--pretrain", "--gpu-id", "0,", "--work-dir", str(work), "--bs", "4", "4", "4",
           "--nepoch", "1", "--workers", "2", "--time", "t0", "--data-num", "8", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logd = work / "SAR-SSL" / "exp" / "pretrain" / "t0"
    recs = [json.loads(l) for l in open(logd / "scalars.jsonl").read().strip().splitlines()]
    assert len(recs) == 1 and recs[0]["epoch"] == 1 and recs[0]["lr"] == 0.0001
    assert all(np.isfinite(recs[0][k]) for k in ("loss_train", "diff_train", "loss_val_real", "diff_val_real")) and "loss_val" not in recs[0]
    assert (logd / "latest_model.tar").exists() and (logd / "best_model.tar").exists() and (logd / "config.json").exists()
    lines = [l for l in r.stdout.splitlines() if "left out of the reference's" in l]
    assert len(lines) == 2 and lines[0].startswith("train corpora: LOCATA, DCASE (weights [1, 5])") and "reference's 13" in lines[0]
    assert all(n + " (not built)" in lines[0] for n in ("MCWSJ", "LibriCSS", "AMI", "AISHELL4", "M2MeT", "RealMAN"))
    assert all(n + " (not on disk)" in lines[0] for n in ("MIR", "Mesh", "ACE", "dEchorate", "BUTReverb"))
    assert lines[1].startswith("val corpora: DCASE (weights [2])") and "reference's 5" in lines[1] and "BUTReverb (not on disk)" in lines[1]
    assert all(n + " (not built)" in lines[1] for n in ("AISHELL4", "M2MeT", "RealMAN"))
