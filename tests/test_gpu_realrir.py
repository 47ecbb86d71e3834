"""GPU: gen_real_rir.py --dataset ACE --data_type rir noise over the synthetic tree of tests/realrir_cases.py against fixture F25 (the
reference's own ACERIRDataset over the same tree, tools/make_golden_realrir.py): the file set, the RIR arrays at parity.RESAMPLE, the
direct-path indices, the labels, the noise cuts within one PCM-16 step, the zeros branch, and the written bank under RirSynthLoader.

DRR / C50 are held to parity.RIRLABELS' caps (1e-3 dB): its gates are for two f64 evaluations of the SAME RIR, while here the RIR itself
is the f32 resampler's, RESAMPLE's gate away from the reference's f64 one.  The command runs once for the module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import realrir_cases as cases
import simsig_cases as sc
from conftest import check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F25 = os.path.join(ROOT, "tests", "golden", "f25_realrir_ace.npz")
LABELS = ("T60fromDataset", "DRRfromDataset", "DRR", "C50", "ABS")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("ace"))
    cases.build_tree(os.path.join(root, "in"))
    save = os.path.join(root, "real")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_real_rir.py"), "--dataset", "ACE", "--data_type", "rir", "noise", "--fs", "16000",
                        "--nmic", "2", "--mic_dist_range", "0.03", "0.20", "--read_dir", os.path.join(root, "in"), "--save_dir", save],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(F25), root, save


def test_file_set_is_f25s(written):
    fx, _, save = written
    stems = [str(s) for s in fx["pairs"]]
    assert cases.tree_listing(os.path.join(save, "ACE")) == sorted([s + ".npy" for s in stems] + [s + "_info.npz" for s in stems])
    assert cases.tree_listing(os.path.join(save, "ACE_noise")) == [str(s) for s in fx["noise_files"]]


def test_rir_arrays_and_direct_path(written):
    from sar_ssl_amd import parity, realrir
    fx, root, save = written
    gate = min(parity.RESAMPLE["gate"], parity.RESAMPLE["ceiling"], parity.RESAMPLE["cap"])
    for array, (i, j) in cases.STORED_PAIRS.items():
        got = np.load(os.path.join(save, "ACE", "Office_2", array, "SP1_MP2-%d-%d.npy" % (i, j)))
        want = fx["rir/" + array]
        assert got.dtype == np.float32 and got.shape == want.shape == (1, 2, 1600, 1)
        check("realrir/rir/" + array, np.abs(got.astype(np.float64) - want).max() / np.abs(want).max(), gate)
    # the direct-path index of every channel of every file, by the same rule on the stored f32 values
    rows = iter(fx["dp"])
    for room in cases.ROOMS:
        for array, nch in cases.ARRAYS.items():
            pairs = realrir.selected_pairs(array)
            cover = {}                                  # microphone -> (a pair that holds it, its row in that pair)
            for idx in pairs:
                for k in (0, 1):
                    cover.setdefault(idx[k], (idx, k))
            assert sorted(cover) == list(range(nch))
            for pos in cases.POSITIONS:
                want = next(rows)
                for c, (idx, k) in cover.items():
                    r = np.load(os.path.join(save, "ACE", room, array, "SP1_MP%s-%d-%d.npy" % (pos, idx[0] + 1, idx[1] + 1)))[0, k, :, 0]
                    assert realrir.find_direct_path(r[:cases.FS // 160].astype(np.float64)) == want[c], (room, array, pos, c)


def test_labels(written):
    from sar_ssl_amd import parity
    fx, _, save = written
    worst = dict(drr=0.0, c50=0.0, other=0.0)
    for k, stem in enumerate(str(s) for s in fx["pairs"]):
        with np.load(os.path.join(save, "ACE", stem + "_info.npz")) as z:
            info = {key: z[key] for key in z.files}
        assert sorted(info) == [str(s) for s in fx["info_keys"]]
        room, array = stem.split("/")[:2]
        assert np.array_equal(info["mic_pos"], fx["mic_pos/" + array][fx["mic_idx"][k]]) and np.array_equal(info["room_sz"], fx["room_sz/" + room])
        assert int(info["fs"]) == cases.FS
        got, want = np.array([float(info[key]) for key in LABELS]), fx["labels"][k]
        worst["drr"] = max(worst["drr"], abs(got[2] - want[2]))
        worst["c50"] = max(worst["c50"], abs(got[3] - want[3]))
        worst["other"] = max(worst["other"], np.abs(got[[0, 1, 4]] / want[[0, 1, 4]] - 1.0).max())
    check("realrir/labels/drr_db", worst["drr"], parity.RIRLABELS["cap"]["drr"])
    check("realrir/labels/c50_db", worst["c50"], parity.RIRLABELS["cap"]["c50"])
    check("realrir/labels/other_rel", worst["other"], 1e-6)


def test_noise_cuts_and_the_zeros_branch(written):
    from sar_ssl_amd import parity
    from sar_ssl_amd.dataset import read_wav_pcm16
    fx, _, save = written
    share = 2 * parity.RESAMPLE["gate"] * 32767          # a sample can differ only within the gate of a rounding boundary (peak <= 1)
    for array, (i, j) in cases.STORED_PAIRS.items():
        for typ in cases.NOISE_TYPES:
            pcm, fs = read_wav_pcm16(os.path.join(save, "ACE_noise", "Office_2", array, "_MP2-%d-%d_%s.wav" % (i, j, typ)))
            want = fx["noise/%s/%s" % (array, typ)]
            assert fs == cases.FS and pcm.shape == want.shape == (4000, 2)
            diff = np.abs(pcm.astype(np.int32) - want)
            assert diff.max() <= 1 and (diff != 0).mean() <= share, (array, typ, diff.max(), (diff != 0).mean())
    assert len(fx["noise_zero"]) == 3
    for rel in fx["noise_zero"]:
        pcm, fs = read_wav_pcm16(os.path.join(save, "ACE_noise", str(rel)))
        assert fs == cases.FS and pcm.shape == (5 * cases.FS, 2) and not pcm.any()


def test_loader_renders_a_batch_from_the_written_bank(written, tmp_path_factory):
    from sar_ssl_amd import rirsynth
    _, _, save = written
    src_dir = sc.write_speech_tree(tmp_path_factory.mktemp("speech"), np.load(sc.F22))
    bank = rirsynth.MeasuredBank([os.path.join(save, "ACE", "Office_2", a) for a in ("Chromebook", "Mobile", "Lin8Ch")], fs=cases.FS, sort=True)
    assert bank.nch == 2 and len(bank) == 2 * (1 + 3 + 18) and all(len(n) == 2 for n in bank.noise_files)
    sources = rirsynth.SourceBank(os.path.join(src_dir, "tr"), fs=cases.FS, sort=True)
    np.random.seed(1)
    T = 0.2                                             # the noise cuts are 0.25 s long
    ld = rirsynth.RirSynthLoader(bank, None, sources, dataset_sz=4, batch_size=4, T=T, fs=cases.FS, nmic=2, real_sim_ratio=(1, 0), seed=1,
                                 device="cuda:0")
    sig, labels = next(iter(ld))
    torch.cuda.synchronize()
    assert sig.shape == (4, int(T * cases.FS), 2) and bool(torch.isfinite(sig).all()) and 0 < float(sig.abs().max()) <= 1.0
    assert set(labels) >= {"T60", "DRR", "C50", "ABS"}
