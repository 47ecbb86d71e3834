"""GPU: the per-room generator (gen_simu_certain_room.py; roomsim.simulate_room_signals / simulate_room_bank) and its kernel -
sarssl_mixing_table against rirsynth.mixing_table (parity.MIXTABLE), the written files against the f64 restatement roomsim.restate_sig
(parity.SIMSIG) for both noise types, batch independence across rooms, the bank as input of rirsynth.SimulatedBank, and the generated
tree as input of ``run_downstream.py --ds-train --simu-exp``."""
import json
import os

import numpy as np
import pytest
import torch

import certainroom_cases as cc
import simsig_cases as sc
from conftest import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 4000000                                                  # stage train


# ---------------------------------------------------------------------------------------------------------------- the table kernel
def test_mixing_table_against_the_host_table():
    from sar_ssl_amd import hip, parity
    tol = min(parity.MIXTABLE["gate"], parity.MIXTABLE["cap"])
    assert tol <= 2.0 ** -22
    worst = 0.0
    for name, mic in cc.table_batches():
        want = cc.host_tables(mic)
        got = hip.mixing_table(torch.from_numpy(mic).to(DEV), float(cc.FS), 343.0).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), name
        assert not got[:, 0].any() and not np.tril(got, -1).any(), name             # row 0 and below the diagonal: exactly zero
        d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print("PARITY mixtable.%s measured=%.3g tol=%.3g" % (name, d, tol))
        worst = max(worst, d)
    print("PARITY mixtable.max measured=%.3e tol=%.3e (at most)" % (worst, tol))
    assert worst <= tol, (worst, tol)


def test_mixing_table_takes_fs_and_c_as_arguments():
    from sar_ssl_amd import hip, rirsynth
    mic = cc.geometries()["pair_20cm"][None]
    got = hip.mixing_table(torch.from_numpy(mic).to(DEV), 8000.0, 340.0).cpu().numpy()
    want = rirsynth.mixing_table(mic[0], 8000, 340.0).astype(np.float32)
    assert np.abs(got[0].astype(np.float64) - want).max() <= 2.0 ** -22
    assert np.abs(want - cc.host_tables(mic)[0]).max() > 1e-2


def test_mixing_table_refuses_nine_microphones_and_leaves_the_output_untouched():
    from sar_ssl_amd import _lib, hip
    mic = torch.from_numpy(np.arange(27, dtype=np.float64).reshape(1, 9, 3) * 0.1).to(DEV)
    out = torch.full((1, 129, 9, 9), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.SarsslHipError, match="1 to 8 microphones"):
        hip.mixing_table(mic, out=out)
    rc = _lib.lib().sarssl_mixing_table(_lib.c_void_p(mic.data_ptr()), _lib.c_int(1), _lib.c_int(9), _lib.c_double(16000.0), _lib.c_double(343.0),
                                        _lib.c_void_p(out.data_ptr()), _lib.c_void_p(0))
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 7.0).all())


def test_coincident_microphones_give_nan_for_that_item_only():
    import scipy.linalg
    from sar_ssl_amd import hip, rirsynth
    geo = cc.geometries()
    twice = np.array([[1.0, 2.0, 1.5], [1.0, 2.0, 1.5]])      # G = [[1, 1], [1, 1]]: the second pivot is 1 - 1 * 1, an exact zero on both sides
    mic = np.stack([geo["pair_3cm"] + 1.0, twice, geo["pair_20cm"][::-1].copy()])
    with pytest.raises(scipy.linalg.LinAlgError):
        rirsynth.mixing_table(twice)
    got = hip.mixing_table(torch.from_numpy(mic).to(DEV)).cpu().numpy()
    assert not got[1, 0].any() and np.isnan(got[1, 1:]).all()
    want = cc.host_tables(mic[[0, 2]])
    from sar_ssl_amd import parity
    assert np.isfinite(got[[0, 2]]).all() and np.abs(got[[0, 2]].astype(np.float64) - want).max() <= min(parity.MIXTABLE["gate"], parity.MIXTABLE["cap"])


# ---------------------------------------------------------------------------------------------------------------- the generator
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return sc.write_speech_tree(tmp_path_factory.mktemp("speech"), np.load(sc.F22))


@pytest.fixture(scope="module")
def plans(tree):
    return cc.room_plans(tree)


def _simulate(tmp, tree, noise_type="diffuse_white", batch=8, noise="numpy", stage="train", rooms=cc.ROOMS, rirs=cc.RIRS, sigs=cc.SIGS,
              T=cc.T_SMALL):
    from sar_ssl_amd import roomsim
    lines = []
    res = roomsim.simulate_room_signals(str(tmp), stage, rooms, rirs, sigs, tree, noise_type, device=DEV, noise=noise, batch=batch, T=T,
                                        sort_sources=True, log=lines.append, **cc.SMALL)
    return res, lines


def _against_restatement(name, wav, want):
    from sar_ssl_amd import parity
    from sar_ssl_amd.dataset import read_wav_pcm16
    pcm, fs = read_wav_pcm16(wav)
    assert fs == cc.FS and pcm.shape == want.shape and pcm.dtype == np.int16
    d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    print("PARITY %s.max_step measured=%d tol=%d (at most)" % (name, d.max(), parity.SIMSIG["pcm_step"]))
    assert d.max() <= parity.SIMSIG["pcm_step"], (name, int(d.max()))
    check(name + ".share", float((d != 0).mean()), parity.SIMSIG["share_bound"])
    assert np.abs(pcm).max() >= 29000


@pytest.fixture(scope="module")
def runs(tmp_path_factory, tree):
    """{noise type: (stage directory, result, log lines)} of the 2 x 2 x 2 run in one batch of 8."""
    out = {}
    for nt in cc.NOISE_TYPES:
        tmp = tmp_path_factory.mktemp(nt)
        res, lines = _simulate(tmp, tree, nt)
        out[nt] = (tmp / "train", res, lines)
    return out


@pytest.mark.parametrize("nt", cc.NOISE_TYPES)
def test_generator_against_the_restatement(runs, plans, nt):
    from sar_ssl_amd import roomsim
    out, res, lines = runs[nt]
    assert res["written"] == list(range(8)) and res["skipped"] == [] and lines == [] and all(res["attempts"][g] == 1 for g in range(8))
    assert sorted(os.listdir(out)) == ["R1", "R2", "all_info.npz"]
    for r in (1, 2):
        assert sorted(os.listdir(out / ("R%d" % r))) == sorted(["%d.wav" % i for i in range(4)] + ["%d_info.npz" % i for i in range(4)])
    for g in range(8):
        r, i = divmod(g, 4)
        n_len = roomsim.plan_rir(plans[g]["cfg"])["n_len"]
        want = roomsim.restate_sig(plans[g], roomsim.numpy_noise(SEED, g, 0, 2, n_len), noise_type=nt)
        _against_restatement("certainroom.%s.g%d" % (nt, g), str(out / ("R%d" % (r + 1)) / ("%d.wav" % i)), want)
    all_info = np.load(out / "all_info.npz", allow_pickle=True)
    cfgs, args = all_info["cfgs"].item(), all_info["args"].item()
    assert sorted(all_info.files) == ["args", "cfgs", "skipped"] and list(cfgs) == ["R0", "R1"] and all(len(v) == 4 for v in cfgs.values())
    assert args["stage"] == "train" and args["seed"] == SEED and args["noise_type"] == nt and args["room_num"] == 2
    assert all_info["skipped"].size == 0


def test_info_files(runs, plans):
    """{i}_info.npz: the labels against roomsim.labels of the same RIRs (rendered again as the generator renders them, and read back),
    the draws exactly; what the items of a room and the signals of a placement share."""
    from sar_ssl_amd import parity, roomsim
    out, res, lines = runs["diffuse_white"]
    tol = {k: min(parity.RIRLABELS["gate"][k], parity.RIRLABELS["cap"][k]) for k in parity.RIRLABELS["gate"]}
    ids = list(range(8))
    batch = roomsim.render_items({g: plans[g]["cfg"] for g in ids}, ids, SEED, 0, torch.device(DEV), noise="numpy",
                                 lmax=roomsim.sig_lmax(cc.SMALL["T60_range"]))
    rir, dp = batch.rir.cpu().numpy(), batch.dp.cpu().numpy()
    infos = []
    for g in ids:
        r, i = divmod(g, 4)
        info = dict(np.load(out / ("R%d" % (r + 1)) / ("%d_info.npz" % i), allow_pickle=True))
        infos.append(info)
        cfg = plans[g]["cfg"]
        want = roomsim.labels(rir[g, :, :batch.plans[g]["n_len"]], dp[g, :, :batch.plans_dp[g]["n_len"]], cfg)
        assert want["ok"]
        check("certainroom.info%d.T60_edc" % g, abs(float(info["T60_edc"]) - want["T60_edc"]), tol["t60"])
        for k in ("DRR", "C50"):
            assert info[k].dtype == np.float16
            assert info[k] == want[k] or abs(float(info[k]) - float(want[k])) <= float(np.spacing(np.float16(want[k]))), (k, info[k], want[k])
        assert info["TDOA"].dtype == np.float32 and info["TDOA"] == want["TDOA"]
        assert float(info["SNR"]) == plans[g]["snr"] and int(info["src_idx"]) == plans[g]["src_idx"]
        for k in cfg:
            assert np.array_equal(np.asarray(info[k]), np.asarray(cfg[k])), k
        assert sorted(info) == sorted(list(cfg) + ["T60_edc", "SNR", "src_idx", "TDOA", "DRR", "C50"])
    for r in (0, 1):
        room = infos[4 * r:4 * r + 4]
        for k in ("room_sz", "beta", "T60_specify"):
            assert all(np.array_equal(room[0][k], x[k]) for x in room), k
        for j in (0, 1):
            a, b = room[2 * j], room[2 * j + 1]
            assert all(np.array_equal(a[k], b[k]) for k in ("mic_pos", "array_pos", "src_traj_pts", "TDOA"))
            assert int(a["src_idx"]) != int(b["src_idx"]) or float(a["SNR"]) != float(b["SNR"])
        assert not np.array_equal(room[0]["mic_pos"], room[2]["mic_pos"])
    assert not np.array_equal(infos[0]["room_sz"], infos[4]["room_sz"])


@pytest.mark.parametrize("nt", cc.NOISE_TYPES)
def test_files_do_not_depend_on_the_batch(tmp_path, tree, runs, nt):
    """batch = 1 and batch = 5 (rooms 1 and 2 share the batch of items 0..4) against the one batch of 8."""
    a, _ = _simulate(tmp_path / "a", tree, nt, batch=1)
    b, _ = _simulate(tmp_path / "b", tree, nt, batch=5)
    assert a["written"] == b["written"] == list(range(8))
    for g in range(8):
        r, i = divmod(g, 4)
        for name in ("%d.wav" % i, "%d_info.npz" % i):
            fa, fb, fc = (d / ("R%d" % (r + 1)) / name for d in (tmp_path / "a" / "train", tmp_path / "b" / "train", runs[nt][0]))
            if name.endswith(".wav"):
                assert fa.read_bytes() == fb.read_bytes() == fc.read_bytes(), (g, name)
            else:
                ia, ib = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
                assert sorted(ia.files) == sorted(ib.files) and all(np.array_equal(ia[k], ib[k]) for k in ia.files), (g, name)


def test_device_noise_and_the_device_table_feed_the_field(tmp_path, tree, runs):
    from sar_ssl_amd.dataset import read_wav_pcm16
    res, lines = _simulate(tmp_path, tree, noise="device", batch=3)
    assert res["written"] == list(range(8)) and res["skipped"] == []
    for g in range(8):
        r, i = divmod(g, 4)
        pcm, fs = read_wav_pcm16(str(tmp_path / "train" / ("R%d" % (r + 1)) / ("%d.wav" % i)))
        other, _ = read_wav_pcm16(str(runs["diffuse_white"][0] / ("R%d" % (r + 1)) / ("%d.wav" % i)))
        assert pcm.shape == (cc.NS_SMALL, 2) and fs == cc.FS and 29000 <= np.abs(pcm).max() <= 32767 and not np.array_equal(pcm, other)


# ---------------------------------------------------------------------------------------------------------------- --mode rir
def test_room_bank_loads_as_a_simulated_bank(tmp_path):
    from sar_ssl_amd import rirsynth, roomsim
    res = roomsim.simulate_room_bank(str(tmp_path), "train", 2, 2, device=DEV, noise="numpy", batch=3, log=print, **cc.SMALL)
    assert res["written"] == [0, 1, 2, 3] and res["skipped"] == []
    out = tmp_path / "train"
    assert sorted(os.listdir(out)) == ["R1", "R2", "all_info.npz"]
    for r in (1, 2):
        assert sorted(os.listdir(out / ("R%d" % r))) == sorted("%d%s" % (j, s) for j in (0, 1) for s in (".npy", "_dp.npy", "_info.npz"))
    placed = roomsim.room_placements(SEED, 2, 2, roomsim.MIC_ARRAY_CFG_2CH, dict(roomsim.DEFAULTS, **cc.SMALL))
    cfgs = np.load(out / "all_info.npz", allow_pickle=True)["cfgs"].item()
    assert list(cfgs) == ["R0", "R1"]
    bank = rirsynth.SimulatedBank([str(out)], sort=True)
    assert len(bank) == 4 and bank.nch == 2
    for n, f in enumerate(bank.files):                          # sorted: R1/0, R1/1, R2/0, R2/1
        r, j = divmod(n, 2)
        assert str(f).endswith(os.path.join("R%d" % (r + 1), "%d_dp.npy" % j))
        assert np.array_equal(bank.mic_pos[n], placed[r][j]["mic_pos"]) and np.array_equal(cfgs["R%d" % r][j]["mic_pos"], placed[r][j]["mic_pos"])
        assert bank.rirs[n].shape == (2, roomsim.plan_rir(placed[r][j])["n_len"]) and bank.dps[n].shape == (2, 1600)
        assert abs(float(bank.labels[n]["T60"]) - placed[r][j]["T60_specify"]) < 0.05
        # the file is the render of that item alone, keyed by its flattened id
        plan = [roomsim.plan_rir(placed[r][j])]
        alone = roomsim.render(plan, torch.device(DEV), roomsim.host_noise(plan, [n], SEED, 0, torch.device(DEV))).cpu().numpy()
        assert np.load(str(f).replace("_dp.npy", ".npy")).tobytes() == alone[:, :, :, None].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the product
def test_generated_tree_feeds_run_downstream(tmp_path, tree):
    """generate -> fine-tune: the command of test_gpu_downstream.py::test_run_downstream_entry_point_finetunes_from_a_pretrain_checkpoint
    on a tree this generator wrote (train: 1 room x 4 x 2, val and test: 1 room x 4 x 1, T = 1.28 s) instead of a fabricated one."""
    import subprocess
    import sys
    import scipy.io
    from conftest import ROOT
    from sar_ssl_amd import dataset, model
    work = tmp_path / "work"
    simu = work / "SAR-SSL" / "data" / "MicSig" / "simu_ds"
    for stage, sigs in (("train", 2), ("val", 1), ("test", 1)):
        res, lines = _simulate(simu, tree, noise="device", stage=stage, rooms=1, rirs=4, sigs=sigs, T=1.28)
        assert res["written"] == list(range(4 * sigs)) and lines == []
        ds = dataset.FixMicSigDataset(str(simu / stage), 16000, load_anno=True, dataset_sz=None)
        assert len(ds) == 4 * sigs
        for n in range(len(ds)):
            sig, anno = ds[n]
            assert sig.shape == (20480, 2) and np.isfinite(sig).all()
            assert sorted(anno) == ["ABS", "C50", "DRR", "T60", "TDOA"] and all(np.isfinite(v).all() for v in anno.values())
            assert 0.1 < float(anno["T60"]) < 0.5 and abs(float(anno["TDOA"])) < 2e-3
    assert sorted(os.listdir(simu / "train")) == ["R1", "all_info.npz"]
    pre = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=True, device="cpu")
    ck = work / "SAR-SSL" / "exp" / "pretrain" / "t1"
    ck.mkdir(parents=True)
    torch.save({"epoch": 3, "max_score": -1.0, "model": pre.state_dict()}, str(ck / "best_model.tar"))
    cmd = [sys.executable, os.path.join(ROOT, "run_downstream.py"), "--ds-train", "--simu-exp", "--ds-trainmode", "finetune", "--ds-task", "TDOA",
           "--ds-nsimroom", "32", "--gpu-id", "0,", "--work-dir", str(work), "--time", "t1", "--workers", "2", "--ds-nepoch", "2",
           "--ds-num", "8", "--ds-lr-set", "0.0001", "--ds-bs-set", "4", "--ds-eval-num", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    tdir = work / "SAR-SSL" / "exp" / "TDOA" / "t1"
    runs = [p for p in tdir.iterdir() if p.is_dir()]
    assert len(runs) == 1 and runs[0].name == "finetune-all-mlp-8-0.0001-4-0-spat-sim_R32"
    recs = [json.loads(l) for l in open(runs[0] / "scalars.jsonl").read().strip().splitlines()]
    assert [r_["epoch"] for r_ in recs] == [1, 2] and all(np.isfinite(r_["loss_val"]) and np.isfinite(r_["metric_test"]) for r_ in recs)
    assert (runs[0] / "ensemble_model.tar").exists() and (runs[0] / "best_model.tar").exists()
    mats = [p for p in tdir.iterdir() if p.name.endswith("-lr_bs_tri_result.mat")]
    assert len(mats) == 1
    res = scipy.io.loadmat(str(mats[0]))
    assert res["val_metrics"].shape == (1, 1, 1) and np.isfinite(res["test_metrics"]).all()
