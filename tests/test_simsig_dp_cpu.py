"""CPU: the host side of gen_simu.py --mode sig --save_dp True - roomsim.restate_sig(with_dp=True) against fixture F24 (the reference's
own generate_microphone_signal(..., save_dp=True) on F22's items, tools/make_golden_simsig_dp.py), the command line's routing and its
refusals, and FixMicSigDataset(load_dp=True) over a directory of ``{i}.wav`` + ``{i}_dp.wav``."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401
import simsig_cases as sc  # noqa: E402

F24 = os.path.join(ROOT, "tests", "golden", "f24_simsig_dp.npz")


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(F22, [plan_sig of its items on the restored tree with the reference's configurations])."""
    from sar_ssl_amd import rirsynth, roomsim
    fx = np.load(sc.F22)
    src_dir = sc.write_speech_tree(tmp_path_factory.mktemp("f24"), fx)
    fs, ns, nmic, seed, items = [int(v) for v in fx["consts"]]
    sources = rirsynth.SourceBank(os.path.join(src_dir, "tr"), fs, sort=True)
    rs = np.random.RandomState()
    return fx, [roomsim.plan_sig(rs, k, seed, sc.f22_cfg(fx, k), sources, float(fx["T"]), tuple(fx["snr_range"]), nmic) for k in range(items)]


def test_restate_sig_with_dp_reproduces_the_reference_dp_file(planned):
    from sar_ssl_amd import parity, roomsim
    fx, plans = planned
    f24 = np.load(F24)
    assert np.array_equal(f24["consts"], fx["consts"])
    assert [str(n) for n in f24["files"]] == sorted("%d%s.wav" % (k, s) for k in range(len(plans)) for s in ("", "_dp"))
    worst = 0.0
    for k, plan in enumerate(plans):
        pre = "item/%d/" % k
        mic, dp = roomsim.restate_sig(plan, rir=fx[pre + "rir"], rir_dp=fx[pre + "rir_dp"], pcm=False, with_dp=True)
        alone = roomsim.restate_sig(plan, rir=fx[pre + "rir"], rir_dp=fx[pre + "rir_dp"], pcm=False)
        assert mic.dtype == dp.dtype == np.float64 and np.array_equal(mic, alone)
        want = f24[pre + "out_dp"].astype(np.float64)
        assert dp.shape == want.shape == mic.shape and 0 < np.abs(want).max() <= 0.9 + 1e-6
        worst = max(worst, float(np.abs(dp - want).max()))
        # the PCM form is the PCM rule on the same pair
        pm, pd = roomsim.restate_sig(plan, rir=fx[pre + "rir"], rir_dp=fx[pre + "rir_dp"], with_dp=True)
        assert pm.dtype == pd.dtype == np.int16 and np.array_equal(pm, roomsim.pcm16(mic)) and np.array_equal(pd, roomsim.pcm16(dp))
    print("restate_sig(with_dp=True) vs F24: max |difference| %.3g (bound %.1g, recorded %.1g)"
          % (worst, parity.RIRMIX["restatement_vs_f20"], parity.RIRMIX["measured"]["restatement_dp_vs_f24"]))
    assert worst <= parity.RIRMIX["restatement_vs_f20"]


def test_restate_mix_returns_the_direct_path_at_the_scale_of_the_mix():
    from sar_ssl_amd import rirsynth
    rs = np.random.RandomState(5)
    src, rir, noise = rs.standard_normal(700), rs.standard_normal((3, 90)) * 0.1, rs.standard_normal((700, 3))
    for kw in (dict(n0=4), dict(rir_dp=rir[:, :20] * (np.arange(20) > 10))):
        mic, dp = rirsynth.restate_mix(src, rir, noise=noise, snr_db=12.0, gain=0.9, return_dp=True, **kw)
        assert np.array_equal(mic, rirsynth.restate_mix(src, rir, noise=noise, snr_db=12.0, gain=0.9, **kw))
        assert mic.shape == dp.shape == (700, 3)
        assert abs(max(np.abs(mic).max(), np.abs(dp).max()) - 0.9) < 1e-12


def _patched(monkeypatch):
    import torch
    from sar_ssl_amd import roomsim
    seen = []

    def fake(*args, **kw):
        seen.append((args, kw))
        return dict(written=[0], skipped=[], attempts={0: 1})

    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(roomsim, "simulate_signals", fake)
    return roomsim, seen


def test_command_line_passes_save_dp_on_the_instance_test_stage(monkeypatch, tmp_path):
    roomsim, seen = _patched(monkeypatch)
    base = ["--mode", "sig", "--save_to", str(tmp_path), "--src_dir", str(tmp_path), "--stage", "pretest_ins_T1000", "--data_num", "10"]
    assert roomsim.main(base + ["--save_dp", "True"]) == 0
    assert len(seen) == 1 and seen[0][1]["save_dp"] is True and seen[0][0][:3] == (str(tmp_path), "pretest_ins_T1000", 10)
    assert roomsim.main(base) == 0 and seen[1][1]["save_dp"] is False
    assert roomsim.main(["--mode", "sig", "--save_to", str(tmp_path), "--src_dir", str(tmp_path), "--stage", "pretest"]) == 0
    assert seen[2][1]["save_dp"] is False


@pytest.mark.parametrize("stage", ["pretest", "preval", "pretrain"])
def test_command_line_refuses_save_dp_on_the_corpus_stages(stage, monkeypatch, tmp_path, capsys):
    roomsim, seen = _patched(monkeypatch)
    with pytest.raises(SystemExit) as e:
        roomsim.main(["--mode", "sig", "--save_to", str(tmp_path), "--src_dir", str(tmp_path), "--stage", stage, "--save_dp", "True"])
    err = capsys.readouterr().err
    assert e.value.code != 0 and "--save_dp True:" in err and "pretest_ins" in err
    assert seen == [] and os.listdir(tmp_path) == []


def test_python_api_takes_save_dp_on_any_stage():
    import inspect
    from sar_ssl_amd import rirsynth, roomsim
    for fn in (roomsim.simulate_signals, roomsim._signals):
        assert inspect.signature(fn).parameters["save_dp"].default is False
    assert inspect.signature(rirsynth.mix_simulated).parameters["out_dp"].default is None
    assert "save_dp" not in inspect.signature(roomsim.simulate_room_signals).parameters


def test_fix_mic_sig_dataset_pairs_every_item_with_its_dp_file(tmp_path):
    from sar_ssl_amd import dataset
    rs = np.random.RandomState(2)
    sigs = {}
    for i in range(3):
        for s in ("", "_dp"):
            sigs[i, s] = rs.randint(-20000, 20000, (640, 2)).astype(np.int16)
            dataset.write_wav_pcm16(str(tmp_path / ("%d%s.wav" % (i, s))), sigs[i, s], 16000)
    ds = dataset.FixMicSigDataset(data_dir=str(tmp_path), load_anno=False, load_dp=True, dataset_sz=None, fs=16000, transforms=None)
    assert len(ds) == 3 and sorted(os.path.basename(str(f)) for f in ds.files) == ["0.wav", "1.wav", "2.wav"]
    for j in range(3):
        i = int(os.path.basename(str(ds.files[j])).split(".")[0])
        item = ds[j]
        assert len(item) == 2
        assert np.array_equal(np.asarray(item[0], np.float32), sigs[i, ""].astype(np.float32) / 32768.0)
        assert np.array_equal(np.asarray(item[1], np.float32), sigs[i, "_dp"].astype(np.float32) / 32768.0)
    assert len(dataset.FixMicSigDataset(data_dir=str(tmp_path), load_anno=False, load_dp=False, dataset_sz=None, fs=16000)) == 3
