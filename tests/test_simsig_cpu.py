"""CPU: the host side of the signal generator (gen_simu.py --mode sig; sar_ssl_amd.roomsim.plan_sig / restate_sig / sig_info, the numpy
twin of the labels kernel, dataset.write_wav_batch, the command line's refusals) against fixture F22 - the reference's own
generate_microphone_signal on canned RIRs (tools/make_golden_simsig.py) - and against roomsim.labels."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401
import simsig_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(sc.F22)


@pytest.fixture(scope="module")
def planned(fx, tmp_path_factory):
    """[(plan, cfg)] of F22's items: plan_sig on the restored tree with the reference's configurations."""
    from sar_ssl_amd import rirsynth, roomsim
    src_dir = sc.write_speech_tree(tmp_path_factory.mktemp("f22"), fx)
    fs, ns, nmic, seed, items = [int(v) for v in fx["consts"]]
    sources = rirsynth.SourceBank(os.path.join(src_dir, "tr"), fs, sort=True)
    assert list(fx["speakers"]) == sources.spk_ids
    rs = np.random.RandomState()
    out = []
    for k in range(items):
        cfg = sc.f22_cfg(fx, k)
        out.append((roomsim.plan_sig(rs, k, seed, cfg, sources, float(fx["T"]), tuple(fx["snr_range"]), nmic), cfg, src_dir))
    return out


def test_plan_sig_reproduces_the_reference_draws(fx, planned):
    for k, (plan, cfg, src_dir) in enumerate(planned):
        pre = "item/%d/" % k
        root = os.path.dirname(src_dir)
        assert plan["src_idx"] == int(fx[pre + "info/src_idx"]) and plan["utt_idx"] == int(fx[pre + "utt_idx"])
        assert plan["crop_start"] == int(fx[pre + "crop_start"])
        assert [os.path.relpath(f, root) for f in plan["utt_files"]] == [str(f) for f in fx[pre + "utt_files"]]
        assert plan["snr"] == float(fx[pre + "info/SNR"])
        w = plan["white"]
        assert np.array_equal(w[:fx[pre + "white_head"].shape[0]], fx[pre + "white_head"])
        assert np.array_equal(np.array([w.sum(), (w ** 2).sum()]), fx[pre + "white_sums"])


def test_plan_sig_without_the_white_draw_keeps_the_other_draws_up_to_the_snr(fx, planned):
    from sar_ssl_amd import rirsynth, roomsim
    plan, cfg, src_dir = planned[0]
    sources = rirsynth.SourceBank(os.path.join(src_dir, "tr"), sc.FS, sort=True)
    p = roomsim.plan_sig(np.random.RandomState(), 0, 1, cfg, sources, float(fx["T"]), tuple(fx["snr_range"]), 2, draw_white=False)
    assert p["white"] is None and p["crop_start"] == plan["crop_start"] and np.array_equal(p["src"], plan["src"])


def test_restate_sig_reproduces_the_reference_output(fx, planned):
    from sar_ssl_amd import parity, roomsim
    worst = 0.0
    for k, (plan, cfg, _) in enumerate(planned):
        pre = "item/%d/" % k
        got = roomsim.restate_sig(plan, rir=fx[pre + "rir"], rir_dp=fx[pre + "rir_dp"], pcm=False)
        want = fx[pre + "out"].astype(np.float64)
        assert got.shape == want.shape and abs(np.abs(want).max() - 0.9) < 1e-6
        worst = max(worst, float(np.abs(got - want).max()))
    print("restate_sig vs F22: max |difference| %.3g (bound %.1g)" % (worst, parity.RIRMIX["restatement_vs_f20"]))
    assert worst <= parity.RIRMIX["restatement_vs_f20"]


def test_info_matches_the_reference(fx, planned):
    from sar_ssl_amd import roomsim
    for k, (plan, cfg, _) in enumerate(planned):
        pre = "item/%d/" % k
        lab = roomsim.labels(fx[pre + "rir"], fx[pre + "rir_dp"], cfg)
        assert lab["ok"]
        info = roomsim.sig_info(cfg, plan, lab["T60_edc"], lab["DRR"], lab["C50"])
        assert sorted(info) == [str(n) for n in fx[pre + "info_keys"]]
        assert info["src_idx"] == int(fx[pre + "info/src_idx"]) and info["SNR"] == float(fx[pre + "info/SNR"])
        for name in ("TDOA", "DRR", "C50"):
            want = fx[pre + "info/" + name]
            assert np.asarray(info[name]).dtype == want.dtype and np.array_equal(np.asarray(info[name]), want), name
        assert abs(float(info["T60_edc"]) - float(fx[pre + "info/T60_edc"])) < 1e-12
        # the device's unrounded values go through the same rounding
        tw = roomsim.labels_twin(fx[pre + "rir"], fx[pre + "rir_dp"], cfg["T60_specify"])
        info = roomsim.sig_info(cfg, plan, tw["t60_edc"], tw["drr"], tw["c50"])
        assert info["DRR"] == fx[pre + "info/DRR"] and info["C50"] == fx[pre + "info/C50"] and info["DRR"].dtype == np.float16


@pytest.mark.parametrize("nch", [1, 2, 3])
def test_labels_twin_equals_the_host_labels(nch):
    """The kernel's arithmetic (closed-form fits from centred suffix sums) in numpy against roomsim.labels (scipy.stats.linregress per
    stretch) on every case the GPU test runs."""
    from sar_ssl_amd import roomsim
    tol = dict(t60=1e-12, corr=1e-12, drr=1e-12, c50=1e-12)
    seen = {}
    for name, rir, dp, t in sc.label_cases(nch):
        want = sc.host_labels(rir, dp, t)
        with np.errstate(all="ignore"):
            got = roomsim.labels_twin(rir, dp, t)
        sc.same_labels(got, want, tol)
        seen[name] = want
    assert all(seen["full_%g_%d" % (t, L)]["flags"] == 3 for _, t, L in sc.FULL)
    assert seen["short_600"]["flags"] == 1 and seen["short_257"]["flags"] == 1 and seen["off_specify"]["flags"] == 1
    assert np.isnan(seen["short_40"]["t60"][-1]) and seen["short_40"]["corr"][-1] == 0
    assert seen["all_zero"]["flags"] == 0 and seen["nan"]["flags"] == 0 and seen["plateau"]["flags"] == 3
    assert seen["negative_dp"]["nd"] == 100


def test_pcm16_rule():
    from sar_ssl_amd import roomsim
    x = np.array([0.9, -0.9, 1.0, -1.0, 1.5, -1.5, 0.0, -0.0, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767])
    assert list(roomsim.pcm16(x)) == [29490, -29490, 32767, -32767, 32767, -32767, 0, 0, 0, 2, 2, 0]
    assert roomsim.pcm16(x).dtype == np.int16


def _built():
    import __graft_entry__ as g
    from sar_ssl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()


def test_write_wav_batch_is_byte_identical_and_round_trips(tmp_path):
    import torch
    from sar_ssl_amd import dataset
    _built()
    rs = np.random.RandomState(0)
    for n, ns, nch, nthreads in ((5, 4352, 2, 0), (1, 1, 1, 1), (3, 65, 4, 2)):
        pcm = rs.randint(-32768, 32768, (n, ns, nch)).astype(np.int16)
        paths = [str(tmp_path / ("%d_%d_%d.wav" % (ns, nch, i))) for i in range(n)]
        dataset.write_wav_batch(paths, torch.from_numpy(pcm), 16000, nthreads)
        for i, p in enumerate(paths):
            ref = str(tmp_path / "ref.wav")
            dataset.write_wav_pcm16(ref, pcm[i], 16000)
            assert open(p, "rb").read() == open(ref, "rb").read()
            assert not os.path.exists(p + ".tmp")
        back = dataset.read_wav_batch(paths, ns, nch, 16000)
        assert np.array_equal(back.numpy(), pcm)
    # a numpy array is taken as well, and a buffer longer than the list of paths
    dataset.write_wav_batch(paths[:2], pcm, 16000)
    assert dataset.read_wav_pcm16(paths[1])[0].shape == (65, 4)


def test_write_wav_batch_names_nothing_half_written(tmp_path):
    import torch
    from sar_ssl_amd import _lib, dataset
    _built()
    pcm = torch.zeros((2, 64, 2), dtype=torch.int16)
    good, bad = str(tmp_path / "a.wav"), str(tmp_path / "missing_dir" / "b.wav")
    with pytest.raises(_lib.SarsslHipError, match="b.wav"):
        dataset.write_wav_batch([bad, good], pcm, 16000, nthreads=1)
    assert sorted(os.listdir(tmp_path)) == []                  # the failing file's .tmp is gone, the file behind it was not started


REFUSALS = [
    (["--stage", "pretrain", "--save_dp", "True"], "--save_dp True"),
    (["--stage", "pretrain", "--noise_type", "babble"], "diffuse_white only"),
    (["--stage", "pretrain", "--gpu_conv", "True"], "--gpu_conv True"),
    (["--stage", "pretrain", "--T", "4.0001"], "not a multiple of 64"),
    (["--stage", "pretrain", "--source_state", "moving"], "static sources only"),
    (["--stage", "pretrain", "--num_source_range", "[1,2]"], "one source only"),
    (["--stage", "pretrain", "--mic_pattern", "card"], "omnidirectional microphones only"),
    (["--stage", "pretrain", "--fs", "8000"], "16000 Hz only"),
    (["--stage", "train"], "only --mode rir generates stages train / val / test"),
    (["--stage", "val"], "as the reference asserts"),
    (["--stage", "test"], "as the reference asserts"),
    ([], "only --mode rir"),                                    # the default stage is --mode rir's
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_command_line_refusals(extra, message, capsys, tmp_path):
    from sar_ssl_amd import roomsim
    with pytest.raises(SystemExit) as e:
        roomsim.main(["--mode", "sig", "--save_to", str(tmp_path), "--src_dir", str(tmp_path)] + extra)
    assert e.value.code != 0 and message in capsys.readouterr().err
    assert os.listdir(tmp_path) == []


def test_unknown_modes_are_refused_with_the_old_wording(capsys, tmp_path):
    from sar_ssl_amd import roomsim
    with pytest.raises(SystemExit):
        roomsim.main(["--mode", "traj", "--save_to", str(tmp_path)])
    assert "only --mode rir" in capsys.readouterr().err


def test_stage_names_seeds_and_source_directories():
    from sar_ssl_amd import roomsim
    assert [roomsim.sig_stage(s) for s in ("pretrain", "preval", "pretest", "pretest_ins_T1000")] == ["pretrain", "preval", "pretest", "pretest"]
    assert roomsim.SIG_STAGE_SEEDS == {"pretrain": 1, "preval": 2000000, "pretest": 3000000}
    assert roomsim.SIG_SRC_SUBDIR == {"pretrain": "tr", "preval": "dt", "pretest": "et"}
    assert roomsim.sig_lmax((0.2, 1.3)) >= int(np.ceil(40 / 60 * 1.305 * 16000)) and roomsim.sig_lmax((0.2, 0.4)) <= 4330
