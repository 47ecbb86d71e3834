"""CPU: the host side of the per-room generator (gen_simu_certain_room.py; sar_ssl_amd.roomsim.random_room / room_placements / room_stem /
plan_sig / restate_sig / sig_info and the command line's refusals) against fixture F23 - the reference's own
GenerateRandomMicSigOfCertainRoom and GenerateRandomRIROfCertainRoom on canned RIRs (tools/make_golden_certainroom.py) - and the
library's new entry point."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401
import certainroom_cases as cc  # noqa: E402
import simsig_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(cc.F23)


@pytest.fixture(scope="module")
def k(fx):
    return cc.consts(fx)


def _same_cfg(got, want):
    assert list(got) == list(want)
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def test_random_room_and_placements_reproduce_the_reference(fx, k):
    from sar_ssl_amd import roomsim
    args = cc.draw_args()
    rooms = roomsim.room_placements(k["seed"], k["rooms"], k["rirs"], roomsim.MIC_ARRAY_CFG_2CH, args)
    assert len(rooms) == k["rooms"] and all(len(room) == k["rirs"] for room in rooms)
    rs = np.random.RandomState()
    for r in range(k["rooms"]):
        rs.seed(k["seed"] + r)
        room = roomsim.random_room(rs, args["room_sz_range"], args["T60_range"], args["abs_weights_range"], args["c"], args["ism_db"])
        assert list(room) == ["room_sz", "T60_sabine", "beta", "T60_specify"]
        for j in range(k["rirs"]):
            want = cc.f23_cfg(fx, r, j)
            _same_cfg(rooms[r][j], want)
            _same_cfg(room, {name: want[name] for name in room})
            # one placement alone, on the given room: seed + r rirs + j
            draw = {name: args[name] for name in roomsim.DEFAULTS if name != "fs"}
            _same_cfg(roomsim.random_spatial_acoustics(rs, k["seed"], r * k["rirs"] + j, room_cfg=room, **draw), want)
        # the placements of one room share the room and differ in the array
        assert rooms[r][0]["room_sz"] == rooms[r][1]["room_sz"] and not np.array_equal(rooms[r][0]["mic_pos"], rooms[r][1]["mic_pos"])
    assert rooms[0][0]["room_sz"] != rooms[1][0]["room_sz"]


def test_without_a_room_cfg_the_draw_is_the_old_one():
    """random_spatial_acoustics(room_cfg=None) draws its own room after seed + idx: the room random_room draws on the same stream."""
    from sar_ssl_amd import roomsim
    rs = np.random.RandomState()
    cfg = roomsim.random_spatial_acoustics(rs, 4000000, 3, **cc.SMALL)
    rs.seed(4000003)
    room = roomsim.random_room(rs, **cc.SMALL)
    _same_cfg(room, {name: cfg[name] for name in room})


def test_paths_and_keys_follow_the_reference(fx, k):
    from sar_ssl_amd import roomsim
    per_room = k["rirs"] * k["sigs"]
    for nt in cc.NOISE_TYPES:
        stems = []
        for g in range(k["rooms"] * per_room):
            r, i = roomsim.room_item(g, per_room)
            assert g == r * per_room + i and 0 <= i < per_room
            stem = os.path.relpath(roomsim.room_stem("out", g, per_room), "out")
            assert stem + ".wav" == str(fx["sig/%s/%d/path" % (nt, g)]) == "R%d/%d.wav" % (r + 1, i)
            stems.append(stem)
        # (the fixture's run hands its signals to a recording soundfile.write: the directory listing holds the other files)
        assert sorted([s + "_info.npz" for s in stems] + ["all_info.npz"]) == [str(p) for p in fx["sig/%s/written" % nt]]
    stems = [os.path.relpath(roomsim.room_stem("out", g, k["rirs"]), "out") for g in range(k["rooms"] * k["rirs"])]
    assert stems == ["R1/0", "R1/1", "R2/0", "R2/1"]
    assert sorted([s + e for s in stems for e in (".npy", "_dp.npy", "_info.npz")] + ["all_info.npz"]) == [str(p) for p in fx["bank/written"]]
    # all_info.npz: the reference's keys and `skipped`; cfgs is keyed from ZERO, the directories count from one
    keys = list(roomsim.rooms_by_key([[0]] * k["rooms"]))
    assert keys == [str(s) for s in fx["all_info_cfgs_keys"]] == [str(s) for s in fx["bank/all_info_cfgs_keys"]] == ["R0", "R1"]
    assert [str(s) for s in fx["all_info_keys"]] == [str(s) for s in fx["bank/all_info_keys"]] == ["args", "cfgs"]
    assert roomsim.STAGE_SEEDS["train"] == k["seed"] and roomsim.STAGE_SEEDS["val"] == 5000000 and roomsim.STAGE_SEEDS["test"] == 6000000
    assert roomsim.ROOM_SRC_SUBDIR == {"train": "tr", "val": "dt", "test": "et"}
    for stage in ("pretrain", "preval", "pretest", "dev"):
        with pytest.raises(ValueError, match="train \\| val \\| test only"):
            roomsim.room_stage(stage)


@pytest.fixture(scope="module")
def planned(fx, k, tmp_path_factory):
    """[plan] of F23's signal items: plan_sig after seed + g on the restored tree with the reference's configurations."""
    from sar_ssl_amd import rirsynth, roomsim
    src_dir = sc.write_speech_tree(tmp_path_factory.mktemp("f23"), fx)
    sources = rirsynth.SourceBank(os.path.join(src_dir, "tr"), k["fs"], sort=True)
    rs = np.random.RandomState()
    per_room = k["rirs"] * k["sigs"]
    plans = []
    for g in range(k["rooms"] * per_room):
        r, i = roomsim.room_item(g, per_room)
        plans.append(roomsim.plan_sig(rs, g, k["seed"], cc.f23_cfg(fx, r, i // k["sigs"]), sources, float(fx["T"]), tuple(fx["snr_range"]), k["nmic"]))
    return plans, os.path.dirname(src_dir)


def test_plan_sig_with_the_room_offset_reproduces_the_reference_draws(fx, planned):
    plans, root = planned
    for nt in cc.NOISE_TYPES:
        for g, plan in enumerate(plans):
            pre = "sig/%s/%d/" % (nt, g)
            assert plan["src_idx"] == int(fx[pre + "info/src_idx"]) and plan["utt_idx"] == int(fx[pre + "utt_idx"])
            assert plan["crop_start"] == int(fx[pre + "crop_start"])
            assert [os.path.relpath(f, root) for f in plan["utt_files"]] == [str(f) for f in fx[pre + "utt_files"]]
            assert plan["snr"] == float(fx[pre + "info/SNR"])
            w = plan["white"]
            assert np.array_equal(w[:fx[pre + "white_head"].shape[0]], fx[pre + "white_head"])
            assert np.array_equal(np.array([w.sum(), (w ** 2).sum()]), fx[pre + "white_sums"])
    # the two signals of a placement are different draws
    assert plans[0]["snr"] != plans[1]["snr"] and plans[0]["cfg"]["mic_pos"] is not None


@pytest.mark.parametrize("nt", cc.NOISE_TYPES)
def test_restate_sig_reproduces_the_reference_output(fx, planned, nt):
    from sar_ssl_amd import parity, roomsim
    worst = 0.0
    for g, plan in enumerate(planned[0]):
        got = roomsim.restate_sig(plan, rir=fx["rir/%d" % g], rir_dp=fx["rir_dp/%d" % g], pcm=False, noise_type=nt)
        want = fx["sig/%s/%d/out" % (nt, g)].astype(np.float64)
        assert got.shape == want.shape and abs(np.abs(want).max() - 0.9) < 1e-6
        worst = max(worst, float(np.abs(got - want).max()))
    print("restate_sig(%s) vs F23: max |difference| %.3g (bound %.1g)" % (nt, worst, parity.RIRMIX["restatement_vs_f20"]))
    assert worst <= parity.RIRMIX["restatement_vs_f20"]
    if nt == "spatial_white":                                   # (the two types are different signals)
        other = roomsim.restate_sig(planned[0][0], rir=fx["rir/0"], rir_dp=fx["rir_dp/0"], pcm=False)
        assert np.abs(other - fx["sig/%s/0/out" % nt]).max() > 1e-3


def test_restate_sig_refuses_other_noise_types(planned):
    from sar_ssl_amd import roomsim
    for nt, message in (("white", "utils_noise.py:45"), ("white", "default"), ("diffuse_babble", "diffuse_white and spatial_white only")):
        with pytest.raises(ValueError, match=message):
            roomsim.restate_sig(planned[0][0], rir=np.zeros((2, 8)), rir_dp=np.zeros((2, 8)), noise_type=nt)


def test_info_matches_the_reference(fx, planned, k):
    from sar_ssl_amd import roomsim
    for nt in cc.NOISE_TYPES:
        for g, plan in enumerate(planned[0]):
            pre = "sig/%s/%d/" % (nt, g)
            cfg = plan["cfg"]
            lab = roomsim.labels(fx["rir/%d" % g], fx["rir_dp/%d" % g], cfg)
            assert lab["ok"]
            info = roomsim.sig_info(cfg, plan, lab["T60_edc"], lab["DRR"], lab["C50"])
            assert sorted(info) == [str(n) for n in fx[pre + "info_keys"]]
            assert info["src_idx"] == int(fx[pre + "info/src_idx"]) and info["SNR"] == float(fx[pre + "info/SNR"])
            for name in ("TDOA", "DRR", "C50"):
                want = fx[pre + "info/" + name]
                assert np.asarray(info[name]).dtype == want.dtype and np.array_equal(np.asarray(info[name]), want), name
            assert np.asarray(info["T60_edc"]).dtype == fx[pre + "info/T60_edc"].dtype
            assert abs(float(info["T60_edc"]) - float(fx[pre + "info/T60_edc"])) < 1e-12
    # the bank's placement files: simulate_bank's keys (configuration, T60_edc, TDOA, DRR, C50, fs)
    for r in range(k["rooms"]):
        for j in range(k["rirs"]):
            cfg = cc.f23_cfg(fx, r, j)
            assert sorted(list(cfg) + ["T60_edc", "TDOA", "DRR", "C50", "fs"]) == [str(n) for n in fx["bank/%d/%d/info_keys" % (r, j)]]
            g = (r * k["rirs"] + j) * k["sigs"]
            lab = roomsim.labels(fx["rir/%d" % g], fx["rir_dp/%d" % g], cfg)
            for name in ("TDOA", "DRR", "C50"):
                want = fx["bank/%d/%d/info/%s" % (r, j, name)]
                assert lab[name].dtype == want.dtype and np.array_equal(lab[name], want), name


REFUSALS = [
    ("sig", ["--noise_type", "white"], "utils_noise.py:45"),
    ("sig", ["--noise_type", "white"], "reference's gen_simu_certain_room.py has this default"),
    ("sig", ["--noise_type", "diffuse_babble"], "diffuse_white and spatial_white only"),
    ("sig", ["--stage", "pretrain"], "train | val | test only, as the reference asserts"),
    ("rir", ["--stage", "pretrain"], "train | val | test only"),
    ("sig", ["--T", "4.0001"], "not a multiple of 64"),
    ("sig", ["--gpu_conv", "True"], "--gpu_conv True"),
    ("sig", ["--source_state", "moving"], "static sources only"),
    ("rir", ["--num_source_range", "[1,2]"], "one source only"),
    ("sig", ["--mic_pattern", "card"], "omnidirectional microphones only"),
    ("sig", ["--fs", "8000"], "16000 Hz only"),
]


@pytest.mark.parametrize("mode,extra,message", REFUSALS)
def test_command_line_refusals(mode, extra, message, capsys, tmp_path, monkeypatch):
    import torch
    from sar_ssl_amd import roomsim

    def touched(*a, **kw):
        raise AssertionError("the GPU was touched before the refusal")

    monkeypatch.setattr(torch.cuda, "set_device", touched)
    with pytest.raises(SystemExit) as e:
        roomsim.main_certain_room(["--mode", mode, "--save_to", str(tmp_path), "--src_dir", str(tmp_path)] + extra)
    assert e.value.code != 0 and message in capsys.readouterr().err
    assert os.listdir(tmp_path) == []


def test_library_functions_refuse_what_the_command_line_refuses(tmp_path):
    from sar_ssl_amd import roomsim
    with pytest.raises(ValueError, match="utils_noise.py:45"):
        roomsim.simulate_room_signals(str(tmp_path), "train", 1, 1, 1, str(tmp_path), noise_type="white")
    with pytest.raises(ValueError, match="train \\| val \\| test only"):
        roomsim.simulate_room_signals(str(tmp_path), "pretrain", 1, 1, 1, str(tmp_path))
    with pytest.raises(ValueError, match="train \\| val \\| test only"):
        roomsim.simulate_room_bank(str(tmp_path), "preval", 1, 1)
    with pytest.raises(ValueError, match="not a multiple of 64"):
        roomsim.simulate_room_signals(str(tmp_path), "train", 1, 1, 1, str(tmp_path), T=0.27)
    with pytest.raises(ValueError, match="16000 Hz only"):
        roomsim.simulate_room_signals(str(tmp_path), "train", 1, 1, 1, str(tmp_path), fs=8000)
    assert os.listdir(tmp_path) == []


def test_the_entry_script_shares_the_argument_definitions():
    """gen_simu_certain_room.py takes the reference's flag names and this project's; both command lines define the shared ones once."""
    import argparse
    from sar_ssl_amd import roomsim
    ap = argparse.ArgumentParser()
    roomsim._shared_arguments(ap)
    shared = {a.dest for a in ap._actions}
    assert {"mode", "stage", "src_dir", "save_to", "snr_range", "noise_type", "T", "T60_range", "room_sz_range", "gpus", "noise", "batch",
            "mic_array"} <= shared
    text = open(os.path.join(ROOT, "gen_simu_certain_room.py")).read()
    assert "main_certain_room" in text
    a = ap.parse_args([])
    assert a.noise_type == "diffuse_white" and a.T == 4.112


def test_the_library_exports_the_mixing_table_and_the_header_binds_it():
    import inspect
    import __graft_entry__ as g
    from sar_ssl_amd import _lib, hip
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    assert hasattr(_lib.lib(), "sarssl_mixing_table") and _lib.lib().sarssl_abi_version() == 3
    hdr = open(os.path.join(ROOT, "include", "sarssl_hip.h")).read()
    m = re.search(r"\bint\s+sarssl_mixing_table\s*\(([^()]*)\)\s*;", hdr)
    assert m is not None
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const double* mic", "int nb", "int m", "double fs", "double c", "float* out", "void* stream"]
    call = re.search(r'_lib\.call\("sarssl_mixing_table",(.*)\)\n', inspect.getsource(hip.mixing_table))
    assert call is not None and call.group(1).count("(") == len(params)        # one wrapped argument per parameter


def test_mixing_table_geometries_factor_on_the_host():
    """The GPU test's inputs: the host factorisation succeeds for each, the 3-microphone line's smallest pivot is about 1e-3, and two
    coincident microphones are refused by LAPACK."""
    import scipy.linalg
    from sar_ssl_amd import rirsynth
    smallest = {}
    for name, mic in cc.table_batches():
        C = cc.host_tables(mic)
        assert C.shape == (mic.shape[0], 129, mic.shape[1], mic.shape[1]) and np.isfinite(C).all() and not C[:, 0].any()
        smallest[name] = float(np.min(np.diagonal(C[:, 1:], axis1=2, axis2=3)))
    assert 5e-4 < smallest["line3_5cm"] < 2e-3, smallest
    with pytest.raises(scipy.linalg.LinAlgError):
        rirsynth.mixing_table(np.array([[1.0, 2.0, 1.5], [1.0, 2.0, 1.5]]))
