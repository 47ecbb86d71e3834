"""GPU: the image-source renderer (csrc/ism.hip: sarssl_ism_rir) against the f64 numpy restatement roomsim.restate_ism, and the
generator built on it (roomsim.simulate_bank, gen_simu.py).  Distances are max |difference| relative to the RIR's absolute peak and are
gated by parity.ISM; the tail's noise is uploaded from numpy so that the comparison is element by element."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT, check

pytestmark = pytest.mark.gpu
SEED = 4000000
ROOM, BETA = [6.0, 5.0, 3.5], [0.9, 0.8, 0.85, 0.7, 0.6, 0.75]


def _gate():
    from sar_ssl_amd import parity
    return min(parity.ISM["gate"], parity.ISM["cap"])


@functools.lru_cache(maxsize=None)
def _f21():
    return dict(np.load(os.path.join(GOLD, "f21_roomsim.npz"), allow_pickle=False))


def _cfg(prefix):
    pre = prefix + "/"
    return {k[len(pre):]: v for k, v in _f21().items() if k.startswith(pre)}


def _plan(nch, nb_img, n_ism, n_len=None, src=(2.1, 1.7, 1.2), mic0=(3.4, 2.9, 1.5), slope=-80.0, room=ROOM):
    mic = np.array([[mic0[0] + 0.07 * m, mic0[1] - 0.05 * m, mic0[2] + 0.02 * m] for m in range(nch)])
    return dict(room=np.array(room), beta=np.array(BETA, np.float32), src=np.array(src, np.float64), mic=mic, nb_img=np.array(nb_img),
                n_ism=n_ism, n_len=n_ism if n_len is None else n_len, tail_slope=slope)


def _launch(plans, noise=None, fill=7.0):
    """One launch into a buffer pre-filled with ``fill`` -> (B, nch, lmax) numpy."""
    from sar_ssl_amd import hip
    B, nch = len(plans), plans[0]["mic"].shape[0]
    lmax, nism_max = max(p["n_len"] for p in plans), max(p["n_ism"] for p in plans)

    def dev(key, dtype):
        return torch.from_numpy(np.stack([np.asarray(p[key]) for p in plans]).astype(dtype)).cuda()
    out = torch.full((B, nch, lmax), fill, dtype=torch.float32, device="cuda")
    nz = None if noise is None else torch.from_numpy(noise).cuda()
    hip.ism_rir(dev("room", np.float64), dev("beta", np.float32), dev("src", np.float64), dev("mic", np.float64), dev("nb_img", np.int32),
                dev("n_ism", np.int32), dev("n_len", np.int32), dev("tail_slope", np.float32), lmax=lmax, nism_max=nism_max,
                nimg_max=max(int(np.prod(p["nb_img"])) for p in plans), noise=nz, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _restate(p, noise=None):
    from sar_ssl_amd import roomsim
    return roomsim.restate_ism(p["room"], p["beta"], p["src"], p["mic"], p["nb_img"], p["n_ism"], p["n_len"], p["tail_slope"], noise)


def _worst(got, plans, noise=None):
    worst = 0.0
    for b, p in enumerate(plans):
        want = _restate(p, None if noise is None else noise[b])
        assert np.all(got[b, :, p["n_len"]:] == 0.0), "samples from n_len on are written as zero"
        worst = max(worst, np.abs(got[b, :, :p["n_len"]] - want).max() / np.abs(want).max())
    return worst


def _ragged(nch):
    k = 20
    return [_plan(nch, (1, 1, 1), 1, src=(3.4, 2.9, 1.5 + 1e-3)),                                  # n_ism 1: the direct sound's window reaches sample 0
            _plan(nch, (2, 1, 1), 127),
            _plan(nch, (3, 2, 5), 128, src=(3.4, 2.9 + 0.3, 1.5)),                                # 0.3 m from microphone 0: window clipped at sample 0
            _plan(nch, (4, 4, 4), 129),
            _plan(nch, (1, 1, 1), 300, src=(0.0, 2.0, 1.0), mic0=(343.0 * k / 16000, 2.0, 1.0)),  # delay of exactly k samples at microphone 0
            _plan(nch, (4, 4, 4), 300),                                                           # images that straddle n_ism, and wholly past it
            _plan(nch, (3, 2, 5), 200)]


@pytest.mark.parametrize("nch", [1, 2, 3])
def test_ragged_batch_against_the_restatement(nch):
    plans = _ragged(nch)
    p = plans[5]
    got = _launch(plans)
    # the shapes the batch is for are really in it
    from sar_ssl_amd import roomsim
    far = roomsim.restate_ism(p["room"], p["beta"], p["src"], p["mic"], p["nb_img"], 2000)
    assert np.abs(far[:, 300 - 60:300 + 60]).max() > 0 and np.abs(far[:, 400:]).max() > 0
    assert np.abs(got[4, 0, 20] - 1.0 / (4 * np.pi * 343.0 * 20 / 16000)) <= 1e-6 * got[4, 0, 20]
    check("ism ragged nch=%d" % nch, _worst(got, plans), _gate())


@pytest.mark.parametrize("extra", [0, 1, 1000])
def test_tail_with_exactly_two_frames(extra):
    from sar_ssl_amd import roomsim
    plans = [_plan(2, (3, 3, 3), 512, 512 + extra), _plan(2, (4, 3, 3), 700, 700 + extra, slope=-55.0)]
    assert roomsim.tail_frames(_restate(_plan(2, (3, 3, 3), 512))[0], 512)[1] == 2
    lmax = max(p["n_len"] for p in plans)
    noise = np.random.RandomState(3).standard_normal((2, 2, lmax)).astype(np.float32)
    got = _launch(plans, noise)
    check("ism tail +%d" % extra, _worst(got, plans, noise), _gate())
    if extra:
        assert np.abs(got[0, :, 512:512 + extra]).max() > 0


def test_refused_shapes_return_minus_one_and_leave_out_untouched():
    from sar_ssl_amd import _lib, hip
    from sar_ssl_amd._lib import c_double, c_int, c_void_p
    B, lmax = 1, 64
    bufs = dict(room=torch.ones(B, 3, dtype=torch.float64), beta=torch.ones(B, 6), src=torch.ones(B, 3, dtype=torch.float64),
                mic=torch.ones(B, 9, 3, dtype=torch.float64), nb=torch.ones(B, 3, dtype=torch.int32), n=torch.full((B,), lmax, dtype=torch.int32),
                slope=torch.zeros(B))
    bufs = {k: v.cuda() for k, v in bufs.items()}
    out = torch.full((B, 9, lmax + 8), 7.0, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def p(t):
        return c_void_p(t.data_ptr() if t is not None else 0)

    def raw(nch, lmax_, nism_max, nimg_max, noise=None):
        fn = _lib.lib().sarssl_ism_rir
        return fn(p(bufs["room"]), p(bufs["beta"]), p(bufs["src"]), p(bufs["mic"]), p(bufs["nb"]), p(bufs["n"]), p(bufs["n"]), p(bufs["slope"]),
                  p(noise), c_double(16000.0), c_double(343.0), c_int(B), c_int(nch), c_int(lmax_), c_int(nism_max), c_int(nimg_max), p(ws),
                  p(out), c_void_p(torch.cuda.current_stream().cuda_stream))

    assert raw(9, lmax, lmax, 1) == -1                                   # nch > 8
    assert raw(2, lmax, lmax, (1 << 20) + 1) == -1                       # image count above the cap
    assert raw(2, lmax + 8, lmax, 1) == -1                               # a tail (lmax > nism_max) without noise
    assert hip.ism_workspace_bytes(B, 9, lmax, lmax, 1) == -1 and hip.ism_workspace_bytes(B, 2, lmax, lmax, (1 << 20) + 1) == -1
    assert hip.ism_workspace_bytes(B, 2, lmax, lmax, 1 << 20) > 0
    with pytest.raises(_lib.SarsslHipError):
        _launch([_plan(2, (1, 1, 1), 64, 72)], None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert raw(2, lmax, lmax, 1) == 0                                    # the same call with an accepted shape runs
    torch.cuda.synchronize()
    assert bool((out.flatten()[:2 * lmax] != 7.0).any())


def test_bit_reproducible_and_independent_of_batch_position():
    plans = _ragged(2)
    a, b = _launch(plans), _launch(plans, fill=-3.0)
    assert a.tobytes() == b.tobytes()
    for i in (3, 5):
        alone = _launch([plans[i]])
        n = plans[i]["n_len"]
        assert alone[0, :, :n].tobytes() == np.ascontiguousarray(a[i, :, :n]).tobytes()
    tail = [_plan(2, (3, 3, 3), 512, 900), _plan(2, (4, 3, 3), 700, 1500, slope=-55.0), _plan(2, (3, 3, 3), 600, 800)]
    noise = np.random.RandomState(5).standard_normal((3, 2, 1500)).astype(np.float32)
    whole = _launch(tail, noise)
    alone = _launch([tail[1]], noise[1:2])
    assert alone[0].tobytes() == np.ascontiguousarray(whole[1]).tobytes()
    assert whole.tobytes() == _launch(tail, noise).tobytes()


@functools.lru_cache(maxsize=None)
def _fullsize():
    """Rooms idx 0 and 5 of F21 in one launch with uploaded numpy noise, and the restatement: computed once."""
    from sar_ssl_amd import roomsim
    ids = [0, 5]
    cfgs = [_cfg("cfg2/%d" % i) for i in ids]
    batch = roomsim.render_items(dict(zip(ids, cfgs)), ids, SEED, 0, torch.device("cuda:0"), noise="numpy")
    plans, got, got_dp = batch.plans, batch.rir.cpu().numpy(), batch.dp.cpu().numpy()
    want = [roomsim.restate_cfg(c, roomsim.numpy_noise(SEED, i, 0, 2, p["n_len"])) for c, i, p in zip(cfgs, ids, plans)]
    want_dp = [roomsim.restate_cfg(c, dp=True) for c in cfgs]
    return ids, cfgs, plans, got, got_dp, want, want_dp


def test_full_size_rooms_against_the_restatement():
    ids, cfgs, plans, got, got_dp, want, want_dp = _fullsize()
    for b, (p, w, wd) in enumerate(zip(plans, want, want_dp)):
        assert np.all(got[b, :, p["n_len"]:] == 0.0)
        check("ism full size idx %d" % ids[b], np.abs(got[b, :, :p["n_len"]] - w).max() / np.abs(w).max(), _gate())
        check("ism direct path idx %d" % ids[b], np.abs(got_dp[b] - wd).max() / np.abs(wd).max(), _gate())


def test_labels_of_the_gpu_rir_against_the_restatement():
    from sar_ssl_amd import parity, roomsim
    ids, cfgs, plans, got, got_dp, want, want_dp = _fullsize()
    for b, (c, p) in enumerate(zip(cfgs, plans)):
        lg = roomsim.labels(got[b, :, :p["n_len"]], got_dp[b], c)
        lw = roomsim.labels(want[b], want_dp[b], c)
        assert lg["ok"] and lw["ok"]
        check("ism T60_edc idx %d" % ids[b], abs(lg["T60_edc"] - lw["T60_edc"]), min(parity.ISM["t60_gate"], parity.ISM["t60_cap"]))
        for name in ("DRR", "C50"):                      # within one float16 step, the storage quantum
            assert abs(float(lg[name]) - float(lw[name])) <= float(np.spacing(np.abs(lw[name]))), (name, lg[name], lw[name])
        assert lg["TDOA"] == lw["TDOA"]


def test_device_noise_of_an_item_does_not_depend_on_its_batch():
    from sar_ssl_amd import roomsim
    ids, cfgs, plans, got, got_dp, want, want_dp = _fullsize()
    dev = torch.device("cuda:0")
    both = roomsim.device_noise(plans, ids, SEED, 0, dev)
    n = plans[1]["n_len"]
    assert n < plans[0]["n_len"]                                # alone, the second item is drawn into a shorter buffer
    alone = roomsim.device_noise(plans[1:], ids[1:], SEED, 0, dev)
    assert torch.equal(alone[0, :, :n], both[1, :, :n])
    assert not torch.equal(roomsim.device_noise(plans[1:], ids[1:], SEED, 1, dev), alone)
    assert not torch.equal(both[0, :, :n], both[1, :, :n]) and not torch.equal(both[1, 0, :n], both[1, 1, :n])


def test_device_noise_passes_the_envelope_test_on_the_first_attempt():
    from sar_ssl_amd import roomsim
    ids, cfgs, plans, got, got_dp, want, want_dp = _fullsize()
    dev = torch.device("cuda:0")
    rir = roomsim.render(plans, dev, roomsim.device_noise(plans, ids, SEED, 0, dev)).cpu().numpy()
    labs = [roomsim.labels(rir[b, :, :p["n_len"]], got_dp[b], c) for b, (c, p) in enumerate(zip(cfgs, plans))]
    for i, c, lab in zip(ids, cfgs, labs):
        print("device noise idx %d: T60_specify %.4f T60_edc %.4f" % (i, float(c["T60_specify"]), lab["T60_edc"]))
    assert all(lab["ok"] for lab in labs)


def test_simulate_bank_feeds_the_loader(tmp_path):
    import importlib.util
    from sar_ssl_amd import rirsynth, roomsim
    res = roomsim.simulate_bank(str(tmp_path), "train", 4, device="cuda:0", batch=3, log=print)
    assert sorted(res["written"] + res["skipped"]) == [0, 1, 2, 3] and len(res["written"]) >= 2
    d = tmp_path / "train"
    want = {"all_info.npz"} | {"%d%s" % (i, s) for i in res["written"] for s in (".npy", "_dp.npy", "_info.npz")}
    assert {f.name for f in d.iterdir()} == want
    allinfo = np.load(d / "all_info.npz", allow_pickle=True)
    assert len(allinfo["cfgs"]) == 4 and list(allinfo["skipped"]) == res["skipped"]
    for i in res["written"]:
        rir, dp, info = np.load(d / ("%d.npy" % i)), np.load(d / ("%d_dp.npy" % i)), dict(np.load(d / ("%d_info.npz" % i)))
        p = roomsim.plan_rir(allinfo["cfgs"][i])
        assert rir.dtype == np.float32 and rir.shape == (1, 2, p["n_len"], 1) and dp.dtype == np.float32 and dp.shape == (1, 2, 1600, 1)
        assert set(info) == {"room_sz", "T60_sabine", "beta", "T60_specify", "array_type", "mic_pos", "array_scale", "array_rotate_azi", "mic_orV",
                             "mic_pattern", "array_orV", "array_pos", "src_traj_pts", "T60_edc", "TDOA", "DRR", "C50", "fs"}
        assert info["TDOA"].dtype == np.float32 and info["DRR"].dtype == np.float16 and info["C50"].dtype == np.float16 and int(info["fs"]) == 16000
        assert info["beta"].dtype == np.float32 and info["mic_pos"].shape == (2, 3) and abs(float(info["T60_edc"]) - float(info["T60_specify"])) < 0.05
    bank = rirsynth.SimulatedBank([str(d)], sort=True)
    assert len(bank) == len(res["written"]) and bank.nch == 2
    spec = importlib.util.spec_from_file_location("make_golden_rirmix", os.path.join(ROOT, "tools", "make_golden_rirmix.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    root = gen.restore_tree(str(tmp_path / "f20"), dict(np.load(os.path.join(GOLD, "f20_rirmix.npz"), allow_pickle=False)))
    sources = rirsynth.SourceBank(gen.dirs_of(root)["src"], fs=gen.FS, sort=True)
    np.random.seed(1)
    ld = rirsynth.RirSynthLoader(None, bank, sources, dataset_sz=4, batch_size=4, T=gen.T, fs=gen.FS, nmic=2, real_sim_ratio=(0, 1), seed=1,
                                 device="cuda:0")
    sig, labels = next(iter(ld))
    torch.cuda.synchronize()
    assert sig.shape == (4, gen.NS, 2) and bool(torch.isfinite(sig).all()) and float(sig.abs().max()) <= 1.0 and float(sig.abs().max()) > 0


def test_gen_simu_command_line_in_a_fresh_process(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_simu.py"), "--mode", "rir", "--stage", "val", "--data_num", "2", "--save_to", str(tmp_path),
                        "--gpus", "[0]"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    names = {f.name for f in (tmp_path / "val").iterdir()}
    assert "all_info.npz" in names and any(n.endswith("_dp.npy") for n in names)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_simu.py"), "--mode", "sig", "--save_to", str(tmp_path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "only --mode rir" in r.stderr
