"""CPU: the host layer of the simulated-RIR generator (sar_ssl_amd.roomsim) against fixture F21 of the real reference
(tools/make_golden_ism.py) and the f64 restatement of the image-source model against its own definition."""
import math
import os

import numpy as np
import pytest

from sar_ssl_amd import roomsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4000000


@pytest.fixture(scope="module")
def f21():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "f21_roomsim.npz"), allow_pickle=False))


def _cfg(f21, prefix):
    pre = prefix + "/"
    return {k[len(pre):]: f21[k] for k in f21 if k.startswith(pre)}


def _same_cfg(got, want):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        g = np.asarray(got[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (k, g, w)
    assert np.asarray(got["beta"]).dtype == np.float32


def test_random_spatial_acoustics_equals_the_reference_key_by_key(f21):
    rs = np.random.RandomState()
    for idx in range(16):
        _same_cfg(roomsim.random_spatial_acoustics(rs, SEED, idx), _cfg(f21, "cfg2/%d" % idx))
    for idx in range(4):
        _same_cfg(roomsim.random_spatial_acoustics(rs, SEED, idx, mic_array_cfg=roomsim.MIC_ARRAY_CFG_CIRCULAR_4CH), _cfg(f21, "cfg4/%d" % idx))
    for k in range(2):
        got = roomsim.random_spatial_acoustics(rs, SEED, k, T60_range=tuple(f21["small_T60_range"]),
                                               room_sz_range=[tuple(r) for r in f21["small_room_sz_range"]])
        _same_cfg(got, _cfg(f21, "rir/%d/cfg" % k))


def test_labels_equal_the_reference_on_the_stored_rirs(f21):
    for k in range(2):
        cfg = _cfg(f21, "rir/%d/cfg" % k)
        lab = roomsim.labels(f21["rir/%d/rir" % k], f21["rir/%d/rir_dp" % k], cfg)
        assert abs(lab["T60_edc"] - float(f21["rir/%d/T60_edc" % k])) <= 1e-9
        assert lab["env_ok"] == bool(f21["rir/%d/env_ok" % k]) and lab["rir_ok"] == bool(f21["rir/%d/rir_ok" % k])
        for name in ("TDOA", "DRR", "C50"):
            want = f21["rir/%d/%s" % (k, name)]
            assert lab[name].dtype == want.dtype and lab[name].tobytes() == want.tobytes(), (name, lab[name], want)
        assert lab["TDOA"].dtype == np.float32 and lab["DRR"].dtype == np.float16 and lab["C50"].dtype == np.float16


def test_stored_rirs_are_the_restatement(f21):
    for k in range(2):
        cfg = _cfg(f21, "rir/%d/cfg" % k)
        p = roomsim.plan_rir(cfg)
        noise = roomsim.numpy_noise(SEED, k, 0, 2, p["n_len"])
        assert np.array_equal(roomsim.restate_cfg(cfg, noise).astype(np.float32), f21["rir/%d/rir" % k])
        assert np.array_equal(roomsim.restate_cfg(cfg, dp=True).astype(np.float32), f21["rir/%d/rir_dp" % k])


@pytest.mark.parametrize("k", [5, 37, 800])
def test_single_image_with_an_integer_delay_is_one_tap(k):
    d = 343.0 * k / 16000
    h = roomsim.restate_ism([50.0, 50.0, 50.0], [0.5] * 6, [0.0, 10.0, 10.0], [[d, 10.0, 10.0]], [1, 1, 1], 1000)[0]   # (source on a wall: the coordinate difference is d exactly)
    A = 1.0 / (4 * math.pi * d)
    # d / c * fs is k up to a few ulp of k in f64; the other taps are A sinc(x) there, |sinc| <= the delay's rounding error
    tol = 8 * k * 2.0 ** -52 * A
    assert abs(h[k] - A) <= tol
    h[k] = 0.0
    assert np.abs(h).max() <= tol


def test_mirroring_an_axis_and_swapping_its_betas_gives_the_same_rir():
    room, src = np.array([5.0, 4.0, 3.0]), np.array([1.3, 2.9, 1.1])
    mic = np.array([[3.1, 1.2, 1.6], [3.3, 1.25, 1.5]])
    beta = np.array([0.9, 0.7, 0.8, 0.6, 0.5, 0.85])
    base = roomsim.restate_ism(room, beta, src, mic, [5, 7, 5], 900)
    for a in range(3):
        s2, m2, b2 = src.copy(), mic.copy(), beta.copy()
        s2[a], m2[:, a] = room[a] - src[a], room[a] - mic[:, a]
        b2[2 * a], b2[2 * a + 1] = beta[2 * a + 1], beta[2 * a]
        got = roomsim.restate_ism(room, b2, s2, m2, [5, 7, 5], 900)
        assert np.abs(got - base).max() <= 1e-12 * np.abs(base).max()       # (the mirrored coordinates round differently in f64)


def test_t2n_and_att2t_are_the_stated_definitions():
    assert roomsim.att2t(12, 0.5) == 12 / 60 * 0.5 and roomsim.att2t(40, 1.3) == 40 / 60 * 1.3
    assert list(roomsim.t2n(0.1, [3.0, 10.0, 2.5], 343.0)) == [math.ceil(2 * 0.1 * 343 / 3.0), math.ceil(2 * 0.1 * 343 / 10.0), math.ceil(2 * 0.1 * 343 / 2.5)]
    cfg = dict(T60_sabine=1.3, room_sz=[3.0, 4.0, 5.0], beta=np.ones(6, np.float32), mic_pos=np.zeros((2, 3)), mic_pattern="omni",
               src_traj_pts=np.ones((1, 3, 1)))
    p = roomsim.plan_rir(cfg)
    assert p["n_ism"] == 4160 and p["n_len"] == math.ceil(40 / 60 * 1.3 * 16000) == 13867 and p["tail_slope"] == -60 / 1.3
    d = roomsim.plan_rir(cfg, dp=True)
    assert list(d["nb_img"]) == [1, 1, 1] and d["n_ism"] == d["n_len"] == 1600


def test_tail_is_refused_without_noise_or_without_two_frames():
    args = ([5.0, 4.0, 3.0], [0.8] * 6, [1.0, 1.0, 1.0], [[2.0, 1.0, 1.0]], [3, 3, 3])
    with pytest.raises(ValueError):
        roomsim.restate_ism(*args, 600, 700)
    with pytest.raises(ValueError):                           # peak at sample 46: frames from 256, one fits into 400
        roomsim.restate_ism(*args, 400, 500, -60.0, np.ones((1, 500), np.float32))
    roomsim.restate_ism(*args, 512, 600, -60.0, np.ones((1, 600), np.float32))     # exactly two


@pytest.mark.parametrize("idx", [0, 1, 5, 6, 8, 9, 15])
def test_restated_rirs_pass_the_envelope_test(f21, idx):
    cfg = _cfg(f21, "cfg2/%d" % idx)
    p = roomsim.plan_rir(cfg)
    rir = roomsim.restate_cfg(cfg, roomsim.numpy_noise(SEED, idx, 0, 2, p["n_len"]))
    ok, t60 = roomsim.check_rir_envelope(rir, float(cfg["T60_specify"]))
    print("idx %d: T60_specify %.4f T60_edc %.4f images %d" % (idx, float(cfg["T60_specify"]), t60, int(np.prod(p["nb_img"]))))
    assert ok
