"""Simulated RIR banks: image-source room simulation on the GPU.

The reference writes ``data/RIR/simu/<stage>/{idx}.npy``, ``{idx}_dp.npy`` and ``{idx}_info.npz`` with ``gen_simu.py --mode rir``
(GenerateRandomRIR -> MicrophoneSignalOrRIR.generate_rir, code/data_generation/utils_simu_rir_sig.py:672-747) and takes the RIR itself
from gpuRIR, a CUDA-only third-party library that is neither part of the reference nor available here.  This module is that generator:
the host restates everything around the call (``random_spatial_acoustics``: the random room, array and source, draw for draw;
``labels``: check_rir, check_rir_envelope, generate_annotation) and the GPU sums the image sources (hip.ism_rir, csrc/ism.hip).
``restate_ism`` is the f64 numpy statement of one RIR that the kernel is tested against.

PARITY WITH gpuRIR IS UNPINNED: the library cannot be run or read, so the RIR is this project's own image-source model (Allen-Berkley
images, 8 ms Hann-windowed sinc fractional delays, an exponentially decaying noise tail at the Sabine slope).  What is pinned against the
reference is its own code around the call (fixture F21, tools/make_golden_ism.py).
"""
import math
import os
import sys

import numpy as np

FS = 16000
ISM_WINDOW = 128                 # 8 ms at 16 kHz: window of the fractional delay and frame of the tail's level fit
MAX_IMAGES = 1 << 20             # csrc/ism.hip ISM_MAX_IMAGES
MAX_ATTEMPTS = 8
STAGE_SEEDS = {"pretrain": 1, "preval": 2000000, "pretest": 3000000, "train": 4000000, "val": 5000000, "test": 6000000}   # gen_simu.py:69-80

# utils_array.py, by value
MIC_ARRAY_CFG_2CH = {
    "array_type": "planar_linear", "array_scale_range": (0.3, 2), "array_rotate_azi_range": (0, 360),
    "mic_pos_relative": np.array(((-0.05, 0.0, 0.0), (0.05, 0.0, 0.0))), "mic_orV": np.array(((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))),
    "mic_pattern": "omni", "array_orV": np.array([0.0, 1.0, 0.0])}
MIC_ARRAY_CFG_CIRCULAR_4CH = {
    "array_type": "planar_linear", "array_scale_range": (1, 1), "array_rotate_azi_range": (0, 0),
    "mic_pos_relative": np.array(((0.05, 0.0, 0.0), (0.0, 0.05, 0.0), (-0.05, 0.0, 0.0), (0.0, -0.05, 0.0))),
    "mic_orV": np.array(((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0))),
    "mic_pattern": "omni", "array_orV": np.array([0.0, 1.0, 0.0])}
MIC_ARRAYS = {"2ch": MIC_ARRAY_CFG_2CH, "circular_4ch": MIC_ARRAY_CFG_CIRCULAR_4CH}

DEFAULTS = dict(room_sz_range=[(3, 15), (3, 10), (2.5, 6)], T60_range=(0.2, 1.3), abs_weights_range=[(0.5, 1)] * 6,
                array_pos_ratio_range=[(0.2, 0.8), (0.2, 0.8), (0.1, 0.5)], num_source_range=(1, 1), source_state="static",
                min_src_array_dist=0.3, min_src_boundary_dist=0.3, fs=FS, c=343.0, ism_db=12)               # gen_simu.py:38-58


# ---------------------------------------------------------------------------------------------------------------- the two gpuRIR helpers
def att2t(att_db, T60):
    """Time for the Sabine decay to fall by ``att_db`` dB.  THIS PROJECT'S definition of gpuRIR.att2t_SabineEstimator, which the
    reference calls (utils_simu_rir_sig.py:484-485); gpuRIR's source is not available to check it against."""
    return att_db / 60.0 * T60


def t2n(T, room_sz, c=343.0):
    """Images per axis that cover reflections up to time ``T``: ceil(2 T c / room_sz).  THIS PROJECT'S definition of gpuRIR.t2n
    (utils_simu_rir_sig.py:487); gpuRIR's source is not available to check it against."""
    return np.ceil(2.0 * T * c / np.asarray(room_sz, np.float64)).astype(np.int64)


def plan_rir(cfg, fs=FS, c=343.0, ism_db=12, dp=False):
    """What one render needs, from a configuration (RoomImpulseResponse.generate_rir's scalars, utils_simu_rir_sig.py:478-487): image
    counts, the length of the image part n_ism = ceil(Tdiff fs), the output length n_len = ceil(Tmax fs) - gpuRIR pads its output to a
    launch-dependent multiple that cannot be known here; SimulatedBank takes any length - and the tail's slope -60 / T60_sabine."""
    T60 = float(cfg["T60_sabine"])
    if T60 == 0 or dp:
        Tdiff = Tmax = 0.1
        nb_img = np.array([1, 1, 1], np.int64)
    else:
        Tdiff, Tmax = att2t(ism_db, T60), att2t(40, T60)
        if T60 < 0.15:
            Tdiff = Tmax
        nb_img = t2n(Tdiff, cfg["room_sz"], c)
    src = np.asarray(cfg["src_traj_pts"], np.float64)
    if src.shape != (1, 3, 1):
        raise ValueError("one static source only (src_traj_pts of shape %s)" % (src.shape,))
    if cfg["mic_pattern"] != "omni":
        raise ValueError("omnidirectional microphones only (mic_pattern %r)" % (cfg["mic_pattern"],))
    return dict(room=np.asarray(cfg["room_sz"], np.float64), beta=np.asarray(cfg["beta"], np.float32), src=src[0, :, 0].copy(),
                mic=np.asarray(cfg["mic_pos"], np.float64), nb_img=nb_img, n_ism=int(math.ceil(Tdiff * fs)), n_len=int(math.ceil(Tmax * fs)),
                tail_slope=-60.0 / T60 if T60 > 0 else 0.0)


# ---------------------------------------------------------------------------------------------------------------- f64 restatement
def tail_frames(h, n_ism):
    """(start, count) of the level fit's frames: consecutive ISM_WINDOW-sample stretches of the image part h[:n_ism], from the first
    multiple of ISM_WINDOW at least ISM_WINDOW samples behind the first index of max |h|."""
    W = ISM_WINDOW
    peak = int(np.argmax(np.abs(h[:n_ism])))
    start = (peak + W + W - 1) // W * W
    return start, max(0, (n_ism - start) // W)


def restate_ism(room, beta, src, mic, nb_img, n_ism, n_len=None, tail_slope=0.0, noise=None, fs=FS, c=343.0):
    """One RIR in f64, the definition csrc/ism.hip is tested against: room (3,), beta (6,) in the order x0, x1, y0, y1, z0, z1, src (3,),
    mic (nch, 3), nb_img (3,), noise (nch, >= n_len) or None -> (nch, n_len).

    n < n_ism: per axis, image i = 0..N-1 has n = i - N // 2, q = n & 1, k = (n + q) / 2, coordinate (1 - 2q) s + 2 k L and wall factor
    beta0^|k - q| beta1^|k|; an image at distance d adds A 0.5 (1 + cos(2 pi x / W)) sinc(x) at the integer samples with |x| <= W / 2,
    x = n - d / c fs, A = factors / (4 pi d); clipped at sample 0 and at n_ism.
    n_ism <= n < n_len: noise[n] 10^((tail_slope n / fs + level) / 20), level per channel = mean over the frames of ``tail_frames`` of
    10 log10(mean power + 1e-30) - tail_slope t with t the frame's centre: the least-squares intercept at fixed slope.  Fewer than two
    frames is refused."""
    W = ISM_WINDOW
    room, src, mic = np.asarray(room, np.float64), np.asarray(src, np.float64), np.asarray(mic, np.float64)
    beta = np.asarray(beta).astype(np.float64)
    n_len = n_ism if n_len is None else n_len
    assert 1 <= n_ism <= n_len
    pos, fac = [], []
    for a in range(3):
        N = int(nb_img[a])
        n = np.arange(N) - N // 2
        q = n & 1
        k = (n + q) // 2
        pos.append((1 - 2 * q) * src[a] + 2.0 * k * room[a])
        fac.append(beta[2 * a] ** np.abs(k - q) * beta[2 * a + 1] ** np.abs(k))
    P = np.stack(np.meshgrid(*pos, indexing="ij"), -1).reshape(-1, 3)                       # row-major over x, y, z
    G = (fac[0][:, None, None] * fac[1][None, :, None] * fac[2][None, None, :]).reshape(-1)
    j = np.arange(-W // 2, W // 2 + 1)
    out = np.zeros((mic.shape[0], n_len))
    for m in range(mic.shape[0]):
        d = np.sqrt(((P - mic[m]) ** 2).sum(-1))
        keep = d > 0
        tau = d[keep] / c * fs
        A = G[keep] / (4.0 * math.pi * d[keep])
        near = np.floor(tau) - W // 2 < n_ism
        tau, A = tau[near], A[near]
        idx = np.floor(tau).astype(np.int64)[:, None] + j[None, :]
        x = idx - tau[:, None]
        ok = (np.abs(x) <= W / 2) & (idx >= 0) & (idx < n_ism)
        val = A[:, None] * 0.5 * (1.0 + np.cos(2.0 * math.pi * x / W)) * np.sinc(x)
        out[m, :n_ism] = np.bincount(idx[ok], weights=val[ok], minlength=n_ism)[:n_ism]
    if n_len > n_ism:
        if noise is None:
            raise ValueError("n_len > n_ism needs the tail's noise")
        t = np.arange(n_ism, n_len) / fs
        for m in range(mic.shape[0]):
            start, nfr = tail_frames(out[m], n_ism)
            if nfr < 2:
                raise ValueError("the image part leaves %d frame(s) behind its peak for the tail's level fit, two are needed" % nfr)
            fr = out[m, start:start + nfr * W].reshape(nfr, W)
            y = 10.0 * np.log10((fr ** 2).mean(1) + 1e-30)
            tc = (start + W * np.arange(nfr) + 0.5 * (W - 1)) / fs
            level = np.mean(y) - tail_slope * np.mean(tc)
            out[m, n_ism:] = np.asarray(noise, np.float64)[m, n_ism:n_len] * 10.0 ** ((tail_slope * t + level) / 20.0)
    return out


def restate_cfg(cfg, noise=None, fs=FS, c=343.0, ism_db=12, dp=False):
    """restate_ism of a configuration (or of its direct path)."""
    p = plan_rir(cfg, fs, c, ism_db, dp)
    return restate_ism(p["room"], p["beta"], p["src"], p["mic"], p["nb_img"], p["n_ism"], p["n_len"], p["tail_slope"], noise, fs, c)


def numpy_noise(seed, idx, attempt, nch, n):
    """The tail's noise as a host draw keyed by (seed, idx, attempt): (nch, n) f32."""
    return np.random.RandomState([int(seed) & 0xffffffff, int(idx), int(attempt)]).standard_normal((nch, n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- random configurations
def _beta_sabine_estimation(room_sz, T60, abs_weights):
    """Reflection coefficients for a wanted reverberation time (utils_simu_rir_sig.py:100-114), float32 as there."""
    from scipy.optimize import minimize

    def t60error(x, T60, room_sz, abs_weights):
        alpha = x * abs_weights
        Sa = (alpha[0] + alpha[1]) * room_sz[1] * room_sz[2] + \
            (alpha[2] + alpha[3]) * room_sz[0] * room_sz[2] + \
            (alpha[4] + alpha[5]) * room_sz[0] * room_sz[1]
        V = np.prod(room_sz)
        if Sa == 0:
            return T60 - 0
        return abs(T60 - 0.161 * V / Sa)

    abs_weights = np.asarray(abs_weights) / np.array(abs_weights).max()
    result = minimize(t60error, 0.5, args=(T60, room_sz, abs_weights), bounds=[[0, 1]])
    return np.sqrt(1 - result.x * abs_weights).astype(np.float32)


def _t60_is_valid(room_sz, T60, alpha, c, ism_db, th=0.005, eps=1e-4):
    """utils_simu_rir_sig.py:116-131; alpha arrives as float32 (1 - beta^2), as there."""
    Sa = (alpha[0] + alpha[1]) * room_sz[1] * room_sz[2] + \
        (alpha[2] + alpha[3]) * room_sz[0] * room_sz[2] + \
        (alpha[4] + alpha[5]) * room_sz[0] * room_sz[1]
    V = np.prod(room_sz)
    if Sa == 0:
        return False, None           # (the reference has no T60_sabine to return here and fails; with absorption weights >= 0.5 it is unreachable)
    T60_sabine = 0.161 * V / (Sa + eps)
    valid_flag = bool(abs(T60 - T60_sabine) < th)
    beta_prod = np.prod(1 - alpha)
    max_dist = np.sqrt(room_sz[0] ** 2 + room_sz[1] ** 2 + room_sz[2] ** 2)
    ism_time = ism_db / 60 * T60_sabine
    return valid_flag & bool(beta_prod != 0) & bool(ism_time >= 3 * max_dist / c), T60_sabine


def random_spatial_acoustics(rs, seed, idx, mic_array_cfg=None, room_sz_range=None, T60_range=None, abs_weights_range=None,
                             array_pos_ratio_range=None, num_source_range=(1, 1), source_state="static", min_src_array_dist=0.3,
                             min_src_boundary_dist=0.3, c=343.0, ism_db=12):
    """SpatialAcoustics.generate_random_spatial_acoustics (utils_simu_rir_sig.py:23-131, 143-378) on the RandomState ``rs``, draw for
    draw: the room with its T60 / abs_weights retry loop, the array, one static source.  Returns the reference's dictionary."""
    mic_array_cfg = MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
    room_sz_range = DEFAULTS["room_sz_range"] if room_sz_range is None else room_sz_range
    T60_range = DEFAULTS["T60_range"] if T60_range is None else T60_range
    abs_weights_range = DEFAULTS["abs_weights_range"] if abs_weights_range is None else abs_weights_range
    array_pos_ratio_range = DEFAULTS["array_pos_ratio_range"] if array_pos_ratio_range is None else array_pos_ratio_range
    if source_state != "static":
        raise ValueError("static sources only (source_state %r): moving sources are out of scope" % (source_state,))
    if mic_array_cfg["array_type"] != "planar_linear":
        raise ValueError("Undefined array type~")
    rs.seed(seed + idx)
    # random_room
    room_sz = [rs.uniform(*r) for r in room_sz_range]
    valid = False
    while not valid:
        T60_specify = rs.uniform(*T60_range)
        abs_weights = [rs.uniform(*r) for r in abs_weights_range]
        beta = _beta_sabine_estimation(room_sz, T60_specify, abs_weights)
        valid, T60_sabine = _t60_is_valid(room_sz, T60_specify, 1 - beta ** 2, c, ism_db)
    # random_mic_array
    array_pos = np.array([rs.uniform(array_pos_ratio_range[i][0] * room_sz[i], array_pos_ratio_range[i][1] * room_sz[i]) for i in range(3)])
    array_scale = rs.uniform(*mic_array_cfg["array_scale_range"])
    array_rotate = rs.uniform(*mic_array_cfg["array_rotate_azi_range"])
    rot = np.array([[np.cos(array_rotate / 180 * np.pi), -np.sin(array_rotate / 180 * np.pi), 0],
                    [np.sin(array_rotate / 180 * np.pi), np.cos(array_rotate / 180 * np.pi), 0],
                    [0, 0, 1]])
    mic_pos = array_pos + np.dot(rot, mic_array_cfg["mic_pos_relative"].transpose(1, 0)).transpose(1, 0) * array_scale
    mic_orV = np.dot(rot, mic_array_cfg["mic_orV"].transpose(1, 0)).transpose(1, 0)
    orV = np.dot(rot, mic_array_cfg["array_orV"])
    # random_src_trajectory
    num_source = rs.randint(num_source_range[0], num_source_range[-1] + 1)
    if num_source != 1:
        raise ValueError("one source only (%d drawn): several sources are out of scope" % num_source)
    src_pos_min = np.array([0.0, 0.0, 0.0]) + np.array([min_src_boundary_dist] * 3)
    src_pos_max = room_sz - np.array([min_src_boundary_dist] * 3)
    nz = np.nonzero(orV)
    if np.sum(orV) > 0:
        src_pos_min[nz] = array_pos[nz]
        src_pos_min += min_src_array_dist * np.abs(orV)
    else:
        src_pos_max[nz] = array_pos[nz]
        src_pos_max -= min_src_array_dist * np.abs(orV)
    for i in range(3):
        assert src_pos_min[i] <= src_pos_max[i], "Src postion range error: " + str(src_pos_min[i]) + ">" + str(src_pos_max[i])
    src_pos = src_pos_min + rs.random_sample(3) * (src_pos_max - src_pos_min)
    traj_pts = np.array([np.ones((1, 1)) * src_pos]).transpose(1, 2, 0)                     # (1, 3, 1)
    return {"room_sz": room_sz, "T60_sabine": T60_sabine, "beta": beta, "T60_specify": T60_specify,
            "array_type": mic_array_cfg["array_type"], "mic_pos": mic_pos, "array_scale": array_scale, "array_rotate_azi": array_rotate,
            "mic_orV": mic_orV, "mic_pattern": mic_array_cfg["mic_pattern"], "array_orV": orV, "array_pos": array_pos,
            "src_traj_pts": traj_pts}


# ---------------------------------------------------------------------------------------------------------------- labels
def check_rir(rir):
    """RoomImpulseResponse.check_rir (utils_simu_rir_sig.py:510-524): no NaN, no Inf, not all zero."""
    rir = np.asarray(rir, np.float64)
    return bool(not np.isnan(rir).any() and not np.isinf(rir).any() and np.sum(rir ** 2) != 0)


def _rt60_from_rir(h, fs, eps=1e-10):
    """__cal_edc + __cal_rt60 (utils_simu_rir_sig.py:551-614): Schroeder curve, a line through every [st, st + duration] dB stretch of it,
    the T60 of the best correlated one."""
    from scipy.stats import linregress
    max_idx = np.argmax(h)
    edc = 10.0 * np.log10(np.cumsum(h[::-1] ** 2)[::-1] / (np.sum(h[max_idx:] ** 2) + eps) + eps)
    times = np.arange(len(edc)) / fs

    def nearest(value):
        v = edc[(np.abs(edc - value)).argmin()]
        return np.where(edc == v)[0][0]

    t60s, rs = [], []
    for st0 in range(-5, -20, -2):
        for dur in range(-10, -30, -2):
            st, ed = nearest(st0), nearest(st0 + dur)
            if abs(st - ed) > 1:
                res = linregress(times[st:ed], edc[st:ed])
                t60s.append(-60 / (res.slope + eps))
                rs.append(res.rvalue)
            else:
                t60s.append(np.nan)
                rs.append(0)
    i = np.argmax(abs(np.array(rs)))
    return t60s[i], rs[i]


def check_rir_envelope(rir, T60_specify, fs=FS):
    """RoomImpulseResponse.check_rir_envelope (utils_simu_rir_sig.py:526-540) on rir (nch, L): -> (ok, T60_edc).  T60_edc is the mean
    over the microphones; the correlation that is tested is the LAST microphone's, as there."""
    rir = np.asarray(rir, np.float64)
    res = [_rt60_from_rir(rir[m], fs) for m in range(rir.shape[0])]
    t60_edc = np.mean([r[0] for r in res])
    corr = res[-1][1]
    return bool(abs(t60_edc - T60_specify) < 0.05) & bool(abs(corr) > 0.5), t60_edc


def annotations(rir, rir_dp, cfg, fs=FS, c=343.0, eps=1e-8):
    """generate_annotation(TDOA, DRR, C50, src_single_static=True) (utils_simu_rir_sig.py:863-994) for rir (nch, L), rir_dp (nch, Ld):
    TDOA float32, DRR and C50 float16, of the reference channel."""
    rir, rir_dp = np.asarray(rir, np.float64), np.asarray(rir_dp, np.float64)
    mic, src = np.asarray(cfg["mic_pos"], np.float64), np.asarray(cfg["src_traj_pts"], np.float64)[0, :, 0]
    dist = np.sqrt(np.sum((src[None, :] - mic) ** 2, axis=1))
    out = {"TDOA": ((dist[1] - dist[0]) / c).astype(np.float32)}
    nsamp = max(rir.shape[1], rir_dp.shape[1])
    h = np.concatenate([rir[0], np.zeros(nsamp - rir.shape[1])])
    nd = np.argmax(np.concatenate([rir_dp[0], np.zeros(nsamp - rir_dp.shape[1])]))
    n = np.arange(nsamp)
    n0 = int(fs * 2.5 / 1000)
    dp_range = ((n >= nd - n0) & (n <= nd + n0)).astype("float")
    dp_pow, rev_pow = np.sum(h ** 2 * dp_range), np.sum(h ** 2 * (np.ones_like(dp_range) - dp_range))
    out["DRR"] = (10 * np.log10(dp_pow / (rev_pow + eps) + eps)).astype(np.float16)
    n0 = int(fs * 50 / 1000)
    early = (n <= nd + n0).astype("float")
    early_pow, late_pow = np.sum(h ** 2 * early), np.sum(h ** 2 * (np.ones_like(early) - early))
    out["C50"] = (10 * np.log10(early_pow / (late_pow + eps) + eps)).astype(np.float16)
    return out


def labels(rir, rir_dp, cfg, fs=FS, c=343.0):
    """The accept test and the annotations of one RIR, in f64 on the values as given (a float32 RIR is widened first): check_rir on both,
    check_rir_envelope against cfg['T60_specify'], TDOA / DRR / C50.  -> dict(ok, rir_ok, env_ok, T60_edc, TDOA, DRR, C50).  Host
    arithmetic on a read-back RIR, once per RIR."""
    rir_ok = check_rir(rir) & check_rir(rir_dp)
    out = dict(rir_ok=rir_ok, env_ok=False, T60_edc=np.float64(np.nan))
    if rir_ok:
        out["env_ok"], out["T60_edc"] = check_rir_envelope(rir, cfg["T60_specify"], fs)
    out["ok"] = rir_ok & out["env_ok"]
    out.update(annotations(rir, rir_dp, cfg, fs, c))
    return out


# ---------------------------------------------------------------------------------------------------------------- GPU render
def _check_tail_frames(p, fs, c):
    """The refusal of restate_ism, before a launch: the direct sound's arrival bounds the peak."""
    if p["n_len"] == p["n_ism"]:
        return
    W = ISM_WINDOW
    for m in range(p["mic"].shape[0]):
        peak = int(np.linalg.norm(p["src"] - p["mic"][m]) / c * fs) + 1
        start = (peak + W + W - 1) // W * W
        if (p["n_ism"] - start) // W < 2:
            raise ValueError("n_ism = %d leaves fewer than two %d-sample frames behind the direct sound (sample %d) for the tail's level fit"
                             % (p["n_ism"], W, peak))


def render(plans, device, noise=None, fs=FS, c=343.0):
    """One hip.ism_rir launch for a list of ``plan_rir`` results -> (B, nch, lmax) f32 on the device.  noise: (B, nch, lmax) f32 device
    tensor, or None when no plan has a tail."""
    import torch
    from . import hip
    B, nch = len(plans), plans[0]["mic"].shape[0]
    for p in plans:
        assert p["mic"].shape == (nch, 3)
        _check_tail_frames(p, fs, c)
    lmax, nism_max = max(p["n_len"] for p in plans), max(p["n_ism"] for p in plans)
    nimg_max = max(int(np.prod(p["nb_img"])) for p in plans)
    if nimg_max > MAX_IMAGES:
        raise ValueError("%d image sources in one RIR, at most %d are rendered" % (nimg_max, MAX_IMAGES))

    def dev(key, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(p[key]) for p in plans]), dtype)).to(device)
    return hip.ism_rir(dev("room", np.float64), dev("beta", np.float32), dev("src", np.float64), dev("mic", np.float64), dev("nb_img", np.int32),
                       dev("n_ism", np.int32), dev("n_len", np.int32), dev("tail_slope", np.float32), lmax=lmax, nism_max=nism_max,
                       nimg_max=nimg_max, noise=noise, fs=float(fs), c=float(c))


def device_noise(plans, ids, seed, attempt, device):
    """(B, nch, lmax) f32 standard normal values on the device: item b from sarssl_gauss_fill keyed by (seed, ids[b], attempt).  Drawn in
    gauss_fill's own (sample, channel) order and transposed, so that the value at (channel, sample) of an item is a function of that key
    alone - not of the longest item of the batch it is rendered in."""
    import torch
    from . import hip
    nch, lmax = plans[0]["mic"].shape[0], max(p["n_len"] for p in plans)
    white = torch.empty((len(plans), lmax, nch), dtype=torch.float32, device=device)
    for b, idx in enumerate(ids):
        hip.gauss_fill(white[b:b + 1], (int(seed) & 0xffffffff) | (int(attempt) << 32), int(idx))
    return white.transpose(1, 2).contiguous()


def host_noise(plans, ids, seed, attempt, device):
    """The same from ``numpy_noise``, uploaded."""
    import torch
    nch, lmax = plans[0]["mic"].shape[0], max(p["n_len"] for p in plans)
    noise = np.zeros((len(plans), nch, lmax), np.float32)
    for b, (p, idx) in enumerate(zip(plans, ids)):
        noise[b, :, :p["n_len"]] = numpy_noise(seed, idx, attempt, nch, p["n_len"])
    return torch.from_numpy(noise).to(device)


# ---------------------------------------------------------------------------------------------------------------- the generator
def simulate_bank(save_to, stage="train", data_num=1024, mic_array_cfg=None, device="cuda", noise="device", batch=16, log=None, **ranges):
    """GenerateRandomRIR (gen_simu.py:38-176): ``data_num`` random configurations of ``stage`` (its seed as there), their RIRs and direct
    paths rendered in batches on ``device``, the reference's accept test on the host, and per accepted item ``{idx}.npy`` (1, nch, L, 1)
    float32, ``{idx}_dp.npy`` and ``{idx}_info.npz`` (configuration, annotations, fs) under ``save_to/stage``, with ``all_info.npz``.

    The tail's noise is keyed by (seed, idx, attempt): noise="device" - sarssl_gauss_fill, "numpy" - an uploaded host draw.  An item that
    fails the accept test is rendered again with the next attempt; the reference retries forever, here an item is skipped after
    MAX_ATTEMPTS with a logged line and listed in all_info.npz (SimulatedBank globs ``*_dp.npy``, so a gap is harmless).
    ranges: room_sz_range, T60_range, abs_weights_range, array_pos_ratio_range, num_source_range, source_state, min_src_array_dist,
    min_src_boundary_dist, fs, c, ism_db (DEFAULTS).  -> dict(written=[idx], skipped=[idx], attempts={idx: n})."""
    import torch
    assert noise in ("device", "numpy")
    unknown = set(ranges) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown arguments: %s" % sorted(unknown))
    args = dict(DEFAULTS, **ranges)
    fs, c, ism_db = args["fs"], args["c"], args["ism_db"]
    if fs != FS:
        raise ValueError("fs = %s: the renderer's window and frames are defined at %d Hz only" % (fs, FS))
    if stage not in STAGE_SEEDS:
        raise ValueError("unknown stage %r (one of %s)" % (stage, sorted(STAGE_SEEDS)))
    log = log or (lambda s: print(s, file=sys.stderr, flush=True))
    seed = STAGE_SEEDS[stage]
    mic_array_cfg = MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
    out_dir = os.path.join(save_to, stage)
    os.makedirs(out_dir, exist_ok=True)
    rs = np.random.RandomState()
    draw = {k: args[k] for k in DEFAULTS if k != "fs"}
    cfgs = [random_spatial_acoustics(rs, seed, idx, mic_array_cfg=mic_array_cfg, **draw) for idx in range(data_num)]
    dev = torch.device(device)
    make_noise = device_noise if noise == "device" else host_noise

    def read_back(t, plans):
        h = t.cpu().numpy()
        return [h[b, :, :p["n_len"]] for b, p in enumerate(plans)]

    dps = {}
    for i0 in range(0, data_num, batch):
        ids = list(range(i0, min(i0 + batch, data_num)))
        plans = [plan_rir(cfgs[i], fs, c, ism_db, dp=True) for i in ids]
        dps.update(zip(ids, read_back(render(plans, dev, None, fs, c), plans)))
    pending, written, attempts = list(range(data_num)), [], {}
    for attempt in range(MAX_ATTEMPTS):
        failed = []
        for i0 in range(0, len(pending), batch):
            ids = pending[i0:i0 + batch]
            plans = [plan_rir(cfgs[i], fs, c, ism_db) for i in ids]
            has_tail = any(p["n_len"] > p["n_ism"] for p in plans)
            rirs = read_back(render(plans, dev, make_noise(plans, ids, seed, attempt, dev) if has_tail else None, fs, c), plans)
            for idx, rir in zip(ids, rirs):
                lab = labels(rir, dps[idx], cfgs[idx], fs, c)
                attempts[idx] = attempt + 1
                if not lab["ok"]:
                    failed.append(idx)
                    continue
                cfg = dict(cfgs[idx], T60_edc=lab["T60_edc"])
                np.save(os.path.join(out_dir, "%d.npy" % idx), rir[None, :, :, None].astype(np.float32))
                np.save(os.path.join(out_dir, "%d_dp.npy" % idx), dps[idx][None, :, :, None].astype(np.float32))
                np.savez(os.path.join(out_dir, "%d_info.npz" % idx), **cfg, TDOA=lab["TDOA"], DRR=lab["DRR"], C50=lab["C50"], fs=fs)
                written.append(idx)
        pending = failed
        if not pending:
            break
    for idx in pending:
        log("simulate_bank: item %d of stage %s failed the accept test %d times and is skipped" % (idx, stage, MAX_ATTEMPTS))
    np.savez_compressed(os.path.join(out_dir, "all_info.npz"), args=dict(args, stage=stage, data_num=data_num, seed=seed, noise=noise),
                        cfgs=cfgs, skipped=np.array(pending, np.int64))
    return dict(written=sorted(written), skipped=pending, attempts=attempts)


# ---------------------------------------------------------------------------------------------------------------- command line
def _literal(text):
    import ast
    return ast.literal_eval(text)


def main(argv=None):
    """``gen_simu.py --mode rir`` with the reference's flag names (argparse; lists are written as Python literals, e.g. --gpus [0])."""
    import argparse
    ap = argparse.ArgumentParser(description="Generate simulated RIRs (image-source model on the GPU)")
    ap.add_argument("--mode", type=str, default="rir")
    ap.add_argument("--stage", type=str, default="train")
    ap.add_argument("--data_num", type=int, default=1024)
    ap.add_argument("--save_to", type=str, default="")
    ap.add_argument("--gpus", type=_literal, default=[0])
    ap.add_argument("--room_sz_range", type=_literal, default=DEFAULTS["room_sz_range"])
    ap.add_argument("--T60_range", type=_literal, default=DEFAULTS["T60_range"])
    ap.add_argument("--abs_weights_range", type=_literal, default=DEFAULTS["abs_weights_range"])
    ap.add_argument("--array_pos_ratio_range", type=_literal, default=DEFAULTS["array_pos_ratio_range"])
    ap.add_argument("--num_source_range", type=_literal, default=DEFAULTS["num_source_range"])
    ap.add_argument("--source_state", type=str, default="static")
    ap.add_argument("--min_src_array_dist", type=float, default=0.3)
    ap.add_argument("--min_src_boundary_dist", type=float, default=0.3)
    ap.add_argument("--mic_pattern", type=str, default="omni")
    ap.add_argument("--fs", type=int, default=FS)
    ap.add_argument("--c", type=float, default=343.0)
    ap.add_argument("--ism_db", type=float, default=12)
    ap.add_argument("--mic_array", type=str, default="2ch", choices=sorted(MIC_ARRAYS))
    ap.add_argument("--noise", type=str, default="device", choices=("device", "numpy"))
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args(argv)
    if a.mode != "rir":
        ap.error("--mode %s: only --mode rir is built (microphone signals come from run_downstream.py's loader, not from files)" % a.mode)
    if "moving" in a.source_state or a.source_state != "static":
        ap.error("--source_state %s: static sources only" % a.source_state)
    if tuple(a.num_source_range) != (1, 1):
        ap.error("--num_source_range %s: one source only" % (a.num_source_range,))
    if a.mic_pattern != "omni":
        ap.error("--mic_pattern %s: omnidirectional microphones only" % a.mic_pattern)
    if a.fs != FS:
        ap.error("--fs %d: %d Hz only" % (a.fs, FS))
    if not a.save_to:
        ap.error("--save_to is required")
    gpus = a.gpus if isinstance(a.gpus, (list, tuple)) else [a.gpus]
    import torch
    torch.cuda.set_device(int(gpus[0]))                  # one process on the first listed GPU
    res = simulate_bank(a.save_to, a.stage, a.data_num, MIC_ARRAYS[a.mic_array], device="cuda:%d" % int(gpus[0]), noise=a.noise, batch=a.batch,
                        room_sz_range=a.room_sz_range, T60_range=a.T60_range, abs_weights_range=a.abs_weights_range,
                        array_pos_ratio_range=a.array_pos_ratio_range, num_source_range=a.num_source_range, source_state=a.source_state,
                        min_src_array_dist=a.min_src_array_dist, min_src_boundary_dist=a.min_src_boundary_dist, c=a.c, ism_db=a.ism_db)
    print("%d RIRs written to %s, %d skipped" % (len(res["written"]), os.path.join(a.save_to, a.stage), len(res["skipped"])))
    return 0
