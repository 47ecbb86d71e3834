"""Simulated RIR banks and the simulated pretraining corpus: image-source room simulation on the GPU.

The reference writes ``data/RIR/simu/<stage>/{idx}.npy``, ``{idx}_dp.npy`` and ``{idx}_info.npz`` with ``gen_simu.py --mode rir``
(GenerateRandomRIR -> MicrophoneSignalOrRIR.generate_rir, code/data_generation/utils_simu_rir_sig.py:672-747) and takes the RIR itself
from gpuRIR, a CUDA-only third-party library that is neither part of the reference nor available here.  This module is that generator:
the host restates everything around the call (``random_spatial_acoustics``: the random room, array and source, draw for draw;
``labels``: check_rir, check_rir_envelope, generate_annotation) and the GPU sums the image sources (hip.ism_rir, csrc/ism.hip).
``restate_ism`` is the f64 numpy statement of one RIR that the kernel is tested against.

``gen_simu.py --mode sig`` (GenerateRandomMicSig -> generate_microphone_signal, utils_simu_rir_sig.py:749-861) is ``simulate_signals``:
the same RIRs judged on the device (hip.rir_labels, csrc/rirlabel.hip - ``labels_twin`` is its arithmetic in numpy), convolved with a
WSJ0-style source, mixed with the diffuse white-noise field at a drawn SNR, converted to PCM-16 and written as ``{idx}.wav`` +
``{idx}_info.npz`` without the RIR leaving the GPU; ``plan_sig`` restates the reference's draws and ``restate_sig`` one item in f64
(fixture F22, tools/make_golden_simsig.py).  The float -> PCM-16 rule is this project's reading of libsndfile's and UNPINNED (``pcm16``).
Both generators are one loop (``_generate``: ``render_items``, the judge on the host or the device, retries) with their own sink.
The signals' sink (``_signal_sink``: gather of the accepted rows, noise, mix, pack) also serves onlinesig.OnlineSignalLoader, which hands
the packed batches to the training step instead of a writer (run_pretrain.py --simu-online) and draws its rooms with
``random_room(beta_solver="closed")``: Sabine's equation solved exactly instead of by scipy.optimize.minimize.

``gen_simu_certain_room.py --mode rir | sig`` (GenerateRandomRIROfCertainRoom / GenerateRandomMicSigOfCertainRoom) is ``simulate_room_bank``
/ ``simulate_room_signals``: a fixed number of rooms drawn once each (``random_room``), placements on each room
(``random_spatial_acoustics(room_cfg=...)``), signals per placement, written as ``<stage>/R{n}/...`` - the corpus of the downstream
sweep.  All rooms' items share one id space and the same loop and sinks; the diffuse field's mixing table is formed on the device
(hip.mixing_table).  Fixture F23 (tools/make_golden_certainroom.py) pins the reference's seed and directory arithmetic.

PARITY WITH gpuRIR IS UNPINNED: the library cannot be run or read, so the RIR is this project's own image-source model (Allen-Berkley
images, 8 ms Hann-windowed sinc fractional delays, an exponentially decaying noise tail at the Sabine slope).  What is pinned against the
reference is its own code around the call (fixture F21, tools/make_golden_ism.py).
"""
import collections
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


def sabine_x_closed(room_sz, T60, abs_weights):
    """The exact minimiser of ``_beta_sabine_estimation``'s t60error over [0, 1]: T60 = 0.161 V / (x S_w) solved for x and clipped, with
    w = abs_weights / max(abs_weights) and S_w = (w0 + w1) Ly Lz + (w2 + w3) Lx Lz + (w4 + w5) Lx Ly -> (x, w), f64."""
    w = np.asarray(abs_weights, np.float64) / np.max(abs_weights)
    Sw = (w[0] + w[1]) * room_sz[1] * room_sz[2] + (w[2] + w[3]) * room_sz[0] * room_sz[2] + (w[4] + w[5]) * room_sz[0] * room_sz[1]
    return float(np.clip(0.161 * np.prod(room_sz) / (T60 * Sw), 0.0, 1.0)), w


def _beta_sabine_closed(room_sz, T60, abs_weights):
    """``_beta_sabine_estimation`` without the optimiser (beta_solver="closed"): its exact solution, float32 as there.  Within 1.1e-3 of
    the minimiser's beta - the minimiser's own imprecision - and never further from the wanted T60."""
    x, w = sabine_x_closed(room_sz, T60, abs_weights)
    return np.sqrt(1 - x * w).astype(np.float32)


BETA_SOLVERS = {"minimize": "_beta_sabine_estimation", "closed": "_beta_sabine_closed"}


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


def _draw_ranges(room_sz_range, T60_range, abs_weights_range):
    return (DEFAULTS["room_sz_range"] if room_sz_range is None else room_sz_range, DEFAULTS["T60_range"] if T60_range is None else T60_range,
            DEFAULTS["abs_weights_range"] if abs_weights_range is None else abs_weights_range)


def random_room(rs, room_sz_range=None, T60_range=None, abs_weights_range=None, c=343.0, ism_db=12, beta_solver="minimize"):
    """SpatialAcoustics.random_room with room_cfg=None (utils_simu_rir_sig.py:74-98) on the RandomState ``rs`` where it stands, draw for
    draw: the room size, then the T60 / abs_weights retry loop -> dict(room_sz, T60_sabine, beta, T60_specify).
    beta_solver: "minimize" - the reference's scipy.optimize.minimize (2.6-12 ms a room); "closed" - its exact solution
    (``_beta_sabine_closed``; the online loader's, which draws rooms at training rate).  The draws and the accept test are the same."""
    if beta_solver not in BETA_SOLVERS:
        raise ValueError("beta_solver %r: one of %s" % (beta_solver, sorted(BETA_SOLVERS)))
    solve = globals()[BETA_SOLVERS[beta_solver]]
    room_sz_range, T60_range, abs_weights_range = _draw_ranges(room_sz_range, T60_range, abs_weights_range)
    room_sz = [rs.uniform(*r) for r in room_sz_range]
    valid = False
    while not valid:
        T60_specify = rs.uniform(*T60_range)
        abs_weights = [rs.uniform(*r) for r in abs_weights_range]
        beta = solve(room_sz, T60_specify, abs_weights)
        valid, T60_sabine = _t60_is_valid(room_sz, T60_specify, 1 - beta ** 2, c, ism_db)
    return {"room_sz": room_sz, "T60_sabine": T60_sabine, "beta": beta, "T60_specify": T60_specify}


def random_spatial_acoustics(rs, seed, idx, mic_array_cfg=None, room_sz_range=None, T60_range=None, abs_weights_range=None,
                             array_pos_ratio_range=None, num_source_range=(1, 1), source_state="static", min_src_array_dist=0.3,
                             min_src_boundary_dist=0.3, c=343.0, ism_db=12, room_cfg=None, beta_solver="minimize", reseed=True):
    """SpatialAcoustics.generate_random_spatial_acoustics (utils_simu_rir_sig.py:23-131, 143-378) on the RandomState ``rs``, draw for
    draw, after seed + idx: the room (``random_room``, with its ``beta_solver``; with a ``room_cfg`` that room is taken and only what
    follows is drawn, :43-70), the array, one static source.  Returns the reference's dictionary.
    reseed=False: ``rs`` is taken where it stands (the online loader seeds it per item with an array; seed and idx are then unused)."""
    mic_array_cfg = MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
    array_pos_ratio_range = DEFAULTS["array_pos_ratio_range"] if array_pos_ratio_range is None else array_pos_ratio_range
    if source_state != "static":
        raise ValueError("static sources only (source_state %r): moving sources are out of scope" % (source_state,))
    if mic_array_cfg["array_type"] != "planar_linear":
        raise ValueError("Undefined array type~")
    if reseed:
        rs.seed(seed + idx)
    if room_cfg is None:
        room_cfg = random_room(rs, room_sz_range, T60_range, abs_weights_range, c, ism_db, beta_solver)
    room_sz = room_cfg["room_sz"]
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
    return {"room_sz": room_sz, "T60_sabine": room_cfg["T60_sabine"], "beta": room_cfg["beta"], "T60_specify": room_cfg["T60_specify"],
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
    out = {"TDOA": tdoa(cfg, c)}
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


def tdoa(cfg, c=343.0):
    """The TDOA annotation alone (geometry only): float32, as ``annotations`` returns it."""
    mic, src = np.asarray(cfg["mic_pos"], np.float64), np.asarray(cfg["src_traj_pts"], np.float64)[0, :, 0]
    dist = np.sqrt(np.sum((src[None, :] - mic) ** 2, axis=1))
    return ((dist[1] - dist[0]) / c).astype(np.float32)


LABEL_TARGETS = -5.0 - 2.0 * np.arange(22)          # the 22 distinct dB levels of the 80 stretches: -5, -7 .. -47


def labels_twin(rir, rir_dp, T60_specify, fs=FS):
    """The arithmetic of csrc/rirlabel.hip (sarssl_rir_labels) in numpy on rir (nch, L), rir_dp (nch, Ld): what ``labels`` computes, by
    the kernel's route - the 80 line fits in closed form from suffix sums of (E + 26), (E + 26)^2 and (n - L / 2)(E + 26) and the variance
    of consecutive integers instead of 80 calls of scipy.stats.linregress - and with the kernel's outputs: dict(t60, corr (nch,), t60_edc,
    drr, c50, nd, flags; bit 0 rir_ok, bit 1 env_ok), DRR / C50 unrounded.  Agrees with ``labels`` to rounding (tests/test_simsig_cpu.py)."""
    rir, rir_dp = np.asarray(rir, np.float64), np.asarray(rir_dp, np.float64)
    nch, L = rir.shape
    Ld = rir_dp.shape[1]
    fs = float(fs)

    def ok(x):
        return bool(np.isfinite(x).all() and (x != 0).any())
    rir_ok = ok(rir) and ok(rir_dp)
    t60, corr = np.full(nch, np.nan), np.full(nch, np.nan)
    for m in range(nch if rir_ok else 0):
        h = rir[m]
        S = np.cumsum(h[::-1] ** 2)[::-1]
        E = 10.0 * np.log10(S / (S[np.argmax(h)] + 1e-10) + 1e-10)
        near = [int(np.argmin(np.abs(E - v))) for v in LABEL_TARGETS]
        y = E + 26.0
        xc = 0.5 * L

        def suffix(v):
            return np.concatenate([np.cumsum(v[::-1])[::-1], [0.0]])
        Q0, Q1, Q2 = suffix(y), suffix(y * y), suffix((np.arange(L) - xc) * y)
        rs, ts = [], []
        for a in range(8):
            for d in range(10):
                st, ed = near[a], near[a + 5 + d]
                if abs(st - ed) > 1 and ed > st:
                    N = float(ed - st)
                    sy, syy, sxy = Q0[st] - Q0[ed], Q1[st] - Q1[ed], Q2[st] - Q2[ed]
                    xm = 0.5 * (st + ed - 1) - xc
                    ssxm, ssym, ssxym = (N * N - 1.0) / 12.0 / (fs * fs), (syy - sy * sy / N) / N, (sxy - xm * sy) / N / fs
                    r = 0.0
                    if ssxm != 0.0 and ssym != 0.0:
                        with np.errstate(invalid="ignore"):
                            r = ssxym / np.sqrt(ssxm * ssym)
                        r = 1.0 if r > 1.0 else -1.0 if r < -1.0 else r
                    rs.append(r)
                    ts.append(-60.0 / (ssxym / ssxm + 1e-10))
                else:
                    rs.append(0.0)
                    ts.append(np.nan)
        i = int(np.argmax(np.abs(np.array(rs))))                # (a NaN wins, as on the host and in the kernel)
        t60[m], corr[m] = ts[i], rs[i]
    t60_edc = np.mean(t60) if rir_ok else np.nan
    env_ok = bool(rir_ok and abs(t60_edc - T60_specify) < 0.05 and abs(corr[-1]) > 0.5)
    nd = int(np.argmax(rir_dp[0]))
    if rir_dp[0, nd] < 0 and L > Ld:
        nd = Ld
    p = rir[0] ** 2
    n = np.arange(L)
    eps = 1e-8
    in_dp, early = (n >= nd - int(fs * 2.5 / 1000)) & (n <= nd + int(fs * 2.5 / 1000)), n <= nd + int(fs * 50 / 1000)
    with np.errstate(invalid="ignore", divide="ignore"):
        fin = bool(np.isfinite(rir[0]).all())
        drr = 10.0 * np.log10(p[in_dp].sum() / (p[~in_dp].sum() + eps) + eps) if fin else np.nan
        c50 = 10.0 * np.log10(p[early].sum() / (p[~early].sum() + eps) + eps) if fin else np.nan
    return dict(t60=t60, corr=corr, t60_edc=t60_edc, drr=drr, c50=c50, nd=nd, flags=int(rir_ok) | (int(env_ok) << 1))


# ---------------------------------------------------------------------------------------------------------------- microphone signals
PCM_GAIN = 0.9                   # utils_simu_rir_sig.py:824
SIG_STAGE_SEEDS = {"pretrain": 1, "preval": 2000000, "pretest": 3000000}        # gen_simu.py:216-231; 'pretest_ins*' takes pretest's
SIG_SRC_SUBDIR = {"pretrain": "tr", "preval": "dt", "pretest": "et"}            # gen_simu.py:282-289


def sig_stage(stage):
    """'pretrain' | 'preval' | 'pretest' for a stage name of --mode sig ('pretest_ins*' counts as pretest), else ValueError with the
    reference's assertion (gen_simu.py:216)."""
    if stage in SIG_STAGE_SEEDS:
        return stage
    if "pretest_ins" in stage:
        return "pretest"
    raise ValueError("--stage %s: only --mode rir generates stages train / val / test; --mode sig takes pretrain | preval | pretest | "
                     "pretest_ins*, as the reference asserts" % stage)


def pcm16(x):
    """float -> PCM-16 as the generator writes it: rint(x 32767) in f64, ties to even, saturated to +-32767.  This is libsndfile's rule
    for float input with normalisation on AS THIS PROJECT READS IT; soundfile is not available to pin it against (UNPINNED)."""
    return np.clip(np.rint(np.asarray(x, np.float64) * 32767.0), -32767.0, 32767.0).astype(np.int16)


def plan_sig(rs, idx, seed, cfg, sources, T, snr_range=(15, 30), nmic=2, draw_white=True, fs=FS):
    """generate_microphone_signal's draws (utils_simu_rir_sig.py:749-816) on the RandomState ``rs`` after seed + idx: rirsynth.draw_item
    - speaker index, SourceBank.draw (utterance, same-speaker padding, crop, mean removal), the white noise (int(T fs), nmic), left out
    with draw_white=False: the device draws its own, and the SNR."""
    from . import rirsynth
    rs.seed(seed + idx)
    return dict(rirsynth.draw_item(rs, sources, T, fs, snr_range, nmic, draw_white), idx=idx, cfg=cfg)


def sig_samples(T, fs=FS, name="T ="):
    """int(T fs), the samples of an item of --mode sig, or ValueError where the diffuse-noise kernel's frames cannot take it."""
    ns = int(T * fs)
    if ns <= 0 or ns % 64 != 0:
        raise ValueError("%s %s: int(T fs) = %d samples is not a multiple of 64, which the diffuse-noise kernel's frames need" % (name, T, ns))
    return ns


NOISE_TYPES = ("diffuse_white", "spatial_white")


def check_noise_type(noise_type):
    """The noise types that are built, else ValueError.  'white' - the default of the reference's gen_simu_certain_room.py - is not in the
    list NoiseSignal accepts (utils_noise.py:45), so the reference's own documented command asserts there."""
    if noise_type == "white":
        raise ValueError("noise_type white: the reference's gen_simu_certain_room.py has this default, but its NoiseSignal accepts no 'white' "
                         "(utils_noise.py:45) and asserts; say diffuse_white (the default here) or spatial_white")
    if noise_type not in NOISE_TYPES:
        raise ValueError("noise_type %s: diffuse_white and spatial_white only (noise from recordings is not built)" % noise_type)
    return noise_type


def restate_sig(plan, tail_noise=None, rir=None, rir_dp=None, pcm=True, fs=FS, c=343.0, ism_db=12, noise_type="diffuse_white", with_dp=False):
    """One item of the generator in f64 from the existing restatements: the RIR and the direct path of plan['cfg'] (restate_cfg; or the
    given ``rir`` / ``rir_dp`` (nch, L)), the diffuse field of the plan's white noise (noise_type="spatial_white": the white noise as
    drawn, utils_noise.py:65-66), the mix at gain 0.9, and with pcm=True the PCM rule -> (Ns, nch) int16 (float64 with pcm=False);
    with_dp=True: -> (that, the direct-path signal of ``{idx}_dp.wav`` in the same form).  The authority for the GPU tests."""
    from . import rirsynth
    cfg = plan["cfg"]
    if rir is None:
        rir = restate_cfg(cfg, tail_noise, fs, c, ism_db)
    if rir_dp is None:
        rir_dp = restate_cfg(cfg, None, fs, c, ism_db, dp=True)
    if check_noise_type(noise_type) == "spatial_white":
        noise = np.asarray(plan["white"], np.float64)
    else:
        noise = rirsynth.restate_diffuse(plan["white"], rirsynth.mixing_table(cfg["mic_pos"], fs, c))
    sigs = rirsynth.restate_mix(plan["src"], rir, rir_dp=rir_dp, noise=noise, snr_db=plan["snr"], gain=PCM_GAIN, return_dp=with_dp)
    if with_dp:
        return tuple(pcm16(x) if pcm else x for x in sigs)
    return pcm16(sigs) if pcm else sigs


def sig_info(cfg, plan, T60_edc, DRR, C50, c=343.0):
    """The dictionary of ``{idx}_info.npz`` (utils_simu_rir_sig.py:798-861): the configuration with T60_edc, src_idx and SNR, and the
    annotations with the reference's dtypes (TDOA float32, DRR and C50 float16)."""
    return dict(cfg, T60_edc=np.float64(T60_edc), src_idx=plan["src_idx"], SNR=plan["snr"], TDOA=tdoa(cfg, c),
                DRR=np.asarray(DRR, np.float64).astype(np.float16), C50=np.asarray(C50, np.float64).astype(np.float16))


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


def render(plans, device, noise=None, fs=FS, c=343.0, lmax=None):
    """One hip.ism_rir launch for a list of ``plan_rir`` results -> (B, nch, lmax) f32 on the device.  noise: (B, nch, lmax) f32 device
    tensor, or None when no plan has a tail.  lmax: the row length, at least every n_len (default: the longest of the batch)."""
    import torch
    from . import hip
    B, nch = len(plans), plans[0]["mic"].shape[0]
    for p in plans:
        assert p["mic"].shape == (nch, 3)
        _check_tail_frames(p, fs, c)
    nism_max = max(p["n_ism"] for p in plans)
    lmax = _row_length(plans, lmax)
    nimg_max = max(int(np.prod(p["nb_img"])) for p in plans)
    if nimg_max > MAX_IMAGES:
        raise ValueError("%d image sources in one RIR, at most %d are rendered" % (nimg_max, MAX_IMAGES))

    def dev(key, dtype):
        return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(p[key]) for p in plans]), dtype)).to(device)
    return hip.ism_rir(dev("room", np.float64), dev("beta", np.float32), dev("src", np.float64), dev("mic", np.float64), dev("nb_img", np.int32),
                       dev("n_ism", np.int32), dev("n_len", np.int32), dev("tail_slope", np.float32), lmax=lmax, nism_max=nism_max,
                       nimg_max=nimg_max, noise=noise, fs=float(fs), c=float(c))


def _row_length(plans, lmax=None):
    longest = max(p["n_len"] for p in plans)
    if lmax is not None and lmax < longest:
        raise ValueError("lmax = %d is shorter than an RIR of %d samples" % (lmax, longest))
    return longest if lmax is None else int(lmax)


def device_noise(plans, ids, seed, attempt, device, lmax=None):
    """(B, nch, lmax) f32 standard normal values on the device: item b from sarssl_gauss_fill keyed by (seed, ids[b], attempt).  Drawn in
    gauss_fill's own (sample, channel) order and transposed, so that the value at (channel, sample) of an item is a function of that key
    alone - not of the longest item of the batch it is rendered in."""
    import torch
    from . import hip
    nch, lmax = plans[0]["mic"].shape[0], _row_length(plans, lmax)
    white = torch.empty((len(plans), lmax, nch), dtype=torch.float32, device=device)
    gauss_fill_items(white, ids, (int(seed) & 0xffffffff) | (int(attempt) << 32))
    return white.transpose(1, 2).contiguous()


def gauss_fill_items(white, ids, key):
    """white[b] = sarssl_gauss_fill's values of (key, ids[b]): one launch per run of consecutive ids (the kernel keys row b of a launch by
    item0 + b, so a run is one call with the same values as a call per item)."""
    from . import hip
    ids = [int(i) for i in ids]
    j = 0
    while j < len(ids):
        k = j + 1
        while k < len(ids) and ids[k] == ids[k - 1] + 1:
            k += 1
        hip.gauss_fill(white[j:k], key, ids[j])
        j = k


def host_noise(plans, ids, seed, attempt, device, lmax=None):
    """The same from ``numpy_noise``, uploaded."""
    import torch
    nch, lmax = plans[0]["mic"].shape[0], _row_length(plans, lmax)
    noise = np.zeros((len(plans), nch, lmax), np.float32)
    for b, (p, idx) in enumerate(zip(plans, ids)):
        noise[b, :, :p["n_len"]] = numpy_noise(seed, idx, attempt, nch, p["n_len"])
    return torch.from_numpy(noise).to(device)


Rendered = collections.namedtuple("Rendered", "ids plans plans_dp rir dp")


def render_items(cfgs, ids, seed, attempt, device, noise="device", lmax=None, fs=FS, c=343.0, ism_db=12):
    """The render batch of the image-source model, enqueued on the current stream: ``plan_rir`` of cfgs[i] and of its direct path for
    every i of ``ids``, the tail's noise keyed by (seed, i, attempt) - noise="device": ``device_noise``, "numpy": ``host_noise``; drawn
    only when some plan has a tail - and the two ``render`` calls -> Rendered(ids, plans, plans_dp, rir (B, nch, lmax), dp (B, nch, 1600)),
    both tensors on the device.  lmax: the RIRs' row length (default: the longest of the batch)."""
    assert noise in ("device", "numpy")
    ids = list(ids)
    plans_dp = [plan_rir(cfgs[i], fs, c, ism_db, dp=True) for i in ids]
    plans = [plan_rir(cfgs[i], fs, c, ism_db) for i in ids]
    dp = render(plans_dp, device, None, fs, c)
    has_tail = any(p["n_len"] > p["n_ism"] for p in plans)
    tail = (device_noise if noise == "device" else host_noise)(plans, ids, seed, attempt, device, lmax) if has_tail else None
    return Rendered(ids, plans, plans_dp, render(plans, device, tail, fs, c, lmax), dp)


# ---------------------------------------------------------------------------------------------------------------- the generator
def judge_on_device(rir, n_len, rir_dp, dp_len, T60_specify, ids=None, attempt=0, fs=FS):
    """The accept test and the annotations of a rendered batch on the GPU (hip.rir_labels, csrc/rirlabel.hip), read back with one small
    copy: rir (B, nch, lmax) and rir_dp (B, nch, ldmax) device tensors, n_len / dp_len / T60_specify sequences -> numpy dict(t60, corr
    (B, nch), t60_edc, drr, c50 (B) f64, nd, flags (B) int32; an item is accepted when flags == 3).  ids / attempt name the items (the
    generators pass them; nothing here depends on them)."""
    import torch
    from . import hip
    dev = rir.device
    lab = hip.rir_labels(rir, torch.tensor(list(n_len), dtype=torch.int32, device=dev), rir_dp,
                         torch.tensor(list(dp_len), dtype=torch.int32, device=dev),
                         torch.tensor([float(t) for t in T60_specify], dtype=torch.float64, device=dev), float(fs))
    return hip.rir_labels_host(lab)


def judge_on_host(batch, cfgs, fs=FS, c=343.0):
    """The same of a ``render_items`` batch by ``labels`` on the host -> numpy dict(flags (B) int32, t60_edc (B) f64, drr, c50 (B) float16
    as ``labels`` rounds them) with the read-back batch beside them: rir (B, nch, lmax), dp (B, nch, 1600)."""
    rir, dp = batch.rir.cpu().numpy(), batch.dp.cpu().numpy()
    labs = [labels(rir[b, :, :p["n_len"]], dp[b, :, :pd["n_len"]], cfgs[idx], fs, c)
            for b, (idx, p, pd) in enumerate(zip(batch.ids, batch.plans, batch.plans_dp))]
    return dict(flags=np.array([int(lab["rir_ok"]) | (int(lab["env_ok"]) << 1) for lab in labs], np.int32),
                t60_edc=np.array([lab["T60_edc"] for lab in labs], np.float64), drr=np.array([lab["DRR"] for lab in labs], np.float16),
                c50=np.array([lab["C50"] for lab in labs], np.float16), rir=rir, dp=dp)


def _generator_args(ranges, noise):
    assert noise in ("device", "numpy")
    unknown = set(ranges) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown arguments: %s" % sorted(unknown))
    args = dict(DEFAULTS, **ranges)
    if args["fs"] != FS:
        raise ValueError("fs = %s: the renderer's window and frames are defined at %d Hz only" % (args["fs"], FS))
    return args


def _rooms(save_to, stage, seed, data_num, mic_array_cfg, args):
    """The output directory of a stage, created, and its ``data_num`` room draws -> (out_dir, cfgs)."""
    out_dir = os.path.join(save_to, stage)
    os.makedirs(out_dir, exist_ok=True)
    rs = np.random.RandomState()
    draw = {k: args[k] for k in DEFAULTS if k != "fs"}
    return out_dir, [random_spatial_acoustics(rs, seed, idx, mic_array_cfg=mic_array_cfg, **draw) for idx in range(data_num)]


def read_back_accepted(batch, acc, lab):
    """The RIRs and direct paths at the positions ``acc`` of a batch as numpy (A, nch, lmax), (A, nch, 1600): from the judge's read-back
    where it judged on the host; else gathered on the device, so that only accepted items cross the bus."""
    if "rir" in lab:
        return lab["rir"][acc], lab["dp"][acc]
    return batch.rir[acc].cpu().numpy(), batch.dp[acc].cpu().numpy()


def _generate(who, out_dir, stage, cfgs, seed, args, device, noise, batch, where, sink, log=None, prepare=None, lmax=None, saved_cfgs=None,
              ids=None, **recorded):
    """The loop of both generators: the pending items are rendered in batches (``render_items``), judged (where="host": ``judge_on_host``,
    "device": ``judge_on_device``) and, where accepted (flags == 3), handed to ``sink(batch, accepted positions, labels) -> ids written``;
    the others are rendered again with the next attempt's noise and skipped with a logged line after MAX_ATTEMPTS.  ``prepare(ids)`` runs
    between the enqueue of a batch's renders and the wait for its labels: host work there overlaps the render.  all_info.npz (``args``,
    the stage's and ``recorded``; every configuration - ``saved_cfgs`` where the caller stores them in another shape -; the skipped ids) is
    written unless out_dir is None.  ids: the items to render where they are not 0 .. len(cfgs) - 1 (the online loader's chunks: ``cfgs``
    is then a dictionary by id).  -> dict(written, skipped, attempts)."""
    fs, c = args["fs"], args["c"]
    log = log or (lambda s: print(s, file=sys.stderr, flush=True))
    pending, written, attempts = list(range(len(cfgs))) if ids is None else list(ids), [], {}
    for attempt in range(MAX_ATTEMPTS):
        failed = []
        for i0 in range(0, len(pending), batch):
            b = render_items(cfgs, pending[i0:i0 + batch], seed, attempt, device, noise, lmax, fs, c, args["ism_db"])
            attempts.update((idx, attempt + 1) for idx in b.ids)
            if prepare is not None:
                prepare(b.ids)
            if where == "host":
                lab = judge_on_host(b, cfgs, fs, c)
            else:
                lab = judge_on_device(b.rir, [p["n_len"] for p in b.plans], b.dp, [p["n_len"] for p in b.plans_dp],
                                      [cfgs[idx]["T60_specify"] for idx in b.ids], b.ids, attempt, fs)
            acc = [j for j in range(len(b.ids)) if lab["flags"][j] == 3]
            failed += [b.ids[j] for j in range(len(b.ids)) if lab["flags"][j] != 3]
            if acc:
                written += sink(b, acc, lab)
        pending = failed
        if not pending:
            break
    for idx in pending:
        log("%s: item %d of stage %s failed the accept test %d times and is skipped" % (who, idx, stage, MAX_ATTEMPTS))
    if out_dir is not None:
        info = dict(args, stage=stage, data_num=len(cfgs), seed=seed, noise=noise, **recorded)
        np.savez_compressed(os.path.join(out_dir, "all_info.npz"), args=info, cfgs=cfgs if saved_cfgs is None else saved_cfgs,
                            skipped=np.array(pending, np.int64))
    return dict(written=sorted(written), skipped=pending, attempts=attempts)


def _bank_sink(cfgs, stem, fs, c):
    """The sink of the RIR banks: item idx goes to ``stem(idx)`` + .npy (1, nch, L, 1) float32, _dp.npy and _info.npz."""
    def sink(batch, acc, lab):
        rir, dp = read_back_accepted(batch, acc, lab)
        for j, b in enumerate(acc):
            idx = batch.ids[b]
            np.save(stem(idx) + ".npy", rir[j, :, :batch.plans[b]["n_len"]][None, :, :, None].astype(np.float32))
            np.save(stem(idx) + "_dp.npy", dp[j, :, :batch.plans_dp[b]["n_len"]][None, :, :, None].astype(np.float32))
            np.savez(stem(idx) + "_info.npz", **dict(cfgs[idx], T60_edc=np.float64(lab["t60_edc"][b])), TDOA=tdoa(cfgs[idx], c),
                     DRR=lab["drr"][b].astype(np.float16), C50=lab["c50"][b].astype(np.float16), fs=fs)
        return [batch.ids[b] for b in acc]
    return sink


def simulate_bank(save_to, stage="train", data_num=1024, mic_array_cfg=None, device="cuda", noise="device", batch=16, log=None,
                  labels="host", **ranges):
    """GenerateRandomRIR (gen_simu.py:38-176): ``data_num`` random configurations of ``stage`` (its seed as there), their RIRs and direct
    paths rendered in batches on ``device``, the reference's accept test, and per accepted item ``{idx}.npy`` (1, nch, L, 1)
    float32, ``{idx}_dp.npy`` and ``{idx}_info.npz`` (configuration, annotations, fs) under ``save_to/stage``, with ``all_info.npz``.

    labels="host": the batch is read back and judged by ``labels`` on the host (``judge_on_host``); "device": it is judged on the GPU
    (``judge_on_device``) and only accepted items are read back - the same files, T60_edc / DRR / C50 to within parity.RIRLABELS.
    The tail's noise is keyed by (seed, idx, attempt): noise="device" - sarssl_gauss_fill, "numpy" - an uploaded host draw.  An item that
    fails the accept test is rendered again with the next attempt; the reference retries forever, here an item is skipped after
    MAX_ATTEMPTS with a logged line and listed in all_info.npz (SimulatedBank globs ``*_dp.npy``, so a gap is harmless).
    ranges: room_sz_range, T60_range, abs_weights_range, array_pos_ratio_range, num_source_range, source_state, min_src_array_dist,
    min_src_boundary_dist, fs, c, ism_db (DEFAULTS).  -> dict(written=[idx], skipped=[idx], attempts={idx: n})."""
    assert labels in ("host", "device")
    args = _generator_args(ranges, noise)
    fs, c = args["fs"], args["c"]
    if stage not in STAGE_SEEDS:
        raise ValueError("unknown stage %r (one of %s)" % (stage, sorted(STAGE_SEEDS)))
    seed = STAGE_SEEDS[stage]
    out_dir, cfgs = _rooms(save_to, stage, seed, data_num, mic_array_cfg, args)

    return _generate("simulate_bank", out_dir, stage, cfgs, seed, args, device, noise, batch, labels,
                     _bank_sink(cfgs, lambda idx: os.path.join(out_dir, "%d" % idx), fs, c), log)


WHITE_STREAM = 1 << 63           # seed bit of the white noise of --mode sig: apart from the RIR tails' (seed | attempt << 32, idx) keys


def sig_lmax(T60_range, fs=FS):
    """The fixed row length --mode sig renders every RIR at: n_len = ceil(40 / 60 T60_sabine fs) of the largest T60_sabine the accepted
    rooms can have (the room draw keeps |T60_sabine - T60_specify| < 0.005)."""
    return int(math.ceil(att2t(40, float(max(T60_range)) + 0.005) * fs)) + 1


def simulate_signals(save_to, stage="pretrain", data_num=1, src_dir="", mic_array_cfg=None, device="cuda", noise="device", batch=16,
                     T=4.112, snr_range=(15, 30), sort_sources=False, nthreads=0, log=None, save_dp=False, **ranges):
    """GenerateRandomMicSig (gen_simu.py:178-360) with generate_microphone_signal (utils_simu_rir_sig.py:749-861): ``data_num`` items of
    ``stage`` (pretrain | preval | pretest | pretest_ins*: its seed, and src_dir + /tr | /dt | /et, as there) as ``{idx}.wav`` PCM-16
    (int(T fs), nch) and ``{idx}_info.npz`` (configuration, T60_edc, SNR, src_idx, TDOA / DRR / C50 with the reference's dtypes) under
    ``save_to/stage``, with ``all_info.npz`` as in ``simulate_bank``.  save_dp=True (any stage; the reference documents it for
    pretest_ins*, whose test stage opens the files): the direct-path signal at the item's scale, dp / max(max|mic|, max|dp|) 0.9, as
    ``{idx}_dp.wav`` beside every ``{idx}.wav`` (utils_simu_rir_sig.py:825, 857-859); all_info.npz's args then record save_dp=True, and
    nothing else that is written changes.

    The generator loop (``_generate``: ``render_items``, ``judge_on_device``, one small read-back of the labels, retries) on a side
    stream, with a sink that never takes the RIR off the device: a gather of the accepted items, the white noise (noise="device":
    sarssl_gauss_fill keyed by (seed, idx); "numpy": the reference's host draw, uploaded), rirsynth.mix_simulated with the item's mixing
    table against the direct path at gain 0.9, hip.pcm16_pack, a copy to a pinned buffer.  A writer thread then writes the batch's files
    (dataset.write_wav_batch, np.savez) while the next batch renders.  Rejected items go to the next attempt; after MAX_ATTEMPTS an item
    is skipped with a logged line and listed in all_info.npz.

    An item's files are a function of (seed, idx, attempt, the source files) alone, not of the batch it was rendered in: hip.rir_mix
    partitions its RIRs by the row length it is given, so every batch is rendered at the one row length ``sig_lmax(T60_range)``.
    The host plans an item once (plan_sig: it reads the utterances) while the GPU renders, and keeps the plan across attempts.
    -> dict(written=[idx], skipped=[idx], attempts={idx: n})."""
    from . import rirsynth
    args = _generator_args(ranges, noise)
    base = sig_stage(stage)
    seed = SIG_STAGE_SEEDS[base]
    sig_samples(T, args["fs"])
    mic_array_cfg = MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
    sources = rirsynth.SourceBank(src_dir + "/" + SIG_SRC_SUBDIR[base], args["fs"], sort=sort_sources)
    out_dir, cfgs = _rooms(save_to, stage, seed, data_num, mic_array_cfg, args)
    return _signals("simulate_signals", out_dir, stage, cfgs, seed, args, sources, lambda idx: os.path.join(out_dir, "%d" % idx), device, noise,
                    batch, T, snr_range, mic_array_cfg["mic_pos_relative"].shape[0], nthreads, log, recorded=dict(src_dir=src_dir),
                    save_dp=save_dp)


def _signal_sink(cfgs, seed, args, dev, noise, T, nmic, plan, emit, load=None, items=None, table="host", noise_type="diffuse_white",
                 save_dp=False):
    """``prepare`` and ``sink`` of a ``_generate`` run that turns accepted RIRs into packed PCM-16 signals without the RIR leaving the
    device: a gather of the accepted rows, the white noise (noise="device": sarssl_gauss_fill keyed by (seed, item); "numpy": the plan's
    host draw, uploaded), rirsynth.mix_simulated against the direct path at gain 0.9, hip.pcm16_pack.  What differs between the
    generators that write files (``_signals``) and the online loader (onlinesig.OnlineSignalLoader) comes in as functions:

    * ``plan(i)``: the signal plan of item i - ``snr``, with noise="numpy" ``white``, and ``src`` unless ``load`` brings the sources;
      called once per item from ``prepare`` (host work while the GPU renders) and kept across attempts,
    * ``items(idx)``: the items a rendered id serves (default: itself; the online loader's ``reuse`` gives several),
    * ``load(plans) -> (A, ns) f32 on the device``: the sources of a batch (default: the plans' host crops, uploaded with the SNRs),
    * ``emit(pcm, aids, rows, lab, plans)``: pcm (nsig A, ns, nmic) int16 on the device - the A signals, then with save_dp their A direct
      paths -, the items' ids, their rows in the judged batch (``lab``'s index) and their plans."""
    import torch
    from . import hip, rirsynth
    from .pipeline import src_snr_rows
    assert table in ("host", "device") and noise_type in NOISE_TYPES
    fs, c = args["fs"], args["c"]
    ns = sig_samples(T, fs)
    diffuse = noise_type == "diffuse_white"
    ntab = 129 * nmic * nmic if diffuse and table == "host" else 0
    assert load is None or not ntab, "sources that are loaded on the device go with table='device'"
    items = items or (lambda idx: [idx])
    nsig = 2 if save_dp else 1                                # signals per item: the microphones', then the direct path's
    sig_plans = {}

    def prepare(ids):                                         # (host work while the GPU renders)
        for idx in ids:
            for i in items(idx):
                if i not in sig_plans:
                    p = plan(i)
                    if ntab:
                        p["C"] = rirsynth.mixing_table(cfgs[idx]["mic_pos"], fs, c).astype(np.float32)
                    sig_plans[i] = p

    def sink(b, acc, lab):
        rows = [j for j in acc for _ in items(b.ids[j])]
        aids = [i for j in acc for i in items(b.ids[j])]
        A = len(aids)
        rir_dev, dp_dev = b.rir, b.dp
        if rows != list(range(len(b.ids))):
            sel = torch.tensor(rows, device=dev)
            rir_dev, dp_dev = rir_dev.index_select(0, sel), dp_dev.index_select(0, sel)
        plans = [sig_plans[i] for i in aids]
        if load is None:
            up = src_snr_rows(plans, ns, ntab).to(dev, non_blocking=True)                              # src | snr | C of each item
            src, snr = up[:, :ns].contiguous(), up[:, ns].contiguous()
        else:
            src = load(plans)
            snr = torch.tensor([p["snr"] for p in plans], dtype=torch.float32, device=dev)
        if noise == "numpy":
            white = torch.from_numpy(np.stack([p["white"] for p in plans]).astype(np.float32)).to(dev)
        else:
            white = torch.empty((A, ns, nmic), dtype=torch.float32, device=dev)
            gauss_fill_items(white, aids, (int(seed) & 0xffffffff) | WHITE_STREAM)
        rir_len = torch.tensor([b.plans[j]["n_len"] for j in rows], dtype=torch.int32, device=dev)
        dp_len = torch.tensor([b.plans_dp[j]["n_len"] for j in rows], dtype=torch.int32, device=dev)
        gain = torch.full((A,), PCM_GAIN, dtype=torch.float32, device=dev)
        sig = torch.empty((nsig, A, ns, nmic), dtype=torch.float32, device=dev)
        out_dp = sig[1] if save_dp else None
        if not diffuse:
            hip.rir_mix(src, rir_dev, rir_len, snr, gain, rir_dp=dp_dev, dp_len=dp_len, noise=white, out=sig[0], out_dp=out_dp)
        else:
            if ntab:
                C = up[:, ns + 1:].reshape(A, 129, nmic, nmic).contiguous()
            else:
                mic_pos = np.ascontiguousarray(np.stack([cfgs[b.ids[j]]["mic_pos"] for j in rows]), np.float64)  # (the draws leave them column-major)
                C = hip.mixing_table(torch.from_numpy(mic_pos).to(dev), float(fs), float(c))
            rirsynth.mix_simulated(src, rir_dev, rir_len, dp_dev, dp_len, white, C, snr, gain, out=sig[0], out_dp=out_dp)
        pcm = hip.pcm16_pack(sig).view(nsig * A, ns, nmic)    # dense: the A signals, then their A direct paths
        emit(pcm, aids, rows, lab, [sig_plans.pop(i) for i in aids])
        return aids

    return prepare, sink


def _signals(who, out_dir, stage, cfgs, seed, args, sources, stem, device, noise, batch, T, snr_range, nmic, nthreads, log, table="host",
             noise_type="diffuse_white", saved_cfgs=None, recorded=None, save_dp=False):
    """The signal generators' run of ``_generate`` (see ``simulate_signals``): item idx of ``cfgs``, planned by plan_sig after seed + idx,
    goes to ``stem(idx)`` + .wav and _info.npz.  table: where the diffuse field's mixing table is formed - "host": rirsynth.mixing_table
    while the GPU renders, uploaded with the source; "device": hip.mixing_table of the batch's uploaded microphone positions.
    noise_type="spatial_white": the white noise goes into hip.rir_mix as it is (no field, no division by its maximum).
    recorded: what all_info.npz's args hold beside the ranges, T and snr_range.  save_dp: the mix also stores the direct-path signal
    (hip.rir_mix's out_dp); it is packed and copied with the microphone signal - pipeline.StagedWriter's buffers take both, the batch's
    signals and then their direct paths - and written as ``stem(idx)`` + _dp.wav in the same write_wav_batch call; all_info.npz's args then hold
    save_dp=True.  The render, the mix and the pack are ``_signal_sink``'s; this is its sink that writes files."""
    import torch
    from .dataset import write_wav_batch
    from .pipeline import StagedWriter
    fs, c = args["fs"], args["c"]
    ns = sig_samples(T, fs)
    rs = np.random.RandomState()
    dev = torch.device(device)
    side = torch.cuda.Stream(dev)
    nsig = 2 if save_dp else 1

    def plan(idx):
        return plan_sig(rs, idx, seed, cfgs[idx], sources, T, snr_range, nmic, draw_white=noise == "numpy", fs=fs)

    def write(buf, ids, infos):
        paths = [stem(i) + ".wav" for i in ids]
        if save_dp:
            paths += [stem(i) + "_dp.wav" for i in ids]
        write_wav_batch(paths, buf, fs, nthreads)
        for i, info in zip(ids, infos):
            np.savez(stem(i) + "_info.npz", **info)

    def emit(pcm, aids, rows, lab, plans):
        infos = [sig_info(cfgs[i], p, lab["t60_edc"][j], lab["drr"][j], lab["c50"][j], c) for i, j, p in zip(aids, rows, plans)]
        writer.stage(pcm, write, aids, infos)

    prepare, sink = _signal_sink(cfgs, seed, args, dev, noise, T, nmic, plan, emit, table=table, noise_type=noise_type, save_dp=save_dp)
    with StagedWriter(nsig * batch, ns, nmic) as writer, torch.cuda.stream(side):
        return _generate(who, out_dir, stage, cfgs, seed, args, dev, noise, batch, "device", sink, log, prepare,
                         sig_lmax(args["T60_range"], fs), saved_cfgs, T=T, snr_range=tuple(snr_range), **(recorded or {}),
                         **(dict(save_dp=True) if save_dp else {}))


# ---------------------------------------------------------------------------------------------------------------- fixed rooms
ROOM_SRC_SUBDIR = {"train": "tr", "val": "dt", "test": "et"}                   # gen_simu_certain_room.py:311-316; seeds: STAGE_SEEDS


def room_stage(stage):
    """train | val | test, else ValueError with the reference's assertion (gen_simu_certain_room.py:239)."""
    if stage not in ROOM_SRC_SUBDIR:
        raise ValueError("--stage %s: gen_simu_certain_room.py generates train | val | test only, as the reference asserts "
                         "(gen_simu.py --mode sig writes pretrain | preval | pretest)" % stage)
    return stage


def room_item(g, per_room):
    """Flattened item id -> (room r, index inside the room): g = r per_room + index."""
    return divmod(int(g), int(per_room))


def room_stem(out_dir, g, per_room):
    """The path of item ``g`` without its extension: ``out_dir/R{r + 1}/{index}`` - the directories count from one
    (gen_simu_certain_room.py:190, 389)."""
    r, i = room_item(g, per_room)
    return os.path.join(out_dir, "R%d" % (r + 1), "%d" % i)


def room_placements(seed, room_num, rir_num_each_room, mic_array_cfg, args):
    """The reference's draws of gen_simu_certain_room.py:270-299, seed collisions between rooms and placements included: room r after
    seed + r (``random_room``), its placement j after seed + r rir_num_each_room + j -> [room][placement] configurations."""
    rs = np.random.RandomState()
    draw = {k: args[k] for k in DEFAULTS if k != "fs"}
    rooms = []
    for r in range(room_num):
        rs.seed(seed + r)
        room_cfg = random_room(rs, args["room_sz_range"], args["T60_range"], args["abs_weights_range"], args["c"], args["ism_db"])
        rooms.append([random_spatial_acoustics(rs, seed, r * rir_num_each_room + j, mic_array_cfg=mic_array_cfg, room_cfg=room_cfg, **draw)
                      for j in range(rir_num_each_room)])
    return rooms


def rooms_by_key(rooms):
    """all_info.npz's ``cfgs`` of the per-room generators: {'R{r}': room r's list} with ZERO-based keys, as the reference stores them
    (gen_simu_certain_room.py:132, 302) - the directories count from one."""
    return {"R%d" % r: room for r, room in enumerate(rooms)}


def _room_dirs(save_to, stage, room_num):
    out_dir = os.path.join(save_to, stage)
    for r in range(room_num):
        os.makedirs(os.path.join(out_dir, "R%d" % (r + 1)), exist_ok=True)
    return out_dir


def simulate_room_bank(save_to, stage="train", room_num=1000, rir_num_each_room=50, mic_array_cfg=None, device="cuda", noise="device",
                       batch=16, log=None, labels="host", **ranges):
    """GenerateRandomRIROfCertainRoom (gen_simu_certain_room.py:32-191): ``room_num`` rooms drawn once each (``room_placements``),
    ``rir_num_each_room`` array and source placements in each, written as ``save_to/stage/R{r + 1}/{j}.npy``, ``{j}_dp.npy`` and
    ``{j}_info.npz`` in ``simulate_bank``'s format, which rirsynth.SimulatedBank([save_to/stage]) loads.  All rooms' placements are one
    id space g = r rir_num_each_room + j and one ``_generate`` run, so a batch may hold several rooms; the tail's noise is keyed by
    (seed, g, attempt).  all_info.npz: args, cfgs = {'R{r}': [configurations]} with ZERO-based keys as the reference stores them, skipped
    (flattened ids).  -> dict(written=[g], skipped=[g], attempts={g: n})."""
    assert labels in ("host", "device")
    args = _generator_args(ranges, noise)
    seed = STAGE_SEEDS[room_stage(stage)]
    mic_array_cfg = MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
    rooms = room_placements(seed, room_num, rir_num_each_room, mic_array_cfg, args)
    out_dir = _room_dirs(save_to, stage, room_num)
    cfgs = [cfg for room in rooms for cfg in room]
    return _generate("simulate_room_bank", out_dir, stage, cfgs, seed, args, device, noise, batch, labels,
                     _bank_sink(cfgs, lambda g: room_stem(out_dir, g, rir_num_each_room), args["fs"], args["c"]), log,
                     saved_cfgs=rooms_by_key(rooms), room_num=room_num, rir_num_each_room=rir_num_each_room)


def simulate_room_signals(save_to, stage="train", room_num=256, rir_num_each_room=50, sig_num_each_rir=2, src_dir="",
                          noise_type="diffuse_white", mic_array_cfg=None, device="cuda", noise="device", batch=16, T=4.112,
                          snr_range=(15, 30), sort_sources=False, nthreads=0, log=None, **ranges):
    """GenerateRandomMicSigOfCertainRoom (gen_simu_certain_room.py:194-393), the corpus of the downstream sweep: ``room_num`` rooms
    drawn once each, ``rir_num_each_room`` placements per room (``room_placements``), ``sig_num_each_rir`` signals per placement.  Item
    i = j sig_num_each_rir + s of room r goes to ``save_to/stage/R{r + 1}/{i}.wav`` and ``{i}_info.npz``; its signal draws (plan_sig)
    follow seed + r rir_num_each_room sig_num_each_rir + i, i.e. seed + g with g the item's id in the ONE id space all rooms share.  The
    run is ``simulate_signals``' (``_signals``): a batch may hold items of several rooms, every item renders its own RIR (own tail noise,
    accept test and T60_edc, as in the reference), the tail-noise and white-noise keys take g, and the diffuse field's mixing table is
    formed on the device (hip.mixing_table) from the batch's microphone positions.
    noise_type: diffuse_white (default) | spatial_white; the reference's default 'white' is refused (``check_noise_type``).
    all_info.npz as in ``simulate_room_bank``, every placement ``sig_num_each_rir`` times.  -> dict(written=[g], skipped=[g], attempts)."""
    from . import rirsynth
    args = _generator_args(ranges, noise)
    check_noise_type(noise_type)
    seed = STAGE_SEEDS[room_stage(stage)]
    sig_samples(T, args["fs"])
    mic_array_cfg = MIC_ARRAY_CFG_2CH if mic_array_cfg is None else mic_array_cfg
    sources = rirsynth.SourceBank(src_dir + "/" + ROOM_SRC_SUBDIR[stage], args["fs"], sort=sort_sources)
    rooms = [[cfg for cfg in room for _ in range(sig_num_each_rir)]
             for room in room_placements(seed, room_num, rir_num_each_room, mic_array_cfg, args)]
    out_dir = _room_dirs(save_to, stage, room_num)
    per_room = rir_num_each_room * sig_num_each_rir
    return _signals("simulate_room_signals", out_dir, stage, [cfg for room in rooms for cfg in room], seed, args, sources,
                    lambda g: room_stem(out_dir, g, per_room), device, noise, batch, T, snr_range, mic_array_cfg["mic_pos_relative"].shape[0],
                    nthreads, log, table="device", noise_type=noise_type, saved_cfgs=rooms_by_key(rooms),
                    recorded=dict(src_dir=src_dir, room_num=room_num, rir_num_each_room=rir_num_each_room,
                                  sig_num_each_rir=sig_num_each_rir, noise_type=noise_type))


# ---------------------------------------------------------------------------------------------------------------- command line
def _literal(text):
    import ast
    return ast.literal_eval(text)


def _flag(text):
    if text in ("True", "true", "1"):
        return True
    if text in ("False", "false", "0"):
        return False
    raise ValueError(text)


def _shared_arguments(ap):
    """The flags gen_simu.py and gen_simu_certain_room.py share: the reference's names, and this project's --mic_array, --noise, --batch,
    --labels."""
    ap.add_argument("--mode", type=str, default="rir")
    ap.add_argument("--stage", type=str, default="train")
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
    ap.add_argument("--labels", type=str, default="host", choices=("host", "device"), help="--mode rir: where the accept test runs")
    # --mode sig
    ap.add_argument("--src_dir", type=str, default="")
    ap.add_argument("--snr_range", type=_literal, default=(15, 30))
    ap.add_argument("--noise_type", type=str, default="diffuse_white")
    ap.add_argument("--T", type=float, default=4.112)
    ap.add_argument("--gpu_conv", type=_flag, default=False)


def _shared_sig_refusals(ap, a):
    if a.gpu_conv:
        ap.error("--gpu_conv True: the trajectory convolution of moving sources is not built; static sources are convolved on the GPU anyway")
    try:
        sig_samples(a.T, a.fs, "--T")
    except ValueError as e:
        ap.error(str(e))
    if not a.src_dir:
        ap.error("--src_dir is required with --mode sig")


def _shared_refusals(ap, a):
    """What both command lines refuse, before a GPU is touched -> (device name, the ranges as keyword arguments)."""
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
    ranges = dict(room_sz_range=a.room_sz_range, T60_range=a.T60_range, abs_weights_range=a.abs_weights_range,
                  array_pos_ratio_range=a.array_pos_ratio_range, num_source_range=a.num_source_range, source_state=a.source_state,
                  min_src_array_dist=a.min_src_array_dist, min_src_boundary_dist=a.min_src_boundary_dist, c=a.c, ism_db=a.ism_db)
    return "cuda:%d" % int(gpus[0]), ranges


def main(argv=None):
    """``gen_simu.py --mode rir | sig`` with the reference's flag names (argparse; lists are written as Python literals, e.g. --gpus [0])."""
    import argparse
    ap = argparse.ArgumentParser(description="Generate simulated RIRs or microphone signals (image-source model on the GPU)")
    _shared_arguments(ap)
    ap.add_argument("--data_num", type=int, default=1024)
    ap.add_argument("--save_dp", type=_flag, default=False)
    a = ap.parse_args(argv)
    if a.mode not in ("rir", "sig"):
        ap.error("--mode %s: only --mode rir and --mode sig are built" % a.mode)
    if a.mode == "sig":
        try:
            sig_stage(a.stage)
        except ValueError as e:
            ap.error(str(e))
        if a.save_dp and "pretest_ins" not in a.stage:
            ap.error("--save_dp True: the direct-path companions {idx}_dp.wav are written for the pretest_ins* stages only, where the "
                     "reference documents the flag and run_pretrain.py --test --test-mode ins reads them; nothing reads them on "
                     "pretrain / preval / pretest, whose corpora they would double")
        if a.noise_type != "diffuse_white":
            ap.error("--noise_type %s: diffuse_white only" % a.noise_type)
        _shared_sig_refusals(ap, a)
    device, ranges = _shared_refusals(ap, a)
    if a.mode == "sig":
        res = simulate_signals(a.save_to, a.stage, a.data_num, a.src_dir, MIC_ARRAYS[a.mic_array], device=device,
                               noise=a.noise, batch=a.batch, T=a.T, snr_range=tuple(a.snr_range), save_dp=a.save_dp, **ranges)
        print("%d microphone signals written to %s, %d skipped" % (len(res["written"]), os.path.join(a.save_to, a.stage), len(res["skipped"])))
        return 0
    res = simulate_bank(a.save_to, a.stage, a.data_num, MIC_ARRAYS[a.mic_array], device=device, noise=a.noise, batch=a.batch,
                        labels=a.labels, **ranges)
    print("%d RIRs written to %s, %d skipped" % (len(res["written"]), os.path.join(a.save_to, a.stage), len(res["skipped"])))
    return 0


def main_certain_room(argv=None):
    """``gen_simu_certain_room.py --mode rir | sig`` with the reference's flag names: ``simulate_room_bank`` / ``simulate_room_signals``."""
    import argparse
    ap = argparse.ArgumentParser(description="Generate simulated RIRs or microphone signals of a fixed number of rooms, for the downstream "
                                             "stages train | val | test (image-source model on the GPU)")
    _shared_arguments(ap)
    ap.add_argument("--room_num", type=int, default=256)
    ap.add_argument("--rir_num_each_room", type=int, default=50)
    ap.add_argument("--sig_num_each_rir", type=int, default=2)
    a = ap.parse_args(argv)
    if a.mode not in ("rir", "sig"):
        ap.error("--mode %s: only --mode rir and --mode sig are built" % a.mode)
    try:
        room_stage(a.stage)
        if a.mode == "sig":
            check_noise_type(a.noise_type)
    except ValueError as e:
        ap.error(str(e))
    if a.mode == "sig":
        _shared_sig_refusals(ap, a)
    device, ranges = _shared_refusals(ap, a)
    where = os.path.join(a.save_to, a.stage)
    if a.mode == "sig":
        res = simulate_room_signals(a.save_to, a.stage, a.room_num, a.rir_num_each_room, a.sig_num_each_rir, a.src_dir, a.noise_type,
                                    MIC_ARRAYS[a.mic_array], device=device, noise=a.noise, batch=a.batch, T=a.T,
                                    snr_range=tuple(a.snr_range), **ranges)
        print("%d microphone signals of %d rooms written to %s, %d skipped" % (len(res["written"]), a.room_num, where, len(res["skipped"])))
        return 0
    res = simulate_room_bank(a.save_to, a.stage, a.room_num, a.rir_num_each_room, MIC_ARRAYS[a.mic_array], device=device, noise=a.noise,
                             batch=a.batch, labels=a.labels, **ranges)
    print("%d RIRs of %d rooms written to %s, %d skipped" % (len(res["written"]), a.room_num, where, len(res["skipped"])))
    return 0
