"""Shared inputs of tests/test_certainroom_cpu.py and tests/test_gpu_certainroom.py: fixture F23 (tools/make_golden_certainroom.py) and
its dictionaries, the microphone geometries the mixing-table kernel is checked on, and the small per-room run of the GPU tests."""
import os

import numpy as np

import simsig_cases as sc

ROOT = sc.ROOT
FS = sc.FS
F23 = os.path.join(ROOT, "tests", "golden", "f23_certainroom.npz")
SMALL = sc.SMALL
T_SMALL = 0.272
NS_SMALL = 4352
NOISE_TYPES = ("diffuse_white", "spatial_white")


def consts(fx):
    """dict(fs, ns, nmic, seed, rooms, rirs, sigs) of F23."""
    return dict(zip(("fs", "ns", "nmic", "seed", "rooms", "rirs", "sigs"), (int(v) for v in fx["consts"])))


def f23_cfg(fx, r, j):
    """Placement j of room r of F23 as the dictionary the reference drew."""
    pre = "room/%d/placement/%d/cfg/" % (r, j)
    cfg = {key[len(pre):]: fx[key] for key in fx.files if key.startswith(pre)}
    assert cfg
    for key in ("array_type", "mic_pattern"):
        cfg[key] = str(cfg[key])
    for key in ("T60_sabine", "T60_specify", "array_scale", "array_rotate_azi"):
        cfg[key] = float(cfg[key])
    cfg["room_sz"] = list(cfg["room_sz"])
    return cfg


def draw_args():
    """The arguments of F23's run as roomsim.room_placements takes them."""
    from sar_ssl_amd import roomsim
    return dict(roomsim.DEFAULTS, **SMALL)


# ---------------------------------------------------------------------------------------------------------------- mixing-table geometries
def _line(n, d):
    return np.array([[i * d, 0.0, 0.0] for i in range(n)])


def geometries():
    """{name: (M, 3) f64}: 2 microphones 3 cm and 20 cm apart, 3 in a line at 5 cm (smallest pivot 1e-3), circular_4ch, the corners of a
    30 cm cube.  The host factorisation succeeds for each of them."""
    from sar_ssl_amd import roomsim
    cube = np.array([[x, y, z] for x in (0.0, 0.3) for y in (0.0, 0.3) for z in (0.0, 0.3)])
    return {"pair_3cm": _line(2, 0.03), "pair_20cm": _line(2, 0.2), "line3_5cm": _line(3, 0.05),
            "circular_4ch": np.array(roomsim.MIC_ARRAY_CFG_CIRCULAR_4CH["mic_pos_relative"], np.float64), "cube_30cm": cube}


def table_batches():
    """[(name, mic (B, M, 3) f64)]: every geometry alone (B = 1), and per microphone count one batch of B = 5 - that count's geometries
    in turn, each moved to another place in a room and turned about the vertical (the distances change in their last bits only)."""
    geo = geometries()
    out = [(name, g[None].copy()) for name, g in geo.items()]
    for M in sorted({g.shape[0] for g in geo.values()}):
        same = [g for g in geo.values() if g.shape[0] == M]
        items = []
        for b in range(5):
            a = 0.7 * b
            rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
            items.append(same[b % len(same)] @ rot.T + np.array([1.0 + 0.37 * b, 2.0 - 0.21 * b, 1.5]))
        out.append(("M%d_B5" % M, np.stack(items)))
    return out


def host_tables(mic, fs=FS, c=343.0):
    """rirsynth.mixing_table of every item of a batch -> (B, 129, M, M) f32."""
    from sar_ssl_amd import rirsynth
    return np.stack([rirsynth.mixing_table(m, fs, c).astype(np.float32) for m in mic])


# ---------------------------------------------------------------------------------------------------------------- the generators' small run
ROOMS, RIRS, SIGS = 2, 2, 2


def room_plans(tree, stage="train", rooms=ROOMS, rirs=RIRS, sigs=SIGS, T=T_SMALL, ranges=None):
    """{g: plan_sig of item g} of a per-room run as the generator plans it (numpy white noise), from the host restatements alone."""
    from sar_ssl_amd import rirsynth, roomsim
    seed = roomsim.STAGE_SEEDS[stage]
    args = dict(roomsim.DEFAULTS, **(SMALL if ranges is None else ranges))
    placed = roomsim.room_placements(seed, rooms, rirs, roomsim.MIC_ARRAY_CFG_2CH, args)
    sources = rirsynth.SourceBank(os.path.join(tree, roomsim.ROOM_SRC_SUBDIR[stage]), FS, sort=True)
    rs = np.random.RandomState()
    cfgs = [cfg for room in placed for cfg in room for _ in range(sigs)]
    return {g: roomsim.plan_sig(rs, g, seed, cfg, sources, T) for g, cfg in enumerate(cfgs)}
