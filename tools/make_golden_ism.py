"""Fixture F21 of the simulated-RIR generator (sar_ssl_amd.roomsim), from the REAL reference (build container only, on the CPU):

    python tools/make_golden_ism.py        ->  tests/golden/f21_roomsim.npz

Imports the reference's code/data_generation/utils_simu_rir_sig.py and utils_array.py through oracle/ref_shim.py's path, with in-process
stand-ins for the third-party modules that are absent (soundfile, gpuRIR, matplotlib where missing).  Nothing of the reference's source
travels; the file holds
  cfg2/<idx>/<key>     SpatialAcoustics.generate_random_spatial_acoustics for idx 0..15 of stage ``train`` (seed 4 000 000), mic_array_cfg_2ch
  cfg4/<idx>/<key>     the same for idx 0..3 with mic_array_cfg_circular_4ch
  rir/<k>/...          for two rooms drawn with T60_range (0.2, 0.4) and room_sz_range SMALL_ROOM (idx 0, 1; short, so the file stays tens of KB): the configuration,
                       roomsim.restate_cfg's RIR (tail noise: roomsim.numpy_noise(seed, idx, 0)) and direct path as float32, and what the
                       reference's check_rir_envelope and generate_annotation(TDOA, DRR, C50, src_single_static=True) return for them,
                       widened to float64 first - gpuRIR, whose float32 output the reference would pass, is not available, and the
                       restatement (roomsim.labels) is defined in f64 on the values as given.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sarssl_boot  # noqa: E402,F401

GOLD = os.path.join(ROOT, "tests", "golden")
SEED, FS, C, ISM_DB = 4000000, 16000, 343.0, 12
N2, N4, NRIR = 16, 4, 2
SMALL_T60 = (0.2, 0.4)
SMALL_ROOM = [(3, 5), (3, 4), (2.5, 3)]     # the T60 retry loop ends only where 0.2 T60 >= 3 diagonal / c: a short T60 needs a small room
ARGS = dict(room_sz_range=[(3, 15), (3, 10), (2.5, 6)], T60_range=(0.2, 1.3), abs_weights_range=[(0.5, 1)] * 6, c=C, ism_db=ISM_DB,
            array_pos_ratio_range=[(0.2, 0.8), (0.2, 0.8), (0.1, 0.5)], num_source_range=(1, 1), source_state="static",
            min_src_array_dist=0.3, min_src_boundary_dist=0.3, nb_points=1, traj_pt_mode="time", room_cfg=None)


def _load_reference():
    import ref_shim
    data_gen = os.path.join(ref_shim.REF_CODE, "data_generation")
    if data_gen not in sys.path:
        sys.path.insert(0, data_gen)
    for name in ("soundfile", "gpuRIR", "matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["mpl_toolkits.mplot3d"], "Axes3D"):
        sys.modules["mpl_toolkits.mplot3d"].Axes3D = None
    import scipy.stats  # noqa: F401  (the reference reaches scipy.stats.linregress through the bare ``scipy`` name)
    import utils_simu_rir_sig as ref
    import utils_array as ref_array
    return ref, ref_array


def _pack(store, prefix, cfg):
    for k, v in cfg.items():
        store["%s/%s" % (prefix, k)] = np.asarray(v)


def main():
    from sar_ssl_amd import roomsim
    ref, ref_array = _load_reference()
    sa = ref.SpatialAcoustics()
    roomir = ref.RoomImpulseResponse(fs=FS, c=C, ism_db=ISM_DB)
    anno = ref.MicrophoneSignalOrRIR()
    store = {"consts": np.array([SEED, FS, N2, N4, NRIR]), "c": np.array(C), "ism_db": np.array(ISM_DB), "small_T60_range": np.array(SMALL_T60),
             "small_room_sz_range": np.array(SMALL_ROOM)}
    for idx in range(N2):
        _pack(store, "cfg2/%d" % idx, sa.generate_random_spatial_acoustics(mic_array_cfg=ref_array.mic_array_cfg_2ch, seed=SEED, idx=idx, **ARGS))
    for idx in range(N4):
        _pack(store, "cfg4/%d" % idx, sa.generate_random_spatial_acoustics(mic_array_cfg=ref_array.mic_array_cfg_circular_4ch, seed=SEED, idx=idx, **ARGS))
    for k in range(NRIR):
        cfg = sa.generate_random_spatial_acoustics(mic_array_cfg=ref_array.mic_array_cfg_2ch, seed=SEED, idx=k, **dict(ARGS, T60_range=SMALL_T60, room_sz_range=SMALL_ROOM))
        _pack(store, "rir/%d/cfg" % k, cfg)
        p = roomsim.plan_rir(cfg, FS, C, ISM_DB)
        noise = roomsim.numpy_noise(SEED, k, 0, p["mic"].shape[0], p["n_len"])
        rir = roomsim.restate_cfg(cfg, noise, FS, C, ISM_DB).astype(np.float32)
        dp = roomsim.restate_cfg(cfg, None, FS, C, ISM_DB, dp=True).astype(np.float32)
        store["rir/%d/rir" % k], store["rir/%d/rir_dp" % k] = rir, dp
        r4, d4 = rir.astype(np.float64)[None, :, :, None], dp.astype(np.float64)[None, :, :, None]
        ok, t60_edc = roomir.check_rir_envelope(r4, cfg["T60_specify"], FS)
        store["rir/%d/env_ok" % k], store["rir/%d/T60_edc" % k] = np.array(bool(ok)), np.array(t60_edc, np.float64)
        store["rir/%d/rir_ok" % k] = np.array(bool(roomir.check_rir(r4) & roomir.check_rir(d4)))
        annos = anno.generate_annotation(traj_pts=cfg["src_traj_pts"], array_pos=cfg["array_pos"], mic_pos=cfg["mic_pos"], rir_srcs=r4,
                                         rir_srcs_dp=d4, DOA=False, TDOA=True, DRR=True, C50=True, C80=False, mic_vad=False, source_vad=None,
                                         mic_sig=False, mic_sig_dp=False, mic_signal_srcs_dp=False, gpu_conv=False, pt2sample=False,
                                         src_single_static=True, fs=FS, c=C)
        for name, v in annos.items():
            store["rir/%d/%s" % (k, name)] = np.asarray(v)
        print("rir %d: T60_specify %.4f T60_edc %.4f ok %s  %s" % (k, cfg["T60_specify"], t60_edc, ok, {n: (v.dtype, float(v)) for n, v in annos.items()}))
    out = os.path.join(GOLD, "f21_roomsim.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
