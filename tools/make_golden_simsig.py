"""Fixture F22 of the signal generator (gen_simu.py --mode sig), from the REAL reference (build container only):

    python tools/make_golden_simsig.py        ->  tests/golden/f22_simsig.npz

Imports the reference's code/data_generation modules through oracle/ref_shim.py's path with in-process stand-ins for ``soundfile`` (reads
served by the project's own PCM reader, ``write`` recorded) and ``gpuRIR`` (``simulateRIR`` returns canned RIRs that this tool draws
itself: decaying noise at the configuration's T60 behind a positive peak, checked here to pass the accept test), writes a tiny speech tree
(2 speakers x 2 utterances, the one of F20) to a temporary directory and calls the reference's own
``MicrophoneSignalOrRIR.generate_microphone_signal`` for ITEMS items of stage pretrain (seed 1) at T = 0.272 s, Ns = 4352.  Nothing of the
reference's source travels: the file holds the tree, the configurations as the reference drew them, the canned RIRs, what was drawn (file
names relative to the tree, crop start, SNR, the head and the sums of the white noise), the annotations of ``{idx}_info.npz`` and the
float signal handed to ``soundfile.write``, as f32.
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sarssl_boot  # noqa: E402,F401
import make_golden_rirmix as f20  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FS, T, NS, NMIC, C, ISM_DB = 16000, 0.272, 4352, 2, 343.0, 12
SEED, ITEMS = 1, 3                 # stage pretrain
SNR_RANGE = (15, 30)
SMALL = dict(room_sz_range=[(3, 4), (3, 4), (2.5, 3)], T60_range=(0.2, 0.4))
ARGS = dict(abs_weights_range=[(0.5, 1)] * 6, c=C, ism_db=ISM_DB, array_pos_ratio_range=[(0.2, 0.8), (0.2, 0.8), (0.1, 0.5)],
            num_source_range=(1, 1), source_state="static", min_src_array_dist=0.3, min_src_boundary_dist=0.3, nb_points=1,
            traj_pt_mode="time", room_cfg=None)
WHITE_HEAD = 32


def canned_rir(k, cfg):
    """(rir (nch, L), rir_dp (nch, 1600)) float32 for item k: this tool's own draw, no room model."""
    from sar_ssl_amd import roomsim
    rs = np.random.RandomState(220 + k)
    L = roomsim.plan_rir(cfg, FS, C, ISM_DB)["n_len"]
    h = rs.standard_normal((NMIC, L)) * 10.0 ** (-3.0 * np.arange(L) / (FS * float(cfg["T60_specify"]))) * 0.05
    dp = np.zeros((NMIC, int(0.1 * FS)))
    for m in range(NMIC):
        p = 40 + 3 * k + 2 * m
        h[m, :p] = 0.0
        h[m, p] = 0.2
        dp[m, p - 1:p + 2] = (0.03, 0.2, -0.02)
    return h.astype(np.float32), dp.astype(np.float32)


def run_reference(save_dp=False):
    """The reference's generate_microphone_signal(..., save_dp=save_dp) for the ITEMS items -> (F22's arrays, {file name: (the float
    array handed to soundfile.write, fs)}).  The generation loop of F22, and of F24 (tools/make_golden_simsig_dp.py: save_dp=True, the
    same draws)."""
    import ref_shim
    from sar_ssl_amd import roomsim
    f20._install_stubs()
    written = {}
    sys.modules["soundfile"].write = lambda file, data, fs, **kw: written.update({os.path.basename(str(file)): (np.array(data), fs)})
    data_gen = os.path.join(ref_shim.REF_CODE, "data_generation")
    if data_gen not in sys.path:
        sys.path.insert(0, data_gen)
    for name in ("matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["mpl_toolkits.mplot3d"], "Axes3D"):
        sys.modules["mpl_toolkits.mplot3d"].Axes3D = None
    import scipy.stats  # noqa: F401
    canned = {}
    g = sys.modules["gpuRIR"]
    g.att2t_SabineEstimator, g.t2n = roomsim.att2t, (lambda Tdiff, room_sz: roomsim.t2n(Tdiff, room_sz, C))
    current = {}

    def simulate_rir(room_sz, beta, pos_src, pos_rcv, nb_img, Tmax, fs, Tdiff, orV_rcv, mic_pattern, c):
        rir, dp = canned[current["idx"]]
        direct = list(np.asarray(nb_img).reshape(-1)) == [1, 1, 1] and Tmax == 0.1
        return (dp if direct else rir).astype(np.float64)[None]             # (npt, nch, nsample), float64 as the labels widen it

    g.simulateRIR = simulate_rir
    import utils_simu_rir_sig as ref
    import utils_array as ref_array
    import utils_src as ref_src
    import utils_noise as ref_noise

    listdir = os.listdir
    os.listdir = lambda p: sorted(listdir(p))                  # sorted listings, in this process only (SourceBank(sort=True) matches)
    files = {k: v for k, v in f20.tree_arrays().items() if k.startswith("src/")}
    store = f20.pack_tree(files)
    sa = ref.SpatialAcoustics()
    cfgs = [sa.generate_random_spatial_acoustics(mic_array_cfg=ref_array.mic_array_cfg_2ch, seed=SEED, idx=k, **dict(ARGS, **SMALL))
            for k in range(ITEMS)]
    for k, cfg in enumerate(cfgs):
        for name, v in cfg.items():
            store["item/%d/cfg/%s" % (k, name)] = np.asarray(v)
        canned[k] = canned_rir(k, cfg)
        lab = roomsim.labels(canned[k][0], canned[k][1], cfg, FS, C)
        assert lab["ok"], (k, lab)                             # (the reference would retry for ever)
        store["item/%d/rir" % k], store["item/%d/rir_dp" % k] = canned[k]
    with tempfile.TemporaryDirectory() as root:
        f20.write_tree(root, files)
        src = ref_src.WSJ0Dataset(path=os.path.join(root, "src", "tr"), T=T, fs=FS, num_source=1)
        noi = ref_noise.NoiseSignal(T=T, fs=FS, nmic=NMIC, noise_type="diffuse_white", noise_path="", c=C)
        roomir = ref.RoomImpulseResponse(fs=FS, c=C, ism_db=ISM_DB)
        store["speakers"] = np.array(src.spkIDs)
        drawn, log = {}, {}
        orig = noi.generate_diffuse_noise

        def spy(noise, mic_pos, **kw):
            drawn["white"] = np.array(noise)
            return orig(noise, mic_pos, **kw)

        noi.generate_diffuse_noise = spy
        pad_orig = ref_src.pad_cut_sig_samespk

        def pad_spy(utt_path_list, current_utt_idx, nsample_desired, fs_desired):
            n0 = len(f20.READS)
            out_sig = pad_orig(utt_path_list, current_utt_idx, nsample_desired, fs_desired)
            used = [f for f, _ in f20.READS[n0:]]
            sig = np.concatenate([sys.modules["soundfile"].read(f)[0] for f in used])
            del f20.READS[n0 + len(used):]
            st = [i for i in np.flatnonzero(sig[:sig.shape[0] - nsample_desired + 1] == out_sig[0]) if np.array_equal(sig[i:i + nsample_desired], out_sig)]
            assert len(st) == 1
            log.update(utt_idx=current_utt_idx, utt_files=used, crop_start=st[0])
            return out_sig

        ref_src.pad_cut_sig_samespk = pad_spy
        gen = ref.MicrophoneSignalOrRIR()
        out_dir = os.path.join(root, "out")
        for k in range(ITEMS):
            current["idx"] = k
            drawn.clear()
            log.clear()
            del f20.READS[:]
            gen.generate_microphone_signal(idx=k, sa_cfgs=[dict(c) for c in cfgs], fs=FS, c=C, roomir=roomir, srcdataset=src, noidataset=noi,
                                           snr_range=SNR_RANGE, save_to=out_dir, save_dp=save_dp, gpu_conv=False, seed=SEED)
            sig, fs = written["%d.wav" % k]
            assert fs == FS and sig.shape == (NS, NMIC)
            pre = "item/%d/" % k
            store[pre + "out"] = np.asarray(sig, np.float32)                # (F20 stores its outputs the same way)
            info = dict(np.load(os.path.join(out_dir, "%d_info.npz" % k), allow_pickle=True))
            for name in ("T60_edc", "SNR", "src_idx", "TDOA", "DRR", "C50"):
                store[pre + "info/" + name] = np.asarray(info[name])
            store[pre + "info_keys"] = np.array(sorted(info))
            store[pre + "utt_idx"], store[pre + "crop_start"] = np.array(log["utt_idx"]), np.array(log["crop_start"])
            store[pre + "utt_files"] = np.array([os.path.relpath(f, root) for f in log["utt_files"]])
            w = drawn["white"]
            store[pre + "white_head"], store[pre + "white_sums"] = w[:WHITE_HEAD].copy(), np.array([w.sum(), (w ** 2).sum()])
            print("item %d: src_idx %d utt %d crop %d SNR %.4f T60_edc %.4f DRR %s C50 %s peak %.4f" % (
                k, info["src_idx"], log["utt_idx"], log["crop_start"], info["SNR"], info["T60_edc"], info["DRR"], info["C50"], np.abs(sig).max()))
    store["consts"] = np.array([FS, NS, NMIC, SEED, ITEMS])
    store["T"], store["snr_range"], store["c"], store["ism_db"] = np.array(T), np.array(SNR_RANGE), np.array(C), np.array(ISM_DB)
    store["small_room_sz_range"], store["small_T60_range"] = np.array(SMALL["room_sz_range"]), np.array(SMALL["T60_range"])
    os.listdir, ref_src.pad_cut_sig_samespk = listdir, pad_orig
    return store, written


def main():
    store, _ = run_reference()
    out = os.path.join(GOLD, "f22_simsig.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
