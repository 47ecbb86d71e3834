"""Fixture F23 of the per-room generator (gen_simu_certain_room.py), from the REAL reference (build container only):

    python tools/make_golden_certainroom.py        ->  tests/golden/f23_certainroom.npz

Imports the reference's code/data_generation/gen_simu_certain_room.py through oracle/ref_shim.py's path with the in-process stand-ins of
tools/make_golden_simsig.py (``soundfile``: reads served by the project's own PCM reader, ``write`` recorded; ``gpuRIR``: ``simulateRIR``
returns canned RIRs that this tool draws itself, checked here to pass the accept test; sorted listings) and one for ``jsonargparse``, writes
F20's speech tree to a temporary directory and calls the reference's OWN ``GenerateRandomMicSigOfCertainRoom`` (use_gpu=False; once with
noise_type diffuse_white, once with spatial_white) and ``GenerateRandomRIROfCertainRoom`` for stage train, ROOMS rooms x RIRS placements
x SIGS signals at T = 0.272 s - so the seed and directory arithmetic is the reference's.  Nothing of the reference's source travels: the
file holds the tree, the rooms' and placements' dictionaries as the reference drew them, the canned RIRs (one per signal item, shared by
both noise types; the bank's placement takes its first signal's), what was drawn, the relative output paths, the annotations of
``{i}_info.npz``, the float signal handed to ``soundfile.write`` as f32 and the key names of ``all_info.npz``.
"""
import importlib.util
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
import make_golden_simsig as f22  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FS, T, NS, NMIC, C, ISM_DB = f22.FS, f22.T, f22.NS, f22.NMIC, f22.C, f22.ISM_DB
STAGE, SEED = "train", 4000000
ROOMS, RIRS, SIGS = 2, 2, 2
NOISE_TYPES = ("diffuse_white", "spatial_white")
INFO_VALUES = ("T60_edc", "SNR", "src_idx", "TDOA", "DRR", "C50")


def canned_rir(g, Tmax):
    """(rir (nch, L), rir_dp (nch, 1600)) float32 for signal item g of a room whose RIRs last Tmax = 40 / 60 T60_sabine: this tool's own
    draw, no room model.  The values keep 11 mantissa bits (the file compresses)."""
    rs = np.random.RandomState(230 + g)
    L = int(np.ceil(Tmax * FS))
    h = rs.standard_normal((NMIC, L)) * 10.0 ** (-3.0 * np.arange(L) / (FS * Tmax * 60.0 / 40.0)) * 0.05
    dp = np.zeros((NMIC, int(0.1 * FS)))
    for m in range(NMIC):
        p = 40 + 3 * g + 2 * m
        h[m, :p] = 0.0
        h[m, p] = 0.2
        dp[m, p - 1:p + 2] = (0.03, 0.2, -0.02)
    h = (np.ascontiguousarray(h, np.float32).view(np.uint32) & np.uint32(0xfffff000)).view(np.float32)
    return h, dp.astype(np.float32)


def main():
    import ref_shim
    from sar_ssl_amd import roomsim
    f20._install_stubs()
    data_gen = os.path.join(ref_shim.REF_CODE, "data_generation")
    if data_gen not in sys.path:
        sys.path.insert(0, data_gen)
    for name in ("matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "jsonargparse", "tqdm"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["mpl_toolkits.mplot3d"], "Axes3D"):
        sys.modules["mpl_toolkits.mplot3d"].Axes3D = None
    if not hasattr(sys.modules["jsonargparse"], "ArgumentParser"):
        sys.modules["jsonargparse"].ArgumentParser = None                   # (only the command line uses it)
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = lambda *a, **k: types.SimpleNamespace(set_description=lambda s: None, update=lambda: None)
    import scipy.stats  # noqa: F401
    g = sys.modules["gpuRIR"]
    g.att2t_SabineEstimator, g.t2n = roomsim.att2t, (lambda Tdiff, room_sz: roomsim.t2n(Tdiff, room_sz, C))
    canned, state = {}, dict(full=0, every=1, limit=0)

    def simulate_rir(room_sz, beta, pos_src, pos_rcv, nb_img, Tmax, fs, Tdiff, orV_rcv, mic_pattern, c):
        direct = list(np.asarray(nb_img).reshape(-1)) == [1, 1, 1] and Tmax == 0.1
        if not direct:
            state["full"] += 1
            if state["full"] > state["limit"]:
                raise RuntimeError("a canned RIR failed the reference's accept test: it asks for another")
            key = (state["full"] - 1) * state["every"]
            if key not in canned:
                canned[key] = canned_rir(key, Tmax)
            assert canned[key][0].shape[1] == int(np.ceil(Tmax * FS))
        rir, dp = canned[(state["full"] - 1) * state["every"]]
        return (dp if direct else rir).astype(np.float64)[None]             # (npt, nch, nsample), float64 as the labels widen it

    g.simulateRIR = simulate_rir
    import utils_src as ref_src
    import utils_noise as ref_noise
    spec = importlib.util.spec_from_file_location("ref_gen_simu_certain_room", os.path.join(data_gen, "gen_simu_certain_room.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)                               # (by path: the repository's own gen_simu_certain_room.py has the same name)

    listdir = os.listdir
    os.listdir = lambda p: sorted(listdir(p))                  # sorted listings, in this process only (SourceBank(sort=True) matches)
    files = {k: v for k, v in f20.tree_arrays().items() if k.startswith("src/")}
    store = f20.pack_tree(files)
    drawn, log, items = {}, {}, []
    for name in ("generate_diffuse_noise", "generate_Gaussian_noise"):
        def spy(self, *a, _orig=getattr(ref_noise.NoiseSignal, name), _first=name == "generate_diffuse_noise", **kw):
            out = _orig(self, *a, **kw)
            drawn["white"] = np.array(a[0] if _first else out)
            return out
        setattr(ref_noise.NoiseSignal, name, spy)
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
    small = dict(room_sz_range=f22.SMALL["room_sz_range"], T60_range=f22.SMALL["T60_range"])
    with tempfile.TemporaryDirectory() as root:
        f20.write_tree(root, files)

        def on_write(file, data, fs, **kw):
            assert fs == FS
            items.append(dict(path=os.path.relpath(str(file), os.path.join(root, "out", nt, STAGE)), sig=np.array(data), white=drawn.pop("white"),
                              log=dict(log)))
            log.clear()

        sys.modules["soundfile"].write = on_write
        placements = None
        for nt in NOISE_TYPES:
            del items[:]
            state.update(full=0, every=1, limit=ROOMS * RIRS * SIGS)
            gen.GenerateRandomMicSigOfCertainRoom(mic_array_cfg=gen.mic_array_cfg_2ch, snr_range=f22.SNR_RANGE, noise_type=nt, fs=FS, c=C,
                                                  ism_db=ISM_DB, T=T, src_dir=os.path.join(root, "src"), stage=STAGE, room_num=ROOMS,
                                                  rir_num_each_room=RIRS, sig_num_each_rir=SIGS, save_to=os.path.join(root, "out", nt),
                                                  use_gpu=False, **small)
            assert len(items) == ROOMS * RIRS * SIGS == state["full"]
            out_dir = os.path.join(root, "out", nt, STAGE)
            all_info = np.load(os.path.join(out_dir, "all_info.npz"), allow_pickle=True)
            cfgs = all_info["cfgs"].item()
            store["all_info_keys"], store["all_info_cfgs_keys"] = np.array(sorted(all_info.files)), np.array(list(cfgs))
            assert int(all_info["args"].item()["seed"]) == SEED
            if placements is None:
                placements = {(r, j): cfgs["R%d" % r][j * SIGS] for r in range(ROOMS) for j in range(RIRS)}
            for r in range(ROOMS):
                assert len(cfgs["R%d" % r]) == RIRS * SIGS
                for i, cfg in enumerate(cfgs["R%d" % r]):
                    assert all(np.array_equal(np.asarray(cfg[k]), np.asarray(placements[r, i // SIGS][k])) for k in cfg)
            store["sig/%s/written" % nt] = np.array(sorted(os.path.relpath(os.path.join(d, f), out_dir) for d, _, fs_ in os.walk(out_dir) for f in fs_))
            for gi, item in enumerate(items):
                pre = "sig/%s/%d/" % (nt, gi)
                r, i = divmod(gi, RIRS * SIGS)
                assert item["sig"].shape == (NS, NMIC)
                lab = roomsim.labels(canned[gi][0], canned[gi][1], placements[r, i // SIGS], FS, C)
                assert lab["ok"], (gi, lab)
                store[pre + "path"] = np.array(item["path"])
                store[pre + "out"] = np.asarray(item["sig"], np.float32)
                info = dict(np.load(os.path.join(out_dir, item["path"].replace(".wav", "_info.npz")), allow_pickle=True))
                for name in INFO_VALUES:
                    store[pre + "info/" + name] = np.asarray(info[name])
                store[pre + "info_keys"] = np.array(sorted(info))
                store[pre + "utt_idx"], store[pre + "crop_start"] = np.array(item["log"]["utt_idx"]), np.array(item["log"]["crop_start"])
                store[pre + "utt_files"] = np.array([os.path.relpath(f, root) for f in item["log"]["utt_files"]])
                w = item["white"]
                store[pre + "white_head"], store[pre + "white_sums"] = w[:f22.WHITE_HEAD].copy(), np.array([w.sum(), (w ** 2).sum()])
                print("%s %s: src_idx %d utt %d crop %d SNR %.4f T60_edc %.4f DRR %s C50 %s peak %.4f" % (
                    nt, item["path"], info["src_idx"], item["log"]["utt_idx"], item["log"]["crop_start"], info["SNR"], info["T60_edc"],
                    info["DRR"], info["C50"], np.abs(item["sig"]).max()))
        for (r, j), cfg in placements.items():
            for name, v in cfg.items():
                store["room/%d/placement/%d/cfg/%s" % (r, j, name)] = np.asarray(v)
        for gi in range(ROOMS * RIRS * SIGS):
            store["rir/%d" % gi], store["rir_dp/%d" % gi] = canned[gi]
        # the bank: placement (r, j) is served the canned RIR of its first signal
        state.update(full=0, every=SIGS, limit=ROOMS * RIRS)
        bank = os.path.join(root, "bank")
        gen.GenerateRandomRIROfCertainRoom(mic_array_cfg=gen.mic_array_cfg_2ch, fs=FS, c=C, ism_db=ISM_DB, T=T, stage=STAGE, room_num=ROOMS,
                                           rir_num_each_room=RIRS, save_to=bank, use_gpu=False, **small)
        assert state["full"] == ROOMS * RIRS
        out_dir = os.path.join(bank, STAGE)
        store["bank/written"] = np.array(sorted(os.path.relpath(os.path.join(d, f), out_dir) for d, _, fs_ in os.walk(out_dir) for f in fs_))
        all_info = np.load(os.path.join(out_dir, "all_info.npz"), allow_pickle=True)
        cfgs = all_info["cfgs"].item()
        store["bank/all_info_keys"], store["bank/all_info_cfgs_keys"] = np.array(sorted(all_info.files)), np.array(list(cfgs))
        for (r, j), cfg in placements.items():
            assert len(cfgs["R%d" % r]) == RIRS and all(np.array_equal(np.asarray(cfgs["R%d" % r][j][k]), np.asarray(cfg[k])) for k in cfg)
            pre = "bank/%d/%d/" % (r, j)
            info = dict(np.load(os.path.join(out_dir, "R%d" % (r + 1), "%d_info.npz" % j), allow_pickle=True))
            store[pre + "info_keys"] = np.array(sorted(info))
            for name in ("T60_edc", "TDOA", "DRR", "C50", "fs"):
                store[pre + "info/" + name] = np.asarray(info[name])
            rir = np.load(os.path.join(out_dir, "R%d" % (r + 1), "%d.npy" % j))
            assert rir.dtype == np.float32 and rir.ndim == 4 and np.array_equal(rir[0, :, :, 0], canned[(r * RIRS + j) * SIGS][0])
    store["consts"] = np.array([FS, NS, NMIC, SEED, ROOMS, RIRS, SIGS])
    store["stage"], store["noise_types"] = np.array(STAGE), np.array(NOISE_TYPES)
    store["T"], store["snr_range"], store["c"], store["ism_db"] = np.array(T), np.array(f22.SNR_RANGE), np.array(C), np.array(ISM_DB)
    store["small_room_sz_range"], store["small_T60_range"] = np.array(small["room_sz_range"]), np.array(small["T60_range"])
    out = os.path.join(GOLD, "f23_certainroom.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
