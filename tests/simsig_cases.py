"""Shared inputs of tests/test_simsig_cpu.py and tests/test_gpu_simsig.py: the synthetic RIRs the labels are checked on, and the small
rooms / speech tree of the end-to-end runs.  Everything is float32 as the kernel reads it; only ``device_labels`` touches the GPU."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
LEAD = 37                        # leading zeros in front of channel 0's peak; channel m's peak is 2 m samples later
F22 = os.path.join(ROOT, "tests", "golden", "f22_simsig.npz")

SMALL = dict(room_sz_range=[(3, 4), (3, 4), (2.5, 3)], T60_range=(0.2, 0.4))


def synth_rir(seed, t60, L, nch=2):
    """standard_normal((nch, L)) 10^(-3 n / (fs T60)), LEAD (+ 2 per channel) leading zeros, then a positive peak -> (nch, L) f32."""
    rs = np.random.RandomState(seed)
    h = rs.standard_normal((nch, L)) * 10.0 ** (-3.0 * np.arange(L) / (FS * t60))
    for m in range(nch):
        p = LEAD + 2 * m
        h[m, :p] = 0.0
        if p < L:
            h[m, p] = 4.0
    return h.astype(np.float32)


def synth_dp(nch=2, Ld=1600, sign=1.0):
    """A direct path: a short windowed pulse around the RIR's peak of each channel -> (nch, Ld) f32."""
    dp = np.zeros((nch, Ld))
    k = np.arange(-4, 5)
    for m in range(nch):
        p = LEAD + 2 * m
        dp[m, p - 4:p + 5] = sign * 4.0 * np.sinc(k + 0.3) * np.hanning(11)[1:-1]
    return dp.astype(np.float32)


FULL = [(3, 0.2, 2049), (0, 0.3, 4097), (1, 0.5, 8000), (2, 0.87, 13867)]          # (seed, T60, L): accepted, full length


def label_cases(nch=2):
    """[(name, rir (nch, L) f32, rir_dp (nch, Ld) f32, T60_specify)]: the full-length cases, then the failing and degenerate ones."""
    cases = [("full_%g_%d" % (t, L), synth_rir(s, t, L, nch), synth_dp(nch), t) for s, t, L in FULL]
    for L in (600, 257, 40):
        cases.append(("short_%d" % L, synth_rir(5, 0.3, L, nch), synth_dp(nch), 0.3))
    for L in (2, 1):
        h = np.full((nch, L), 0.5, np.float32)
        h[:, -1] = 1.0
        cases.append(("tiny_%d" % L, h, synth_dp(nch), 0.3))
    cases.append(("all_zero", np.zeros((nch, 2049), np.float32), synth_dp(nch), 0.3))
    h = synth_rir(6, 0.3, 4097, nch)
    h[-1, 1000] = np.nan
    cases.append(("nan", h, synth_dp(nch), 0.3))
    h = synth_rir(7, 0.3, 4097, nch)
    h[:, 900:1400] = 0.0
    cases.append(("plateau", h, synth_dp(nch), 0.3))
    h = synth_rir(8, 0.3, 4097, nch)
    h[:, 60] = -9.0                                      # the absolute maximum is negative: the signed one stays at the peak
    cases.append(("signed_max", h, synth_dp(nch), 0.3))
    cases.append(("off_specify", synth_rir(0, 0.3, 4097, nch), synth_dp(nch), 0.4))          # 0.1 s off: env_ok False
    # every value of the direct path below zero: the host's argmax lands on the zero padding behind it
    cases.append(("negative_dp", synth_rir(0, 0.3, 4097, nch), -np.abs(synth_dp(nch, 100)) - np.float32(0.01), 0.3))
    return cases


def host_labels(rir, rir_dp, t60_specify):
    """roomsim.labels with the per-channel estimates added (t60, corr), unrounded DRR / C50 and nd: what the kernel's outputs are held to."""
    from sar_ssl_amd import roomsim
    cfg = {"T60_specify": t60_specify, "mic_pos": np.zeros((max(2, rir.shape[0]), 3)), "src_traj_pts": np.ones((1, 3, 1))}
    with np.errstate(all="ignore"):
        lab = roomsim.labels(rir, rir_dp, cfg)
        out = dict(flags=int(lab["rir_ok"]) | (int(lab["env_ok"]) << 1), t60_edc=float(lab["T60_edc"]))
        nch = rir.shape[0]
        out["t60"], out["corr"] = np.full(nch, np.nan), np.full(nch, np.nan)
        if lab["rir_ok"]:
            for m in range(nch):
                out["t60"][m], out["corr"][m] = roomsim._rt60_from_rir(np.asarray(rir[m], np.float64), FS)
        # annotations(), before the float16 rounding
        r64, d64 = np.asarray(rir, np.float64), np.asarray(rir_dp, np.float64)
        nsamp = max(r64.shape[1], d64.shape[1])
        h = np.concatenate([r64[0], np.zeros(nsamp - r64.shape[1])])
        nd = int(np.argmax(np.concatenate([d64[0], np.zeros(nsamp - d64.shape[1])])))
        n = np.arange(nsamp)
        n0 = int(FS * 2.5 / 1000)
        dpr = ((n >= nd - n0) & (n <= nd + n0)).astype("float")
        out["drr"] = float(10 * np.log10(np.sum(h ** 2 * dpr) / (np.sum(h ** 2 * (1 - dpr)) + 1e-8) + 1e-8))
        early = (n <= nd + int(FS * 50 / 1000)).astype("float")
        out["c50"] = float(10 * np.log10(np.sum(h ** 2 * early) / (np.sum(h ** 2 * (1 - early)) + 1e-8) + 1e-8))
        out["nd"] = nd
        assert np.float16(out["drr"]) == lab["DRR"] or (np.isnan(out["drr"]) and np.isnan(lab["DRR"]))
        assert np.float16(out["c50"]) == lab["C50"] or (np.isnan(out["c50"]) and np.isnan(lab["C50"]))
    return out


def same_labels(got, want, tol):
    """The pass conditions: flags and nd equal, NaN where the host has NaN, otherwise within tol[key] -> {key: largest distance}."""
    assert got["flags"] == want["flags"], (got["flags"], want["flags"])
    assert int(got["nd"]) == want["nd"], (got["nd"], want["nd"])
    dist = {}
    for k in ("t60", "corr", "drr", "c50", "t60_edc"):
        g, w = np.atleast_1d(np.asarray(got[k], np.float64)), np.atleast_1d(np.asarray(want[k], np.float64))
        assert g.shape == w.shape and (np.isnan(g) == np.isnan(w)).all(), (k, g, w)
        ok = ~np.isnan(w)
        d = float(np.abs(g[ok] - w[ok]).max()) if ok.any() else 0.0
        assert d <= tol["t60" if k == "t60_edc" else k], (k, d, g, w)
        dist[k] = d
    return dist


def device_labels(items, lmax=None, ldmax=None, device="cuda:0"):
    """hip.rir_labels of [(name, rir, rir_dp, T60_specify)] as one ragged batch -> one dict of numpy values per item."""
    import torch
    from sar_ssl_amd import hip
    dev = torch.device(device)
    B, nch = len(items), items[0][1].shape[0]
    lmax = lmax or max(i[1].shape[1] for i in items)
    ldmax = ldmax or max(i[2].shape[1] for i in items)
    rir, dp = np.zeros((B, nch, lmax), np.float32), np.zeros((B, nch, ldmax), np.float32)
    for b, (_, h, d, _) in enumerate(items):
        rir[b, :, :h.shape[1]], dp[b, :, :d.shape[1]] = h, d
    lab = hip.rir_labels(torch.from_numpy(rir).to(dev), torch.tensor([i[1].shape[1] for i in items], dtype=torch.int32, device=dev),
                         torch.from_numpy(dp).to(dev), torch.tensor([i[2].shape[1] for i in items], dtype=torch.int32, device=dev),
                         torch.tensor([i[3] for i in items], dtype=torch.float64, device=dev), float(FS))
    h = hip.rir_labels_host(lab)
    return [{k: v[b].copy() for k, v in h.items()} for b in range(B)]


def write_speech_tree(root, fx):
    """F22's speech tree below ``root`` (src/<tr|dt|et>/<set>/<speaker>/<utterance>.wav; F22 holds tr, which is written under all three
    stage directories) -> the --src_dir to pass."""
    from sar_ssl_amd.dataset import write_wav_pcm16
    for rel in [str(r) for r in fx["tree_order"]]:
        for sub in ("tr", "dt", "et"):
            path = os.path.join(str(root), rel.replace("src/tr/", "src/%s/" % sub, 1))
            os.makedirs(os.path.dirname(path), exist_ok=True)
            write_wav_pcm16(path, fx["tree/" + rel], FS)
    return os.path.join(str(root), "src")


def f22_cfg(fx, k):
    """Configuration k of F22 as the dictionary the reference drew."""
    pre = "item/%d/cfg/" % k
    cfg = {key[len(pre):]: fx[key] for key in fx.files if key.startswith(pre)}
    for key in ("array_type", "mic_pattern"):
        cfg[key] = str(cfg[key])
    for key in ("T60_sabine", "T60_specify", "array_scale", "array_rotate_azi"):
        cfg[key] = float(cfg[key])
    cfg["room_sz"] = list(cfg["room_sz"])
    return cfg
