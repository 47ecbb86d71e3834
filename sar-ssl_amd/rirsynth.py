"""Microphone signals synthesised from stored RIRs: the real-data branch of the downstream stage.

The reference builds every training item of its real-world room-acoustics experiment on the fly in DataLoader workers
(RandomMicSigFromRIRDataset, code/dataset.py:287-382): a source utterance convolved with a measured or a simulated RIR, noise scaled
to a drawn SNR against the direct-path power, peak normalisation.  Here the host only picks files and draws scalars (``plan_*``: the
reference's numpy draw order, call for call; ``draw_item`` is the part all items share, roomsim.plan_sig's too) and the GPU renders whole
batches (hip.rir_mix / diffuse_noise / gauss_fill, csrc/rirmix.hip; ``mix_simulated`` is also roomsim.simulate_signals' mix).
``restate_*`` are the f64 numpy / scipy restatement of one item that the kernels and the reference fixture are checked against.
``DeviceSourceBank`` is ``SourceBank`` with the corpus on the device: it plans a crop from its length table and hip.src_gather
(csrc/srcbank.hip) cuts it there - the online loader's source (onlinesig.py).
"""
import math
import os
import warnings
from pathlib import Path

import numpy as np

from .pipeline import EpochLoader

FS = 16000
DP_TIME_MS = 2.5                 # gen_sig_from_real_rir.py:231
GAIN_MEASURED, GAIN_SIMULATED = 0.9, 1.0


def dp_halfwidth(fs=FS):
    return int(fs * DP_TIME_MS / 1000)


# ---------------------------------------------------------------------------------------------------------------- f64 restatement
def direct_path_window(rir, n0):
    """rir (nch, L) -> rir kept where nd - n0 <= n <= nd + n0, nd = np.argmax per channel (_find_dpmax_from_RIR)."""
    rir = np.asarray(rir)
    nd = np.argmax(rir, axis=1)[:, None]
    n = np.arange(rir.shape[1])[None, :]
    return rir * ((n >= nd - n0) & (n <= nd + n0))


def restate_mix(src, rir, rir_dp=None, n0=None, noise=None, snr_db=0.0, gain=1.0, return_dp=False):
    """One item in f64: src (Ns,), rir (nch, L), rir_dp (nch, Ld) or a window half-width n0, noise (Ns, nch) or None -> (Ns, nch);
    return_dp=True: -> (that, the direct-path signal (Ns, nch) at the same scale, dp / value * gain)."""
    import scipy.signal
    src = np.asarray(src, np.float64)
    rir = np.asarray(rir, np.float64)
    ns = src.shape[0]
    if rir_dp is None:
        rir_dp = direct_path_window(rir, n0)
    rir_dp = np.asarray(rir_dp, np.float64)
    clean = scipy.signal.fftconvolve(src[:, None], rir.T, mode="full", axes=0)[:ns]
    dp = scipy.signal.fftconvolve(src[:, None], rir_dp.T, mode="full", axes=0)[:ns]
    noise = np.zeros_like(clean) if noise is None else np.asarray(noise, np.float64)
    p_dp = np.mean(np.sum(dp ** 2, axis=0) / ns)
    p_n = np.mean(np.sum(noise ** 2, axis=0) / ns)
    mic = clean + np.sqrt(p_dp / (10 ** (snr_db / 10))) / (np.sqrt(p_n) + 1e-10) * noise
    value = max(np.abs(mic).max(), np.abs(dp).max())
    return (mic / value * gain, dp / value * gain) if return_dp else mic / value * gain


def mixing_table(mic_pos, fs=FS, c=343.0, nfft=256):
    """(129, M, M) f64: row 0 zero, rows k >= 1 the upper Cholesky factor of the spherical coherence sinc(w_k d_pq / (c pi))
    (utils_noise.py:178-232)."""
    import scipy.linalg
    mic_pos = np.asarray(mic_pos, np.float64)
    M = mic_pos.shape[0]
    w_rad = 2 * math.pi * fs * np.arange(nfft // 2 + 1) / nfft
    dist = np.linalg.norm(mic_pos[:, None, :] - mic_pos[None, :, :], axis=-1)
    C = np.zeros((nfft // 2 + 1, M, M))
    for k in range(1, nfft // 2 + 1):
        DC = np.sinc(w_rad[k] * dist / (c * math.pi))
        np.fill_diagonal(DC, 1.0)
        C[k] = scipy.linalg.cholesky(DC)
    return C


def restate_diffuse(white, C, eps=1e-8):
    """white (Ns, M), C (129, M, M) -> the diffuse field (Ns, M) / (its signed maximum + eps) (utils_noise.py:68-71, 234-253)."""
    import scipy.signal
    K = (C.shape[0] - 1) * 2
    white = np.asarray(white, np.float64)
    assert white.shape[0] % (K // 4) == 0, "the stft / istft round trip returns another length"
    # scipy's boundary='zeros' (K/2 zeros on both sides, removed again by istft) written out: scipy itself shortens nperseg when the
    # UNPADDED input is shorter than K, which no item of the reference ever is.  Identical to the reference's two calls from Ns = K on.
    pad = np.zeros((K // 2, white.shape[1]))
    _, _, N = scipy.signal.stft(np.concatenate([pad, white, pad]).T, window="hann", nperseg=K, noverlap=0.75 * K, nfft=K,
                                boundary=None, padded=False)
    X = np.einsum("fmn,mft->nft", np.conj(C), N)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)          # NOLA at the first / last padded sample, which is cut off below
        _, y = scipy.signal.istft(X, window="hann", nperseg=K, noverlap=0.75 * K, nfft=K, boundary=False)
    y = y.T[K // 2:-(K // 2)]
    return y / (np.max(y) + eps)


# ---------------------------------------------------------------------------------------------------------------- file banks
def _listing(entries, sort):
    """Directory listings are taken in the file system's order, as the reference takes them (os.listdir, Path.rglob), so the same seed
    draws the same files as the reference does on that machine; sort=True makes the order (and the draws) portable."""
    entries = list(entries)
    return sorted(entries) if sort else entries


def explore_corpus(path, file_extension, sort=False):
    """{name: subtree | file path} and the flat path list of a directory, in os.listdir order (utils_src.py:11-21)."""
    tree, paths = {}, []
    for item in _listing(os.listdir(path), sort):
        full = os.path.join(path, item)
        if os.path.isdir(full):
            tree[item], sub = explore_corpus(full, file_extension, sort)
            paths += sub
        elif item.split(".")[-1] == file_extension:
            tree[item.split(".")[0]] = full
            paths += [full]
    return tree, paths


def _read_f64(path, fs):
    from .dataset import read_wav_pcm16
    pcm, wav_fs = read_wav_pcm16(path)
    if wav_fs != fs:
        raise ValueError("%s: sampling rate %d, expected %d (the reference raises here too, utils_src.py:52-54)" % (path, wav_fs, fs))
    if pcm.shape[1] != 1:
        raise ValueError("%s: %d channels, a source utterance has one" % (path, pcm.shape[1]))
    return pcm[:, 0].astype(np.float64) / 32768.0           # soundfile.read's default float64 conversion of PCM-16


class SourceBank:
    """WSJ0Dataset (utils_src.py:65-122): ``path/<set>/<speaker>/<utterance>.wav``; item ``idx`` is a speaker, the utterance and the crop
    are drawn."""

    def __init__(self, path, fs=FS, sort=False):
        corpus, self.paths = explore_corpus(path, "wav", sort)
        self.spk_wavs, self.spk_ids = [], []
        for spks in corpus.values():
            if not isinstance(spks, dict) or not all(isinstance(v, dict) for v in spks.values()):
                raise ValueError("%s: expected <set>/<speaker>/<utterance>.wav below the source directory" % path)
            self.spk_wavs += [list(v.values()) for v in spks.values()]
            self.spk_ids += list(spks.keys())
        if not self.spk_ids:
            raise ValueError("%s: no speakers found" % path)
        self.fs = fs

    def __len__(self):
        return len(self.spk_ids)

    def draw(self, rs, idx, nsample):
        """-> (source (nsample,) f64 with its mean removed, {'utt_idx', 'crop_start', 'utt_files'}): utterance index, then same-speaker
        padding from that utterance on, then the crop start (pad_cut_sig_samespk)."""
        idx = idx % len(self.spk_ids)
        utts = self.spk_wavs[idx]
        utt_idx = int(rs.randint(0, len(utts)))
        _read_f64(self.paths[utt_idx], self.fs)             # (sic) the reference reads this entry of the GLOBAL list, for its rate only
        sig, used, cur = np.zeros(0), [], utt_idx
        while sig.shape[0] < nsample:
            sig = np.concatenate((sig, _read_f64(utts[cur], self.fs)))
            used.append(utts[cur])
            cur = cur + 1 if cur + 1 < len(utts) else 0
        st = int(rs.randint(0, sig.shape[0] - nsample + 1))
        s = sig[st:st + nsample].copy()
        s -= s.mean()
        return s, {"utt_idx": utt_idx, "crop_start": st, "utt_files": used}


MAXSEG = 32                      # utterances a crop may run through (csrc/srcbank.hip SB_MAXSEG)


class DeviceSourceBank:
    """``SourceBank``'s corpus kept on the device: every utterance is read once (``min(16, workers)`` threads) into ONE flat int16 tensor
    on ``device``; the host keeps each utterance's offset and length and each speaker's utterances in ``SourceBank``'s order.  ``plan``
    makes ``SourceBank.draw``'s draws from the length table alone - no file is opened - and hip.src_gather (csrc/srcbank.hip) cuts the
    crops on the device, bit-equal to ``draw(...)[0].astype(float32)``.  A corpus of more than ``max_bytes`` bytes of PCM-16 is refused
    (never truncated); files at another rate or with several channels raise as in ``SourceBank``."""

    def __init__(self, path, fs=FS, device="cuda", sort=False, max_bytes=8 << 30, workers=8):
        import torch
        from concurrent.futures import ThreadPoolExecutor
        from .dataset import read_wav_pcm16
        names = SourceBank(path, fs, sort)
        self.fs, self.paths, self.spk_ids = fs, names.paths, names.spk_ids
        index = {p: k for k, p in enumerate(self.paths)}
        self.spk_utts = [[index[p] for p in utts] for utts in names.spk_wavs]
        on_disk = sum(os.path.getsize(p) for p in self.paths)
        if on_disk - 4096 * len(self.paths) > max_bytes:          # (no header is that long: refused before anything is read)
            raise ValueError("%s: the corpus' files hold %d bytes, the device-resident bank is limited to max_bytes = %d: nothing is "
                             "truncated - raise the limit (--simu-online-bank-gb) or use a smaller corpus" % (path, on_disk, max_bytes))

        def read(p):
            pcm, wav_fs = read_wav_pcm16(p)
            if wav_fs != fs:
                raise ValueError("%s: sampling rate %d, expected %d (the reference raises here too, utils_src.py:52-54)" % (p, wav_fs, fs))
            if pcm.shape[1] != 1:
                raise ValueError("%s: %d channels, a source utterance has one" % (p, pcm.shape[1]))
            return np.ascontiguousarray(pcm[:, 0])
        with ThreadPoolExecutor(max_workers=max(1, min(16, int(workers)))) as pool:
            utts = list(pool.map(read, self.paths))
        self.lengths = np.array([u.shape[0] for u in utts], np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        nbytes = 2 * int(self.lengths.sum())
        if nbytes > max_bytes:
            raise ValueError("%s: the corpus holds %d bytes of PCM-16, the device-resident bank is limited to max_bytes = %d: nothing is "
                             "truncated - raise the limit (--simu-online-bank-gb) or use a smaller corpus" % (path, nbytes, max_bytes))
        if any(self.lengths[u].sum() == 0 for u in self.spk_utts):
            raise ValueError("%s: a speaker without a single sample" % path)
        self.flat = torch.from_numpy(np.concatenate(utts)).to(torch.device(device))
        self.device = self.flat.device

    def __len__(self):
        return len(self.spk_ids)

    def plan(self, rs, idx, nsample):
        """``SourceBank.draw``'s draws on ``rs`` - utterance index, then the crop start over the same-speaker concatenation from that
        utterance on (it wraps to the speaker's first) - -> its record {'utt_idx', 'crop_start', 'utt_files'} with 'segments':
        [(offset, length), ...] of the utterances the crop covers in the bank, and 'seg_start': the crop's first sample inside the first."""
        utts = self.spk_utts[idx % len(self.spk_ids)]
        utt_idx = int(rs.randint(0, len(utts)))
        total, used, cur = 0, [], utt_idx
        while total < nsample:
            used.append(utts[cur])
            total += int(self.lengths[utts[cur]])
            cur = cur + 1 if cur + 1 < len(utts) else 0
        st = int(rs.randint(0, total - nsample + 1))
        segments, pos, seg_start = [], 0, 0
        for k in used:
            n = int(self.lengths[k])
            if n and pos + n > st and pos < st + nsample:
                if not segments:
                    seg_start = st - pos
                segments.append((int(self.offsets[k]), n))
            pos += n
        if len(segments) > MAXSEG:
            raise ValueError("a crop of %d samples of speaker %s runs through %d utterances, more than MAXSEG = %d: the speaker's utterances "
                             "are too short for this segment length" % (nsample, self.spk_ids[idx % len(self.spk_ids)], len(segments), MAXSEG))
        return {"utt_idx": utt_idx, "crop_start": st, "utt_files": [self.paths[k] for k in used], "segments": segments, "seg_start": seg_start}

    def host_crop(self, rec, nsample):
        """The crop of a ``plan`` record as ``SourceBank.draw`` returns it ((nsample,) f64, mean removed), gathered in numpy."""
        sig = np.concatenate([self.flat[o:o + n].cpu().numpy() for o, n in rec["segments"]]).astype(np.float64) / 32768.0
        s = sig[rec["seg_start"]:rec["seg_start"] + nsample].copy()
        s -= s.mean()
        return s

    @staticmethod
    def tables(recs):
        """The host arrays hip.src_gather takes for a batch of ``plan`` records -> (seg_off (B, 32) i64, seg_len (B, 32) i32, nseg, start)."""
        B = len(recs)
        off, ln = np.zeros((B, MAXSEG), np.int64), np.zeros((B, MAXSEG), np.int32)
        for b, r in enumerate(recs):
            n = len(r["segments"])
            off[b, :n], ln[b, :n] = [s[0] for s in r["segments"]], [s[1] for s in r["segments"]]
        return (off, ln, np.array([len(r["segments"]) for r in recs], np.int32), np.array([r["seg_start"] for r in recs], np.int64))

    def gather(self, recs, nsample, out=None):
        """(B, nsample) f32 on the device: the crops of a batch of ``plan`` records (hip.src_gather)."""
        from . import hip
        return hip.src_gather(self.flat, *self.tables(recs), nsample, out=out)


def _static_rir(path, rir):
    if rir.ndim != 4:
        raise ValueError("%s: expected (npoint, nch, nsample, nsrc), got shape %s" % (path, rir.shape))
    if rir.shape[0] != 1 or rir.shape[3] != 1:
        raise ValueError("%s: npoint = %d, nsrc = %d: only one static source is rendered (the reference raises for npoint > 1 and sums "
                         "sources; neither is emulated)" % (path, rir.shape[0], rir.shape[3]))
    return rir[0, :, :, 0]


def _check_fs(path, info, fs):
    if int(info["fs"]) != fs:
        raise ValueError("%s: RIR sampled at %s Hz, fs = %d: not resampled (the reference's resample_poly call runs along the wrong axis of "
                         "its 4-D array; that is not emulated)" % (path, info["fs"], fs))


def _pad_stack(arrs, dtype=np.float32):
    L = max(a.shape[1] for a in arrs)
    out = np.zeros((len(arrs), arrs[0].shape[0], L), dtype)
    for i, a in enumerate(arrs):
        out[i, :, :a.shape[1]] = a
    return out, np.array([a.shape[1] for a in arrs], np.int32)


class MeasuredBank:
    """real_dataset.RIRDataset (gen_sig_from_real_rir.py:70-135): every ``*.npy`` below the directories, ``_info.npz`` next to it, noise
    recordings ``*_<mic>*.wav`` below the sibling ``<dataset>_noise`` tree.  RIRs and labels stay resident."""

    def __init__(self, rir_dir_list, fs=FS, sort=False):
        dirs = rir_dir_list if isinstance(rir_dir_list, list) else [rir_dir_list]
        self.files = []
        for d in dirs:
            self.files += _listing(Path(d).rglob("*.npy"), sort)
        if not self.files:
            raise ValueError("no measured RIRs (*.npy) below %s" % (dirs,))
        self.fs, self.rirs, self.labels, self.noise_files, self._probe = fs, [], [], [], {}
        for f in self.files:
            info = dict(np.load(str(f).replace(".npy", "_info.npz")))
            _check_fs(f, info, fs)
            self.rirs.append(_static_rir(f, np.load(f).astype(np.float32)))
            self.labels.append({"T60": info["T60fromDataset"].astype(np.float32), "DRR": info["DRR"].astype(np.float32),
                                "C50": info["C50"].astype(np.float32), "ABS": info["ABS"].astype(np.float32)})
            attrs = str(f).split("/")
            if len(attrs) < 4:
                raise ValueError("%s: the noise directory rule needs <dataset>/<a>/<b>/<file>.npy" % f)
            mic = attrs[-1].split("_")[1].split(".")[0]
            noise_dir = str(f.parent).replace(attrs[-4], attrs[-4] + "_noise")
            self.noise_files.append(_listing(Path(noise_dir).rglob("*_%s*.wav" % mic), sort))
        self.nch = self.rirs[0].shape[0]

    def __len__(self):
        return len(self.files)

    def probe(self, path):
        """(nch, fs, nsample) of a noise recording, cached."""
        from .dataset import wav_probe
        p = self._probe.get(path)
        if p is None:
            p = self._probe[path] = wav_probe(path)
            if p[1] != self.fs:
                raise ValueError("%s: noise sampled at %d Hz, fs = %d: not resampled" % (path, p[1], self.fs))
        return p

    def to_device(self, device):
        import torch
        rir, lens = _pad_stack(self.rirs)
        self.dev_rir, self.dev_len = torch.from_numpy(rir).to(device), torch.from_numpy(lens).to(device)


class SimulatedBank:
    """simu_dataset.RIRDataset (utils_simu_rir_sig.py:1080-1120): every ``*_dp.npy`` with its ``.npy`` and ``_info.npz``."""

    def __init__(self, rir_dir_list, fs=FS, c=343.0, sort=False):
        dirs = rir_dir_list if isinstance(rir_dir_list, list) else [rir_dir_list]
        self.files = []
        for d in dirs:
            self.files += _listing(Path(d).rglob("*_dp.npy"), sort)
        if not self.files:
            raise ValueError("no simulated RIRs (*_dp.npy) below %s" % (dirs,))
        self.fs, self.rirs, self.dps, self.labels, self.mic_pos, self.tables = fs, [], [], [], [], []
        for f in self.files:
            rir_file = str(f).replace("_dp.npy", ".npy")
            info = dict(np.load(rir_file.replace(".npy", "_info.npz")))
            _check_fs(rir_file, info, fs)
            self.rirs.append(_static_rir(rir_file, np.load(rir_file).astype(np.float32)))
            self.dps.append(_static_rir(f, np.load(f)))
            room = info["room_sz"]
            vol, sur = room[0] * room[1] * room[2], room[0] * room[1] + room[0] * room[2] + room[1] * room[2]
            self.labels.append({"T60": info["T60_edc"].astype(np.float32), "DRR": info["DRR"].astype(np.float32),
                                "C50": info["C50"].astype(np.float32), "ABS": np.array(0.161 * vol / sur / info["T60_edc"]).astype(np.float32)})
            self.mic_pos.append(np.asarray(info["mic_pos"], np.float64))
            self.tables.append(mixing_table(self.mic_pos[-1], fs=fs, c=c))
        self.nch = self.rirs[0].shape[0]

    def __len__(self):
        return len(self.files)

    def to_device(self, device):
        import torch
        rir, lens = _pad_stack(self.rirs)
        dp, dlens = _pad_stack(self.dps)
        self.dev_rir, self.dev_len = torch.from_numpy(rir).to(device), torch.from_numpy(lens).to(device)
        self.dev_dp, self.dev_dplen = torch.from_numpy(dp).to(device), torch.from_numpy(dlens).to(device)
        self.dev_C = torch.from_numpy(np.stack(self.tables).astype(np.float32)).to(device)


# ---------------------------------------------------------------------------------------------------------------- host plans
def draw_item(rs, sources, T, fs=FS, snr_range=(15, 30), nmic=2, draw_white=False):
    """The draws every kind of item ends with, on ``rs`` where it stands: source index, SourceBank.draw (utterance index, crop start), with
    draw_white=True the white noise (int(T fs), nmic), the SNR -> SourceBank.draw's record with src_idx, src, white (or None) and snr."""
    src_idx = int(rs.randint(0, len(sources)))
    src, rec = sources.draw(rs, src_idx, int(T * fs))
    white = rs.standard_normal((int(T * fs), nmic)) if draw_white else None
    snr = float(rs.uniform(*snr_range))
    return dict(rec, src_idx=src_idx, src=src, white=white, snr=snr)


def plan_measured(rs, idx, seed, bank, sources, T, fs=FS, snr_range=(15, 30)):
    """real_dataset.MicSigFromRIRDataset.__getitem__'s draws (gen_sig_from_real_rir.py:215-236) on the RandomState ``rs``: seed + idx,
    RIR index, noise file and its start sample, then ``draw_item`` without white noise."""
    rs.seed(seed + idx)
    rir_idx = int(rs.randint(0, len(bank)))
    noise_file, noise_start = None, 0
    files = bank.noise_files[rir_idx]
    if files:
        noise_file = files[int(rs.choice(len(files), 1, replace=False)[0])]
        _, nfs, frames = bank.probe(noise_file)
        nsample_noise, want = int(frames / nfs * nfs), int(T * nfs)
        assert nsample_noise >= want, "the sample number of noise signal is smaller than desired duration~"
        noise_start = int(rs.randint(0, nsample_noise - want + 1))
    return dict(draw_item(rs, sources, T, fs, snr_range), variant="measured", idx=idx, rir_idx=rir_idx, rir_file=bank.files[rir_idx],
                noise_file=noise_file, noise_start=noise_start, labels=bank.labels[rir_idx])


def plan_simulated(rs, idx, seed, bank, sources, T, fs=FS, snr_range=(15, 30), nmic=2, draw_white=True):
    """simu_dataset.MicSigFromRIRDataset.__getitem__'s draws (utils_simu_rir_sig.py:1203-1223): seed + idx, RIR index, then ``draw_item``
    (the white noise is left out with draw_white=False: the device draws its own)."""
    rs.seed(seed + idx)
    rir_idx = int(rs.randint(0, len(bank)))
    return dict(draw_item(rs, sources, T, fs, snr_range, nmic, draw_white), variant="simulated", idx=idx, rir_idx=rir_idx,
                rir_file=bank.files[rir_idx], noise_file=None, noise_start=0, labels=bank.labels[rir_idx])


def variants_of(real_sim_ratio):
    r = list(real_sim_ratio)
    assert r in [[0, 1], [1, 0], [1, 1]], real_sim_ratio
    return {(0, 1): ["simulated"], (1, 0): ["measured"], (1, 1): ["measured", "simulated"]}[tuple(r)]


def plan_random(rs, variants, seed, measured, simulated, sources, T, fs=FS, snr_range=(15, 30), nmic=2, draw_white=True):
    """RandomMicSigFromRIRDataset.__getitem__ (code/dataset.py:372-377): variant, then the item index below 1e8, both on the stream
    that the item then reseeds and continues."""
    variant = variants[int(rs.randint(0, len(variants)))]
    idx = int(rs.randint(0, int(1e8)))
    if variant == "measured":
        return plan_measured(rs, idx, seed, measured, sources, T, fs, snr_range)
    return plan_simulated(rs, idx, seed, simulated, sources, T, fs, snr_range, nmic, draw_white)


def restate_item(plan, measured, simulated, fs=FS, c=343.0):
    """The f64 restatement of a planned item (numpy-drawn white noise) -> (Ns, nch)."""
    ns = plan["src"].shape[0]
    if plan["variant"] == "measured":
        noise = None
        if plan["noise_file"] is not None:
            noise = read_noise(plan["noise_file"], plan["noise_start"], ns, measured.nch, fs)
        return restate_mix(plan["src"], measured.rirs[plan["rir_idx"]], n0=dp_halfwidth(fs), noise=noise, snr_db=plan["snr"],
                           gain=GAIN_MEASURED)
    i = plan["rir_idx"]
    noise = restate_diffuse(plan["white"], simulated.tables[i])
    return restate_mix(plan["src"], simulated.rirs[i], rir_dp=simulated.dps[i], noise=noise, snr_db=plan["snr"], gain=GAIN_SIMULATED)


def read_noise(path, start, nsample, nch, fs=FS):
    """Samples [start, start + nsample) of a noise recording as f32 (nsample, nch) (soundfile.read(..., dtype='float32'))."""
    from .dataset import read_wav_batch
    return read_wav_batch([path], nsample, nch, fs, start, nthreads=1)[0].numpy().astype(np.float32) / np.float32(32768.0)


# ---------------------------------------------------------------------------------------------------------------- batch loader
def mix_simulated(src, rir, rir_len, dp, dp_len, white, C, snr, gain, out=None, out_dp=None):
    """The mix of a batch of simulated items on the current stream: ``white`` (B, Ns, nch) becomes, in place, the diffuse field of the
    mixing tables C (B, 129, nch, nch), and hip.rir_mix adds it to src * rir at snr dB against the direct path dp -> (B, Ns, nch);
    out_dp (B, Ns, nch), where given, receives the direct-path signal at the same scale.
    Where ``white`` comes from stays with the caller: the loader and roomsim.simulate_signals key their device draws differently."""
    from . import hip
    field = hip.diffuse_noise(white, C, out=white)
    return hip.rir_mix(src, rir, rir_len, snr, gain, rir_dp=dp, dp_len=dp_len, noise=field, out=out, out_dp=out_dp)


class RirSynthLoader(EpochLoader):
    """Batches of RandomMicSigFromRIRDataset items, rendered on the GPU: yields ``(mic_sig (B, Ns, nch) f32 on the device,
    {task: (B,) f32 tensor})`` in the shape Learner.train_epoch / test_epoch iterate.

    pipeline.EpochLoader's producer thread plans the items (``plan_item``: the reference's draws on the epoch's one host stream) and reads
    sources and noise segments; the consumer enqueues the render of batch i + 1 on a side stream before it hands out batch i.
    noise="numpy": the simulated variant's white noise is the reference's host draw (parity); noise="device" (default):
    sarssl_gauss_fill keyed by (seed, running item index) - not numpy's stream, and the SNR draw then follows the source crop directly."""

    def __init__(self, measured, simulated, sources, dataset_sz, batch_size, T, fs=FS, nmic=2, snr_range=(15, 30), real_sim_ratio=(1, 0),
                 seed=1, noise="device", device="cuda", c=343.0, drop_last=False, prefetch=2):
        assert noise in ("numpy", "device")
        super().__init__(dataset_sz, batch_size, device, drop_last, prefetch)
        self.variants = variants_of(real_sim_ratio)
        assert ("measured" not in self.variants or measured is not None) and ("simulated" not in self.variants or simulated is not None)
        self.measured, self.simulated, self.sources = measured, simulated, sources
        self.T, self.fs, self.nmic, self.snr_range, self.seed, self.noise = T, fs, nmic, tuple(snr_range), seed, noise
        self.nsample = int(T * fs)
        for bank in (measured, simulated):
            if bank is not None:
                if bank.nch != nmic:
                    raise ValueError("RIRs with %d channels, nmic = %d" % (bank.nch, nmic))
                if not hasattr(bank, "dev_rir") or bank.dev_rir.device != self.device:
                    bank.to_device(self.device)

    def plan_item(self, rs):
        return plan_random(rs, self.variants, self.seed, self.measured, self.simulated, self.sources, self.T, self.fs, self.snr_range,
                           self.nmic, draw_white=self.noise == "numpy")

    def handout(self, res):
        return res, [res[0]] + list(res[1].values())

    def host_batch(self, plans):
        """Pinned host tensors of one batch: what the render uploads.  Filled through their numpy views (no torch op runs on the host)."""
        import torch
        pin = self.device.type == "cuda"
        ns, nch = self.nsample, self.nmic

        def buf(*shape):
            t = torch.empty(shape, dtype=torch.float32, pin_memory=pin)
            return t, t.numpy()
        h = {"plans": plans}
        h["src"], src = buf(len(plans), ns)
        for i, p in enumerate(plans):
            src[i] = p["src"]
        m = [i for i, p in enumerate(plans) if p["variant"] == "measured"]
        s = [i for i, p in enumerate(plans) if p["variant"] == "simulated"]
        if any(plans[i]["noise_file"] is not None for i in m):
            h["noise"], noise = buf(len(m), ns, nch)
            for j, i in enumerate(m):
                if plans[i]["noise_file"] is not None:
                    noise[j] = read_noise(plans[i]["noise_file"], plans[i]["noise_start"], ns, nch, self.fs)
                else:
                    noise[j] = 0.0
        if s and self.noise == "numpy":
            h["white"], white = buf(len(s), ns, nch)
            for j, i in enumerate(s):
                white[j] = plans[i]["white"]
        h["scal"], scal = buf(2, len(plans))
        scal[0] = [p["snr"] for p in plans]
        scal[1] = [GAIN_MEASURED if p["variant"] == "measured" else GAIN_SIMULATED for p in plans]
        h["m"], h["s"] = m, s
        h["ridx"] = torch.from_numpy(np.array([p["rir_idx"] for p in plans], np.int64))
        keys = plans[0]["labels"].keys()
        h["labels"] = {k: torch.from_numpy(np.stack([np.asarray(p["labels"][k], np.float32) for p in plans])) for k in keys}
        return h

    def render(self, h, item0=0):
        """Enqueue the render of a host batch on the current stream -> (mic_sig (B, Ns, nch), labels)."""
        import torch
        from . import hip
        dev = self.device
        src = h["src"].to(dev, non_blocking=True)
        scal = h["scal"].to(dev, non_blocking=True)
        ridx = h["ridx"].to(dev, non_blocking=True)
        B = src.shape[0]
        out = torch.empty((B, self.nsample, self.nmic), dtype=torch.float32, device=dev)
        for ids, variant in ((h["m"], "measured"), (h["s"], "simulated")):
            if not ids:
                continue
            whole = len(ids) == B
            sel = None if whole else torch.from_numpy(np.array(ids, np.int64)).to(dev, non_blocking=True)
            pick = (lambda t: t) if whole else (lambda t: t.index_select(0, sel).contiguous())
            bank = self.measured if variant == "measured" else self.simulated
            r = pick(ridx)
            lens = bank.dev_len.index_select(0, r)
            lmax = int(max(bank.rirs[h["plans"][i]["rir_idx"]].shape[1] for i in ids))
            rir = bank.dev_rir.index_select(0, r)[:, :, :lmax].contiguous()
            dst = out if whole else torch.empty((len(ids), self.nsample, self.nmic), dtype=torch.float32, device=dev)
            if variant == "measured":
                noise = h["noise"].to(dev, non_blocking=True) if "noise" in h else None
                hip.rir_mix(pick(src), rir, lens, pick(scal[0]), pick(scal[1]), n0=dp_halfwidth(self.fs), noise=noise, out=dst)
            else:
                if self.noise == "numpy":
                    white = h["white"].to(dev, non_blocking=True)
                else:
                    white = hip.gauss_fill(torch.empty((len(ids), self.nsample, self.nmic), dtype=torch.float32, device=dev), self.seed, item0)
                ldmax = int(max(bank.dps[h["plans"][i]["rir_idx"]].shape[1] for i in ids))
                mix_simulated(pick(src), rir, lens, bank.dev_dp.index_select(0, r)[:, :, :ldmax].contiguous(), bank.dev_dplen.index_select(0, r),
                              white, bank.dev_C.index_select(0, r).contiguous(), pick(scal[0]), pick(scal[1]), out=dst)
            if not whole:
                out.index_copy_(0, sel, dst)
        labels = {k: v.to(dev, non_blocking=True) for k, v in h["labels"].items()}
        return out, labels
