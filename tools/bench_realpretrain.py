"""Real-data pretraining on the shapes it was built for -> profiles/realpretrain.txt

    python tools/bench_realpretrain.py [--items 256] [--crops 64] [--batch 64] [--steps 24] [--out profiles/realpretrain.txt]

1. generator   items/s of realsig.generate (gen_sig_from_real_rir.py) as a whole - plan, read, render, pack, write - at T = 4.112 s, batch 16,
               over a synthetic measured bank (16 RIRs of 4 000 - 16 000 taps, noise cuts for half of them) and a synthetic speech tree;
               second pass, so the files of the first are overwritten as a re-run overwrites them.
2. kernel      ONE sarssl_resample_poly_batch launch over --crops crops of 197 376 x 2 PCM-16 samples at 48 kHz -> 16 kHz against the same
               crops through --crops sarssl_resample_poly launches, device events, the two interleaved pass by pass, median of 20
               [min, max]; bytes moved over the batch launch's time as a share of the HBM peak.
3. step        segments/s of STFTLearner.pretrain_epoch (the captured step, STFT inside the replay) fed by realsig.RealMixLoader over a
               50 % LOCATA mix - one 15-channel 48 kHz recording and fixed files, weights 1 : 1 - against the same epoch over the same
               number of batches resident on the device; one untimed epoch each (capture), then the two interleaved epoch by epoch.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sarssl_boot  # noqa: E402,F401

FS, FS_REC, T, NS = 16000, 48000, 4.112, 65792
HBM_PEAK = 8.0e12              # bytes/s (MI355X)


def synthetic_bank(root, nrir=16):
    from sar_ssl_amd.dataset import write_wav_pcm16
    rs = np.random.RandomState(1)
    for k in range(nrir):
        L = int(rs.randint(4000, 16001))
        h = rs.standard_normal((1, 2, L, 1)) * np.exp(-np.arange(L) / (L / 6.0))[None, None, :, None] * 0.1
        h[0, 0, 40, 0], h[0, 1, 47, 0] = 1.0, 0.9
        d = os.path.join(root, "rir", "ACE", "Room%d" % (k // 4), "Lin8Ch")
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, "SP1_MP%d-1-2.npy" % k), h.astype(np.float32))
        np.savez(os.path.join(d, "SP1_MP%d-1-2_info.npz" % k), fs=np.array(FS), T60fromDataset=np.array(0.5), DRR=np.array(1.0), C50=np.array(9.0),
                 ABS=np.array(0.2))
        if k % 2 == 0:
            nd = os.path.join(root, "rir", "ACE_noise", "Room%d" % (k // 4), "Lin8Ch")
            os.makedirs(nd, exist_ok=True)
            write_wav_pcm16(os.path.join(nd, "_MP%d-1-2_Fan.wav" % k), (rs.standard_normal((6 * FS, 2)) * 2000).astype(np.int16), FS)
    for s in range(4):
        for u in range(4):
            p = os.path.join(root, "src", "tr", "si_tr_s", "spk%d" % s, "utt%d.wav" % u)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            x = np.cumsum(rs.standard_normal(6 * FS)) * 200 + rs.standard_normal(6 * FS) * 2000
            write_wav_pcm16(p, np.clip(x, -30000, 30000).astype(np.int16)[:, None], FS)
    return os.path.join(root, "rir"), os.path.join(root, "src")


def bench_generator(torch, root, items):
    from sar_ssl_amd import realsig, rirsynth
    rir, src = synthetic_bank(root)
    bank = rirsynth.MeasuredBank(realsig.rir_dirs(rir, "pretrain", "ACE"), FS, sort=True)
    sources = rirsynth.SourceBank(src + "/tr", FS, sort=True)
    save = os.path.join(root, "micsig")
    out = {}
    for rep in ("first", "second"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        realsig.generate(save, "pretrain", "ACE", bank, sources, items, T, FS, (15, 30), "cuda", 16)
        out[rep] = items / (time.perf_counter() - t0)
    return out, os.path.join(save, "pretrain", "ACE")


def bench_kernel(torch, crops, reps=20):
    from sar_ssl_amd import hip
    rs = np.random.RandomState(2)
    n = int(T * FS_REC)
    x = torch.from_numpy(rs.randint(-20000, 20000, (crops, n, 2)).astype(np.int16)).cuda()
    n_in = torch.full((crops,), n, dtype=torch.int32, device="cuda")
    out = torch.empty((crops, NS, 2), dtype=torch.float32, device="cuda")

    def batch():
        hip.resample_poly_batch(x, n_in, FS, FS_REC, out=out)

    def singles():
        for b in range(crops):
            hip.resample_poly(x[b], FS, FS_REC, out=out[b])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for fn in (batch, singles):
        fn()
    ref = out.clone()
    batch()
    torch.cuda.synchronize()
    assert torch.equal(ref.view(torch.int32), out.view(torch.int32)), "the batch launch and the single launches differ"
    tb, ts = [], []
    for _ in range(reps):
        tb.append(timed(batch))
        ts.append(timed(singles))
    nbytes = x.numel() * 2 + out.numel() * 4
    return dict(batch=tb, singles=ts, nbytes=nbytes, crops=crops)


def bench_step(torch, root, fixed_dir, batch, steps):
    import random
    from sar_ssl_amd import learner as L, model, realsig, runtime
    from sar_ssl_amd.dataset import write_wav_pcm16
    rs = np.random.RandomState(3)
    frames, nch = 30 * FS_REC, 15
    t = np.arange(frames)[:, None] / FS_REC
    rec = 6000 * np.sin(2 * np.pi * (300 + 40 * np.arange(nch)[None, :]) * t) + 1500 * rs.standard_normal((frames, nch))
    p = os.path.join(root, "locata", "eval", "task1", "recording1", "dicit", "audio_array_dicit.wav")
    os.makedirs(os.path.dirname(p), exist_ok=True)
    write_wav_pcm16(p, rec.astype(np.int16), FS_REC)
    corpora = [realsig.FixedCorpus(fixed_dir, "train", sort=True), realsig.RecordingCorpus(os.path.join(root, "locata"), T, FS, "train", sort=True)]
    loader = realsig.RealMixLoader(corpora, [1, 1], steps * batch, batch, T, FS, device="cuda", nthreads=8)
    np.random.seed(5)
    share = np.mean([pl["kind"] == "recording" for b in loader.plan_batches() for pl in b])
    resident = [[b[0].clone()] for b, _ in zip(loader, range(4))]
    resident = [resident[i % len(resident)] for i in range(steps)]
    torch.manual_seed(4321)
    net = model.SARSSL(sig_shape=(256, 256, 2, 2), pretrain=True, device="cuda")
    lrn = L.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=FS, task=None, ch_mode="M")
    lrn.cuda()
    lrn.amp()
    runtime.set_precision("hybrid")
    random.seed(99)
    lrn.pretrain_epoch(resident, lr=1e-4, epoch=0)                # capture + first replays
    res = {"loader": [], "resident": []}
    for ep in range(1, 4):
        for name, data in (("loader", loader), ("resident", resident)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lrn.pretrain_epoch(data, lr=1e-4, epoch=ep)
            torch.cuda.synchronize()
            res[name].append(steps * batch / (time.perf_counter() - t0))
    # the loader alone: what it can deliver when nothing consumes
    t0 = time.perf_counter()
    for b in loader:
        pass
    torch.cuda.synchronize()
    res["loader_alone"] = steps * batch / (time.perf_counter() - t0)
    res["share"] = float(share)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realpretrain.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_realpretrain.py measures on the GPU; there is nothing to time without one")
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    root = tempfile.mkdtemp(prefix="sarssl_realpretrain_", dir=base)
    try:
        gen, fixed_dir = bench_generator(torch, root, a.items)
        k = bench_kernel(torch, a.crops)
        s = bench_step(torch, root, fixed_dir, a.batch, a.steps)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    med = lambda v: float(np.median(v))
    tb, ts = med(k["batch"]), med(k["singles"])
    lines = ["tools/bench_realpretrain.py on %s (one box, one process; files on %s)" % (torch.cuda.get_device_name(0), "/dev/shm" if base else "a tmp dir"),
             "",
             "1. gen_sig_from_real_rir.py (realsig.generate), T = 4.112 s, batch 16, %d items, 16 measured RIRs of 4 000 - 16 000 taps:" % a.items,
             "   first pass  %8.1f items/s      second pass (files overwritten)  %8.1f items/s" % (gen["first"], gen["second"]),
             "",
             "2. %d crops of 197 376 x 2 PCM-16 samples, 48 kHz -> 16 kHz, f32 out (device events, interleaved, median of 20 [min, max]):" % k["crops"],
             "   one sarssl_resample_poly_batch launch    %8.3f ms [%.3f, %.3f]   %.1f GB/s = %.1f %% of the HBM peak"
             % (tb, min(k["batch"]), max(k["batch"]), k["nbytes"] / tb / 1e6, 100 * k["nbytes"] / (tb * 1e-3) / HBM_PEAK),
             "   %d sarssl_resample_poly launches          %8.3f ms [%.3f, %.3f]   x %.2f" % (k["crops"], ts, min(k["singles"]), max(k["singles"]), ts / tb),
             "   (outputs of the two bit-equal)",
             "",
             "3. STFTLearner.pretrain_epoch, hybrid mode, batch %d, %d steps per epoch, %.0f %% of the items LOCATA crops (15-channel recording):"
             % (a.batch, a.steps, 100 * s["share"]),
             "   fed by realsig.RealMixLoader   %s segments/s (epochs 1 - 3)" % ", ".join("%.0f" % v for v in s["loader"]),
             "   batches resident on the device %s segments/s" % ", ".join("%.0f" % v for v in s["resident"]),
             "   the loader alone, nothing consuming    %.0f segments/s" % s["loader_alone"]]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
