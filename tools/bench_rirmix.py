"""The RIR renderer against what it has to keep up with: the real-data downstream branch's shape - 16 items of Ns = 65 792 samples
(4.112 s), two channels, RIR lengths spread over 0.3 to 1.3 s, both variants - in one process on one box, interleaved rounds, medians
with [min, max]:

  render        the GPU render of one batch, alone (device events): measured variant (windowed direct path, recorded noise), simulated
                variant (explicit direct path; sarssl_gauss_fill -> sarssl_diffuse_noise -> sarssl_rir_mix)
  restatement   the f64 numpy / scipy restatement of one item on this host's CPU, one thread (what the reference's loader workers do)
  step          the captured downstream training step at T = 256 frames, batch 16 (hybrid mode), through Learner.train_epoch, fed
                (a) one resident batch, (b) a RirSynthLoader in noise="device" mode over a generated tree; and the host plan of a batch
                alone (file reads, draws, pinned buffers - no GPU work)

Requirement the profile states: render < step (one batch ahead hides it).  Prints one JSON line; --out also writes the text summary.

    python tools/bench_rirmix.py [--steps 24] [--rounds 5] [--out profiles/rirmix.txt]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sarssl_boot  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402

FS, T_SEC, FRAMES, B = 16000, 4.112, 256, 16
NS = int(T_SEC * FS)


def med(v):
    return {"median": round(statistics.median(v), 3), "min_max": [round(min(v), 3), round(max(v), 3)]}


def write_tree(root, rs):
    """8 measured RIRs in 4 rooms (one room with a noise recording), 4 simulated RIRs, 4 speakers x 3 utterances of about 3 s."""
    from sar_ssl_amd.dataset import write_wav_pcm16
    lens = np.linspace(0.3 * FS, 1.3 * FS, 12).astype(int)
    rs.shuffle(lens)

    def rir(L, delay):
        h = (rs.standard_normal((1, 2, L, 1)) * np.exp(-np.arange(L) / (L / 6.0))[None, None, :, None] * 0.1).astype(np.float32)
        h[0, 0, delay, 0], h[0, 1, delay + 4, 0] = 1.0, 0.9
        return h

    for i in range(8):
        d = os.path.join(root, "real", "ACE", "Room%d" % (i // 2), "conf%d" % (i % 2))
        os.makedirs(d)
        np.save(os.path.join(d, "rir_mic%d.npy" % (i % 2)), rir(lens[i], 40 + i))
        np.savez(os.path.join(d, "rir_mic%d_info.npz" % (i % 2)), fs=FS, T60fromDataset=0.3 + 0.05 * i, DRR=1.0 * i, C50=10.0 + i, ABS=0.2)
    d = os.path.join(root, "real", "ACE_noise", "Room1", "conf0")
    os.makedirs(d)
    write_wav_pcm16(os.path.join(d, "ambient_mic0_fan.wav"), (rs.standard_normal((10 * FS, 2)) * 2000).astype(np.int16), FS)
    for i in range(4):
        d = os.path.join(root, "simu", "train", "R%d" % (i + 1))
        os.makedirs(d)
        h = rir(lens[8 + i], 50 + i)
        dp = np.zeros((1, 2, 128, 1), np.float32)
        dp[0, 0, 50 + i, 0], dp[0, 1, 54 + i, 0] = 1.0, 0.9
        np.save(os.path.join(d, "%d.npy" % i), h)
        np.save(os.path.join(d, "%d_dp.npy" % i), dp)
        np.savez(os.path.join(d, "%d_info.npz" % i), fs=FS, T60_edc=0.4 + 0.1 * i, DRR=1.0, C50=8.0, room_sz=np.array([5.0 + i, 4.0, 3.0]),
                 mic_pos=np.array([[2.0, 2.0, 1.5], [2.08, 2.0, 1.5]]))
    for s in range(4):
        d = os.path.join(root, "src", "tr", "set0", "spk%d" % s)
        os.makedirs(d)
        for u in range(3):
            x = np.cumsum(rs.standard_normal(3 * FS)) * 30 + rs.standard_normal(3 * FS) * 2000
            write_wav_pcm16(os.path.join(d, "utt%d.wav" % u), np.clip(x, -30000, 30000).astype(np.int16)[:, None], FS)
    real = os.path.join(root, "real", "ACE")
    return dict(real=[os.path.join(real, r) for r in sorted(os.listdir(real))], simu=os.path.join(root, "simu", "train"), src=os.path.join(root, "src", "tr"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="hybrid")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sar_ssl_amd import learner, model, rirsynth, runtime
    if not torch.cuda.is_available():
        raise SystemExit("bench_rirmix.py measures on the GPU; there is nothing to time without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    res = {"tool": "bench_rirmix", "items": B, "nsample": NS, "nch": 2, "frames": FRAMES, "precision": a.precision, "rounds": a.rounds,
           "steps_per_epoch": a.steps, "device": torch.cuda.get_device_name(0), "host_cpus_used": 1}
    with tempfile.TemporaryDirectory() as root:
        d = write_tree(root, rs)
        measured, simulated, sources = rirsynth.MeasuredBank(d["real"], fs=FS), rirsynth.SimulatedBank(d["simu"], fs=FS), rirsynth.SourceBank(d["src"], fs=FS)
        res["rir_taps"] = sorted(int(r.shape[1]) for r in measured.rirs + simulated.rirs)

        def loader(ratio, n, noise="device"):
            return rirsynth.RirSynthLoader(measured, simulated, sources, dataset_sz=n, batch_size=B, T=T_SEC, fs=FS, real_sim_ratio=ratio, seed=1,
                                           noise=noise, device=dev)
        # ---- the render of one batch, alone
        host = {}
        for name, ratio in (("measured", (1, 0)), ("simulated", (0, 1))):
            ld = loader(ratio, B)
            np.random.seed(1)
            host[name] = (ld, ld.host_batch(next(ld.plan_batches())))
        times = {k: [] for k in host}
        for r in range(a.rounds + 1):                       # round 0 warms up and is dropped
            for name, (ld, h) in host.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(4):
                    ld.render(h)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    times[name].append(e0.elapsed_time(e1) / 4)
        res["render_ms_per_batch"] = {k: med(v) for k, v in times.items()}
        # ---- the f64 restatement of one item on this host, one thread
        cpu = {k: [] for k in host}
        for r in range(min(a.rounds, 3) + 1):               # round 0 warms up (scipy's imports and plans) and is dropped
            for name, (ld, h) in host.items():
                p = h["plans"][r]
                if p["white"] is None and name == "simulated":
                    p = dict(p, white=rs.standard_normal((NS, 2)))
                t0 = time.perf_counter()
                rirsynth.restate_item(p, measured, simulated, fs=FS)
                if r:
                    cpu[name].append((time.perf_counter() - t0) * 1e3)
        res["restatement_ms_per_item_cpu_1thread"] = {k: med(v) for k, v in cpu.items()}
        # ---- the host plan of a batch alone
        ld = loader((1, 1), B * a.steps)
        np.random.seed(2)
        t0 = time.perf_counter()
        n = sum(1 for plans in ld.plan_batches() if ld.host_batch(plans))
        res["host_plan_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3 / n, 3)
        # ---- the captured training step, resident against loader-fed
        torch.manual_seed(0)
        net = model.SARSSL(sig_shape=(256, FRAMES, 2, 2), pretrain=False, device=dev, downstream_token="all", downstream_head="mlp",
                           downstream_embed="spat", downstream_dlabel=1)
        lrn = learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=FS, task="T60", ch_mode="M")
        lrn.cuda()
        lrn.amp(a.precision)
        np.random.seed(3)
        first = next(iter(loader((1, 1), B)))
        resident = [(first[0].clone(), {"T60": first[1]["T60"].clone()})] * a.steps

        def epoch(batches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lrn.train_epoch(batches, lr=1e-5, epoch=1, return_metric=True)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3
        steps = {"resident": [], "loader": []}
        for r in range(a.rounds + 1):
            np.random.seed(10 + r)
            for name in ("resident", "loader"):
                t = epoch(resident if name == "resident" else loader((1, 1), B * a.steps))
                if r:
                    steps[name].append(t)
        res["train_step_ms"] = {k: med(v) for k, v in steps.items()}
        res["loader_over_resident"] = round(statistics.median(steps["loader"]) / statistics.median(steps["resident"]), 3)
        runtime.set_precision("bf16")
    worst = max(v["median"] for v in res["render_ms_per_batch"].values())
    res["render_below_step"] = bool(worst < res["train_step_ms"]["resident"]["median"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(summary(res))


def summary(res):
    r, c, s = res["render_ms_per_batch"], res["restatement_ms_per_item_cpu_1thread"], res["train_step_ms"]
    lines = ["tools/bench_rirmix.py on %s (one box, one process, %d interleaved rounds after a warm-up round; median [min, max])" % (res["device"], res["rounds"]),
             "shape: %d items x %d samples x %d channels, RIR taps %s" % (res["items"], res["nsample"], res["nch"], res["rir_taps"]), ""]
    for k in ("measured", "simulated"):
        lines.append("GPU render of one batch, %-9s variant, alone (device events):   %8.3f ms  %s" % (k, r[k]["median"], r[k]["min_max"]))
    for k in ("measured", "simulated"):
        lines.append("f64 restatement of ONE item, %-9s variant, host CPU, 1 thread: %8.3f ms  %s" % (k, c[k]["median"], c[k]["min_max"]))
    lines += ["captured training step, T = %d frames, batch %d, %s mode, Learner.train_epoch, %d steps per epoch (host clock around an epoch that ends in a synchronise):"
              % (res["frames"], res["items"], res["precision"], res["steps_per_epoch"]),
              "  fed one resident batch:                       %8.3f ms / step  %s" % (s["resident"]["median"], s["resident"]["min_max"]),
              "  fed by RirSynthLoader(noise='device'), 1:1:   %8.3f ms / step  %s" % (s["loader"]["median"], s["loader"]["min_max"]),
              "  loader-fed / resident:                        %8.3f" % res["loader_over_resident"],
              "host plan of one batch alone (draws, source and noise file reads, pinned buffers; no GPU work): %.3f ms" % res["host_plan_ms_per_batch"],
              "render of a batch below the resident step (one batch ahead hides it): %s" % ("yes" if res["render_below_step"] else "NO"), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
