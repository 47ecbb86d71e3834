"""Throughput of the generators with the accept test on the device -> profiles/simsig.txt

    python tools/bench_simsig.py [--items 32] [--sig-items 64] [--save_dp] [--out profiles/simsig.txt]

1. gen_simu.py --mode rir at batch 1 / 4 / 16, default ranges, stage train: RIRs/s of a whole pass of the generator's own loop (plan,
   render, accept test, read-back; one attempt, no file is written) with roomsim.judge_on_host against roomsim.judge_on_device
   (csrc/rirlabel.hip), the two interleaved pass by pass on the same box, median of --reps passes each; the labels kernel alone, event-timed.
2. gen_simu.py --mode sig at batch 16, default ranges, T = 4.112 s, device noise, on a synthetic speech tree: items/s of
   roomsim.simulate_signals as a whole, and in a second, profiled pass the time per item of every stage - the GPU stages between events
   (hip.profile_start(all_calls=True): every C-ABI call under its entry point's name), the host stages by wall clock.
   --save_dp: part 2 at stage pretest_ins_T1000 with save_dp=True ({idx}_dp.wav beside every item: the mix is sarssl_rir_mix_dp).
Also the distances of parity.RIRLABELS over the cases of tests/simsig_cases.py.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sarssl_boot  # noqa: E402,F401


def rir_pass(roomsim, torch, dev, cfgs, seed, bs, where):
    """One pass of the generator's own loop (roomsim._generate, as simulate_bank runs it) over all items, with a sink that reads back what
    simulate_bank's reads back and writes nothing -> seconds.  One attempt: every item is rendered once, a rejected one not again."""
    def sink(batch, acc, lab):
        roomsim.read_back_accepted(batch, acc, lab)
        return [batch.ids[b] for b in acc]

    attempts, roomsim.MAX_ATTEMPTS = roomsim.MAX_ATTEMPTS, 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    roomsim._generate("bench", None, "train", cfgs, seed, roomsim.DEFAULTS, dev, "device", bs, where, sink, log=lambda s: None)
    torch.cuda.synchronize()
    roomsim.MAX_ATTEMPTS = attempts
    return time.perf_counter() - t0


def speech_tree(root, nspk=4, nutt=4, seconds=6.0, fs=16000, sub="tr"):
    from sar_ssl_amd.dataset import write_wav_pcm16
    rs = np.random.RandomState(0)
    for s in range(nspk):
        for u in range(nutt):
            path = os.path.join(root, sub, "si_tr_s", "spk%d" % s, "utt%d.wav" % u)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            x = np.cumsum(rs.standard_normal(int(seconds * fs))) * 200 + rs.standard_normal(int(seconds * fs)) * 2000
            write_wav_pcm16(path, np.clip(x, -30000, 30000).astype(np.int16)[:, None], fs)
    return root


class Wall:
    """Wraps a function and adds up the wall time spent in it."""

    def __init__(self, fn):
        self.fn, self.t, self.n = fn, 0.0, 0

    def __call__(self, *a, **k):
        t0 = time.perf_counter()
        try:
            return self.fn(*a, **k)
        finally:
            self.t += time.perf_counter() - t0
            self.n += 1


def main():
    import torch
    import simsig_cases as sc
    from sar_ssl_amd import dataset, hip, rirsynth, roomsim
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--sig-items", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--save_dp", action="store_true", help="--mode sig at stage pretest_ins_T1000 with the direct-path files")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "simsig.txt"))
    a = ap.parse_args()
    seed, dev = roomsim.STAGE_SEEDS["train"], torch.device("cuda:0")
    rs = np.random.RandomState()
    t0 = time.perf_counter()
    cfgs = [roomsim.random_spatial_acoustics(rs, seed, i) for i in range(a.items)]
    t_cfg = (time.perf_counter() - t0) / a.items
    lines = ["accept test and labels on the device (csrc/rirlabel.hip), stage train idx 0..%d, default ranges, n_len <= %d" %
             (a.items - 1, max(roomsim.plan_rir(c)["n_len"] for c in cfgs)), "",
             "--mode rir, a whole pass (render, accept test, read-back; no files), RIRs/s, median of %d interleaved passes" % a.reps,
             "batch   host labels   device labels   ratio"]
    ratio16 = None
    for bs in (1, 4, 16):
        rir_pass(roomsim, torch, dev, cfgs, seed, bs, "device")                        # warm-up (allocations, first launches)
        th, td = [], []
        for _ in range(a.reps):
            th.append(rir_pass(roomsim, torch, dev, cfgs, seed, bs, "host"))
            td.append(rir_pass(roomsim, torch, dev, cfgs, seed, bs, "device"))
        h, d = a.items / np.median(th), a.items / np.median(td)
        ratio16 = d / h
        lines.append("%5d   %11.1f   %13.1f   %5.1f" % (bs, h, d, d / h))
    # the kernel alone
    ids, pl, dp, rir, rdp = roomsim.render_items(cfgs, range(16), seed, 0, dev)
    nl = torch.tensor([p["n_len"] for p in pl], dtype=torch.int32, device=dev)
    dl = torch.tensor([p["n_len"] for p in dp], dtype=torch.int32, device=dev)
    ts = torch.tensor([c["T60_specify"] for c in cfgs[:16]], dtype=torch.float64, device=dev)
    for _ in range(3):
        hip.rir_labels(rir, nl, rdp, dl, ts)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(20):
        hip.rir_labels(rir, nl, rdp, dl, ts)
    e1.record()
    torch.cuda.synchronize()
    t_k = e0.elapsed_time(e1) / 20
    t0 = time.perf_counter()
    h, hd = rir.cpu().numpy(), rdp.cpu().numpy()
    for b in range(16):
        roomsim.labels(h[b, :, :pl[b]["n_len"]], hd[b], cfgs[b])
    t_h = (time.perf_counter() - t0) * 1e3
    lines += ["sarssl_rir_labels alone, batch 16 (32 rows): %.3f ms per call = %.1f us per RIR; roomsim.labels on the host, one thread: %.1f ms "
              "for the same 16 = %.2f ms per RIR" % (t_k, t_k / 16 * 1e3, t_h, t_h / 16),
              "device labels against host labels at batch 16: %.1fx the RIRs/s of a pass" % ratio16, ""]

    # parity.RIRLABELS
    worst = {}
    for nch in (1, 2, 3):
        for case in sc.label_cases(nch):
            d = sc.same_labels(sc.device_labels([case])[0], sc.host_labels(case[1], case[2], case[3]), dict(t60=1, corr=1, drr=1, c50=1))
            for k, v in d.items():
                worst[k] = max(worst.get(k, 0.0), v)
    lines += ["parity.RIRLABELS, largest |device - host| over the cases of tests/simsig_cases.py at 1 / 2 / 3 channels: t60 %.1e s, corr %.1e, "
              "DRR %.1e dB, C50 %.1e dB" % (worst["t60"], worst["corr"], worst["drr"], worst["c50"]), ""]

    # --mode sig
    with tempfile.TemporaryDirectory() as tmp:
        stage, kw, mix = ("pretest_ins_T1000", dict(save_dp=True), "sarssl_rir_mix_dp") if a.save_dp else ("pretrain", {}, "sarssl_rir_mix")
        src = speech_tree(os.path.join(tmp, "src"), sub=roomsim.SIG_SRC_SUBDIR[roomsim.sig_stage(stage)])
        n = a.sig_items
        roomsim.simulate_signals(os.path.join(tmp, "warm"), stage, 16, src, device="cuda:0", batch=16, log=lambda s: None, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = roomsim.simulate_signals(os.path.join(tmp, "a"), stage, n, src, device="cuda:0", batch=16, log=lambda s: None, **kw)
        t_all = time.perf_counter() - t0
        walls = {}
        for mod, name in ((roomsim, "random_spatial_acoustics"), (roomsim, "plan_sig"), (rirsynth, "mixing_table"), (roomsim, "judge_on_device"),
                          (dataset, "write_wav_batch"), (np, "savez")):
            walls[name] = Wall(getattr(mod, name))
            setattr(mod, name, walls[name])
        hip.profile_start(all_calls=True)
        t0 = time.perf_counter()
        roomsim.simulate_signals(os.path.join(tmp, "b"), stage, n, src, device="cuda:0", batch=16, log=lambda s: None, **kw)
        t_prof = time.perf_counter() - t0
        prof = hip.profile_stop()
        for mod, name in ((roomsim, "random_spatial_acoustics"), (roomsim, "plan_sig"), (rirsynth, "mixing_table"), (roomsim, "judge_on_device"),
                          (dataset, "write_wav_batch"), (np, "savez")):
            setattr(mod, name, walls[name].fn)
        nw = len(res["written"])
        pin = torch.empty((16, 65792, 2), dtype=torch.int16, pin_memory=True)
        g = torch.zeros((16, 65792, 2), dtype=torch.int16, device=dev)
        pin.copy_(g)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            pin.copy_(g, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        t_copy = e0.elapsed_time(e1) / 10 / 16

        def gpu(name):
            return prof.get("call:" + name, (0, 0.0))[1] / n

        stages = [("RIR render (sarssl_ism_rir, RIR + direct path, all attempts)", gpu("sarssl_ism_rir")),
                  ("tail + white noise (sarssl_gauss_fill)", gpu("sarssl_gauss_fill")),
                  ("labels (sarssl_rir_labels)", gpu("sarssl_rir_labels")),
                  ("diffuse field (sarssl_diffuse_noise)", gpu("sarssl_diffuse_noise")),
                  ("mix (%s)" % mix, gpu(mix)),
                  ("pack (sarssl_pcm16_pack)", gpu("sarssl_pcm16_pack")),
                  ("copy to the pinned buffer (measured apart, 16 items per copy)", t_copy)]
        host = [("room draws (random_spatial_acoustics, before the first batch)", walls["random_spatial_acoustics"].t / n * 1e3),
                ("plan_sig (reads the utterances)", walls["plan_sig"].t / n * 1e3),
                ("mixing_table (128 Cholesky factors per item)", walls["mixing_table"].t / n * 1e3),
                ("wait for the labels (judge_on_device, includes the render it waits for)", walls["judge_on_device"].t / n * 1e3),
                ("file write, writer thread (write_wav_batch)", walls["write_wav_batch"].t / n * 1e3),
                ("info files, writer thread (np.savez)", walls["savez"].t / n * 1e3)]
        lines += ["--mode sig, stage %s%s idx 0..%d, batch 16, default ranges, T = 4.112 s (65 792 samples), device noise: %d written, %d skipped, "
                  "%d renders" % (stage, " with save_dp" if a.save_dp else "", n - 1, nw, len(res["skipped"]), sum(res["attempts"].values())),
                  "whole call: %.2f s = %.1f items/s (%.1f ms per item; the room draws alone, measured above: %.1f ms per item)"
                  % (t_all, nw / t_all, 1e3 * t_all / nw, 1e3 * t_cfg),
                  "profiled pass (%.2f s; every C-ABI call between two events), ms per item:" % t_prof]
        lines += ["  GPU   %-78s %8.3f" % s for s in stages]
        lines += ["  host  %-78s %8.3f" % s for s in host]
        gsum = sum(v for _, v in stages)
        hmain = sum(v for _, v in host[:3])
        bound = max(stages + host[:3] + host[4:], key=lambda s: s[1])
        lines += ["  GPU stages together %.3f ms per item, host stages of the main thread (draws, plan, table) %.3f ms per item" % (gsum, hmain),
                  "  the largest single stage, which bounds the generator: %s" % bound[0]]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
