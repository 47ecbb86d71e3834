"""Throughput of the per-room generator and of its mixing-table kernel -> profiles/certainroom.txt

    python tools/bench_certainroom.py [--rooms 2] [--rirs 50] [--sigs 2] [--reps 3] [--out profiles/certainroom.txt]

One box, one run, the compared passes interleaved:
1. the mixing table: rirsynth.mixing_table on the host, ms per item, against hip.mixing_table (csrc/rirmix.hip: sarssl_mixing_table)
   per batch of 16, event-timed; and the distance of parity.MIXTABLE over the geometries of tests/certainroom_cases.py;
2. items/s of roomsim.simulate_room_signals at the reference's defaults (--rooms x --rirs x --sigs, T = 4.112 s, default ranges, device
   noise) against roomsim.simulate_signals - the parent's generator, one room draw per item - on as many items, on a synthetic speech tree;
3. in a profiled pass of simulate_room_signals the time per item of every stage (the GPU stages between events, the host stages by wall
   clock), in the style of profiles/simsig.txt.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sarssl_boot  # noqa: E402,F401
from bench_simsig import Wall, speech_tree  # noqa: E402


def main():
    import torch
    import certainroom_cases as cc
    from sar_ssl_amd import dataset, hip, rirsynth, roomsim
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=2)
    ap.add_argument("--rirs", type=int, default=50)
    ap.add_argument("--sigs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "certainroom.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    seed = roomsim.STAGE_SEEDS["train"]
    n = a.rooms * a.rirs * a.sigs
    quiet = lambda s: None                                      # noqa: E731

    # 1. the table
    placed = roomsim.room_placements(seed, 1, 16, roomsim.MIC_ARRAY_CFG_2CH, roomsim.DEFAULTS)[0]
    mic = np.ascontiguousarray(np.stack([c["mic_pos"] for c in placed]), np.float64)
    mic_dev = torch.from_numpy(mic).to(dev)
    out = hip.mixing_table(mic_dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t_host, t_dev = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        for m in mic:
            rirsynth.mixing_table(m).astype(np.float32)
        t_host.append((time.perf_counter() - t0) / 16 * 1e3)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            hip.mixing_table(mic_dev, out=out)
        e1.record()
        torch.cuda.synchronize()
        t_dev.append(e0.elapsed_time(e1) / 20)
    worst = {}
    for name, m in cc.table_batches():
        got = hip.mixing_table(torch.from_numpy(m).to(dev)).cpu().numpy().astype(np.float64)
        worst[name] = float(np.abs(got - cc.host_tables(m)).max())
    th, td = float(np.median(t_host)), float(np.median(t_dev))
    lines = ["the mixing table of the diffuse field (129 bins x M x M per item), 16 two-microphone arrays of stage train, median of %d interleaved passes" % a.reps,
             "  rirsynth.mixing_table on the host, one thread: %.3f ms per item" % th,
             "  hip.mixing_table (sarssl_mixing_table), one launch per batch of 16: %.4f ms per batch = %.2f us per item" % (td, td / 16 * 1e3),
             "parity.MIXTABLE, max |device - host| of the f32 tables over the geometries of tests/certainroom_cases.py:",
             "  " + ", ".join("%s %.1e" % kv for kv in worst.items()),
             "  largest: %.1e (cap 2^-22 = %.1e)" % (max(worst.values()), 2.0 ** -22), ""]

    # 2. and 3. the generators
    with tempfile.TemporaryDirectory() as tmp:
        src = speech_tree(os.path.join(tmp, "src"))

        def rooms(name):
            t0 = time.perf_counter()
            res = roomsim.simulate_room_signals(os.path.join(tmp, name), "train", a.rooms, a.rirs, a.sigs, src, device="cuda:0", batch=16, log=quiet)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res

        def flat(name):
            t0 = time.perf_counter()
            res = roomsim.simulate_signals(os.path.join(tmp, name), "pretrain", n, src, device="cuda:0", batch=16, log=quiet)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res

        roomsim.simulate_room_signals(os.path.join(tmp, "warm_r"), "train", 1, 8, 2, src, device="cuda:0", batch=16, log=quiet)
        roomsim.simulate_signals(os.path.join(tmp, "warm_f"), "pretrain", 16, src, device="cuda:0", batch=16, log=quiet)
        tr, tf = [], []
        for rep in range(a.reps):
            t, res_r = rooms("r%d" % rep)
            tr.append(t)
            t, res_f = flat("f%d" % rep)
            tf.append(t)
        wr, wf = len(res_r["written"]), len(res_f["written"])
        mr, mf = float(np.median(tr)), float(np.median(tf))
        lines += ["%d items, batch 16, default ranges, T = 4.112 s (65 792 samples), device noise, median of %d interleaved calls:" % (n, a.reps),
                  "  simulate_room_signals, stage train, %d rooms x %d placements x %d signals: %d written, %d skipped, %d renders; %.2f s = %.1f items/s "
                  "(%.2f ms per item)" % (a.rooms, a.rirs, a.sigs, wr, len(res_r["skipped"]), sum(res_r["attempts"].values()), mr, wr / mr, 1e3 * mr / wr),
                  "  simulate_signals (gen_simu.py --mode sig, one room draw per item), stage pretrain: %d written, %d skipped, %d renders; %.2f s = "
                  "%.1f items/s (%.2f ms per item)" % (wf, len(res_f["skipped"]), sum(res_f["attempts"].values()), mf, wf / mf, 1e3 * mf / wf)]
        watched = ((roomsim, "room_placements"), (roomsim, "plan_sig"), (rirsynth, "mixing_table"), (roomsim, "judge_on_device"),
                   (dataset, "write_wav_batch"), (np, "savez"))
        walls = {}
        for mod, name in watched:
            walls[name] = Wall(getattr(mod, name))
            setattr(mod, name, walls[name])
        hip.profile_start(all_calls=True)
        t_prof, res_p = rooms("p")
        prof = hip.profile_stop()
        for mod, name in watched:
            setattr(mod, name, walls[name].fn)

        def gpu(name):
            return prof.get("call:" + name, (0, 0.0))[1] / n

        stages = [("RIR render (sarssl_ism_rir, RIR + direct path, all attempts)", gpu("sarssl_ism_rir")),
                  ("tail + white noise (sarssl_gauss_fill)", gpu("sarssl_gauss_fill")),
                  ("labels (sarssl_rir_labels)", gpu("sarssl_rir_labels")),
                  ("mixing table (sarssl_mixing_table)", gpu("sarssl_mixing_table")),
                  ("diffuse field (sarssl_diffuse_noise)", gpu("sarssl_diffuse_noise")),
                  ("mix (sarssl_rir_mix)", gpu("sarssl_rir_mix")),
                  ("pack (sarssl_pcm16_pack)", gpu("sarssl_pcm16_pack"))]
        host = [("room and placement draws (room_placements, before the first batch)", walls["room_placements"].t / n * 1e3),
                ("plan_sig (reads the utterances)", walls["plan_sig"].t / n * 1e3),
                ("mixing_table on the host (not called: %d calls)" % walls["mixing_table"].n, walls["mixing_table"].t / n * 1e3),
                ("wait for the labels (judge_on_device, includes the render it waits for)", walls["judge_on_device"].t / n * 1e3),
                ("file write, writer thread (write_wav_batch)", walls["write_wav_batch"].t / n * 1e3),
                ("info files, writer thread (np.savez, all_info.npz included)", walls["savez"].t / n * 1e3)]
        lines += ["profiled pass of simulate_room_signals (%.2f s; every C-ABI call between two events), ms per item:" % t_prof]
        lines += ["  GPU   %-78s %8.3f" % s for s in stages]
        lines += ["  host  %-78s %8.3f" % s for s in host]
        bound = max(stages + host[:3] + host[4:], key=lambda s: s[1])
        lines += ["  GPU stages together %.3f ms per item, host stages of the main thread (draws, plan) %.3f ms per item"
                  % (sum(v for _, v in stages), sum(v for _, v in host[:3])),
                  "  the largest single stage: %s" % bound[0]]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
