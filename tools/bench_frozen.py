"""Training step of the frozen-encoder probe stage (`--pretrain-frozen-encoder`) next to the launch-by-launch pretraining step
(SARSSL_GRAPH=0), B = 64, T = 256, through the learner's own pretrain_epoch: one learner per (stage, numeric mode), the stages interleaved
round by round in one process.  Times are host wall clock per epoch of --steps batches (an epoch ends in a device synchronise), divided by
the steps; the batches already sit on the GPU, so a step is the step and not the loader.  Prints one JSON line; --out also writes the table.

    python tools/bench_frozen.py [--steps 20] [--rounds 5] [--out profiles/frozen_step.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sarssl_boot  # noqa: E402,F401
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precisions", default="hybrid,fp16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sar_ssl_amd import learner, model, runtime, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_frozen.py measures on the GPU; there is nothing to time without one")
    os.environ["SARSSL_GRAPH"] = "0"                       # both stages launch by launch (the frozen stage has no captured form)
    dev = torch.device("cuda:0")
    T, B = 256, a.batch
    sig = torch.from_numpy(synth.make_batch(1, B)).to(dev)
    batches = [[sig]] * a.steps
    res = {"tool": "bench_frozen", "T": T, "batch": B, "steps_per_epoch": a.steps, "rounds": a.rounds, "SARSSL_GRAPH": "0",
           "device": torch.cuda.get_device_name(0), "step_ms": {}}
    for prec in a.precisions.split(","):
        lrns = {}
        for stage in ("pretrain", "frozen"):
            torch.manual_seed(0)
            net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=stage == "pretrain", pretrain_frozen_encoder=stage == "frozen", device=dev)
            if stage == "frozen":
                for k, v in net.named_parameters():
                    if "encoder" in k:
                        v.requires_grad = False
            lrns[stage] = learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=None, ch_mode="M")
            lrns[stage].cuda()
        times = {s: [] for s in lrns}
        for r in range(a.rounds + 1):                       # round 0 warms up (kernel loading, workspaces) and is dropped
            for stage, lrn in lrns.items():
                lrn.amp(prec)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lrn.pretrain_epoch(batches, lr=1e-4, epoch=1)
                torch.cuda.synchronize()
                if r:
                    times[stage].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {s: statistics.median(t) for s, t in times.items()}
        res["step_ms"][prec] = {"pretrain_launch_by_launch": round(med["pretrain"], 3), "frozen": round(med["frozen"], 3),
                                "pretrain_min_max": [round(min(times["pretrain"]), 3), round(max(times["pretrain"]), 3)],
                                "frozen_min_max": [round(min(times["frozen"]), 3), round(max(times["frozen"]), 3)],
                                "frozen_over_pretrain": round(med["frozen"] / med["pretrain"], 3)}
        del lrns
        torch.cuda.empty_cache()
    runtime.set_precision("bf16")
    line = json.dumps(res)
    print(line)
    if a.out:
        rows = ["python tools/bench_frozen.py        (one %s; B = %d, T = 256; SARSSL_GRAPH=0: both stages launch by launch through" % (res["device"], B),
                "pretrain_epoch, one learner per stage, the stages interleaved round by round; median of %d rounds of %d-step epochs, host wall" % (a.rounds, a.steps),
                "clock per step ending in a device synchronise, the batch resident on the GPU; [min, max] over the rounds)", "",
                "mode      pretraining step [min, max]        frozen-encoder step [min, max]      frozen / pretraining"]
        for prec, v in res["step_ms"].items():
            rows.append("%-8s  %7.3f ms [%.3f, %.3f]       %7.3f ms [%.3f, %.3f]        %.3f" % (
                prec, v["pretrain_launch_by_launch"], *v["pretrain_min_max"], v["frozen"], *v["frozen_min_max"], v["frozen_over_pretrain"]))
        rows += ["", "the line the tool printed:", line, ""]
        with open(a.out, "w") as f:
            f.write("\n".join(rows))


if __name__ == "__main__":
    main()
