"""Downstream (fine-tuning) step, launch by launch against captured: the TDOA configuration `opt_downstream` sets up (batch 8 for training,
16 for evaluation, T = 64 frames, --use-amp = hybrid), 'finetune' and 'lineareval', through the learner's own train_epoch / test_epoch
with SARSSL_GRAPH=0 and =1 on ONE learner (same weights, same optimizer semantics), the two forms interleaved round by round in one
process.  Times are host wall clock per epoch of --steps batches (an epoch ends in a device synchronise), divided by the steps; the
batches already sit on the GPU, so a step is the step and not the loader.  Prints one JSON line.

    python tools/bench_downstream.py [--steps 40] [--rounds 5] [--task TDOA --frames 64 --batch-train 8 --batch-eval 16]

--task / --frames / --batch-train / --batch-eval time another shape of the same step, e.g. the real-data branch's
(``--task T60 --frames 256 --batch-train 16``: 4.112 s items, batch 16 - what tools/bench_rirmix.py compares the render against)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sarssl_boot  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", default="hybrid")
    ap.add_argument("--task", default="TDOA", choices=["TDOA", "T60", "DRR", "C50", "ABS"])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch-train", type=int, default=8)
    ap.add_argument("--batch-eval", type=int, default=16)
    a = ap.parse_args()
    from sar_ssl_amd import learner, model, runtime, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_downstream.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda:0")
    T, B_train, B_eval = a.frames, a.batch_train, a.batch_eval
    nsample = 512 + 256 * (T - 1)
    rng = np.random.default_rng(0)
    res = {"tool": "bench_downstream", "task": a.task, "T": T, "batch_train": B_train, "batch_eval": B_eval, "precision": a.precision,
           "steps_per_epoch": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for mode in ("finetune", "lineareval"):
        torch.manual_seed(0)
        net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=False, device=dev, downstream_token="all", downstream_head="mlp",
                           downstream_embed="spat", downstream_dlabel=1)
        if mode == "lineareval":
            for k, v in net.named_parameters():
                if k.startswith(("spec_encoder.", "spat_encoder.")):
                    v.requires_grad = False
        lrn = learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=16000, task=a.task, ch_mode="M")
        lrn.cuda()
        lrn.amp(a.precision)

        def loader(B):
            sig = torch.from_numpy(synth.make_batch(1, B, nsample=nsample)).to(dev)
            tdoa = torch.from_numpy(rng.uniform(-5e-4, 5e-4, B).astype(np.float32)).to(dev)
            return [(sig, {a.task: tdoa if a.task == "TDOA" else tdoa * 1000 + 0.5})] * a.steps
        train, evalb = loader(B_train), loader(B_eval)

        def epoch(kind, graph):
            os.environ["SARSSL_GRAPH"] = "1" if graph else "0"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "train":
                lrn.train_epoch(train, lr=1e-5, epoch=1, return_metric=True)
            else:
                lrn.test_epoch(evalb, return_metric=True)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3
        times = {(k, g): [] for k in ("train", "eval") for g in (False, True)}
        for r in range(a.rounds + 1):                       # round 0 warms up (kernel loading, the two captures) and is dropped
            for kind in ("train", "eval"):
                for graph in (False, True):
                    t = epoch(kind, graph)
                    if r:
                        times[(kind, graph)].append(t)
        out = {}
        for kind in ("train", "eval"):
            e, c = times[(kind, False)], times[(kind, True)]
            out[kind + "_step_ms"] = {"eager": round(statistics.median(e), 3), "captured": round(statistics.median(c), 3),
                                      "eager_min_max": [round(min(e), 3), round(max(e), 3)],
                                      "captured_min_max": [round(min(c), 3), round(max(c), 3)],
                                      "eager_over_captured": round(statistics.median(e) / statistics.median(c), 2)}
        res[mode] = out
        runtime.set_precision("bf16")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
