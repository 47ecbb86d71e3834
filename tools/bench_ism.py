"""Throughput of the simulated-RIR generator at its default ranges -> profiles/ism.txt

    python tools/bench_ism.py [--items 32] [--batches 1,4,16] [--out profiles/ism.txt]

Per batch size: RIRs/s of the render alone (roomsim.render_items: both plans, device noise, hip.ism_rir for the RIR and the direct path,
event-timed), of render + read-back, and of render + read-back + labels (roomsim.labels on the host).  Beside it the f64 numpy restatement (roomsim.restate_cfg) on the same host in the same run: gpuRIR
cannot be run, so the restatement is the baseline.  Also the distances of parity.ISM, measured against the restatement.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sarssl_boot  # noqa: E402,F401


def main():
    import torch
    from sar_ssl_amd import roomsim
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--batches", type=str, default="1,4,16")
    ap.add_argument("--restated", type=int, default=8, help="items the numpy restatement is timed on")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ism.txt"))
    a = ap.parse_args()
    seed, dev = roomsim.STAGE_SEEDS["train"], torch.device("cuda:0")
    rs = np.random.RandomState()
    cfgs = [roomsim.random_spatial_acoustics(rs, seed, i) for i in range(a.items)]
    plans = [roomsim.plan_rir(c) for c in cfgs]
    nimg = [int(np.prod(p["nb_img"])) for p in plans]
    lines = ["image-source RIR generator, stage train idx 0..%d, default ranges: %d .. %d images per RIR (mean %.0f), n_ism <= %d, n_len <= %d"
             % (a.items - 1, min(nimg), max(nimg), np.mean(nimg), max(p["n_ism"] for p in plans), max(p["n_len"] for p in plans)), ""]

    t0 = time.perf_counter()
    want = [roomsim.restate_cfg(c, roomsim.numpy_noise(seed, i, 0, 2, plans[i]["n_len"])) for i, c in enumerate(cfgs[:a.restated])]
    t_ref = (time.perf_counter() - t0) / a.restated
    got = roomsim.render(plans[:a.restated], dev, roomsim.host_noise(plans[:a.restated], range(a.restated), seed, 0, dev)).cpu().numpy()
    dist = max(np.abs(got[i, :, :plans[i]["n_len"]] - w).max() / np.abs(w).max() for i, w in enumerate(want))
    lines += ["f64 numpy restatement on this host: %.1f ms per RIR = %.1f RIRs/s" % (1e3 * t_ref, 1.0 / t_ref),
              "largest distance kernel - restatement over these %d RIRs, relative to the peak: %.3e" % (a.restated, dist), "",
              "batch   kernel ms/RIR   kernel RIRs/s   +read-back RIRs/s   +labels RIRs/s"]
    for bs in [int(x) for x in a.batches.split(",")]:
        tk = tr = tl = 0.0
        for rep in range(2):                                  # the first pass warms up (allocations, first launches) and is dropped
            tk = tr = tl = 0.0
            for i0 in range(0, a.items, bs):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ids, pl, _, rir, rdp = roomsim.render_items(cfgs, range(i0, min(i0 + bs, a.items)), seed, 0, dev)
                e1.record()
                h, hd = rir.cpu().numpy(), rdp.cpu().numpy()
                w1 = time.perf_counter()
                for b, i in enumerate(ids):
                    roomsim.labels(h[b, :, :pl[b]["n_len"]], hd[b], cfgs[i])
                w2 = time.perf_counter()
                tk += e0.elapsed_time(e1) * 1e-3
                tr += w1 - w0
                tl += w2 - w0
        lines.append("%5d   %13.3f   %13.1f   %17.1f   %14.1f" % (bs, 1e3 * tk / a.items, a.items / tk, a.items / tr, a.items / tl))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
