"""The LOCATA TDOA corpus generator on the shapes it was built for -> profiles/locatads.txt

    python tools/bench_locatads.py [--items 512] [--batch 16] [--out profiles/locatads.txt]

Over the synthetic LOCATA tree of tests/locatads_cases.py (48 kHz recordings of 3 - 12 s, 12 / 15 / 32 channels), stage train:

1. generator    items/s of locatads.generate as a whole - plan, read, upload, resample, normalise, pack, label, write - at --batch; second
                pass of two (the first warms the file cache and the annotation tables).
2. restatement  items/s of locatads.TdoaCorpus.restate_item, the f64 numpy statement of the same items, on this host (one thread; what
                the reference does per item in a DataLoader worker, with restate_resample in the place of scipy's resample_poly).
3. producer     seconds per item of the producer thread's two parts, measured on the host alone over the same plans: reading the crop
                with ALL the recording's channels (TdoaCorpus.read) against the rest of host_batch (tables, pinned buffers) - whether the
                all-channel read bounds the generator, as it does the pretraining loader.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import sarssl_boot  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "locatads.txt"))
    a = ap.parse_args()
    import torch
    import locatads_cases as cases
    from sar_ssl_amd import locatads
    lines = []
    with tempfile.TemporaryDirectory() as root:
        tree = cases.build_tree(os.path.join(root, "locata"))
        corpus = locatads.TdoaCorpus(tree, "train", sort=True)
        rate = {}
        for rep in ("first", "second"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plans, _ = locatads.generate(tree, os.path.join(root, "out"), "train", data_num=a.items, batch=a.batch, sort=True, overwrite=True,
                                         corpus=corpus)
            rate[rep] = a.items / (time.perf_counter() - t0)
        lines.append("generator     %d items at batch %d: %.0f items/s (first pass %.0f)" % (a.items, a.batch, rate["second"], rate["first"]))
        n = min(a.items, 64)
        t0 = time.perf_counter()
        for p in plans[:n]:
            corpus.restate_item(p)
        host = n / (time.perf_counter() - t0)
        lines.append("restatement   %d items in f64 numpy on one host thread: %.1f items/s (generator / restatement = %.0fx)" % (n, host, rate["second"] / host))
        loader = locatads._TdoaLoader(corpus, a.items, a.batch, "cuda")
        t_read = t_all = 0.0
        nb = 0
        for k in range(0, n, a.batch):
            batch = plans[k:k + a.batch]
            t0 = time.perf_counter()
            for p in batch:
                corpus.read(p)
            t1 = time.perf_counter()
            loader.host_batch(batch)
            t2 = time.perf_counter()
            t_read, t_all, nb = t_read + (t1 - t0), t_all + (t2 - t1), nb + len(batch)
        nch = {}
        for p in plans:
            c = corpus.header(p["path"])[0]
            nch[c] = nch.get(c, 0) + 1
        lines.append("producer      crop read (all channels, one thread) %.2f ms/item; host_batch as a whole (reads on 4 threads, tables, pinned "
                     "buffers) %.2f ms/item = %.0f items/s; channels of the drawn recordings: %s"
                     % (1e3 * t_read / nb, 1e3 * t_all / nb, nb / t_all, ", ".join("%d x %d ch" % (v, k) for k, v in sorted(nch.items()))))
        lines.append("              -> the producer thread %s the generator (%.0f items/s against %.0f)"
                     % ("bounds" if nb / t_all < 1.25 * rate["second"] else "does not bound", nb / t_all, rate["second"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# tools/bench_locatads.py --items %d --batch %d (synthetic LOCATA tree, one MI355X)\n" % (a.items, a.batch) + text)


if __name__ == "__main__":
    main()
