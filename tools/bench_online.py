"""Online simulated pretraining (onlinesig.OnlineSignalLoader, run_pretrain.py --simu-online) -> profiles/online.txt

    python tools/bench_online.py [--items 2048] [--steps 64] [--reps 3] [--out profiles/online.txt]
    python tools/bench_online.py --disk-only --corpus DIR [--steps 64] [--reps 3]        # the disk loader alone (runs on a parent commit too)

1. The loader alone at B = 64, T = 4.112 s, default ranges, device noise, on tools/bench_simsig.py's speech tree: items/s of a whole
   epoch of --items items (worker thread, queue, events; the consumer only waits for each batch) for reuse 1 and 4, passes interleaved,
   median of --reps; and in a profiled pass of one chunk per reuse (render_chunk on the calling thread) the time per item of every
   stage - the GPU stages between events (hip.profile_start(all_calls=True)), the host stages by wall clock.
2. The training step (learner.STFTLearner.pretrain_epoch, --use-amp's hybrid mode, B = 64, --steps steps an epoch) fed by the online
   loader against dataset.PcmSegmentLoader over a corpus on disk (1024 rendered segments, listed --steps / 16 times), epochs interleaved,
   median of --reps: ms per step by the host clock around an epoch that ends in a device synchronise.
--disk-only prints the disk loader's figure of part 2 over an existing corpus: the same lines run on the parent commit.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sarssl_boot  # noqa: E402,F401

B, T, FS = 64, 4.112, 16000
NS = int(T * FS)


def learner_for(device):
    from sar_ssl_amd import learner as at_learner, model
    nt = int((T * FS - 256) / 256)
    net = model.SARSSL(sig_shape=(256, nt, 2, 2), pretrain=True, device=device)
    lrn = at_learner.STFTLearner(net, win_len=512, win_shift_ratio=0.5, nfft=512, fre_used_ratio=1, fs=FS, task=None, ch_mode="M")
    lrn.cuda()
    lrn.amp()
    return lrn


def epoch_ms(torch, lrn, dl, epoch):
    if hasattr(dl, "set_epoch"):
        dl.set_epoch(epoch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lrn.pretrain_epoch(dl, lr=1e-4, epoch=epoch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(dl)


def disk_loader(corpus, steps, device):
    from sar_ssl_amd import dataset
    files = dataset.segment_files(corpus)
    files = (files * (steps * B // len(files) + 1))[:steps * B]
    return dataset.PcmSegmentLoader(files, B, NS, 2, fs=FS, shuffle=True, seed=1, device=device, nthreads=8)


def disk_only(a):
    import torch
    dev = torch.device("cuda:0")
    lrn, dl = learner_for(dev), disk_loader(a.corpus, a.steps, dev)
    epoch_ms(torch, lrn, dl, 0)                                  # warm-up: capture, first launches, page cache
    ms = [epoch_ms(torch, lrn, dl, e) for e in range(1, a.reps + 1)]
    print("DISK_ONLY step ms, %d steps an epoch, B = %d: %s  median %.2f" % (a.steps, B, "  ".join("%.2f" % m for m in ms), np.median(ms)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--disk-only", action="store_true")
    ap.add_argument("--corpus", type=str, default="")
    ap.add_argument("--keep-corpus", type=str, default="", help="write part 2's disk corpus here and keep it (for --disk-only on another commit)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "online.txt"))
    a = ap.parse_args()
    if a.disk_only:
        return disk_only(a)
    import torch
    from bench_simsig import Wall, speech_tree
    from sar_ssl_amd import dataset, hip, onlinesig, rirsynth, roomsim
    dev = torch.device("cuda:0")
    quiet = lambda s: None                                       # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        src = speech_tree(os.path.join(tmp, "src"), nspk=8, nutt=6)
        t0 = time.perf_counter()
        bank = rirsynth.DeviceSourceBank(os.path.join(src, "tr"), FS, dev, sort=True)
        t_bank = time.perf_counter() - t0
        lines = ["online simulated pretraining (onlinesig.OnlineSignalLoader): B = %d, T = %.3f s (%d samples), default ranges, device noise, "
                 "chunk %d, render batch 128" % (B, T, NS, onlinesig.CHUNK),
                 "source bank: %d utterances of %d speakers, %.1f MB on the device, read in %.2f s" %
                 (len(bank.paths), len(bank), bank.flat.numel() * 2 / 1e6, t_bank), ""]

        def mk(reuse, n=a.items):
            return onlinesig.OnlineSignalLoader(bank, n, B, T, 1, dev, reuse=reuse, log=quiet)

        def loader_pass(ld, epoch):
            ld.set_epoch(epoch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for (pcm,) in ld:
                n += pcm.shape[0]
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        # ---- 1. the loader alone
        lds = {k: mk(k) for k in (1, 4)}
        for k in lds:
            loader_pass(mk(k, 2 * B), 0)                         # warm-up: allocations, first launches
        rate = {k: [] for k in lds}
        for rep in range(a.reps):
            for k in lds:
                rate[k].append(loader_pass(lds[k], rep))
        lines += ["1. the loader alone, an epoch of %d items, items/s, %d interleaved passes:" % (a.items, a.reps)]
        lines += ["  reuse %d   %s   median %.0f" % (k, "  ".join("%7.0f" % r for r in rate[k]), np.median(rate[k])) for k in lds]
        for k in lds:
            ld = mk(k, onlinesig.CHUNK)
            G = [g for s in range(len(ld)) for g in ld.indices(7, s)]
            walls = {}
            for obj, name in ((ld, "room_cfg"), (ld, "item_plan"), (rirsynth.DeviceSourceBank, "tables"), (roomsim, "plan_rir"), (roomsim, "judge_on_device")):
                walls[name] = Wall(getattr(obj, name))
                setattr(obj, name, walls[name])
            hip.profile_start(all_calls=True)
            t0 = time.perf_counter()
            with torch.cuda.stream(ld.side):
                ld.render_chunk(G)
            torch.cuda.synchronize()
            t_prof = time.perf_counter() - t0
            prof = hip.profile_stop()
            rirsynth.DeviceSourceBank.tables = staticmethod(walls["tables"].fn)
            roomsim.plan_rir, roomsim.judge_on_device = walls["plan_rir"].fn, walls["judge_on_device"].fn
            n = len(G)

            def gpu(name):
                return prof.get("call:" + name, (0, 0.0))[1] / n
            stages = [("RIR render (sarssl_ism_rir, RIR + direct path, all attempts)", gpu("sarssl_ism_rir")),
                      ("tail + white noise (sarssl_gauss_fill)", gpu("sarssl_gauss_fill")),
                      ("labels (sarssl_rir_labels)", gpu("sarssl_rir_labels")),
                      ("source crops (sarssl_src_gather, with its table upload)", gpu("sarssl_src_gather")),
                      ("mixing table (sarssl_mixing_table)", gpu("sarssl_mixing_table")),
                      ("diffuse field (sarssl_diffuse_noise)", gpu("sarssl_diffuse_noise")),
                      ("mix (sarssl_rir_mix)", gpu("sarssl_rir_mix")),
                      ("pack (sarssl_pcm16_pack)", gpu("sarssl_pcm16_pack"))]
            host = [("room draws (room_cfg: random_spatial_acoustics, closed-form Sabine solve)", walls["room_cfg"].t / n * 1e3),
                    ("render plans (plan_rir, RIR + direct path)", walls["plan_rir"].t / n * 1e3),
                    ("signal plans (item_plan: speaker, DeviceSourceBank.plan, SNR)", walls["item_plan"].t / n * 1e3),
                    ("segment tables (DeviceSourceBank.tables)", walls["tables"].t / n * 1e3),
                    ("wait for the labels (judge_on_device, includes the render it waits for)", walls["judge_on_device"].t / n * 1e3)]
            lines += ["  profiled chunk, reuse %d: %d items, %d rooms, %d renders, %.3f s = %.3f ms per item on one thread; ms per item:"
                      % (k, n, len(set(g // k for g in G)), sum(ld.attempts.values()), t_prof, t_prof / n * 1e3)]
            lines += ["    GPU   %-78s %8.3f" % s for s in stages]
            lines += ["    host  %-78s %8.3f" % s for s in host]
            lines += ["    GPU stages together %.3f ms per item; host stages without the wait %.3f ms per item"
                      % (sum(v for _, v in stages), sum(v for _, v in host[:4]))]
        lines.append("")

        # ---- 2. the training step, online against disk
        corpus = a.keep_corpus or os.path.join(tmp, "corpus")
        os.makedirs(corpus, exist_ok=True)
        ld = mk(1, 1024)
        k = 0
        for (pcm,) in ld:
            dataset.write_wav_batch([os.path.join(corpus, "%d.wav" % (k + j)) for j in range(pcm.shape[0])], pcm.cpu(), FS)
            k += pcm.shape[0]
        lrn = learner_for(dev)
        feeds = {"disk": disk_loader(corpus, a.steps, dev), "online reuse 1": mk(1, a.steps * B), "online reuse 4": mk(4, a.steps * B)}
        for name, dl in feeds.items():
            epoch_ms(torch, lrn, dl, 0)                          # warm-up: capture, first launches, page cache
        ms = {name: [] for name in feeds}
        for rep in range(1, a.reps + 1):
            for name, dl in feeds.items():
                ms[name].append(epoch_ms(torch, lrn, dl, rep))
        lines += ["2. the training step (pretrain_epoch, hybrid mode, B = %d, %d steps an epoch), ms per step, %d interleaved epochs:" % (B, a.steps, a.reps)]
        lines += ["  %-16s %s   median %.2f  (%.0f segments/s)" % (name, "  ".join("%6.2f" % m for m in v), np.median(v), B / np.median(v) * 1e3)
                  for name, v in ms.items()]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
