"""The polyphase resampler on the shape it was built for: one 32-channel 48 kHz recording of 10 s and one of 120 s, resampled to
16 kHz - in one process on one box, medians with [min, max]:

  launch        device time of ONE sarssl_resample_poly launch over the whole resident file (device events, warm, median of 20), f32 in
                and PCM-16 out (the noise step's call) and f32 in and out (the RIR step's), with the bytes the algorithm has to move
                (input + output + taps) over that time as a fraction of the HBM peak (8.0 TB/s)
  noise step    realrir.noise_cuts of that recording as a PCM-24 file, host clock: read_wav, chunked upload / resample / download
                (DeviceResampler), column picks and the batch WAV writer for the 32-capsule array's pairs - all pairs for the 10 s file,
                the first 16 for the 120 s file (411 cuts of 7.7 MB are a disk benchmark); the resample stage is also timed on its own
  scipy         scipy.signal.resample_poly on this host's CPU in f64 in the same run: once per file (all 32 channels), and the reference's
                way, once per selected pair on the pair's two columns - measured on 3 pairs and multiplied by the number of pairs

No ratio is promised.  Prints one JSON line; --out also writes the text summary.

    python tools/bench_resample.py [--seconds 10 120] [--out profiles/resample.txt]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import sarssl_boot  # noqa: E402,F401
import numpy as np  # noqa: E402
import torch  # noqa: E402

FS_IN, FS, NCH = 48000, 16000, 32
HBM_PEAK = 8.0e12


def med(v):
    return {"median": round(statistics.median(v), 3), "min_max": [round(min(v), 3), round(max(v), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, nargs="+", default=[10, 120])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scipy.signal
    import realrir_cases as cases
    from sar_ssl_amd import hip, realrir
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU; there is nothing to time without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    pairs = realrir.selected_pairs("EM32")
    res = {"tool": "bench_resample", "nch": NCH, "fs_in": FS_IN, "fs": FS, "pairs": len(pairs), "device": torch.cuda.get_device_name(0), "files": {}}
    rs = np.random.RandomState(0)
    for sec in a.seconds:
        n_in = sec * FS_IN
        n_out = -(-n_in // 3)
        x = np.clip(0.2 * rs.standard_normal((n_in, NCH)), -0.99, 0.99).astype(np.float32)
        r = {"n_in": n_in, "n_out": n_out}
        # ---- one launch over the resident file
        xd = torch.from_numpy(x).to(dev)
        for name, odt, osz in (("f32_to_pcm16", torch.int16, 2), ("f32_to_f32", torch.float32, 4)):
            out = torch.empty((n_out, NCH), dtype=odt, device=dev)
            for _ in range(3):
                hip.resample_poly(xd, FS, FS_IN, out_dtype=odt, out=out)
            ms = []
            for _ in range(20):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.resample_poly(xd, FS, FS_IN, out_dtype=odt, out=out)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            nbytes = n_in * NCH * 4 + n_out * NCH * osz + 61 * 4
            r["launch_ms_" + name] = med(ms)
            r["hbm_fraction_" + name] = round(nbytes / (statistics.median(ms) * 1e-3) / HBM_PEAK, 4)
            r["bytes_" + name] = nbytes
            del out
        del xd
        torch.cuda.empty_cache()
        # ---- the noise step of that recording, from a PCM-24 file
        with tempfile.TemporaryDirectory() as root:
            path = os.path.join(root, "EM32_Room_1_Noise_Ambient.wav")
            cases.write_wav(path, x, FS_IN, "pcm24")
            part = pairs if sec <= 10 else pairs[:16]
            stem = os.path.join(root, "_MP1-%d-%d_Ambient.wav")
            rsm = realrir.DeviceResampler(dev)
            realrir.noise_cuts(path, "EM32", pairs[:1], stem, rsm, FS)                    # warm-up: code objects, the tap upload
            t0 = time.perf_counter()
            written = realrir.noise_cuts(path, "EM32", part, stem, rsm, FS)
            r["noise_step_s"] = round(time.perf_counter() - t0, 3)
            r["noise_step_pairs_written"] = len(written)
            from sar_ssl_amd.dataset import read_wav
            t0 = time.perf_counter()
            xf, _ = read_wav(path)
            r["read_wav_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            rsm.pcm16(xf, FS, FS_IN)
            torch.cuda.synchronize()
            r["resample_stage_s"] = round(time.perf_counter() - t0, 3)                      # f32 conversion, upload, launches, download
        # ---- scipy on this host, f64
        t0 = time.perf_counter()
        scipy.signal.resample_poly(xf, FS, FS_IN, axis=0)
        r["scipy_once_per_file_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        for idx in pairs[:3]:
            scipy.signal.resample_poly(xf[:, idx], FS, FS_IN)
        per_pair = (time.perf_counter() - t0) / 3
        r["scipy_per_pair_s"] = round(per_pair, 4)
        r["scipy_reference_way_s_extrapolated"] = round(per_pair * len(pairs), 2)
        del xf, x
        res["files"]["%ds" % sec] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(summary(res))


def summary(res):
    lines = ["tools/bench_resample.py on %s (one box, one process; launch times: device events, warm, median of 20 [min, max])" % res["device"],
             "shape: %d channels, %d Hz -> %d Hz (ratio 1 : 3, 61 taps); the 32-capsule array has %d pairs inside 0.03 .. 0.20 m" % (res["nch"], res["fs_in"], res["fs"], res["pairs"]), ""]
    for name, r in res["files"].items():
        lines += ["%s file: %d rows in, %d rows out" % (name, r["n_in"], r["n_out"])]
        for k, label in (("f32_to_pcm16", "f32 -> PCM-16"), ("f32_to_f32", "f32 -> f32   ")):
            m = r["launch_ms_" + k]
            lines.append("  one launch, %s: %9.3f ms  %s   %.1f MB moved, %.1f %% of the HBM peak (8.0 TB/s)"
                         % (label, m["median"], m["min_max"], r["bytes_" + k] / 1e6, 100 * r["hbm_fraction_" + k]))
        lines += ["  realrir.noise_cuts from a PCM-24 file, %d pairs written (host clock):      %8.3f s" % (r["noise_step_pairs_written"], r["noise_step_s"]),
                  "    of which read_wav alone:                                              %8.3f s" % r["read_wav_s"],
                  "    of which f32 conversion + chunked upload / resample / download alone: %8.3f s" % r["resample_stage_s"],
                  "  scipy.signal.resample_poly, f64, host CPU, once per file (32 channels):   %8.3f s" % r["scipy_once_per_file_s"],
                  "  scipy the reference's way: %.4f s per pair (mean of 3) x %d pairs =        %8.2f s (extrapolated)"
                  % (r["scipy_per_pair_s"], res["pairs"], r["scipy_reference_way_s_extrapolated"]), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
