"""Fixture F24 of the signal generator's direct-path files (gen_simu.py --mode sig --save_dp True), from the REAL reference (build
container only):

    python tools/make_golden_simsig_dp.py        ->  tests/golden/f24_simsig_dp.npz

F22's run (tools/make_golden_simsig.py ``run_reference``: the same three items, canned RIRs, speech tree and stand-ins) with the reference's
own ``generate_microphone_signal(..., save_dp=True)``.  The draws are the same, so the array written as ``{k}.wav`` must equal F22's
``item/k/out`` exactly; the tool asserts it and leaves f22_simsig.npz alone.  The file holds per item the float array handed to
``soundfile.write`` for ``{k}_dp.wav`` as f32 (``item/k/out_dp``) and the written file names - data only, nothing of the reference's source.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden_simsig as f22  # noqa: E402


def main():
    _, written = f22.run_reference(save_dp=True)
    fx = np.load(os.path.join(f22.GOLD, "f22_simsig.npz"))
    store = {"files": np.array(sorted(written)), "consts": np.array([f22.FS, f22.NS, f22.NMIC, f22.SEED, f22.ITEMS])}
    assert sorted(written) == sorted(["%d%s.wav" % (k, s) for k in range(f22.ITEMS) for s in ("", "_dp")]), sorted(written)
    for k in range(f22.ITEMS):
        sig, fs = written["%d.wav" % k]
        assert fs == f22.FS and np.array_equal(np.asarray(sig, np.float32), fx["item/%d/out" % k]), k        # the same draws as F22
        dp, fs = written["%d_dp.wav" % k]
        assert fs == f22.FS and dp.shape == (f22.NS, f22.NMIC)
        store["item/%d/out_dp" % k] = np.asarray(dp, np.float32)
        print("item %d: peak |mic| %.4f, peak |dp| %.4f" % (k, np.abs(sig).max(), np.abs(dp).max()))
    out = os.path.join(f22.GOLD, "f24_simsig_dp.npz")
    np.savez_compressed(out, **store)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
