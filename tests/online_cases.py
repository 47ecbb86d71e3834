"""Shared inputs of tests/test_online_cpu.py, tests/test_gpu_srcbank.py and tests/test_gpu_online.py: a synthetic speaker tree and the
host restatement of a source crop."""
import os

import numpy as np

FS = 16000
# <set>/<speaker>: utterance lengths.  spkA's utterances are all shorter than the 4352-sample segment of the small runs (a crop runs
# through several and wraps to the first), spkB has ONE utterance (it is repeated), spkC's are longer than a segment (a crop lies inside one)
SPEAKERS = (("s1", "spkA", (1500, 1200, 2001, 777)), ("s1", "spkB", None), ("s2", "spkC", (9000, 12000)))


def write_tree(root, single=100, sub="tr", scale=1):
    """The tree below ``root``/<sub>: -> (the directory SourceBank takes, {path: int16 samples}).  single: the length of spkB's utterance;
    scale: a factor on the other speakers' lengths (16 for segments of 4.112 s)."""
    from sar_ssl_amd.dataset import write_wav_pcm16
    rs = np.random.RandomState(77)
    top, utts = os.path.join(str(root), sub), {}
    for st, spk, lens in SPEAKERS:
        d = os.path.join(top, st, spk)
        os.makedirs(d, exist_ok=True)
        for k, n in enumerate([scale * n for n in lens] if lens else (single,)):
            x = rs.randint(-32768, 32768, size=n).astype(np.int16)
            x[:2] = (-32768, 32767)
            path = os.path.join(d, "u%02d.wav" % k)
            write_wav_pcm16(path, x[:, None], FS)
            utts[path] = x
    return top, utts


def host_crop(segments, start, ns):
    """The restatement of hip.src_gather: segments [int16 array], crop start over their concatenation -> (ns,) f32, SourceBank.draw's
    arithmetic (f64 samples / 32768, the crop's mean removed, one rounding to f32)."""
    sig = np.concatenate(segments).astype(np.float64) / 32768.0
    s = sig[start:start + ns].copy()
    assert s.shape[0] == ns
    s -= s.mean()
    return s.astype(np.float32)
