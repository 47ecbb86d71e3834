"""GPU: hip.src_gather (csrc/srcbank.hip) against the host restatement of a source crop (online_cases.host_crop: SourceBank.draw's f64
arithmetic, rounded to f32 once) - bit for bit - and its refusals."""
import numpy as np
import pytest
import torch

import online_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def corpus():
    """Utterances of odd lengths at odd offsets of one flat int16 array, extreme values included -> (host array, device tensor, {name: (off, len)})."""
    rs = np.random.RandomState(3)
    lens = dict(a=5001, b=1777, c=333, one=413, long=12001)
    flat = rs.randint(-32768, 32768, size=sum(lens.values()) + 7).astype(np.int16)
    utt, pos = {}, 3
    for k, n in lens.items():
        utt[k] = (pos, n)
        pos += n
    flat[utt["a"][0]:utt["a"][0] + 4] = (-32768, 32767, -32768, 32767)
    flat[utt["c"][0]:utt["c"][0] + 333] = 32767                 # a constant stretch: the largest sums
    return flat, torch.from_numpy(flat).to(DEV), utt


def _item(utt, names, start):
    return [utt[n] for n in names], start


def _tables(items):
    B = len(items)
    off, ln = np.zeros((B, 32), np.int64), np.zeros((B, 32), np.int32)
    for b, (segs, _) in enumerate(items):
        off[b, :len(segs)], ln[b, :len(segs)] = [s[0] for s in segs], [s[1] for s in segs]
    return off, ln, np.array([len(s) for s, _ in items], np.int32), np.array([st for _, st in items], np.int64)


def _want(flat, item, ns):
    segs, start = item
    return oc.host_crop([flat[o:o + n] for o, n in segs], start, ns)


def _cases(utt, ns):
    """name -> (segments, crop start) for a crop of ns samples."""
    total = lambda names: sum(utt[n][1] for n in names)         # noqa: E731
    wrap = ["a", "b", "c", "a"] if ns > 1000 else ["c", "a"]     # 4352 from sample 4001: the end of a, b, c and back into a
    reps = ["one"] * max(3, -(-ns // utt["one"][1]) + 1)
    return {
        "inside": _item(utt, ["long"], 2501),
        "inside_start0": _item(utt, ["long"], 0),
        "inside_last": _item(utt, ["long"], utt["long"][1] - ns),
        "wraps": _item(utt, wrap, 4001 if ns > 1000 else 300),
        "wraps_last": _item(utt, wrap, total(wrap) - ns),
        "one_utterance_repeated": _item(utt, reps, 7),
        "one_utterance_repeated_last": _item(utt, reps, total(reps) - ns),
        "starts_behind_the_first": _item(utt, ["c", "long"], 333 + 11),
    }


@pytest.mark.parametrize("ns", [64, 1000, 4352])
def test_src_gather_is_bit_equal_to_the_host_crop(corpus, ns):
    from sar_ssl_amd import hip
    flat, bank, utt = corpus
    cases = _cases(utt, ns)
    assert len(cases["one_utterance_repeated"][0]) >= 3 and cases["wraps"][1] % 2 == (1 if ns > 1000 else 0)
    for name, item in cases.items():                            # each alone
        got = hip.src_gather(bank, *_tables([item]), ns).cpu().numpy()
        want = _want(flat, item, ns)
        assert got.dtype == np.float32 and got.shape == (1, ns) and got[0].tobytes() == want.tobytes(), (name, ns)
    # a ragged batch of 5 (1 to 12 segments), the first item again at position 4
    batch = [cases["wraps"], cases["inside"], cases["one_utterance_repeated"], cases["inside_last"], cases["wraps"]]
    got = hip.src_gather(bank, *_tables(batch), ns).cpu().numpy()
    for b, item in enumerate(batch):
        assert got[b].tobytes() == _want(flat, item, ns).tobytes(), (b, ns)
    assert got[0].tobytes() == got[4].tobytes()
    assert abs(float(got.astype(np.float64).mean(axis=1).max())) < 1e-7


def test_src_gather_takes_32_segments_and_an_odd_crop_start(corpus):
    from sar_ssl_amd import hip
    flat, bank, utt = corpus
    item = _item(utt, ["c"] * 32, 333 * 32 - 4353 - 2)           # an odd start; the crop ends two samples before the last segment does
    assert item[1] % 2 == 1
    got = hip.src_gather(bank, *_tables([item]), 4352).cpu().numpy()
    assert got[0].tobytes() == _want(flat, item, 4352).tobytes() and not got.any()      # a constant signal minus its mean


def test_src_gather_refuses_and_leaves_out_untouched(corpus):
    from sar_ssl_amd import _lib, hip
    flat, bank, utt = corpus
    good = _item(utt, ["a", "b"], 100)
    off, ln, nseg, start = _tables([good, good])

    def refused(off=off, ln=ln, nseg=nseg, start=start, ns=64, what=""):
        out = torch.full((2, max(ns, 0)), 7.0, device=DEV)
        with pytest.raises(_lib.SarsslHipError, match=what):
            hip.src_gather(bank, off, ln, nseg, start, ns, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())

    refused(nseg=np.array([2, 0], np.int32), what="nseg 1..32")
    refused(nseg=np.array([33, 2], np.int32), what="nseg 1..32")
    past = off.copy()
    past[1, 1] = flat.shape[0] - ln[1, 1] + 1
    refused(off=past, what="inside the bank")
    neg = off.copy()
    neg[0, 0] = -1
    refused(off=neg, what="inside the bank")
    empty = ln.copy()
    empty[0, 1] = 0
    refused(ln=empty, what="inside the bank")
    refused(ns=0, what="Ns 1")
    refused(ns=5001 + 1777 - 100 + 1, what="cover the crop")
    refused(start=np.array([100, -1], np.int64), what="crop start")
    out = torch.full((2, 64), 7.0, device=DEV)
    hip.src_gather(bank, off, ln, nseg, start, 64, out=out)      # and the same tables are taken
    assert out[0].cpu().numpy().tobytes() == _want(flat, good, 64).tobytes()
