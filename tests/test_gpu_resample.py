"""GPU: the polyphase resampler - sarssl_resample_poly (hip.resample_poly) against the f64 restatement realrir.restate_resample on the
input as the kernel reads it (parity.RESAMPLE, a fraction of the case's peak), its PCM-16 output against roomsim.pcm16 of the
restatement, bit reproducibility across channel counts, chunkings and runs, and the refusals.

Every output tensor is filled with a sentinel before the call: an element the kernel leaves out fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import check

pytestmark = pytest.mark.gpu
RATIOS = [(1, 3), (2, 3), (160, 441), (2, 1)]
NCHS = (1, 2, 3, 8, 32)
_REF = {}                        # (up, down, n, nch, dtype) -> (input, f64 restatement): computed once, shared, left unchanged


def _gate():
    from sar_ssl_amd import parity
    return min(parity.RESAMPLE["gate"], parity.RESAMPLE["ceiling"], parity.RESAMPLE["cap"])


def _lengths(up, down):
    """1, 7 (shorter than one filter span), 1000, 1001 and the shortest inputs with at least T - 1, T, T + 1 outputs."""
    from sar_ssl_amd import hip
    T = hip.RESAMPLE_TILE
    return sorted({1, 7, 1000, 1001} | {(k - 1) * down // up + 1 for k in (T - 1, T, T + 1)})


def _case(up, down, n, nch, pcm):
    from sar_ssl_amd import realrir
    key = (up, down, n, nch, pcm)
    if key not in _REF:
        rs = np.random.RandomState(hash(key) % (1 << 31))
        x = rs.randint(-32768, 32768, (n, nch)).astype(np.int16) if pcm else (0.3 * rs.standard_normal((n, nch))).astype(np.float32)
        x64 = x.astype(np.float64) / 32768.0 if pcm else x.astype(np.float64)
        y = realrir.restate_resample(x64, up, down)
        x.setflags(write=False); y.setflags(write=False)
        _REF[key] = (x, y)
    return _REF[key]


def _run(x, up, down, out_dtype=torch.float32, **kw):
    from sar_ssl_amd import hip
    up_r, down_r = hip.resample_ratio(up, down)
    n_in = kw.get("n_in", x.shape[0])
    n_out = -(-n_in * up_r // down_r)
    rows = kw.get("m1", n_out) - kw.get("m0", 0)
    out = torch.full((rows, x.shape[1]), 777, dtype=out_dtype, device="cuda")
    got = hip.resample_poly(torch.from_numpy(np.array(x)).cuda(), up, down, out_dtype=out_dtype, out=out, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _distance(got, want):
    peak = np.abs(want).max()
    d = np.abs(got.astype(np.float64) - want).max()
    return (d / peak if peak > 0 else d), peak


def test_lengths_straddle_the_tile():
    from sar_ssl_amd import hip
    T = hip.RESAMPLE_TILE
    n_out = lambda n, up, down: -(-n * up // down)
    for up, down in RATIOS:
        for k in (T - 1, T, T + 1):                    # the shortest input with at least k outputs (2 : 1 has even counts only)
            n = (k - 1) * down // up + 1
            assert n in _lengths(up, down) and n_out(n, up, down) >= k > n_out(n - 1, up, down)
        outs = [n_out(n, up, down) for n in _lengths(up, down)]
        assert any(o <= T for o in outs if o >= T - 2) and any(T < o <= T + 2 for o in outs)


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_value_parity(up, down, pcm):
    import scipy.signal
    worst, worst_scipy = 0.0, 0.0
    for nch in NCHS:
        for n in _lengths(up, down):
            x, want = _case(up, down, n, nch, pcm)
            got = _run(x, up, down)
            assert got.shape == want.shape and got.dtype == np.float32
            d, _ = _distance(got, want)
            worst = max(worst, d)
            x32 = (x.astype(np.float32) / np.float32(32768.0)) if pcm else x
            worst_scipy = max(worst_scipy, _distance(scipy.signal.resample_poly(x32, up, down, axis=0), want)[0])
    print("RESAMPLE %d/%d %s: kernel %.3e of peak, scipy float32 path %.3e of peak" % (up, down, "pcm16" if pcm else "f32", worst, worst_scipy))
    check("resample/%d_%d/%s" % (up, down, "pcm16" if pcm else "f32"), worst, _gate())


@pytest.mark.parametrize("up,down", RATIOS)
def test_zero_padding_at_both_ends_and_special_inputs(up, down):
    from sar_ssl_amd import realrir
    n, nch = 300, 3
    zero = np.zeros((n, nch), np.float32)
    assert not _run(zero, up, down).any()
    for row in (0, n - 1):
        x = zero.copy()
        x[row] = (1.0, -0.5, 0.25)
        want = realrir.restate_resample(x.astype(np.float64), up, down)
        check("resample/impulse_row%d/%d_%d" % (row, up, down), _distance(_run(x, up, down), want)[0], _gate())
    for v in (32767, -32768):
        x = np.full((n, nch), v, np.int16)
        want = realrir.restate_resample(x.astype(np.float64) / 32768.0, up, down)
        check("resample/full_scale%d/%d_%d" % (v, up, down), _distance(_run(x, up, down), want)[0], _gate())


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_pcm16_output(up, down, pcm):
    from sar_ssl_amd.roomsim import pcm16
    for nch, n in ((2, 1001), (32, 1000), (3, 7)):
        x, y64 = _case(up, down, n, nch, pcm)
        got = _run(x, up, down, out_dtype=torch.int16)
        want = pcm16(y64)
        assert got.dtype == np.int16 and got.shape == want.shape
        assert np.abs(got.astype(np.int32) - want).max() <= 1
        v = 32767.0 * y64
        clear = np.abs(v - np.floor(v) - 0.5) > 32767.0 * _gate() * np.abs(y64).max()          # farther from a half-integer than the gate
        assert clear.mean() > 0.5 and np.array_equal(got[clear], want[clear])


@pytest.mark.parametrize("up,down", RATIOS)
def test_full_scale_pcm_saturates(up, down):
    from sar_ssl_amd import realrir
    from sar_ssl_amd.roomsim import pcm16
    x = np.concatenate([np.full((200, 2), 32767, np.int16), np.full((200, 2), -32768, np.int16)])
    y64 = realrir.restate_resample(x.astype(np.float64) / 32768.0, up, down)
    assert y64.max() > 1.0 and y64.min() < -1.0                                                # the step overshoots
    got = _run(x, up, down, out_dtype=torch.int16)
    assert got.max() == 32767 and got.min() == -32767
    assert np.abs(got.astype(np.int32) - pcm16(y64)).max() <= 1


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_bit_reproducibility(up, down, pcm):
    from sar_ssl_amd import hip, realrir
    x, _ = _case(up, down, 1001, 32, pcm)
    for out_dtype in (torch.float32, torch.int16):
        full = _run(x, up, down, out_dtype=out_dtype)
        assert np.array_equal(_bits(full), _bits(_run(x, up, down, out_dtype=out_dtype)))            # two runs
        for c in (0, 13, 31):                                                                                        # a column alone
            assert np.array_equal(_bits(full[:, c:c + 1]), _bits(_run(x[:, c:c + 1], up, down, out_dtype=out_dtype))), c
        up_r, down_r = hip.resample_ratio(up, down)
        n_out = full.shape[0]
        off = lambda m: m + 1 if down_r > 1 and m % down_r == 0 else m                                                # (2 : 1 has no such boundary)
        cuts = [0, off(n_out // 3), off(2 * n_out // 3), n_out]                                                       # three chunks with halos
        assert down_r == 1 or all(m % down_r for m in cuts[1:-1])
        parts = []
        for m0, m1 in zip(cuts[:-1], cuts[1:]):
            lo, hi = realrir._chunk_rows(m0, m1, x.shape[0], up_r, down_r)
            assert hi - lo < x.shape[0]
            parts.append(_run(x[lo:hi], up, down, out_dtype=out_dtype, n_in=x.shape[0], row0=lo, m0=m0, m1=m1))
        assert np.array_equal(_bits(np.concatenate(parts)), _bits(full))


def test_refusals_launch_nothing():
    from sar_ssl_amd import _lib, hip
    from sar_ssl_amd._lib import SarsslHipError
    dev = "cuda"
    x = torch.zeros((100, 2), dtype=torch.float32, device=dev)
    with pytest.raises(SarsslHipError):
        hip.resample_poly(torch.zeros((100, 33), dtype=torch.float32, device=dev), 1, 3)          # nch > 32
    with pytest.raises(SarsslHipError):
        hip.resample_poly(x, 443, 1)                                                             # up out of range
    with pytest.raises(SarsslHipError):
        hip.resample_poly(x, 1, 443)
    with pytest.raises(SarsslHipError):
        hip.resample_poly(torch.zeros((0, 2), dtype=torch.float32, device=dev), 1, 3)             # empty input
    with pytest.raises(SarsslHipError):
        hip.resample_poly(x, 1, 3, out=torch.zeros((33, 2), dtype=torch.float32, device=dev))     # n_out is 34
    with pytest.raises(SarsslHipError):
        hip.resample_poly(x.double(), 1, 3)
    with pytest.raises(SarsslHipError):
        hip.resample_poly(x.cpu(), 1, 3)
    assert hip.resample_poly_supported(32, 16000, 48000) and hip.resample_poly_supported(2, 16000, 44100)
    assert not hip.resample_poly_supported(33, 1, 3) and not hip.resample_poly_supported(2, 1, 443)

    # the entry point itself: every refusal returns before the launch and leaves the output as it was
    taps = torch.from_numpy(hip.resample_taps(1, 3).astype(np.float32)).to(dev)
    out = torch.full((34, 2), 777.0, dtype=torch.float32, device=dev)
    c_int, c_long, p = ctypes.c_int, ctypes.c_long, lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nch=2, up=1, down=3, ntaps=61, row0=0, nrows=100, n_in=100, n_out=34, m0=0, m1=34, idt=hip.F32, odt=hip.F32):
        _lib.call("sarssl_resample_poly", p(x), c_int(idt), c_long(row0), c_long(nrows), c_long(n_in), c_int(nch), c_int(up), c_int(down),
                  p(taps), c_int(ntaps), c_long(n_out), c_long(m0), c_long(m1), p(out), c_int(odt), stream)

    for bad in (dict(nch=33), dict(nch=0), dict(up=2, down=6, ntaps=121), dict(up=442, down=1, ntaps=8841), dict(ntaps=60), dict(n_out=33),
                dict(n_in=0, nrows=0), dict(m0=5, m1=5), dict(m1=35), dict(row0=10, nrows=90), dict(nrows=50), dict(idt=hip.BF16),
                dict(odt=hip.F16)):
        with pytest.raises(SarsslHipError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())
    call()                                                                                       # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
