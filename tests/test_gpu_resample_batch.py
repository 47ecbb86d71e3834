"""GPU: a batch of crops resampled in one launch - sarssl_resample_poly_batch (hip.resample_poly_batch) item by item against
hip.resample_poly of that item alone (bit for bit: one tile body serves both launches) and against the f64 restatement
realrir.restate_resample (parity.RESAMPLE), the zeros behind an item's last output, the refusals and two runs.

B = 4 crops of lengths (191, 192, 193, 7) at 1 : 3 and (63, 64, 65, 130) at 2 : 3 - outputs on either side of the 64-output tile, an item
shorter than the filter's half length, more than one tile - in a slot of n_max rows that no item reaches.  Every output tensor is filled
with a sentinel (NaN for f32) before the call: an element the kernel leaves out fails the comparison."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import check

pytestmark = pytest.mark.gpu
GROUPS = {(1, 3): (191, 192, 193, 7), (2, 3): (63, 64, 65, 130)}
SLACK = 37                         # rows of the slot behind the longest item
SENTINEL = 777
_REF = {}                          # (up, down, nch, pcm) -> (x (B, n_max, nch), [f64 restatement per item]): computed once, left unchanged


def _gate():
    from sar_ssl_amd import parity
    return min(parity.RESAMPLE["gate"], parity.RESAMPLE["ceiling"], parity.RESAMPLE["cap"])


def _case(up, down, nch, pcm):
    from sar_ssl_amd import realrir
    key = (up, down, nch, pcm)
    if key not in _REF:
        lens = GROUPS[up, down]
        rs = np.random.RandomState(1000 * up + 100 * down + 2 * nch + pcm)
        shape = (len(lens), max(lens) + SLACK, nch)
        x = rs.randint(-32768, 32768, shape).astype(np.int16) if pcm else (0.3 * rs.standard_normal(shape)).astype(np.float32)
        want = [realrir.restate_resample(x[b, :n].astype(np.float64) / (32768.0 if pcm else 1.0), up, down) for b, n in enumerate(lens)]
        x.setflags(write=False)
        _REF[key] = (x, want)
    return _REF[key]


def _filled(shape, dtype):
    return torch.full(shape, float("nan") if dtype == torch.float32 else SENTINEL, dtype=dtype, device="cuda")


def _run(x, lens, up, down, out_dtype):
    from sar_ssl_amd import hip
    B, n_max, nch = x.shape
    out = _filled((B, -(-n_max * up // down), nch), out_dtype)
    got = hip.resample_poly_batch(torch.from_numpy(np.array(x)).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda"), up, down,
                                  out_dtype=out_dtype, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_the_lengths_are_the_edge_cases_they_are_meant_to_be():
    from sar_ssl_amd import hip
    T = hip.RESAMPLE_TILE
    outs = {r: [-(-n * r[0] // r[1]) for n in lens] for r, lens in GROUPS.items()}
    assert outs[1, 3] == [64, 64, 65, 3] and outs[2, 3] == [42, 43, 44, 87]
    assert T in outs[1, 3] and T + 1 in outs[1, 3] and any(o > T for o in outs[2, 3]) and any(o < T for o in outs[2, 3])
    assert 7 * 1 < 10 * 3                                      # an item shorter than the filter's half length (in input rows: half / up)
    for (up, down), lens in GROUPS.items():                    # the slot's last tile lies wholly behind every item at 1 : 3
        assert -(-(max(lens) + SLACK) * up // down) > max(outs[up, down])
    assert -(-(193 + SLACK) // 3) > T + 1 and (-(-(193 + SLACK) // 3) - 1) // T == 1


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.int16], ids=["to_f32", "to_pcm16"])
@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("nch", [2, 15])
@pytest.mark.parametrize("up,down", list(GROUPS))
def test_every_item_is_bit_equal_to_the_single_launch_and_zero_behind(up, down, nch, pcm, out_dtype):
    from sar_ssl_amd import hip
    from sar_ssl_amd.roomsim import pcm16
    lens = GROUPS[up, down]
    x, want = _case(up, down, nch, pcm)
    got = _run(x, lens, up, down, out_dtype)
    worst = 0.0
    for b, n in enumerate(lens):
        n_out = -(-n * up // down)
        alone = hip.resample_poly(torch.from_numpy(np.array(x[b, :n])).cuda(), up, down, out_dtype=out_dtype).cpu().numpy()
        assert alone.shape == (n_out, nch)
        assert np.array_equal(_bits(got[b, :n_out]), _bits(alone)), (b, n)
        behind = got[b, n_out:]
        assert behind.size > 0 and np.array_equal(_bits(behind), _bits(np.zeros_like(behind))), (b, n)      # exactly +0.0, no NaN left
        if out_dtype == torch.float32:
            peak = np.abs(want[b]).max()
            worst = max(worst, float(np.abs(got[b, :n_out].astype(np.float64) - want[b]).max() / peak))
        else:
            assert np.abs(got[b, :n_out].astype(np.int32) - pcm16(want[b])).max() <= 1
    if out_dtype == torch.float32:
        check("resample_batch/%d_%d/nch%d/%s" % (up, down, nch, "pcm16" if pcm else "f32"), worst, _gate())
    assert np.array_equal(_bits(got), _bits(_run(x, lens, up, down, out_dtype)))                              # a second run of the same launch


def test_lengths_outside_the_slot_are_clamped_and_an_empty_item_is_all_zero():
    """n_in lives on the device; nothing on the host has seen it.  A value above n_max reads n_max rows, a value <= 0 none."""
    from sar_ssl_amd import hip
    x, _ = _case(1, 3, 2, False)
    n_max = x.shape[1]
    got = _run(x, (n_max + 1000, 0, -5, 192), 1, 3, torch.float32)
    whole = hip.resample_poly(torch.from_numpy(np.array(x[0])).cuda(), 1, 3).cpu().numpy()
    assert np.array_equal(_bits(got[0]), _bits(whole))
    assert np.array_equal(_bits(got[1:3]), _bits(np.zeros_like(got[1:3])))
    alone = hip.resample_poly(torch.from_numpy(np.array(x[3, :192])).cuda(), 1, 3).cpu().numpy()
    assert np.array_equal(_bits(got[3, :64]), _bits(alone)) and not got[3, 64:].any()


def test_refusals_raise_and_leave_out_untouched():
    from sar_ssl_amd import _lib, hip
    from sar_ssl_amd._lib import SarsslHipError
    dev = "cuda"
    x = torch.zeros((4, 100, 2), dtype=torch.float32, device=dev)
    n = torch.full((4,), 100, dtype=torch.int32, device=dev)
    out = _filled((4, 34, 2), torch.float32)
    for bad in (lambda: hip.resample_poly_batch(torch.zeros((4, 100, 33), dtype=torch.float32, device=dev), n, 1, 3),       # nch > 32
                lambda: hip.resample_poly_batch(x, n, 443, 1, out=out), lambda: hip.resample_poly_batch(x, n, 1, 443, out=out),
                lambda: hip.resample_poly_batch(torch.zeros((4, 0, 2), dtype=torch.float32, device=dev), n, 1, 3),
                lambda: hip.resample_poly_batch(x, n, 1, 3, out=torch.zeros((4, 33, 2), dtype=torch.float32, device=dev)),
                lambda: hip.resample_poly_batch(x, n[:3].contiguous(), 1, 3, out=out), lambda: hip.resample_poly_batch(x, n.long(), 1, 3, out=out),
                lambda: hip.resample_poly_batch(x.double(), n, 1, 3, out=out), lambda: hip.resample_poly_batch(x[0], n, 1, 3, out=out),
                lambda: hip.resample_poly_batch(x.cpu(), n.cpu(), 1, 3)):
        with pytest.raises(SarsslHipError):
            bad()
    assert hip.resample_poly_batch_supported(65535, 32, 16000, 44100) and not hip.resample_poly_batch_supported(65536, 2, 1, 3)
    assert not hip.resample_poly_batch_supported(0, 2, 1, 3) and not hip.resample_poly_batch_supported(4, 33, 1, 3)

    # the entry point itself: every refusal returns before the launch
    taps = torch.from_numpy(hip.resample_taps(1, 3).astype(np.float32)).to(dev)
    c_int, c_long, p = ctypes.c_int, ctypes.c_long, lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nb=4, nch=2, up=1, down=3, ntaps=61, n_max=100, n_out=34, idt=hip.F32, odt=hip.F32):
        _lib.call("sarssl_resample_poly_batch", p(x), c_int(idt), p(n), c_int(nb), c_long(n_max), c_int(nch), c_int(up), c_int(down),
                  p(taps), c_int(ntaps), c_long(n_out), p(out), c_int(odt), stream)

    for bad in (dict(nb=0), dict(nb=65536), dict(nch=33), dict(nch=0), dict(up=2, down=6, ntaps=121), dict(up=442, down=1, ntaps=8841),
                dict(ntaps=60), dict(n_out=33), dict(n_max=0, n_out=0), dict(idt=hip.BF16), dict(odt=hip.F16)):
        with pytest.raises(SarsslHipError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    call()                                                                                       # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
