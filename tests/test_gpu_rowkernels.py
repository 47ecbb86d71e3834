"""The row / elementwise kernels (csrc/elementwise.hip, the row kernels of csrc/dwconv.hip, csrc/head.hip, the small relayout / affine
kernels) in every dtype pairing and launch shape the library dispatches, each against the f64 restatement of tests/rowkernel_refs.py
on the operands as stored.  Every f64 comparison goes through _chk -> conftest.check with the tolerance of sar_ssl_amd/parity.py ROWKERNELS:
min(gate = 4x measured, cap), cap = 2 ulp of the output dtype, or L * 2^-23 for an f32 output that is a sum of L addends (parity.py says
which outputs count as sums and why).  profiles/rowkernels.txt holds the measured figures."""
import pytest
import torch

import rowkernel_refs as refs
from conftest import check

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "fp16"}
STORE = [F32, BF16, F16]
# (name, gradient dtype, saved-activation dtype) -> the DISPATCH_GA instantiation <T, TA>
PAIRS = [("f32", F32, F32), ("bf16", BF16, BF16), ("mix16", BF16, F16), ("mixf32", BF16, F32)]
PAIRS_DW = PAIRS[:3]                                      # DW_DISPATCH_GA has no (bf16, f32) instantiation
_ids = lambda p: p[0] if isinstance(p, tuple) else NAME.get(p, str(p))


def _hip():
    from sar_ssl_amd import hip
    return hip


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _st(shape, dtype, g, scale=1.0, shift=0.0):
    """A CPU tensor as stored in `dtype`."""
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype)


def _d(t):
    return t.detach().double().cpu()


def _err(got, ref):
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def _tol(family, key, L=None):
    from sar_ssl_amd import parity
    return parity.rowkernel_tol(family, key, L)


def _chk(family, key, case, got, ref, L=None):
    check("rowk.%s.%s[%s]" % (family, key, case), _err(got, ref), _tol(family, key, L))


def _view(t, dev, lead, tail):
    """t [M, d] as a column window of a wider zero buffer on the device (row stride d + lead + tail) -> (view, buffer)."""
    M, d = t.shape
    buf = torch.zeros((M, lead + d + tail), dtype=t.dtype, device=dev)
    buf[:, lead:lead + d] = t.to(dev)
    return buf[:, lead:lead + d], buf


def _rest_is_zero(buf, lead, d):
    return float(buf[:, :lead].float().abs().sum()) == 0.0 and float(buf[:, lead + d:].float().abs().sum()) == 0.0


def _stored(dtype):
    return (lambda t: t) if dtype == F32 else (lambda t: t.to(dtype).double())


# ================================================================================================ a. LayerNorm
@pytest.mark.parametrize("d", [4, 252, 260, 768, 1024])
@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_layernorm_fwd(dtp, d):
    """layernorm_fwd_kernel<T> (one row per wave, 1 .. 4 float4 registers per lane; d = 252 / 260 end inside a register), T = f32, bf16 and
    fp16, strided input, strided output into a wider buffer."""
    hip, dev = _hip(), _dev()
    for M in (1, 5, 70):
        g = _gen(1000 * d + M)
        x = _st((M, d), dtp, g, 1.5, 0.3)
        gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
        xs, _ = _view(x, dev, 8, 4)
        wide = torch.zeros((M, d + 12), dtype=dtp, device=dev)
        y, stats = hip.layernorm_fwd(xs, gamma.to(dev), beta.to(dev), 1e-5, out=wide[:, 4:4 + d])
        ref, mean, rstd = refs.layernorm_fwd(_d(x), _d(gamma), _d(beta), 1e-5)
        case = "M%d,d%d" % (M, d)
        _chk("ln_fwd", NAME[dtp], case, y, ref)
        assert _rest_is_zero(wide, 4, d)
        _chk("ln_fwd_stats", NAME[dtp], case + ",mean", stats[0], mean, L=d)
        _chk("ln_fwd_stats", NAME[dtp], case + ",rstd", stats[1], rstd, L=d)


def _ln_bwd_case(hip, dev, name, gt, at, M, d, seed):
    g = _gen(seed)
    x = _st((M, d), at, g, 1.5, 0.3)
    dy, res = _st((M, d), gt, g), _st((M, d), gt, g)
    gamma, beta = (torch.rand(d, generator=g) + 0.5).to(dev), torch.randn(d, generator=g).to(dev)
    xs, _ = _view(x, dev, 4, 8)                           # row strides d + 12, d + 16, d + 4, d + 8
    dys, _ = _view(dy, dev, 8, 8)
    ress, _ = _view(res, dev, 0, 4)
    outbuf = torch.zeros((M, d + 8), dtype=gt, device=dev)
    _, stats = hip.layernorm_fwd(xs, gamma, beta, 1e-5)
    dg0, db0 = torch.randn(d, generator=g), torch.randn(d, generator=g)
    dg, db = dg0.to(dev), db0.to(dev)
    out = hip.layernorm_bwd(dys, xs, gamma, stats, resid=ress, dgamma=dg, dbeta=db, out=outbuf[:, 4:4 + d])
    assert out.dtype == gt
    rdx, rdg, rdb = refs.layernorm_bwd(_d(dy), _d(x), _d(gamma), _d(stats[0]), _d(stats[1]), _d(res))
    case = "M%d,d%d" % (M, d)
    _chk("ln_bwd_dx", name, case, out, rdx)
    assert _rest_is_zero(outbuf, 4, d)
    _chk("ln_bwd_dparam", name, case + ",dgamma", dg, _d(dg0) + rdg, L=M + 1)
    _chk("ln_bwd_dparam", name, case + ",dbeta", db, _d(db0) + rdb, L=M + 1)


@pytest.mark.parametrize("d", [32, 256, 512, 768, 1024])
@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_layernorm_bwd(pair, d):
    """layernorm_bwd_kernel<T, TA, NV>: NV = 1 (d <= 256), 2 (d <= 512), 4 (d = 768, 1024), in the four DISPATCH_GA pairings (f32,
    bf16, MIX16 = bf16 gradient / fp16 x, MIXF32 = bf16 gradient / f32 x), row strides != d on dy, x, resid and the result, dgamma /
    dbeta accumulated onto non-zero values.  M = 1 and 7 leave waves of the only workgroup idle; at M = 70 and 4100 a wave goes through
    its two-rows-in-flight loop several times, M = 4100 = 4 * (129 workgroups * 4 waves * 2 rows) - 28 ends with second rows missing."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    for M in (1, 7, 70, 4100):
        _ln_bwd_case(hip, dev, name, gt, at, M, d, 7000 * d + M)


def test_layernorm_bwd_beyond_the_workgroup_cap():
    """M = 16400 rows: more than 512 workgroups x 4 waves x 8 rows, so the grid is capped at 512 workgroups and every wave sweeps its
    two-row loop more than four times; the last sweep has 16 rows (f32)."""
    _ln_bwd_case(_hip(), _dev(), "f32", F32, F32, 16400, 256, 99)


@pytest.mark.parametrize("M,d", [(7, 32), (70, 768)])
@pytest.mark.parametrize("pair", PAIRS[2:], ids=_ids)
def test_layernorm_bwd_drop_in_the_mixed_pairings(pair, M, d):
    """sarssl_layernorm_bwd with dx2 in MIX16 and MIXF32: the first output is the plain call's bit for bit, the second has the keep mask of
    act_bwd(first, None, 0, p, seed, gscale) and its values within one bf16 rounding (rounded once from the f32 gradient, not twice)."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    g = _gen(31 * M + d)
    x = _st((M, d), at, g, 1.5, 0.3).to(dev)
    dy, res = _st((M, d), gt, g).to(dev), _st((M, d), gt, g).to(dev)
    gamma, beta = (torch.rand(d, generator=g) + 0.5).to(dev), torch.zeros(d, device=dev)
    _, stats = hip.layernorm_fwd(x, gamma, beta, 1e-5)
    p, seed, gs = 0.25, 0x1234567887654321, 1.25
    out, out2 = hip.layernorm_bwd(dy, x, gamma, stats, resid=res, drop=(p, seed, gs))
    plain = hip.layernorm_bwd(dy, x, gamma, stats, resid=res)
    assert out.dtype == gt and out2.dtype == gt and torch.equal(out, plain)
    want = hip.act_bwd(plain, None, 0, p_drop=p, seed=seed, gscale=gs)
    assert torch.equal(out2 == 0, want == 0)
    if M * d >= 1000:
        assert 0.2 < float((out2 == 0).float().mean()) < 0.3
    # one bf16 rounding: a unit in the last place is at most 2^-7 of the value
    assert bool(((out2.double() - want.double()).abs() <= 2.0 ** -7 * want.double().abs()).all())


def test_layernorm_bwd_with_dropout_output_is_refused_past_1024_columns():
    """d > 1024 runs the one-workgroup-per-row kernel, which has no second output: hip.layernorm_bwd(..., drop=...) is refused on the host
    (nothing is launched, dx stays as it was), the plain call at the same shape goes through."""
    from sar_ssl_amd._lib import SarsslHipError
    hip, dev = _hip(), _dev()
    M, d = 4, 1536
    g = _gen(9)
    x, dy = torch.randn((M, d), generator=g).to(dev), torch.randn((M, d), generator=g).to(dev)
    gamma, beta = (torch.rand(d, generator=g) + 0.5).to(dev), torch.zeros(d, device=dev)
    _, stats = hip.layernorm_fwd(x, gamma, beta, 1e-5)
    out = torch.full((M, d), 7.0, device=dev)
    with pytest.raises(SarsslHipError, match="d <= 1024"):
        hip.layernorm_bwd(dy, x, gamma, stats, out=out, drop=(0.25, 3, 1.0))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    hip.layernorm_bwd(dy, x, gamma, stats, out=out)
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())


# ================================================================================================ b. convolution-module row kernels
GLU_SHAPES = [(1, 4), (195, 72), (37, 260)]
DW_T = (1, 15, 16, 31, 32, 33, 65)


def _dw_shapes(ds):
    """(B, T, d): every T with B = 3, T = 1 and 33 with B = 1 as well."""
    return [(3, T, d) for d in ds for T in DW_T] + [(1, T, d) for d in ds for T in (1, 33)]


DWCONV_SHAPES = _dw_shapes((4, 72, 256, 260))            # one partial 256-thread block, one full block, a second block of 4 live lanes
DWGLU_SHAPES = _dw_shapes((8, 72, 256, 264))
DW_WRAP = (9, 1825, 8)                                    # 522 tiles of 32 frames > 128 partial rows x 4 waves; 261 tiles of 64 > 64 parts


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_glu_fwd(dtp):
    """glu_fwd_kernel<T>, T = f32 / bf16 / fp16."""
    hip, dev = _hip(), _dev()
    for M, d in GLU_SHAPES:
        h = _st((M, 2 * d), dtp, _gen(M + d), 2.0)
        _chk("glu_fwd", NAME[dtp], "M%d,d%d" % (M, d), hip.glu_fwd(h.to(dev)), refs.glu_fwd(_d(h)))


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_glu_bwd(pair):
    """glu_bwd_kernel<T, TA> in the four DISPATCH_GA pairings."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    for M, d in GLU_SHAPES:
        g = _gen(3 * M + d)
        h, dg = _st((M, 2 * d), at, g, 2.0), _st((M, d), gt, g)
        dh = hip.glu_bwd(dg.to(dev), h.to(dev))
        assert dh.dtype == gt
        _chk("glu_bwd", name, "M%d,d%d" % (M, d), dh, refs.glu_bwd(_d(dg), _d(h)))


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_dwconv_fwd_and_flipped(dtp):
    """dwconv_fwd_kernel<T> with flip = 0 (forward) and flip = 1 (data gradient): T shorter than, equal to and longer than the 31 taps and
    the 32-frame tile, channel counts that leave the 256-thread block partly idle, fill it, and start a second one."""
    hip, dev = _hip(), _dev()
    for B, T, d in DWCONV_SHAPES + [DW_WRAP]:
        g = _gen(B * 10000 + T * 10 + d)
        x, w = _st((B, T, d), dtp, g), torch.randn((d, 31), generator=g) * 0.2
        case = "B%d,T%d,d%d" % (B, T, d)
        _chk("dwconv_fwd", NAME[dtp], case, hip.dwconv(x.to(dev), w.to(dev)), refs.dwconv_fwd(_d(x), _d(w)), L=31)
        _chk("dwconv_fwd", NAME[dtp], case + ",flip", hip.dwconv(x.to(dev), w.to(dev), flip=True), refs.dwconv_dgrad(_d(x), _d(w)), L=31)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_dwconv_wgrad(pair):
    """dwconv_wgrad_kernel<T, TA> in the four DISPATCH_GA pairings, += onto a non-zero gradient; (9, 1825, 8) has more 32-frame tiles than
    the 128 partial rows x 4 waves take in one pass."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    for B, T, d in DWCONV_SHAPES + [DW_WRAP]:
        g = _gen(B * 10000 + T * 10 + d + 1)
        x, dy = _st((B, T, d), at, g), _st((B, T, d), gt, g)
        dw0 = torch.randn((d, 31), generator=g)
        dw = dw0.to(dev)
        hip.dwconv_wgrad(dy.to(dev), x.to(dev), dw)
        _chk("dwconv_wgrad", name, "B%d,T%d,d%d" % (B, T, d), dw, _d(dw0) + refs.dwconv_wgrad(_d(dy), _d(x)), L=B * T + 1)


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_dwglu_fwd(dtp):
    """dwglu_fwd_kernel<T> (GLU + depthwise conv on 64-frame x 64-channel tiles), T = f32 / bf16 / fp16."""
    hip, dev = _hip(), _dev()
    for B, T, d in DWGLU_SHAPES + [DW_WRAP]:
        g = _gen(B * 10000 + T * 10 + d + 2)
        h, w = _st((B * T, 2 * d), dtp, g), torch.randn((d, 31), generator=g) * 0.2
        c = hip.dwglu_fwd(h.to(dev), w.to(dev), B, T)
        ref = refs.dwglu_fwd(_d(h).view(B, T, 2 * d), _d(w), _stored(dtp))
        _chk("dwglu_fwd", NAME[dtp], "B%d,T%d,d%d" % (B, T, d), c.view(B, T, d), ref, L=31)


@pytest.mark.parametrize("pair", PAIRS_DW, ids=_ids)
def test_dwglu_bwd_and_wgrad(pair):
    """dwglu_bwd_kernel / dwglu_wgrad_kernel<T, TA> in the three DW_DISPATCH_GA pairings.  The weight gradient starts non-zero, and is
    taken a second time inside hip.splitk_batched() - the model's path: dw == NULL, the partials folded by the batch's reduce launch -
    which must give the same bits as the call that folds its own partials (both add the partials in slice order; with more than three
    partials, T = 65 at B = 3 and the (9, 1825, 8) case, a fold in another order differs in the last bit)."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    for B, T, d in DWGLU_SHAPES + [DW_WRAP]:
        g = _gen(B * 10000 + T * 10 + d + 3)
        h, dc = _st((B * T, 2 * d), at, g), _st((B * T, d), gt, g)
        w = torch.randn((d, 31), generator=g) * 0.2
        hd, dcd = h.to(dev), dc.to(dev)
        case = "B%d,T%d,d%d" % (B, T, d)
        dh = hip.dwglu_bwd(dcd, hd, w.to(dev), B, T)
        assert dh.dtype == gt
        _chk("dwglu_bwd", name, case, dh.view(B, T, 2 * d), refs.dwglu_bwd(_d(dc).view(B, T, d), _d(h).view(B, T, 2 * d), _d(w)), L=31)
        dw0 = torch.randn((d, 31), generator=g)
        dw, dwb = dw0.to(dev), dw0.to(dev)
        hip.dwglu_wgrad(dcd, hd, dw, B, T)
        ref = _d(dw0) + refs.dwglu_wgrad(_d(dc).view(B, T, d), _d(h).view(B, T, 2 * d), _stored(at))
        _chk("dwglu_wgrad", name, case, dw, ref, L=B * T + 1)
        with hip.splitk_batched():
            hip.dwglu_wgrad(dcd, hd, dwb, B, T)
            assert torch.equal(dwb.cpu(), dw0)            # queued: nothing folded before the batch closes
        assert torch.equal(dwb, dw), case


def test_dwglu_refuses_the_bf16_f32_pairing():
    """DW_DISPATCH_GA has no MIXF32 instantiation: a bf16 gradient next to an f32 h is refused, nothing is launched."""
    hip, dev = _hip(), _dev()
    from sar_ssl_amd._lib import SarsslHipError
    B, T, d = 1, 16, 8
    g = _gen(5)
    h, dc = _st((B * T, 2 * d), F32, g).to(dev), _st((B * T, d), BF16, g).to(dev)
    w = torch.randn((d, 31), generator=g).to(dev)
    with pytest.raises(SarsslHipError):
        hip.dwglu_bwd(dc, h, w, B, T)
    dw = torch.ones((d, 31), device=dev)
    with pytest.raises(SarsslHipError):
        hip.dwglu_wgrad(dc, h, dw, B, T)
    torch.cuda.synchronize()
    assert float((dw - 1.0).abs().max()) == 0.0


# ================================================================================================ c. attention fallback path
SM_T = [(1, 6), (2, 6), (8, 6), (63, 6), (64, 6), (65, 6), (100, 6), (1024, 1)]          # (T, nmat): 1 .. 16 registers of 64 columns


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_softmax_relshift_fwd(dtp):
    """softmax_relshift_fwd_kernel<T>, T = f32 / bf16 / fp16, rows of 1 .. 1024 columns: one short register, exactly one (T = 64), one
    column into the second (65), all sixteen (1024)."""
    hip, dev = _hip(), _dev()
    for T, nmat in SM_T:
        g = _gen(T)
        content, pos = torch.randn((nmat, T, T), generator=g) * 3, torch.randn((nmat, T, T), generator=g) * 3
        p, pd = hip.softmax_relshift_fwd(content.to(dev), pos.to(dev), 0.17, dtp)
        assert pd is p and p.dtype == dtp
        _chk("softmax_fwd", NAME[dtp], "T%d" % T, p, refs.softmax_relshift_fwd(_d(content), _d(pos), 0.17), L=T)


@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_softmax_bwd(pair, monkeypatch):
    """softmax_bwd_kernel<T, TA> in the four DISPATCH_GA pairings; the wrapper derives the gradient dtype through hip.gdtype_of, so MIXF32
    (bf16 gradient next to f32 probabilities) is reached with hip._hybrid set."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    if name == "mixf32":
        monkeypatch.setattr(hip, "_hybrid", True)
    for T, nmat in SM_T:
        g = _gen(T + 5000)
        p = torch.softmax(torch.randn((nmat, T, T), generator=g, dtype=torch.float64) * 2, -1).to(at)
        dpd = torch.randn((nmat, T, T), generator=g)
        ds = hip.softmax_bwd(dpd.to(dev), p.to(dev), 0.17)
        assert ds.dtype == gt
        _chk("softmax_bwd", name, "T%d" % T, ds, refs.softmax_bwd(_d(dpd), _d(p), 0.17), L=T)


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_relshift_bwd_moves_elements_exactly(dtp):
    """relshift_bwd_kernel<T> (f32; 16-bit with T % 8 != 0) and relshift_bwd8_kernel (bf16 / fp16 bit patterns, T % 8 == 0, T = 8 its
    smallest): the inverse shift only moves elements, so the result equals refs.shift_bwd of the stored values exactly - including
    mat = 0, r = 0, whose sources lie before the buffer and must read as zero - and the 8-wide kernel equals the generic one run on the
    same values held in f32."""
    hip, dev = _hip(), _dev()
    for T, nmat in SM_T:
        ds = _st((nmat, T, T), dtp, _gen(T + 9000))
        dsd = ds.to(dev)                                   # a fresh allocation: the input starts its buffer
        got = hip.relshift_bwd(dsd)
        assert got.dtype == dtp and torch.equal(_d(got), refs.shift_bwd(_d(ds))), "T=%d" % T
        if dtp != F32 and T % 8 == 0:
            assert torch.equal(got, hip.relshift_bwd(dsd.float()).to(dtp)), "T=%d" % T


# ================================================================================================ d. small elementwise kernels
@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_bias2_on_a_column_slice(dtp):
    """bias2_kernel<T> with q a column slice of a [M, 3d] buffer (the engine's view into qkv)."""
    hip, dev = _hip(), _dev()
    for M, d in ((50, 72), (3, 260)):
        g = _gen(M + d)
        qkv = _st((M, 3 * d), dtp, g)
        u, v = torch.randn(d, generator=g), torch.randn(d, generator=g)
        qu, qv = hip.bias2(qkv.to(dev)[:, d:2 * d], u.to(dev), v.to(dev))
        q = _d(qkv)[:, d:2 * d]
        _chk("bias2", NAME[dtp], "M%d,d%d,u" % (M, d), qu, q + _d(u))
        _chk("bias2", NAME[dtp], "M%d,d%d,v" % (M, d), qv, q + _d(v))


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_axpby_with_and_without_y(dtp):
    hip, dev = _hip(), _dev()
    g = _gen(17)
    x, y = _st((50, 72), dtp, g), _st((50, 72), dtp, g)
    a, b = 0.5, 2.0                                        # exact in f32: the scalars are stored operands too
    _chk("axpby", NAME[dtp], "xy", hip.axpby(x.to(dev), y.to(dev), a, b), a * _d(x) + b * _d(y))
    _chk("axpby", NAME[dtp], "x", hip.axpby(x.to(dev), None, 0.75), 0.75 * _d(x))


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_axpby2d_in_place_on_row_strided_views(dtp):
    """axpby2d_kernel<T> with out aliasing x, every operand row-strided; the columns around the views keep their values."""
    hip, dev = _hip(), _dev()
    g = _gen(18)
    M, N = 37, 68
    x, y = _st((M, N), dtp, g), _st((M, N), dtp, g)
    xs, xbuf = _view(x, dev, 4, 8)
    ys, _ = _view(y, dev, 8, 12)
    out = hip.axpby2d(xs, ys, 0.5, -1.5, out=xs)
    assert out.data_ptr() == xs.data_ptr()
    _chk("axpby2d", NAME[dtp], "inplace", xbuf[:, 4:4 + N], 0.5 * _d(x) - 1.5 * _d(y))
    assert _rest_is_zero(xbuf, 4, N)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("pair", PAIRS, ids=_ids)
def test_act_bwd(pair, act):
    """act_bwd_kernel<T, TA>: act 0 (scale only, h unused), 1 (ReLU on the saved output: exact zeros and negative zeros pass nothing),
    2 (Swish' of the saved pre-activation), in the four DISPATCH_GA pairings."""
    hip, dev = _hip(), _dev()
    name, gt, at = pair
    g = _gen(40 + act)
    n = 4 * 643
    dz, h = _st((n,), gt, g), _st((n,), at, g, 2.0)
    h[::7] = 0.0
    h[3::11] = -0.0
    got = hip.act_bwd(dz.to(dev), h.to(dev) if act else None, act, gscale=0.5)
    assert got.dtype == gt
    ref = 0.5 * _d(dz) * (1.0 if act == 0 else refs.relu_grad(_d(h)) if act == 1 else refs.swish_grad(_d(h)))
    _chk("act_bwd", name, "act%d" % act, got, ref)
    if act == 1:
        assert float(got[::7].float().abs().max()) == 0.0 and float(got[3::11].float().abs().max()) == 0.0


CASTS = [(F32, BF16), (BF16, F32), (F32, F32), (F32, F16), (F16, F32), (F16, BF16), (BF16, F16)]


@pytest.mark.parametrize("src,dst", CASTS, ids=["%s_to_%s" % (NAME[a], NAME[b]) for a, b in CASTS])
def test_cast_equals_torch_bit_for_bit(src, dst):
    """The seven cast_kernel<TS, TD> instantiations at one element, around one 256-thread block and beyond the 4096-block grid (the
    grid-stride loop), values from fp16 subnormals up to 4e3."""
    hip, dev = _hip(), _dev()
    for n in (1, 255, 256, 257, 1048583):
        g = _gen(n)
        v = (torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 10 - 7)).to(src)
        got = hip.cast(v.to(dev), dst)
        assert got.dtype == dst and torch.equal(got.cpu(), v.to(dst)), n


@pytest.mark.parametrize("src,dst", [(BF16, BF16), (F16, F16)], ids=["bf16_to_bf16", "fp16_to_fp16"])
def test_cast_refuses_the_pairs_it_has_no_kernel_for(src, dst):
    hip, dev = _hip(), _dev()
    from sar_ssl_amd._lib import SarsslHipError
    with pytest.raises(SarsslHipError):
        hip.cast(torch.ones(8, dtype=src, device=dev), dst)


@pytest.mark.parametrize("n", [1, 64, 300])
def test_f64_accum(n):
    """f64_accum (scale != 1) and f64_accum2 onto non-zero destinations."""
    hip, dev = _hip(), _dev()
    g = _gen(n)
    src = torch.randn(2 * n, generator=g, dtype=torch.float64)
    d0, d1, d2 = (torch.randn(n, generator=g) for _ in range(3))
    scale = 0.37
    dst = d0.to(dev)
    hip.f64_accum(src[:n].to(dev), dst, scale)
    _chk("f64_accum", "f32", "n%d,scale" % n, dst, _d(d0) + src[:n] * float(torch.tensor(scale, dtype=F32)))
    a, b = d1.to(dev), d2.to(dev)
    hip.f64_accum2(src.to(dev), a, b)
    _chk("f64_accum", "f32", "n%d,first" % n, a, _d(d1) + src[:n])
    _chk("f64_accum", "f32", "n%d,second" % n, b, _d(d2) + src[n:])


# (M, N): one row; N no multiple of 64; one more row than a 256-row slice; 20 slices of 17 column tiles; more row slices than the
# 512 / 17 = 30 the launch allows (the cap)
COLSUM_SHAPES = [(1, 4), (50, 68), (257, 64), (5000, 1028), (8200, 1028)]


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_colsum_store_and_colsum_now(dtp):
    """colsum_store_kernel<T> (result in the activation dtype) and colsum(now=True) (colsum_multi_kernel<T> with one problem + the fold,
    += onto non-zero values) on inputs with row stride != N."""
    hip, dev = _hip(), _dev()
    for M, N in COLSUM_SHAPES:
        g = _gen(M + N)
        x = _st((M, N), dtp, g)
        xs, _ = _view(x, dev, 4, 8)
        ref = refs.colsum(_d(x))
        case = "M%d,N%d" % (M, N)
        got = hip.colsum_store(xs)
        assert got.dtype == dtp
        _chk("colsum_store", NAME[dtp], case, got, ref, L=M)
        o0 = torch.randn(N, generator=g)
        out = o0.to(dev)
        hip.colsum(xs, out, now=True)
        _chk("colsum", NAME[dtp], case, out, _d(o0) + ref, L=M + 1)


# ================================================================================================ e. batched folds
def _colsum_problems(n, dev):
    """n bf16 column-sum problems of mixed shape; problems 3 and 17 share one destination."""
    xs, outs, refsum, terms = [], [], [], []
    for q in range(n):
        M, N = COLSUM_SHAPES[q % 4] if q != 17 else COLSUM_SHAPES[3]
        g = _gen(500 + q)
        x = _st((M, N), BF16, g)
        xs.append(_view(x, dev, 4, 4)[0])
        if q == 17:
            outs.append(outs[3]); refsum[3] = refsum[3] + refs.colsum(_d(x)); terms[3] += M
            refsum.append(None); terms.append(0)
        else:
            o0 = torch.randn(N, generator=g)
            outs.append(o0); refsum.append(_d(o0) + refs.colsum(_d(x))); terms.append(M + 1)
    return xs, outs, refsum, terms


@pytest.mark.parametrize("n,splitk_outside", [(25, False), (33, True)], ids=["25_sums", "33_sums_33_folds_queued"])
def test_batched_column_sums_equal_the_same_sums_one_by_one(n, splitk_outside):
    """colsum_batched() + splitk_batched(): 25 sums (24 fill one colsum_multi launch, the 25th takes a second) / 33 sums with the split-K
    batch as the outer context, so that all 33 folds are queued there and the 32-problem reduce launch is issued twice.  Two problems
    share a destination (the reduce is a non-atomic read-modify-write: _splitk_flush_items splits the launch).  Every destination equals
    the f64 sum to the f32 gate and, bit for bit, the same sums issued one by one with now=True in the same order."""
    hip, dev = _hip(), _dev()
    xs, o0, refsum, terms = _colsum_problems(n, dev)
    own = {}
    for q in range(n):
        own[q] = own[3] if q == 17 else o0[q].to(dev)
    outer, inner = (hip.splitk_batched, hip.colsum_batched) if splitk_outside else (hip.colsum_batched, hip.splitk_batched)
    with outer(), inner():
        for q in range(n):
            hip.colsum(xs[q], own[q])
    one = {}
    for q in range(n):
        one[q] = one[3] if q == 17 else o0[q].to(dev)
        hip.colsum(xs[q], one[q], now=True)
    for q in range(n):
        if q == 17:
            continue
        _chk("colsum", "bf16", "batched%d,q%d" % (n, q), own[q], refsum[q], L=terms[q])
        assert torch.equal(own[q], one[q]), q


LN_BATCH = [(7, 32), (70, 256), (4100, 512), (33, 768), (5, 1028), (1, 4), (300, 1024), (64, 260), (129, 512)]


def test_batched_layernorm_parameter_folds_equal_the_unbatched_ones():
    """ln_reduce_batched() around nine layernorm_bwd calls (MIX16) of mixed (M, d): eight problems fill one ln_param_reduce_multi launch, the
    ninth takes a second; d = 1028 goes through layernorm_bwd_wide_kernel, which shares the partial layout.  dgamma / dbeta, accumulated
    onto non-zero values, equal the unbatched calls' bit for bit."""
    hip, dev = _hip(), _dev()
    args, batched, plain = [], [], []
    for q, (M, d) in enumerate(LN_BATCH):
        g = _gen(800 + q)
        x, dy = _st((M, d), F16, g, 1.5, 0.3).to(dev), _st((M, d), BF16, g).to(dev)
        gamma, beta = (torch.rand(d, generator=g) + 0.5).to(dev), torch.randn(d, generator=g).to(dev)
        _, stats = hip.layernorm_fwd(x, gamma, beta, 1e-5)
        args.append((dy, x, gamma, stats))
        p0 = torch.randn((2, d), generator=g).to(dev)
        batched.append(p0.clone()); plain.append(p0.clone())
    with hip.ln_reduce_batched():
        dxb = [hip.layernorm_bwd(*a, dgamma=b[0], dbeta=b[1]) for a, b in zip(args, batched)]
    dxp = [hip.layernorm_bwd(*a, dgamma=b[0], dbeta=b[1]) for a, b in zip(args, plain)]
    for q in range(len(LN_BATCH)):
        assert torch.equal(batched[q], plain[q]) and torch.equal(dxb[q], dxp[q]), LN_BATCH[q]
        assert not torch.equal(batched[q], batched[q] * 0)


# ================================================================================================ f. entry points no other test calls
@pytest.mark.parametrize("C", [4, 64, 256])
def test_bn_eval_affine(C):
    hip, dev = _hip(), _dev()
    g = _gen(C)
    gamma, beta, rm = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g), torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.1
    aff = hip.bn_eval_affine(C, gamma.to(dev), beta.to(dev), rm.to(dev), rv.to(dev), eps=1e-5)
    eps32 = float(torch.tensor(1e-5, dtype=F32))
    for nm, got, ref in zip(("scale", "shift", "mean", "rstd"), aff, refs.bn_eval_affine(_d(gamma), _d(beta), _d(rm), _d(rv), eps32)):
        _chk("bn_eval_affine", "f32", "C%d,%s" % (C, nm), got, ref)


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_patch_w_is_the_relayout_of_the_rounded_weight(dtp):
    hip, dev = _hip(), _dev()
    for d, F in ((8, 5), (72, 33)):
        W = torch.randn((d, 4, F, 1), generator=_gen(d + F))
        got = hip.patch_w(W.to(dev), dtp)
        assert got.dtype == dtp and torch.equal(got.cpu(), refs.patch_w(W.to(dtp)))


@pytest.mark.parametrize("dtype,gdtype", [(F32, None), (BF16, None), (F16, BF16)], ids=["f32", "bf16", "fp16_bf16"])
def test_conv_taps_is_the_relayout_of_the_rounded_weight(dtype, gdtype):
    """conv_taps_kernel<T, TD>: <f32, f32>, <bf16, bf16> and <fp16, bf16>, the pair of the fp16-forward modes."""
    hip, dev = _hip(), _dev()
    W = torch.randn((64, 64, 3, 3), generator=_gen(64))
    fwd, dgr = hip.conv_taps(W.to(dev), dtype, gdtype)
    assert fwd.dtype == dtype and dgr.dtype == (gdtype or dtype)
    assert torch.equal(fwd.cpu(), refs.conv_taps(W.to(dtype))[0])
    assert torch.equal(dgr.cpu(), refs.conv_taps(W.to(gdtype or dtype))[1])


def test_conv_taps_refuses_fp16_gradient_taps():
    """There is no <fp16, fp16> instantiation (no numeric mode has fp16 gradients): refused with an error, not reinterpreted."""
    hip, dev = _hip(), _dev()
    from sar_ssl_amd._lib import SarsslHipError
    with pytest.raises(SarsslHipError):
        hip.conv_taps(torch.randn((64, 64, 3, 3), generator=_gen(1)).to(dev), F16)


MEAN_SHAPES = [(1, 1, 4), (3, 37, 72), (2, 256, 256)]


@pytest.mark.parametrize("dtp", STORE, ids=_ids)
def test_mean_rows(dtp):
    """mean_rows_kernel<T>, T = f32 / fp16 / bf16."""
    hip, dev = _hip(), _dev()
    for B, T, d in MEAN_SHAPES:
        x = _st((B, T, d), dtp, _gen(B + T + d), 1.0, 0.5)
        _chk("mean_rows", NAME[dtp], "B%d,T%d,d%d" % (B, T, d), hip.mean_rows(x.to(dev)), refs.mean_rows(_d(x)), L=T)


@pytest.mark.parametrize("dtp", [F32, BF16], ids=_ids)
def test_mean_rows_bwd(dtp):
    """mean_rows_bwd_kernel<T>; (2, 4100, 256) has more elements than 8192 workgroups of 256 threads: the grid-stride loop repeats."""
    hip, dev = _hip(), _dev()
    for B, T, d in MEAN_SHAPES + [(2, 4100, 256)]:
        dy = torch.randn((B, d), generator=_gen(B + T + d + 1))
        dx = hip.mean_rows_bwd(dy.to(dev), T, dtp)
        assert dx.dtype == dtp
        _chk("mean_rows_bwd", NAME[dtp], "B%d,T%d,d%d" % (B, T, d), dx, refs.mean_rows_bwd(_d(dy), T))


def test_mean_rows_bwd_refuses_fp16():
    hip, dev = _hip(), _dev()
    from sar_ssl_amd._lib import SarsslHipError
    with pytest.raises(SarsslHipError):
        hip.mean_rows_bwd(torch.ones((2, 8), device=dev), 3, F16)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (3, 1, 70), (5, 7, 256), (300, 2, 65)])
def test_small_linear(M, N, K, with_bias, act):
    """small_linear_fwd / _bwd (one wave per output; K below, at and beyond a wave's 64 lanes and 4 x 64): with and without bias, ReLU with
    outputs exactly 0 (row 0 of x is zero and bias[0] is zero), need_dx=False, dW / db accumulated onto non-zero values."""
    hip, dev = _hip(), _dev()
    g = _gen(M * 1000 + N * 100 + K)
    x, W = torch.randn((M, K), generator=g), torch.randn((N, K), generator=g)
    x[0] = 0.0
    b = torch.randn(N, generator=g) if with_bias else None
    if with_bias:
        b[0] = 0.0
    dy = torch.randn((M, N), generator=g)
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev) if with_bias else None
    y = hip.small_linear_fwd(xd, Wd, bd, act)
    _chk("small_linear_fwd", "f32", "M%d,N%d,K%d,act%d" % (M, N, K, act), y, refs.small_linear_fwd(_d(x), _d(W), _d(b) if with_bias else None, act),
         L=K + 1)
    assert float(y[0, 0]) == 0.0
    rdx, rdW, rdb = refs.small_linear_bwd(_d(dy), _d(y), _d(x), _d(W), act)
    # start values with the sign of the sum they receive: with N = 1 the deviation is that of ONE number, and a start value that cancels
    # the sum would measure the conditioning of that subtraction, not the kernel
    sgn = lambda r: torch.where(r < 0, -1.0, 1.0).float()
    dW0, db0 = torch.randn((N, K), generator=g).abs() * sgn(rdW), torch.randn(N, generator=g).abs() * sgn(rdb)
    for need_dx in (True, False):
        dW, db = dW0.to(dev), db0.to(dev)
        dx = hip.small_linear_bwd(dy.to(dev), y, xd, Wd, act, dW, db, need_dx=need_dx)
        case = "M%d,N%d,K%d,act%d,dx%d" % (M, N, K, act, need_dx)
        if need_dx:
            _chk("small_linear_bwd", "f32", case + ",dx", dx, rdx, L=N)
        else:
            assert dx is None
        _chk("small_linear_bwd", "f32", case + ",dW", dW, _d(dW0) + rdW, L=M + 1)
        _chk("small_linear_bwd", "f32", case + ",db", db, _d(db0) + rdb, L=M + 1)
