"""The GEMM family of csrc/gemm.hip, term by term, at shapes aimed at every instantiation its dispatcher has: sarssl_gemm in every dtype triple, layout, tile height
(FM = 1, 2, 4: 64-, 128-, 256-row tiles) and ragged / plain (EDGE) instantiation, every epilogue term of csrc/gemm_epilogue.h on its own,
the scalar-store path, the dropout mask as one function of the flat element index, split-K, the fp16-pair products of sarssl_gemm_split
and the grouped weight-gradient launch with fp16 activations - each against the f64 restatement of tests/gemm_refs.py on the operands
as stored.  Every case writes C and the saved pre-activation as windows of wider buffers filled with a sentinel (extra columns, rows
before and after) and asserts that nothing outside the window changed.
WHICH instantiation a case runs is NOT asserted: the library has no query for it.  The case names (fm1 / fm2 / fm4 = 64- / 128- / 256-row
tiles, plain / ragged) say what each shape was aimed at by reading pick_fm / launch_layout / launch_seg when this file was written; the
shape tables (_points, _term_points, _pair_points) repeat that rule's thresholds and nothing ties them to the library, so when the
rule moves these cases move with it silently.  What the file does pin is the arithmetic of whatever instantiation the dispatcher
picks for these shapes.  A query computed by the helper the launch itself uses, asserted in every case, is still to be built.
Batch counts follow the device's CU count; large grids come from shared operands (batch_inner = 16, sA = (s, 0), sB = (0, s): every A
against every B).  Every f64 comparison goes through conftest.check with the tolerance of sar_ssl_amd/parity.py GEMM: min(gate = 4x
measured, cap); profiles/gemm.txt holds the measured figures.

  instantiation aimed at                                         by
  gemm_kernel FM = 1 plain           (BIG triples)               test_instantiation[*-fm1_plain], [*-fm1_plain_xcd] (grid_y = 16: XCD remap
                                                                 over two groups; fm1_plain has grid_y = 2: no remap), test_epilogue_terms[*-fm1_plain]
  gemm_kernel FM = 1 ragged          (BIG triples)               test_instantiation[*-fm1_ragged], test_epilogue_terms[*-fm1_ragged],
                                                                 test_scalar_path (N % 8 != 0, ldc % 8 != 0, ldr % 8 != 0)
  gemm_kernel FM = 2 plain           (BIG triples)               test_instantiation[*-fm2_plain_grid] (tiles > 1.12 x CUs),
                                                                 test_epilogue_terms[*-fm2_plain] (one tall matrix, the has_ex prefetch over two slices)
  gemm_kernel FM = 2 plain           (the other triples)         test_instantiation[*-fm2_plain]
  gemm_kernel FM = 2 ragged          (all triples)               test_instantiation[*-fm2_ragged_48], [*-fm2_ragged_72], test_split_k (K % 64 != 0)
  the relative shift (ragged FM = 1, 2)                           test_row_shift
  gemm_kernel FM = 4 plain / ragged  (BIG triples)               test_instantiation[*-fm4_plain], [*-fm4_ragged], test_has_ex_fm4
  the two reachable hash branches' common mask, all of the above test_dropout_mask_*
  gemm_seg_kernel FM = 1, 2 x plain, ragged x NSEG 2, 3 x C fp16, f32     test_pair_products (the ragged points also in test_gpu_hybrid.py)
  gemm_group_tn_kernel<f16> (and <bf16>: test_gpu_kernels.py)    test_group_tn_fp16_x
(BIG triples: (bf16, bf16, bf16), (bf16, bf16, f32), (fp16, fp16, fp16) - the ones dispatched with all three tile heights.)"""
import math

import pytest
import torch

import gemm_refs as refs
from conftest import check

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
#          name          A     B     C    precise
TRIPLES = [("bf16", BF16, BF16, BF16, False), ("bf16_f32", BF16, BF16, F32, False), ("fp16", F16, F16, F16, False),
           ("fp16_f32", F16, F16, F32, False), ("mix_ga", BF16, F16, BF16, False), ("mix_ga_f32", BF16, F16, F32, False),
           ("mix_ag", F16, BF16, BF16, False), ("f32_fast", F32, F32, F32, False), ("f32_precise", F32, F32, F32, True)]
BIG = ("bf16", "bf16_f32", "fp16")
TRIPLE = {t[0]: t for t in TRIPLES}
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
SENT = -1.75                       # exact in every dtype: an unchanged element is bit-unchanged
PRE, POST, XCOL = 3, 2, 8          # rows before / after the window, extra columns (ldc = N + 8 keeps the vector path's alignment)


def _hip():
    from sar_ssl_amd import hip
    return hip


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tol(family, key, L=None):
    from sar_ssl_amd import parity
    return parity.gemm_tol(family, key, L)


def _err(got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    return ((got.double() - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def _chk(family, key, case, got, ref, L=None):
    check("gemm.%s.%s[%s]" % (family, key, case), _err(got, ref), _tol(family, key, L))


def _rand(shape, dtype, seed, scale=1.0):
    """Seeded on the host, stored in `dtype` on the device."""
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(_dev())


def _window(lead, M, N, dtype, ldc, fill=None):
    """[*lead, M, N] window of a sentinel-filled buffer [*lead, PRE + M + POST, ldc] (fill: the window's initial content) -> (view, buffer)."""
    buf = torch.full(tuple(lead) + (PRE + M + POST, ldc), SENT, dtype=dtype, device=_dev())
    view = buf[..., PRE:PRE + M, :N]
    if fill is not None:
        view.copy_(fill)
    return view, buf


def _outside_unchanged(buf, M, N):
    chk = buf.clone()
    chk[..., PRE:PRE + M, :N] = SENT
    return bool((chk == SENT).all())


def _lay(T, kc):
    """A logical [.., rows, K] operand as laid out in memory for layout flag kc."""
    return T.contiguous() if kc else T.transpose(-1, -2).contiguous()


def _run(case, A, B, dtC, M, N, K, a_kc=True, b_kc=True, outer=None, precise=False, ldc=None, ldr=None, bias=None, act=0, alpha=1.0,
         out_scale=1.0, want_pre=False, aux=None, aux_act=0, resid=None, res_scale=1.0, p=0.0, seed=0):
    """One sarssl_gemm launch on operands as laid out (A: [.., M, K] | [.., K, M], B likewise).  outer = (nA, nB): nA x nB batch products
    from nA A's and nB B's.  aux / resid: [*lead, M, N] tensors as stored; aux travels in C's geometry (it shares ldc and the batch strides
    of C), resid in its own (ldr).  Asserts the sentinels; -> (C window, pre-activation window or None)."""
    hip = _hip()
    lead = tuple(outer) if outer else ()
    nb = outer[0] * outer[1] if outer else 1
    ldc = N + XCOL if ldc is None else ldc
    ldr = (N + 2 * XCOL if ldr is None else ldr) if resid is not None else 0
    Cv, Cb = _window(lead, M, N, dtC, ldc)
    Pv, Pb = _window(lead, M, N, dtC, ldc) if want_pre else (None, None)
    Xv = _window(lead, M, N, aux.dtype, ldc, aux)[0] if aux is not None else None
    Rv = _window(lead, M, N, dtC, ldr, resid)[0] if resid is not None else None
    rows = PRE + M + POST
    kw = {}
    if outer:
        kw = dict(nbatch=nb, batch_inner=outer[1], sA=(A.stride(0), 0), sB=(0, B.stride(0)), sC=(outer[1] * rows * ldc, rows * ldc),
                  sR=(outer[1] * rows * ldr, rows * ldr))
    hip.gemm(A, B, a_kc=a_kc, b_kc=b_kc, M=M, N=N, K=K, lda=A.stride(-2), ldb=B.stride(-2), out=Cv, ldc=ldc, bias=bias, act=act, alpha=alpha,
             out_scale=out_scale, preact=Pv, aux=Xv, aux_act=aux_act, resid=Rv, ldr=ldr, res_scale=res_scale, p_drop=p, seed=seed,
             precise=precise, **kw)
    assert _outside_unchanged(Cb, M, N), case + ": C written outside its window"
    assert Pb is None or _outside_unchanged(Pb, M, N), case + ": pre-activation written outside its window"
    return Cv, Pv


# ---- shared operands and f64 products: one per (shape, operand dtypes), whatever the layout or the output dtype -------------------------
_cache = {}


def _operands(shape, outer, dtA, dtB, precise=False):
    """-> (A [nA, M, K] | [M, K], B, f64 product [nA, nB, M, N] | [M, N]) as stored in dtA / dtB; cached, never modified."""
    key = (shape, outer, dtA, dtB, precise)
    if key not in _cache:
        M, N, K = shape
        la, lb = ((outer[0],), (outer[1],)) if outer else ((), ())
        A = _rand(la + (M, K), dtA, 7 * M + K)
        B = _rand(lb + (N, K), dtB, 11 * N + K + 1)
        _cache[key] = (A, B, refs.product(A, B, precise=precise, outer=bool(outer)))
    return _cache[key]


def _points():
    """name -> (shape, outer).  The names say which instantiation the shape is AIMED at by pick_fm's rule as it stood when this file was
    written (64-row tiles while the 128-row tiles number at most 1.12 x CUs, 256-row tiles from 2 x CUs of them on with K >= 1536 and
    M >= 192, ragged for M, N, K off the tile); nothing here asserts that the library still agrees.  Batch counts from the CU count."""
    cus = _cus()
    n_fm2 = int(1.12 * cus) // 16 + 1                # nA x 16 products of one 128 x 128 tile each: more than 1.12 x CUs
    n_fm4 = -(-cus // 16)                            # 2 x nA x 16 256-row tiles >= 2 x CUs
    n_fm4r = -(-cus // 32)                           # 4 x nA x 16 (264 x 136: 2 x 2 tiles) >= 2 x CUs
    return {
        "fm1_plain": ((128, 128, 64), None),
        "fm1_plain_xcd": ((1024, 256, 64), None),    # 64-row tiles: grid (2, 16), grid_y % 8 == 0, two groups of 8 row panels
        "fm1_ragged": ((136, 72, 40), None),
        "fm2_plain": ((128, 128, 64), None),         # (the triples that are dispatched with 128-row tiles only)
        "fm2_plain_grid": ((128, 128, 64), (n_fm2, 16)),
        "fm2_ragged_48": ((48, 136, 32), None),
        "fm2_ragged_72": ((72, 136, 40), None),
        "fm4_plain": ((256, 256, 1536), (n_fm4, 16)),
        "fm4_ragged": ((264, 136, 1544), (n_fm4r, 16)),
    }


POINTS = ("fm1_plain", "fm1_plain_xcd", "fm1_ragged", "fm2_plain", "fm2_plain_grid", "fm2_ragged_48", "fm2_ragged_72", "fm4_plain", "fm4_ragged")
MATRIX = [(t[0], p) for t in TRIPLES for p in POINTS if (p != "fm2_plain") == (t[0] in BIG) or p.startswith("fm2_ragged")]


# ================================================================================================ a. instantiation matrix
@pytest.mark.parametrize("triple,point", MATRIX, ids=["%s-%s" % tp for tp in MATRIX])
def test_instantiation(triple, point):
    """bias + alpha + Swish + saved pre-activation in all four layouts at the smallest shape that reaches the instantiation."""
    name, dtA, dtB, dtC, precise = TRIPLE[triple]
    shape, outer = _points()[point]
    M, N, K = shape
    A, B, acc = _operands(shape, outer, dtA, dtB, precise)
    bias = _rand((N,), F32, 5)
    want, want_pre = refs.epilogue(acc, alpha=0.5, bias=bias, act=2)
    for a_kc, b_kc in LAYOUTS:
        case = "%s,%s,%d%d" % (point, "x".join(map(str, shape)), a_kc, b_kc)
        C, P = _run(case, _lay(A, a_kc), _lay(B, b_kc), dtC, M, N, K, a_kc, b_kc, outer, precise, bias=bias, act=2, alpha=0.5, want_pre=True)
        _chk("product", triple, case, C, want, L=K + 1)
        _chk("preact", triple, case, P, want_pre, L=K + 1)


# ================================================================================================ b. epilogue terms one at a time
def _term_points():
    tall = 128 * (int(1.12 * _cus()) + 1)            # one matrix of more 128 x 128 tiles than 1.12 x CUs: FM = 2, grid_y % 8 != 0 or == 0
    return {"fm1_plain": (128, 128, 64), "fm2_plain": (tall, 128, 64), "fm1_ragged": (136, 72, 40)}


@pytest.mark.parametrize("point", ["fm1_plain", "fm2_plain", "fm1_ragged"])
@pytest.mark.parametrize("triple", ["bf16", "fp16", "bf16_f32"])
def test_epilogue_terms(triple, point):
    """Each term of epilogue8 on its own, for each C dtype.  has_ex: 16-bit C, plain instantiation, exactly one of residual / aux - their
    rows are prefetched into registers one slice ahead (load_ex: row stride ldr for the residual, ldc for aux); residual and aux together
    turn the prefetch off."""
    name, dtA, dtB, dtC, precise = TRIPLE[triple]
    M, N, K = _term_points()[point]
    A, B, acc = _operands((M, N, K), None, dtA, dtB)
    bias, R, H = _rand((N,), F32, 5), _rand((M, N), dtC, 6), _rand((M, N), dtC, 8)
    ex = "has_ex," if dtC != F32 and not (M % 128 or N % 128 or K % 64) else ""          # (the prefetch exists in the plain instantiations only)
    tag = lambda term: "%s,%s,%s" % (point, "x".join(map(str, (M, N, K))), term)
    run = lambda term, **kw: _run(tag(term), A, B, dtC, M, N, K, **kw)

    def one(term, family, L, **kw):
        rk = {k: v for k, v in kw.items() if k != "want_pre"}
        C, P = run(term, **kw)
        want, pre = refs.epilogue(acc, **rk)
        _chk(family, triple, tag(term), C, want, L=L)
        if P is not None:
            _chk("preact", triple, tag(term) + ".pre", P, pre, L=L)
        return C

    one("bias", "product", K + 1, bias=bias)
    one("relu", "product", K + 1, bias=bias, act=1)
    one("swish", "product", K + 1, bias=bias, act=2)
    one("preact", "product", K + 1, bias=bias, act=2, want_pre=True)
    one("out_scale", "product", K + 1, bias=bias, out_scale=0.25)
    one(ex + "resid", "product", K + 1, resid=R, res_scale=0.5)                      # ldr = N + 16 != ldc = N + 8
    for aux_act in (1, 2):
        one(ex + "aux%d" % aux_act, "actbwd", K, aux=H, aux_act=aux_act)
        if dtC == BF16:                                                             # the fp16-forward mode: fp16 pre-activation beside a bf16 gradient
            one(ex + "aux%d_fp16" % aux_act, "actbwd", K, aux=H.to(F16), aux_act=aux_act)
    # residual and aux together: what the two single-term runs imply, added up
    C, _ = run("resid+aux", aux=H, aux_act=2, resid=R, res_scale=0.5)
    _chk("actbwd", triple, tag("resid+aux"), C, refs.epilogue(acc, aux=H, aux_act=2)[0] + 0.5 * R.double(), L=K + 1)


@pytest.mark.parametrize("triple", ["bf16", "fp16"])
def test_has_ex_fm4(triple):
    """The prefetch over the four slices of a 256-row tile (two register sets, ping-pong), residual and aux rows with batch strides."""
    name, dtA, dtB, dtC, precise = TRIPLE[triple]
    shape, outer = _points()["fm4_plain"]
    M, N, K = shape
    A, B, acc = _operands(shape, outer, dtA, dtB)
    R = _rand(tuple(outer) + (M, N), dtC, 16, scale=30.0)
    C, _ = _run("fm4_plain,has_ex,resid", A, B, dtC, M, N, K, outer=outer, resid=R, res_scale=0.5)
    _chk("product", triple, "fm4_plain,has_ex,resid", C, refs.epilogue(acc, resid=R, res_scale=0.5)[0], L=K + 1)
    C, _ = _run("fm4_plain,has_ex,aux2", A, B, dtC, M, N, K, outer=outer, aux=(R * (1.0 / 30.0)).to(dtC), aux_act=2)
    _chk("actbwd", triple, "fm4_plain,has_ex,aux2", C, refs.epilogue(acc, aux=(R * (1.0 / 30.0)).to(dtC), aux_act=2)[0], L=K)


# ================================================================================================ c. scalar path
@pytest.mark.parametrize("N,ldc,ldr", [(9, None, None), (36, None, None), (100, None, None), (72, 76, None), (72, None, 75)],
                         ids=["N9", "N36", "N100", "N72_ldc76", "N72_ldr75"])
@pytest.mark.parametrize("triple", ["bf16", "fp16", "bf16_f32"])
def test_scalar_path(triple, N, ldc, ldr):
    """vec_ok == false (N, ldc or ldr no multiple of 8): scalar stores, nvalid < 8, scalar aux / residual loads, and for N = 9 the
    per-element dropout branch (odd base indices) - with bias, saved pre-activation, aux, residual and dropout in one launch."""
    name, dtA, dtB, dtC, precise = TRIPLE[triple]
    M, K = 136, 40
    ldc = N + 3 if ldc is None and N % 8 else ldc          # (N = 72: the default window N + 8, unless the case sets ldc)
    ldr = N + 16 if ldr is None else ldr
    A, B, acc = _operands((M, N, K), None, dtA, dtB)
    bias, R, H = _rand((N,), F32, 5), _rand((M, N), dtC, 6), _rand((M, N), dtC, 8)
    p, seed = 0.25, 0x5eed0000beef
    keep = torch.from_numpy(refs.keep_mask(seed, M * N, p)).view(M, N).to(_dev())
    for a_kc in (True, False):
        case = "scalar,%dx%dx%d,ldc%s,ldr%d,%d1" % (M, N, K, ldc, ldr, a_kc)
        C, P = _run(case, _lay(A, a_kc), B, dtC, M, N, K, a_kc, True, ldc=ldc, ldr=ldr, bias=bias, want_pre=True, aux=H, aux_act=2,
                    resid=R, res_scale=0.5, p=p, seed=seed)
        want, pre = refs.epilogue(acc, bias=bias, aux=H, aux_act=2, keep=keep, p=p, resid=R, res_scale=0.5)
        _chk("actbwd", triple, case, C, want, L=K + 2)
        _chk("preact", triple, case + ".pre", P, pre, L=K + 1)
        # dropped elements are exactly the residual's share: the mask sits where the restatement puts it
        assert torch.equal(C[~keep].double(), (0.5 * R.double())[~keep].to(dtC).double())
        if dtC == BF16:                                 # the scalar load of an fp16 pre-activation beside a bf16 C
            C, _ = _run(case + ",aux_fp16", _lay(A, a_kc), B, dtC, M, N, K, a_kc, True, ldc=ldc, ldr=ldr, aux=H.to(F16), aux_act=2,
                        resid=R, res_scale=0.5)
            _chk("actbwd", triple, case + ",aux_fp16", C, refs.epilogue(acc, aux=H.to(F16), aux_act=2, resid=R, res_scale=0.5)[0], L=K + 1)


@pytest.mark.parametrize("triple", ["bf16", "fp16", "bf16_f32"])
def test_row_shift(triple):
    """c_row_shift (M = N = ldc = T, always the ragged instantiation): row m of every batch matrix lands m + 1 - T elements further, what
    falls before its own matrix is dropped - not written into the batch before -, and the elements (i, i + 1) are never stored."""
    hip = _hip()
    name, dtA, dtB, dtC, precise = TRIPLE[triple]
    nb, K = 3, 40
    for T in (72, 136):                               # 128-row and (BIG triples) 64-row tiles
        A, B = _rand((nb, T, K), dtA, 70 + T), _rand((nb, T, K), dtB, 71 + T)
        Cv, Cb = _window((nb,), T, T, dtC, T)
        hip.gemm(A, B, M=T, N=T, K=K, lda=K, ldb=K, out=Cv, ldc=T, nbatch=nb, sA=(T * K, 0), sB=(T * K, 0), sC=((PRE + T + POST) * T, 0),
                 alpha=0.5, c_row_shift=True)
        want, written = refs.shift(0.5 * refs.product(A, B))
        assert _outside_unchanged(Cb, T, T) and bool((Cv[:, ~written] == SENT).all())
        _chk("product", triple, "row_shift,%dx%dx%d" % (T, T, K), torch.where(written, Cv.double(), torch.zeros_like(want)), want, L=K)


# ================================================================================================ d. dropout mask
def _mask_of(case, A, B, dtC, M, N, K, p, seed, bias, **kw):
    """Y0 (p = 0, no exact zero), Yd; asserts Yd == where(mask, Y0 * inv_keep, 0) bit for bit and the keep fraction -> (mask, Yd)."""
    Y0, _ = _run(case + ",p0", A, B, dtC, M, N, K, bias=bias, **kw)
    Yd, _ = _run(case + ",p%g" % p, A, B, dtC, M, N, K, bias=bias, p=p, seed=seed, **kw)
    assert bool((Y0 != 0).all())
    mask = Yd != 0
    if dtC == F32:
        assert torch.equal(Yd, torch.where(mask, Y0 * refs.inv_keep(p), torch.zeros_like(Y0))), case      # (inv_keep: an f32 value)
    n = mask.numel()
    assert abs(mask.double().mean().item() - (1.0 - p)) < 5.0 * math.sqrt(p * (1.0 - p) / n), case      # five binomial standard deviations
    return mask, Yd


def _host_mask(seed, n, p):
    return torch.from_numpy(refs.keep_mask(seed, n, p)).to(_dev())


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("point", [q for q in POINTS if q != "fm2_plain"])
def test_dropout_mask_every_tile_height(point, p):
    """f32 output, out_scale 1, no residual, in every tile height and EDGE setting (batched launches: flat index (z M + m) N + n): the mask
    is the restatement's function of (seed, flat index), and Yd is Y0 scaled by an f32 1 / (1 - p) where kept.  Not reached: the two
    branches for an 8-wide piece at or across a multiple of 2^33 elements - they need a 32 GB output."""
    name, dtA, dtB, dtC, precise = TRIPLE["bf16_f32"]
    shape, outer = _points()[point]
    M, N, K = shape
    A, B, _acc = _operands(shape, outer, dtA, dtB)
    seed = 0x1234567887654321
    mask, _ = _mask_of("mask," + point, A, B, dtC, M, N, K, p, seed, _rand((N,), F32, 5), outer=outer)
    assert torch.equal(mask.reshape(-1), _host_mask(seed, mask.numel(), p))


@pytest.mark.parametrize("p", [0.1, 0.25])
def test_dropout_mask_every_triple_and_pair_product(p):
    """(128, 128, 64) in every dtype triple (64-row tiles for the BIG ones, 128-row tiles for the others) and through sarssl_gemm_split:
    one mask; a 16-bit output is the f32 run's output rounded to its dtype."""
    hip = _hip()
    M, N, K = 128, 128, 64
    seed = 0xabcdef0123
    want = _host_mask(seed, M * N, p).view(M, N)
    bias = _rand((N,), F32, 5)
    yd = {}
    for name, dtA, dtB, dtC, precise in TRIPLES:
        A, B, _acc = _operands((M, N, K), None, dtA, dtB, precise)
        mask, yd[name] = _mask_of("mask,triple," + name, A, B, dtC, M, N, K, p, seed, bias, precise=precise)
        assert torch.equal(mask, want), name
    for k16, k32 in (("bf16", "bf16_f32"), ("fp16", "fp16_f32"), ("mix_ga", "mix_ga_f32")):
        assert torch.equal(yd[k16], yd[k32].to(yd[k16].dtype)), k16
    x, w = _rand((M, K), F32, 31), _rand((N, K), F32, 32, scale=0.03)
    xp, wp = hip.split_pair(x), hip.split_pair(w)
    for nseg, a in ((3, xp), (2, xp.hi)):
        y0, b0 = _window((), M, N, F32, N + XCOL)
        ydv, bd = _window((), M, N, F32, N + XCOL)
        hip.gemm_split(a, wp.hi, wp.lo, M=M, N=N, K=K, out=y0, ldc=N + XCOL, bias=bias)
        hip.gemm_split(a, wp.hi, wp.lo, M=M, N=N, K=K, out=ydv, ldc=N + XCOL, bias=bias, p_drop=p, seed=seed)
        assert _outside_unchanged(b0, M, N) and _outside_unchanged(bd, M, N) and bool((y0 != 0).all())
        assert torch.equal(ydv != 0, want), nseg
        assert torch.equal(ydv, torch.where(want, y0 * refs.inv_keep(p), torch.zeros_like(y0)))


@pytest.mark.parametrize("p", [0.1, 0.25])
def test_dropout_mask_same_elements_other_shape(p):
    """Batch z of an (nbatch, M, N) launch against rows z M .. of one (nbatch M, N) launch; (64, 72) against (512, 9): the same 4608
    elements, the first through the hoisted pair-hash branch, the second - odd base indices - through the per-element branch."""
    name, dtA, dtB, dtC, precise = TRIPLE["bf16_f32"]
    seed = 0x0badc0ffee
    bias72, bias9 = _rand((72,), F32, 5), _rand((9,), F32, 5)
    K = 40
    A, B, _acc = _operands((64, 72, K), None, dtA, dtB)
    m_a, _ = _mask_of("mask,64x72", A, B, dtC, 64, 72, K, p, seed, bias72)
    A9, B9, _acc = _operands((512, 9, K), None, dtA, dtB)
    m_b, _ = _mask_of("mask,512x9", A9, B9, dtC, 512, 9, K, p, seed, bias9)
    assert torch.equal(m_a.reshape(-1), m_b.reshape(-1)) and torch.equal(m_a.reshape(-1), _host_mask(seed, 4608, p))
    Ab, Bb, _acc = _operands((64, 72, K), (4, 16), dtA, dtB)            # 64 batch products of (64, 72) ...
    m_z, _ = _mask_of("mask,64x(64x72)", Ab, Bb, dtC, 64, 72, K, p, seed, bias72, outer=(4, 16))
    At, Bt, _acc = _operands((64 * 64, 72, K), None, dtA, dtB)          # ... against one (4096, 72) launch
    m_t, _ = _mask_of("mask,4096x72", At, Bt, dtC, 4096, 72, K, p, seed, bias72)
    assert torch.equal(m_z.reshape(-1), m_t.reshape(-1))


# ================================================================================================ e. split-K
@pytest.mark.parametrize("K,split", [(1000, 1), (1000, 2), (1000, 3), (1000, 4), (1000, 8), (136, 8)])
@pytest.mark.parametrize("triple", ["bf16_f32", "mix_ga_f32", "fp16_f32", "f32_fast", "f32_precise"])
def test_split_k(triple, K, split):
    """C (non-zero) += alpha A B in the weight-gradient layout (0, 0).  K = 1000: splits 2, 4 and 8 take the slice-major workgroup order, 1
    and 3 the row-panel order; K = 136 with 8 requested slices runs 3, the last one ragged.  For the triples with a bf16 A - the only ones
    hip.gemm defers - the partials-only form (C = NULL inside splitk_batched(), folded by sarssl_splitk_reduce_multi) is bit-equal to the
    direct call."""
    hip = _hip()
    name, dtA, dtB, dtC, precise = TRIPLE[triple]
    M, N = 136, 72
    A, B, acc = _operands((M, N, K), None, dtA, dtB, precise)
    At, Bt = _lay(A, False), _lay(B, False)
    C0 = _rand((M, N), F32, 9)
    ldc = N + XCOL
    case = "splitk,%dx%dx%d,s%d" % (M, N, K, split)
    per = -(-(-(-K // split)) // 64) * 64
    assert -(-K // per) == {(1000, 1): 1, (1000, 2): 2, (1000, 3): 3, (1000, 4): 4, (1000, 8): 8, (136, 8): 3}[(K, split)]
    Cv, Cb = _window((), M, N, F32, ldc, C0)
    hip.gemm(At, Bt, a_kc=False, b_kc=False, M=M, N=N, K=K, lda=M, ldb=N, out=Cv, ldc=ldc, alpha=0.5, split_k=split, precise=precise)
    assert _outside_unchanged(Cb, M, N)
    _chk("splitk", triple, case, Cv, refs.accumulate(C0, acc, 0.5), L=K + 1)
    if dtA == BF16:                                     # only a bf16 A defers (hip.gemm): the other triples would take the direct path again
        Dv, Db = _window((), M, N, F32, ldc, C0)
        with hip.splitk_batched():
            hip.gemm(At, Bt, a_kc=False, b_kc=False, M=M, N=N, K=K, lda=M, ldb=N, out=Dv, ldc=ldc, alpha=0.5, split_k=split)
            assert torch.equal(Dv, C0)                  # partials only: nothing folded before the batch closes
        assert torch.equal(Dv, Cv) and _outside_unchanged(Db, M, N)


# ================================================================================================ f. pair products
def _pair_points():
    cols = _cus() // 16 + 1                           # 16 x cols 128 x 128 tiles: more than one per CU, K > 256 -> 128-row tiles
    return {"fm2_plain": (2048, 128 * cols, 320), "fm1_plain": (128, 128, 64), "fm2_ragged": (80, 96, 32), "fm1_ragged": (130, 64, 40)}


@pytest.mark.parametrize("point", ["fm2_plain", "fm1_plain", "fm2_ragged", "fm1_ragged"])
@pytest.mark.parametrize("dtC", [F16, F32], ids=["fp16", "f32"])
@pytest.mark.parametrize("nseg", [2, 3])
def test_pair_products(nseg, dtC, point):
    """gemm_seg_kernel<C, FM, EDGE, NSEG>: hi hi + hi lo [+ lo hi] on fp16 pairs with bias + Swish + saved pre-activation.  Weight scale
    0.03: the weights' lo halves are fp16 subnormals."""
    hip = _hip()
    M, N, K = _pair_points()[point]
    x, w, bias = _rand((M, K), F32, 41), _rand((N, K), F32, 42, scale=0.03), _rand((N,), F32, 5)
    xp, wp = hip.split_pair(x), hip.split_pair(w)
    ldc = N + XCOL
    case = "pair,%s,%dx%dx%d,nseg%d" % (point, M, N, K, nseg)
    Cv, Cb = _window((), M, N, dtC, ldc)
    Pv, Pb = _window((), M, N, dtC, ldc)
    hip.gemm_split(xp if nseg == 3 else xp.hi, wp.hi, wp.lo, M=M, N=N, K=K, out=Cv, ldc=ldc, bias=bias, act=2, preact=Pv)
    assert _outside_unchanged(Cb, M, N) and _outside_unchanged(Pb, M, N)
    (xh, xl), (wh, wl) = refs.split16(x, F16), refs.split16(w, F16)
    assert torch.equal(xp.hi.double(), xh) and torch.equal(wp.lo.double(), wl)
    want, pre = refs.epilogue(refs.pair_product(xh, xl if nseg == 3 else None, wh, wl), bias=bias, act=2)
    key = "fp16" if dtC == F16 else "f32"
    _chk("pair", key, case, Cv, want)
    _chk("pair", key, case + ".pre", Pv, pre)


# ================================================================================================ g. grouped weight gradient, fp16 X
def test_group_tn_fp16_x():
    """gemm_group_tn_kernel<f16>: two weight-gradient products dY^T X with saved fp16 activations X (re-encoded to bf16 while staged) in one
    launch, against the same products launched one by one (bit-equal: same tiles, same split, same fold order) and against f64; the
    bias gradients (column sums of dY) ride on the launch."""
    hip = _hip()
    K, split = 1024, 4
    items, sep, accs, dys = [], [], [], []
    for q, (M, N) in enumerate([(256, 128), (128, 384)]):
        dy, x = _rand((K, M), BF16, 50 + q, scale=0.1), _rand((K, N), F16, 60 + q)
        items.append((dy, x, torch.ones((M, N), dtype=F32, device=_dev()), split, torch.full((M,), 2.0, dtype=F32, device=_dev())))
        accs.append(refs.product(dy, x, a_kc=False, b_kc=False))
        o = torch.ones((M, N), dtype=F32, device=_dev())
        hip.gemm(dy, x, a_kc=False, b_kc=False, M=M, N=N, K=K, lda=M, ldb=N, out=o, ldc=N, split_k=split)
        sep.append(o)
    with hip.splitk_batched():
        assert hip.gemm_group_tn(items), "the grouped kernel did not launch"
    for q, ((dy, x, out, _s, bias_out), o, acc) in enumerate(zip(items, sep, accs)):
        assert torch.equal(out, o)
        _chk("splitk", "mix_ga_f32", "group_tn,q%d" % q, out, 1.0 + acc, L=K + 1)
        _chk("splitk", "mix_ga_f32", "group_tn,q%d,colsum" % q, bias_out, 2.0 + dy.double().sum(0), L=K + 1)
