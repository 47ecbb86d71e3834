"""The two K-tile depths of the pair products (csrc/gemm.hip gemm_seg_kernel<C, FM, EDGE, NSEG, KB>, KB = 64 | 32; NOTES.md 20): forced through
sarssl_ctx_set_pair_kdepth, the depth-32 and the depth-64 results of one call are the same bits - a k-step is 16 wide at either depth and
its products keep their order hi hi, hi lo_B, lo_A hi - and each meets the f64 restatement of tests/gemm_refs.py within the bounds
tests/test_gpu_gemm.py applies to the pair products (parity.gemm_tol("pair", ...)).
Shapes: the smallest at which a K-tile depth can go wrong.  M = 64 (one tile), 96 (ragged against 64 and 128), 200 (two row panels of the
128-row tile / four of the 64-row tile, the last ragged); N = 128, 136; K = 32 (one 32-tile), 40 (a tail inside a 16-step), 64 (one
64-tile = two 32-tiles), 96 (an odd number of 32-tiles), 160 (2.5 64-tiles).  Tile height by the rule of launch_seg: M < 128 -> 128-row
tiles (FM = 2), M = 200 -> 64-row tiles (FM = 1); all of those are ragged (EDGE) instantiations, the plain ones are the two points of
test_gpu_gemm.py's _pair_points (FM = 2: a grid of more tiles than CUs, K = 320; FM = 1: (128, 128, 64)) and (128, 128, 96), plain at
depth 32 and ragged at depth 64.  Every case runs four epilogues: bias + Swish + saved pre-activation, bias + dropout (fixed seed) +
out_scale + residual, bias + ReLU, nothing."""
import random

import pytest
import torch

import gemm_refs as refs
from conftest import check

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
SENT = -1.75
PRE, POST, XCOL = 3, 2, 8
SEED, P = 0x5eed1234abcd, 0.25


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _rand(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(_dev())


def _window(M, N, dtype, ldc):
    buf = torch.full((PRE + M + POST, ldc), SENT, dtype=dtype, device=_dev())
    return buf[PRE:PRE + M, :N], buf


def _outside_unchanged(buf, M, N):
    chk = buf.clone()
    chk[PRE:PRE + M, :N] = SENT
    return bool((chk == SENT).all())


def _err(got, ref):
    return ((got.double() - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


class _depth:
    """``with _depth(32):`` - pair products issued inside run at that K-tile depth; the launcher's own rule afterwards."""

    def __init__(self, d):
        self.d = d

    def __enter__(self):
        from sar_ssl_amd import hip
        hip.pair_kdepth_override(self.d)

    def __exit__(self, *exc):
        from sar_ssl_amd import hip
        hip.pair_kdepth_override(0)
        return False


_ops = {}


def _operands(M, N, K, wide):
    """-> x pair, w pair (device, fp16 halves), f64 products for NSEG 3 and 2; cached, never modified.  wide: the fp16 halves are column
    windows [:, 8:8 + K] of buffers K + 24 wide (lda = ldb = K + 24 > K), filled with a value that would show if it were contracted."""
    key = (M, N, K, wide)
    if key not in _ops:
        from sar_ssl_amd import hip
        x, w = _rand((M, K), F32, 41 + M + K), _rand((N, K), F32, 42 + N + K, scale=0.03)     # (weight scale 0.03: lo halves are fp16 subnormals)
        xp, wp = hip.split_pair(x), hip.split_pair(w)
        (xh, xl), (wh, wl) = refs.split16(x, F16), refs.split16(w, F16)
        assert torch.equal(xp.hi.double(), xh) and torch.equal(xp.lo.double(), xl) and torch.equal(wp.hi.double(), wh) and torch.equal(wp.lo.double(), wl)
        if wide:
            def widen(t):
                b = torch.full((t.shape[0], K + 24), 3.0, dtype=F16, device=t.device)
                b[:, 8:8 + K] = t
                return b[:, 8:8 + K]
            xp, wp = hip.Pair(widen(xp.hi), widen(xp.lo)), hip.Pair(widen(wp.hi), widen(wp.lo))
        _ops[key] = (xp, wp, {3: refs.pair_product(xh, xl, wh, wl), 2: refs.pair_product(xh, None, wh, wl)})
    return _ops[key]


def _epilogues(M, N, dtC):
    bias, R = _rand((N,), F32, 5), _rand((M, N), dtC, 6)
    keep = torch.from_numpy(refs.keep_mask(SEED, M * N, P)).to(_dev()).view(M, N)
    #        name            kernel arguments                                                            restatement's arguments                      pre
    return [("swish_pre", dict(bias=bias, act=2), dict(bias=bias, act=2), True),
            ("drop_resid", dict(bias=bias, p_drop=P, seed=SEED, out_scale=0.5, resid=R, ldr=N, res_scale=0.75),
             dict(bias=bias, keep=keep, p=P, out_scale=0.5, resid=R, res_scale=0.75), False),
            ("relu", dict(bias=bias, act=1), dict(bias=bias, act=1), False),
            ("plain", dict(), dict(), False)]


def _case(M, N, K, nseg, dtC, wide=False):
    from sar_ssl_amd import hip
    xp, wp, acc = _operands(M, N, K, wide)
    A = xp if nseg == 3 else xp.hi
    assert (A.hi if nseg == 3 else A).stride(0) == (K + 24 if wide else K)
    key = "fp16" if dtC == F16 else "f32"
    from sar_ssl_amd import parity
    tol = parity.gemm_tol("pair", key)
    ldc = N + XCOL
    for name, kw, rk, want_pre in _epilogues(M, N, dtC):
        got = {}
        for depth in (32, 64):
            Cv, Cb = _window(M, N, dtC, ldc)
            Pv, Pb = _window(M, N, dtC, ldc) if want_pre else (None, None)
            with _depth(depth):
                hip.gemm_split(A, wp.hi, wp.lo, M=M, N=N, K=K, out=Cv, ldc=ldc, preact=Pv, **kw)
            assert _outside_unchanged(Cb, M, N) and (Pb is None or _outside_unchanged(Pb, M, N)), (name, depth)
            got[depth] = (Cv, Pv)
        tag = "pair_bk[%dx%dx%d,nseg%d,%s%s,%s]" % (M, N, K, nseg, key, ",wide" if wide else "", name)
        C32, C64 = got[32][0], got[64][0]
        assert torch.equal(C32, C64), tag + ": depth 32 and depth 64 differ"
        assert bool((C32 != 0).any()) and bool(torch.isfinite(C32).all()), tag
        want, pre = refs.epilogue(acc[nseg], **rk)
        for depth in (32, 64):
            check("gemm.%s.d%d" % (tag, depth), _err(got[depth][0], want), tol)
        if want_pre:
            assert torch.equal(got[32][1], got[64][1]) and bool((got[32][1] != 0).any()), tag + ".pre"
            for depth in (32, 64):
                check("gemm.%s.pre.d%d" % (tag, depth), _err(got[depth][1], pre), tol)


@pytest.mark.parametrize("K", [32, 40, 64, 96, 160])
@pytest.mark.parametrize("N", [128, 136])
@pytest.mark.parametrize("M", [64, 96, 200])
@pytest.mark.parametrize("dtC", [F16, F32], ids=["fp16", "f32"])
@pytest.mark.parametrize("nseg", [2, 3])
def test_depths_agree_ragged(nseg, dtC, M, N, K):
    """EDGE instantiations: FM = 2 (M = 64, 96) and FM = 1 (M = 200)."""
    _case(M, N, K, nseg, dtC)


def _plain_points():
    cols = torch.cuda.get_device_properties(0).multi_processor_count // 16 + 1      # 16 x cols 128 x 128 tiles: more than one per CU, K > 256 -> FM = 2
    return {"fm2_plain": (2048, 128 * cols, 320), "fm1_plain": (128, 128, 64), "fm1_plain32_ragged64": (128, 128, 96)}


@pytest.mark.parametrize("point", ["fm2_plain", "fm1_plain", "fm1_plain32_ragged64"])
@pytest.mark.parametrize("dtC", [F16, F32], ids=["fp16", "f32"])
@pytest.mark.parametrize("nseg", [2, 3])
def test_depths_agree_plain(nseg, dtC, point):
    """Plain instantiations (the residual-row prefetch of the fp16 epilogue included): FM = 2 and FM = 1."""
    M, N, K = _plain_points()[point]
    _case(M, N, K, nseg, dtC)


@pytest.mark.parametrize("dtC", [F16, F32], ids=["fp16", "f32"])
@pytest.mark.parametrize("nseg", [2, 3])
@pytest.mark.parametrize("M,N,K", [(96, 136, 40), (200, 128, 96), (128, 128, 64)])
def test_depths_agree_on_views_into_wider_buffers(M, N, K, nseg, dtC):
    """lda = ldb = K + 24 > K, the operands starting 8 elements into their rows (the q / k / v and decoder-input operands are such views)."""
    _case(M, N, K, nseg, dtC, wide=True)


def test_the_setter_refuses_other_depths():
    from sar_ssl_amd import hip, _lib
    for bad in (16, 48, 128, -32):
        with pytest.raises(_lib.SarsslHipError):
            hip.pair_kdepth_override(bad)
    hip.pair_kdepth_override(0)


def test_three_adam_steps_are_the_same_bits_at_either_depth(monkeypatch):
    """B = 2, T = 16, hybrid, dropout on: loss, flat gradients and flat parameters after each of three Adam steps."""
    from sar_ssl_amd import hip, model, runtime, synth
    dev = _dev()
    B, T = 2, 16
    runtime.set_precision("hybrid")
    try:
        sig = torch.from_numpy(synth.make_batch(3, 3 * B, nsample=512 + 256 * (T - 1))).cuda()
        xs = [hip.stft_frontend(sig[i * B:(i + 1) * B]) for i in range(3)]
        pairs = []
        real = hip.gemm_split
        monkeypatch.setattr(hip, "gemm_split", lambda A, B_, B_lo, **k: (pairs.append(B_lo is not None), real(A, B_, B_lo, **k))[1])

        def run(depth):
            del pairs[:]
            torch.manual_seed(11)
            random.seed(77)
            runtime.RT.manual_seed(1234)
            net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=True, device=dev).to(dev).train()
            flat = runtime.FlatParams(net)
            opt = runtime.FusedAdam(flat, lr=1e-3)
            opt.zero_grad()
            out = []
            with _depth(depth):
                for x in xs:
                    loss, _, _ = net(x)
                    loss.backward()
                    grad = flat.grad.clone()
                    opt.step()
                    opt.zero_grad()
                    out.append((loss.detach().clone(), grad, flat.flat.clone()))
            return out, sum(pairs)

        ref, n64 = run(64)
        got, n32 = run(32)
        assert n64 == n32 >= 3                                  # every step launched pair products
        for step, (r, g) in enumerate(zip(ref, got)):
            assert bool(torch.isfinite(r[0])) and bool((r[1] != 0).any())
            for what, a, b in zip(("loss", "gradients", "parameters"), r, g):
                assert torch.equal(a, b), "step %d: %s differ" % (step, what)
    finally:
        runtime.set_precision("bf16")
