"""GPU: the stem's two 3x3 weight gradients with the BatchNorm backward of their dy operand formed by the staging waves
(hip.conv3x3_wgrad_c4 / hip.conv3x3_wgrad_c1_apply) against the streaming pass + plain weight gradient they replace.  Both sides share
their arithmetic (csrc/common.h: bn_bwd_apply_relu / stem_c4_bwd_apply), so everything is compared with torch.equal; one f64
restatement per launch keeps the comparison from being the library against itself only."""
import random

import pytest
import torch

from conftest import check

pytestmark = pytest.mark.gpu

# (B, F, T, workgroups): full tiles in one round | F % 8 != 0 and T % 32 != 0 | ragged last column tile, several tiles per image |
# 32 tiles on 8 workgroups = four rounds (the two-tiles-ahead prefetch and both LDS buffers)
SHAPES = [(2, 16, 32, 0), (1, 12, 48, 0), (1, 24, 136, 0), (1, 32, 256, 8)]
SENTINEL = 12345.0


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def _aff(g):
    """(4, 64) scale | shift | mean | rstd with scales of both signs and one zero (every branch of the ReLU threshold)."""
    sc = torch.rand(64, generator=g) + 0.5
    sc[5:9] *= -1.0
    sc[17] = 0.0
    return torch.stack([sc, torch.randn(64, generator=g) * 0.3, torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5]).contiguous()


def _padded(t, T):
    """Copy of the (B,F,T,64) tensor at the head of a buffer whose tail (8 image rows and a bit) holds a sentinel: a store for a
    position below the last image row would land there.  -> (view, tail)"""
    n = t.numel()
    buf = torch.full((n + (8 * T + 64) * 64,), SENTINEL, dtype=t.dtype, device=t.device)
    buf[:n] = t.reshape(-1)
    return buf[:n].view(t.shape), buf[n:]


def _c4_inputs(B, F, T, ydt, seed):
    dev, g = _dev(), torch.Generator().manual_seed(seed)
    y3 = torch.randn((B, F, T, 64), generator=g).to(ydt).to(dev)
    y2 = torch.randn((B, F, T, 64), generator=g).to(ydt).to(dev)
    dy4 = torch.randn((B, T, F, 4), generator=g).to(torch.bfloat16).to(dev)
    W4 = (torch.randn((4, 64), generator=g) * 0.2).to(dev)
    aff3, aff2 = _aff(g).to(dev), _aff(g).to(dev)
    acc0 = torch.randn((64, 64, 3, 3), generator=g).to(dev)
    pg0 = [torch.randn(s, generator=g).to(dev) for s in ((4, 64), (64,), (64,))]
    return y3, y2, dy4, W4, aff3, aff2, acc0, pg0


def _apply_inputs(B, F, T, ydt, seed):
    dev, g = _dev(), torch.Generator().manual_seed(seed)
    dz = torch.randn((B, F, T, 64), generator=g).to(torch.bfloat16).to(dev)
    y = torch.randn((B, F, T, 64), generator=g).to(ydt).to(dev)
    a0 = torch.randn((B, F, T, 4), generator=g).to(ydt).to(dev)
    W1 = (torch.randn((64, 4), generator=g) * 0.5).to(dev)
    aff, aff1 = _aff(g).to(dev), _aff(g).to(dev)
    acc0 = torch.randn((64, 64, 3, 3), generator=g).to(dev)
    pg0 = [torch.randn(64, generator=g).to(dev) for _ in range(2)]
    return dz, y, a0, W1, aff, aff1, acc0, pg0


@pytest.mark.parametrize("use_stats", [1, 0])
@pytest.mark.parametrize("ydt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,F,T,cus", SHAPES)
def test_wgrad_c4_equals_the_apply_pass_plus_the_plain_weight_gradient(B, F, T, cus, ydt, use_stats):
    from sar_ssl_amd import hip
    y3, y2, dy4, W4, aff3, aff2, acc0, pg0 = _c4_inputs(B, F, T, ydt, 31 + F)
    hip.conv_cus_override(cus)
    try:
        pg_ref = [p.clone() for p in pg0]
        dy3_ref, red = hip.stem_c4_bwd_two_phase(y3, dy4, W4, aff3, bool(use_stats), pgrads=tuple(pg_ref))
        acc_ref = acc0.clone()
        assert hip.conv3x3_wgrad(dy3_ref, y2, aff2[0], aff2[1], acc_into=acc_ref) is None
        pg, acc = [p.clone() for p in pg0], acc0.clone()
        out, tail = _padded(torch.zeros_like(dy3_ref), T)
        dy3 = hip.conv3x3_wgrad_c4(y3, dy4, W4, aff3, bool(use_stats), red, y2, aff2[0], aff2[1], acc, out=out, pgrads=tuple(pg))
        torch.cuda.synchronize()
    finally:
        hip.conv_cus_override(0)
    assert dy3.data_ptr() == out.data_ptr() and torch.equal(dy3, dy3_ref)
    assert bool((tail == SENTINEL).all())                    # nothing stored for out-of-image positions
    assert torch.equal(acc, acc_ref) and not torch.equal(acc, acc0)
    for a, b in zip(pg, pg_ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("use_stats", [1, 0])
@pytest.mark.parametrize("ydt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,F,T,cus", SHAPES)
def test_wgrad_c1_apply_equals_the_apply_pass_plus_the_first_layer_weight_gradient(B, F, T, cus, ydt, use_stats, alias):
    from sar_ssl_amd import hip
    dz, y, a0, W1, aff, aff1, acc0, pg0 = _apply_inputs(B, F, T, ydt, 57 + F)
    red = hip.cl_bn_bwd_reduce(dz, y, 64, aff, 1)
    hip.conv_cus_override(cus)
    try:
        pg_ref, acc_ref = [p.clone() for p in pg0], acc0.clone()
        dy_ref = hip.cl_bn_bwd_apply(dz, y, 64, aff, 1, False, bool(use_stats), red, out=torch.empty_like(dz), pgrads=tuple(pg_ref))
        hip.conv3x3_wgrad_c1(dy_ref, a0, W1, aff1[0], aff1[1], acc_ref)
        pg, acc = [p.clone() for p in pg0], acc0.clone()
        # dy_out over dz itself (as the engine runs it) or a buffer of its own; either way with a sentinel tail behind it
        src, tail_src = _padded(dz, T)
        out, tail = (src, tail_src) if alias else _padded(torch.zeros_like(dz), T)
        dy = hip.conv3x3_wgrad_c1_apply(src, y, aff, bool(use_stats), red, a0, W1, aff1[0], aff1[1], acc, out=out, pgrads=tuple(pg))
        torch.cuda.synchronize()
    finally:
        hip.conv_cus_override(0)
    assert dy.data_ptr() == out.data_ptr() and torch.equal(dy, dy_ref)
    assert bool((tail == SENTINEL).all()) and bool((tail_src == SENTINEL).all())      # nothing stored for out-of-image positions
    if not alias:
        assert torch.equal(src, dz)
    assert torch.equal(acc, acc_ref) and not torch.equal(acc, acc0)
    for a, b in zip(pg, pg_ref):
        assert torch.equal(a, b)


def _wgrad64(dy_cl, z_cl):
    """f64 weight gradient (64,64,3,3) of a 3x3 / pad 1 convolution from channels-last dy and input z."""
    z = z_cl.permute(0, 3, 1, 2).double().requires_grad_(False)
    W = torch.zeros((64, 64, 3, 3), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(z, W, padding=1).backward(dy_cl.permute(0, 3, 1, 2).double())
    return W.grad


def _bn_bwd64(g, y, aff, use_stats):
    """sc * (g - mean(g) - xhat * mean(g * xhat)) over the pixels, f64 (sc = gamma * rstd)."""
    sc, mu, rs = aff[0].double(), aff[2].double(), aff[3].double()
    xhat = (y - mu) * rs
    if not use_stats:
        return sc * g
    n = g.numel() // 64
    m1, m2 = g.reshape(n, 64).sum(0) / n, (g * xhat).reshape(n, 64).sum(0) / n
    return sc * (g - m1 - xhat * m2)


def test_new_weight_gradients_against_an_f64_restatement():
    """Bound: the one test_conv3x3_wgrad_and_dgrad applies to the same quantity (1e-2 of the largest element; bf16 operands)."""
    from sar_ssl_amd import hip
    B, F, T = 1, 24, 136
    ydt = torch.float16
    # second convolution: dy3 from (y3, dy4)
    y3, y2, dy4, W4, aff3, aff2, acc0, _ = _c4_inputs(B, F, T, ydt, 77)
    red = hip.stem_c4_bwd_sums(y3, dy4, W4, aff3)
    acc = acc0.clone()
    hip.conv3x3_wgrad_c4(y3, dy4, W4, aff3, True, red, y2, aff2[0], aff2[1], acc)
    y3d, a3, a2 = y3.double().cpu(), aff3.double().cpu(), aff2.double().cpu()
    g = dy4.double().cpu().permute(0, 2, 1, 3) @ W4.double().cpu()                  # (B,F,T,64)
    g = g * ((y3d * a3[0] + a3[1]) > 0)
    dy3 = _bn_bwd64(g, y3d, a3, True)
    z2 = torch.relu(y2.double().cpu() * a2[0] + a2[1]).to(torch.bfloat16).double()    # the operand the kernel contracts with
    check("wgrad_c4.vs_f64", _relerr(acc, acc0.double().cpu() + _wgrad64(dy3, z2)), 1e-2)
    # first convolution: dy2 from (dz2, y2), input operand from a0
    dz, y, a0, W1, aff, aff1, acc0, _ = _apply_inputs(B, F, T, ydt, 78)
    red = hip.cl_bn_bwd_reduce(dz, y, 64, aff, 1)
    acc = acc0.clone()
    hip.conv3x3_wgrad_c1_apply(dz, y, aff, True, red, a0, W1, aff1[0], aff1[1], acc)
    yd, a, a1 = y.double().cpu(), aff.double().cpu(), aff1.double().cpu()
    g = dz.double().cpu() * ((yd * a[0] + a[1]) > 0)
    dy2 = _bn_bwd64(g, yd, a, True)
    z1 = torch.relu((a0.double().cpu() @ W1.double().cpu().t()) * a1[0] + a1[1]).to(torch.bfloat16).double()
    check("wgrad_c1_apply.vs_f64", _relerr(acc, acc0.double().cpu() + _wgrad64(dy2, z1)), 1e-2)


@pytest.mark.parametrize("prec", ["hybrid", "fp16", "bf16"])
def test_three_adam_steps_are_the_same_bits_with_and_without_the_fused_weight_gradients(prec, monkeypatch):
    from sar_ssl_amd import engine, hip, model, runtime, synth
    dev = _dev()
    B, T = 2, 16
    runtime.set_precision(prec)
    try:
        sig = torch.from_numpy(synth.make_batch(3, 3 * B, nsample=512 + 256 * (T - 1))).cuda()
        xs = [hip.stft_frontend(sig[i * B:(i + 1) * B]) for i in range(3)]
        calls = []
        for name in ("conv3x3_wgrad_c4", "conv3x3_wgrad_c1_apply"):
            monkeypatch.setattr(hip, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(hip, name), name))

        def run(on):
            monkeypatch.setattr(engine, "_WGRAD_FUSE_C4", on)
            monkeypatch.setattr(engine, "_WGRAD_FUSE_APPLY", on)
            del calls[:]
            torch.manual_seed(11)
            net = model.SARSSL(sig_shape=(256, T, 2, 2), pretrain=True, device=dev)
            for m in net.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
            net.to(dev).train()
            flat = runtime.FlatParams(net)
            opt = runtime.FusedAdam(flat, lr=1e-3)
            opt.zero_grad()
            random.seed(77)
            out = []
            for x in xs:
                loss, _, _ = net(x)
                loss.backward()
                grad = flat.grad.clone()
                opt.step()
                opt.zero_grad()
                out.append((loss.detach().clone(), grad, flat.flat.clone()))
            return out, list(calls)

        ref, ncalls_off = run(False)
        got, ncalls_on = run(True)
        assert not ncalls_off and ncalls_on.count("conv3x3_wgrad_c4") == ncalls_on.count("conv3x3_wgrad_c1_apply") >= 3      # every step took them
        for step, (r, g) in enumerate(zip(ref, got)):
            for what, a, b in zip(("loss", "gradients", "parameters"), r, g):
                assert torch.equal(a, b), "step %d: %s differ" % (step, what)
    finally:
        runtime.set_precision("bf16")
