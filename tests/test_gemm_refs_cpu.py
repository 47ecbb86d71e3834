"""tests/gemm_refs.py - the f64 restatement tests/test_gpu_gemm.py holds the GEMM kernels to - against torch.nn.functional and autograd in
f64.  No GPU."""
import numpy as np
import pytest
import torch

import gemm_refs as refs

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("act", [1, 2])
def test_linear_activation_forward_is_torch_functional(act):
    g = _g(act)
    x, w, b = torch.randn(37, 24, generator=g).to(BF16), torch.randn(19, 24, generator=g).to(BF16), torch.randn(19, generator=g)
    r = torch.randn(37, 19, generator=g)
    F = torch.nn.functional
    h = F.linear(x.double(), w.double(), b.double())
    want = 0.5 * (F.relu(h) if act == 1 else F.silu(h)) + 0.25 * r.double()
    for a_kc, b_kc in [(True, True), (True, False), (False, True), (False, False)]:
        A = x if a_kc else x.t().contiguous()
        B = w if b_kc else w.t().contiguous()
        y, pre = refs.epilogue(refs.product(A, B, a_kc, b_kc), bias=b, act=act, out_scale=0.5, resid=r, res_scale=0.25)
        assert _rel(pre, h) < 1e-15 and _rel(y, want) < 1e-15
    # alpha scales the product, not the bias
    y, pre = refs.epilogue(refs.product(x, w), alpha=0.5, bias=b)
    assert _rel(pre, 0.5 * (x.double() @ w.double().t()) + b.double()) < 1e-15 and torch.equal(y, pre)


@pytest.mark.parametrize("aux_act", [1, 2])
def test_activation_backward_factor_is_autograd(aux_act):
    g = _g(10 + aux_act)
    h = torch.randn(33, 40, generator=g).double().requires_grad_(True)
    dy = torch.randn(33, 40, generator=g).double()
    F = torch.nn.functional
    (F.relu(h) if aux_act == 1 else F.silu(h)).backward(dy)
    got, _ = refs.epilogue(dy, aux=h.detach(), aux_act=aux_act)
    assert _rel(got, h.grad) < 1e-15
    # the factor reads aux as stored: an fp16 pre-activation is used at its fp16 value
    h16 = h.detach().to(F16)
    got16, _ = refs.epilogue(dy, aux=h16, aux_act=aux_act)
    want = dy * ((h16.double() > 0).double() if aux_act == 1 else refs.swish_grad(h16.double()))
    assert torch.equal(got16, want)


def test_operand_staging():
    g = _g(3)
    a, b = torch.randn(16, 32, generator=g), torch.randn(24, 32, generator=g)
    plain = a.double() @ b.double().t()
    # mixed pairing: the fp16 operand enters re-encoded to bf16, the bf16 one as stored
    a_bf, b_fp = a.to(BF16), b.to(F16)
    assert torch.equal(refs.product(a_bf, b_fp), a_bf.double() @ b_fp.to(BF16).double().t())
    assert torch.equal(refs.product(b_fp, a_bf), b_fp.to(BF16).double() @ a_bf.double().t())
    assert not torch.equal(refs.product(a_bf, b_fp), a_bf.double() @ b_fp.double().t())
    # fp16 x fp16 and bf16 x bf16: as stored
    assert torch.equal(refs.product(a.to(F16), b.to(F16)), a.to(F16).double() @ b.to(F16).double().t())
    # f32 fast: both rounded to bf16; f32 precise: hi hi + hi lo + lo hi, 2^-16 per product
    assert torch.equal(refs.product(a, b), a.to(BF16).double() @ b.to(BF16).double().t())
    e = _rel(refs.product(a, b, precise=True), plain)
    assert 0 < e < 2.0 ** -14
    # batch forms: leading dimensions pair up, or every A against every B
    A3, B3 = torch.randn(3, 16, 32, generator=g).to(BF16), torch.randn(2, 24, 32, generator=g).to(BF16)
    o = refs.product(A3, B3, outer=True)
    assert o.shape == (3, 2, 16, 24) and torch.equal(o[2, 1], refs.product(A3[2], B3[1]))


def test_pair_product_is_the_f64_product_to_2_pow_minus_20():
    g = _g(4)
    x, w = torch.randn(64, 96, generator=g), torch.randn(48, 96, generator=g) * 0.03
    (xh, xl), (wh, wl) = refs.split16(x, F16), refs.split16(w, F16)
    plain = x.double() @ w.double().t()
    e3 = _rel(refs.pair_product(xh, xl, wh, wl), plain)
    e2 = _rel(refs.pair_product(xh, None, wh, wl), xh @ w.double().t())
    e1 = _rel(refs.pair_product(xh, None, wh, None), plain)
    assert e3 < 2.0 ** -20 and e2 < 2.0 ** -20 and e1 > 2.0 ** -14, (e3, e2, e1)
    # what is left out is the lo lo term (and the pairs' own 2^-22 rounding)
    full = (xh + xl) @ (wh + wl).t()
    assert _rel(refs.pair_product(xh, xl, wh, wl) + xl @ wl.t(), full) < 1e-15


def test_shift_is_pad_and_reshape():
    """refs.shift against RelativeMultiHeadAttention._relative_shift's pad-and-reshape (tests/test_gpu_kernels.py _ref_shift): equal wherever
    the kernel stores; what it does not store are the elements (i, i + 1), where the reshape puts the pad's zeros."""
    g = _g(5)
    for T in (1, 2, 8, 13):
        R = torch.randn(2, 3, T, T, generator=g).double()
        padded = torch.cat([R.new_zeros(2, 3, T, 1), R], dim=-1).view(2, 3, T + 1, T)
        want = padded[:, :, 1:].reshape(2, 3, T, T)
        got, written = refs.shift(R)
        assert torch.equal(got, want)
        i = torch.arange(T)
        unwritten = torch.zeros(T, T, dtype=torch.bool)
        unwritten[i[:-1], i[:-1] + 1] = True
        assert torch.equal(~written, unwritten)


def test_dropout_and_accumulate_forms():
    g = _g(6)
    acc = torch.randn(8, 16, generator=g).double()
    keep = torch.from_numpy(refs.keep_mask(77, 128, 0.25)).view(8, 16)
    r = torch.randn(8, 16, generator=g)
    y, _ = refs.epilogue(acc, keep=keep, p=0.25, out_scale=0.5, resid=r)
    assert torch.equal(y[~keep], r.double()[~keep])                      # dropped elements are exactly the residual
    assert _rel(y[keep], (0.5 * acc / 0.75 + r.double())[keep]) < 1e-7      # (inv_keep is formed in f32)
    assert refs.inv_keep(0.25) == float(np.float32(4.0) / np.float32(3.0)) and refs.inv_keep(0.0) == 1.0
    c0 = torch.randn(8, 16, generator=g)
    assert torch.equal(refs.accumulate(c0, acc, 0.5), c0.double() + 0.5 * acc)


def test_keep_mask_properties():
    """Pure function of (seed, index): a prefix of a longer stream, another stream for another seed (either half), keep fraction inside
    five binomial standard deviations, threshold round(p 65536)."""
    n = 1 << 16
    m = refs.keep_mask(0x1234567887654321, n, 0.1)
    assert np.array_equal(m[:1001], refs.keep_mask(0x1234567887654321, 1001, 0.1))
    for other in (0x1234567887654322, 0x1234567987654321):
        assert (refs.keep_mask(other, n, 0.1) != m).mean() > 0.1
    for p in (0.1, 0.25, 0.5):
        k = refs.keep_mask(5, n, p)
        assert abs(k.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n)
    assert np.array_equal(refs.keep_mask(5, n, 0.1) | refs.keep_mask(5, n, 0.25), refs.keep_mask(5, n, 0.1))     # nested in p
