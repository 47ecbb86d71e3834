"""The f64 restatements of tests/rowkernel_refs.py against torch autograd / torch.nn.functional in f64, to 1e-12: the references are
proved on the CPU before tests/test_gpu_rowkernels.py holds a kernel to them."""
import pytest
import torch
import torch.nn.functional as Fn

import rowkernel_refs as refs

TOL = 1e-12


def _close(got, want):
    got, want = got.double(), want.double()
    assert got.shape == want.shape
    err = float((got - want).abs().max() / (want.abs().max() + 1e-300))
    assert err < TOL, err


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


@pytest.mark.parametrize("M,d", [(3, 8), (17, 260)])
def test_layernorm(M, d):
    x = (_rand((M, d), 1, 1.5) + 0.3).requires_grad_(True)
    gamma = (_rand((d,), 2) * 0.3 + 1.0).requires_grad_(True)
    beta = _rand((d,), 3).requires_grad_(True)
    dy, resid = _rand((M, d), 4), _rand((M, d), 5)
    y, mean, rstd = refs.layernorm_fwd(x.detach(), gamma.detach(), beta.detach(), 1e-5)
    want = Fn.layer_norm(x, (d,), gamma, beta, 1e-5)
    _close(y, want.detach())
    _close(mean, x.detach().mean(-1))
    _close(rstd, 1.0 / torch.sqrt(x.detach().var(-1, unbiased=False) + 1e-5))
    want.backward(dy)
    dx, dg, db = refs.layernorm_bwd(dy, x.detach(), gamma.detach(), mean, rstd, resid)
    _close(dx, x.grad + resid)
    _close(dg, gamma.grad)
    _close(db, beta.grad)
    _close(refs.layernorm_bwd(dy, x.detach(), gamma.detach(), mean, rstd)[0], x.grad)


@pytest.mark.parametrize("M,d", [(2, 4), (9, 36)])
def test_glu(M, d):
    h = _rand((M, 2 * d), 6, 2.0).requires_grad_(True)
    dg = _rand((M, d), 7)
    want = Fn.glu(h, -1)
    _close(refs.glu_fwd(h.detach()), want.detach())
    want.backward(dg)
    _close(refs.glu_bwd(dg, h.detach()), h.grad)


@pytest.mark.parametrize("B,T,d", [(1, 5, 4), (2, 40, 12)])
def test_depthwise_conv(B, T, d):
    x = _rand((B, T, d), 8).requires_grad_(True)
    w = _rand((d, 31), 9, 0.2).requires_grad_(True)
    dy = _rand((B, T, d), 10)
    want = Fn.conv1d(x.transpose(1, 2), w.unsqueeze(1), None, padding=15, groups=d).transpose(1, 2)
    _close(refs.dwconv_fwd(x.detach(), w.detach()), want.detach())
    want.backward(dy)
    _close(refs.dwconv_dgrad(dy, w.detach()), x.grad)
    _close(refs.dwconv_wgrad(dy, x.detach()), w.grad)


@pytest.mark.parametrize("B,T,d", [(1, 7, 8), (2, 33, 16)])
def test_glu_then_depthwise_conv(B, T, d):
    h = _rand((B, T, 2 * d), 11).requires_grad_(True)
    w = _rand((d, 31), 12, 0.2).requires_grad_(True)
    dc = _rand((B, T, d), 13)
    want = Fn.conv1d(Fn.glu(h, -1).transpose(1, 2), w.unsqueeze(1), None, padding=15, groups=d).transpose(1, 2)
    _close(refs.dwglu_fwd(h.detach(), w.detach()), want.detach())
    want.backward(dc)
    _close(refs.dwglu_bwd(dc, h.detach(), w.detach()), h.grad)
    _close(refs.dwglu_wgrad(dc, h.detach()), w.grad)
    # `stored`: the convolution sees the GLU output through the rounding it is given
    bf = lambda t: t.to(torch.bfloat16).double()
    g = bf(Fn.glu(h.detach(), -1))
    _close(refs.dwglu_fwd(h.detach(), w.detach(), bf), refs.dwconv_fwd(g, w.detach()))
    _close(refs.dwglu_wgrad(dc, h.detach(), bf), refs.dwconv_wgrad(dc, g))


def _shift_by_reshape(pos):
    """conformer/attention.py:105-113: a zero column in front, viewed as (T + 1, T), first row dropped."""
    *lead, T, _ = pos.shape
    padded = torch.cat([pos.new_zeros(*lead, T, 1), pos], -1).view(*lead, T + 1, T)
    return padded[..., 1:, :].reshape(pos.shape)


@pytest.mark.parametrize("nmat,T", [(1, 1), (2, 2), (3, 9), (2, 16)])
def test_relative_shift_and_its_adjoint(nmat, T):
    P = _rand((nmat, T, T), 14).requires_grad_(True)
    D = _rand((nmat, T, T), 15)
    want = _shift_by_reshape(P)
    got = refs.shift(P.detach())
    assert torch.equal(got, want.detach())                               # a move: exact
    i = torch.arange(T - 1)
    if T > 1:
        assert float(got[:, i, i + 1].abs().max()) == 0.0                # the j == i + 1 column
    want.backward(D)
    assert torch.equal(refs.shift_bwd(D), P.grad)
    lhs, rhs = (got * D).sum(), (P.detach() * refs.shift_bwd(D)).sum()
    assert abs(float(lhs - rhs)) <= TOL * max(1.0, abs(float(lhs)))
    # the column j == i + 1 of D is never read
    D2 = D.clone()
    D2[:, i, i + 1] = 1e30
    assert torch.equal(refs.shift_bwd(D2), refs.shift_bwd(D))


@pytest.mark.parametrize("nmat,T", [(2, 5), (3, 70)])
def test_softmax_with_relative_shift(nmat, T):
    c = _rand((nmat, T, T), 16, 3.0).requires_grad_(True)
    pos = _rand((nmat, T, T), 17, 3.0).requires_grad_(True)
    dp = _rand((nmat, T, T), 18)
    want = torch.softmax((c + _shift_by_reshape(pos)) * 0.17, -1)
    p = refs.softmax_relshift_fwd(c.detach(), pos.detach(), 0.17)
    _close(p, want.detach())
    want.backward(dp)
    ds = refs.softmax_bwd(dp, p, 0.17)
    _close(ds, c.grad)
    _close(refs.shift_bwd(ds), pos.grad)


@pytest.mark.parametrize("n", [7, 300])
def test_activation_derivatives_and_column_sums(n):
    h = _rand((n,), 19, 2.0)
    h[0] = 0.0
    h[1] = -0.0
    hh = h.clone().requires_grad_(True)
    Fn.silu(hh).sum().backward()
    _close(refs.swish_grad(h), hh.grad)
    hr = h.clone().requires_grad_(True)
    torch.relu(hr).sum().backward()
    assert torch.equal(refs.relu_grad(h), hr.grad) and float(refs.relu_grad(h)[:2].abs().max()) == 0.0
    x = _rand((n, 12), 20)
    _close(refs.colsum(x), x.sum(0))


@pytest.mark.parametrize("C", [4, 64])
def test_batchnorm_eval_affine(C):
    gamma, beta, rm = _rand((C,), 21) * 0.3 + 1.0, _rand((C,), 22), _rand((C,), 23)
    rv = _rand((C,), 24).abs() + 0.1
    x = _rand((5, C, 3), 25)
    scale, shift, mean, rstd = refs.bn_eval_affine(gamma, beta, rm, rv, 1e-5)
    _close(x * scale[None, :, None] + shift[None, :, None], Fn.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5))
    _close(mean, rm)
    _close(rstd, 1.0 / torch.sqrt(rv + 1e-5))


@pytest.mark.parametrize("d,F", [(3, 2), (8, 5)])
def test_patch_weight_relayout(d, F):
    """The (d, 4, F, 1) convolution over (B, 4, F, T) equals the Linear with the relaid weight over (B, T, F * 4) rows."""
    W = _rand((d, 4, F, 1), 26)
    x = _rand((2, 4, F, 6), 27)
    want = Fn.conv2d(x, W)[:, :, 0, :]                                  # (B, d, T)
    rows = x.permute(0, 3, 2, 1).reshape(2, 6, F * 4)                   # [b][t][f * 4 + c]
    _close((rows @ refs.patch_w(W).t()).transpose(1, 2), want)
    assert torch.equal(refs.patch_w(W), W[..., 0].permute(0, 2, 1).reshape(d, F * 4))


@pytest.mark.parametrize("co,ci", [(2, 3), (64, 64)])
def test_3x3_tap_relayout(co, ci):
    W = _rand((co, ci, 3, 3), 28).requires_grad_(True)
    x = _rand((1, ci, 5, 6), 29).requires_grad_(True)
    dy = _rand((1, co, 5, 6), 30)
    want = Fn.conv2d(x, W, padding=1)
    fwd, dgr = refs.conv_taps(W.detach())
    xp = Fn.pad(x.detach(), (1, 1, 1, 1))
    y = sum(torch.einsum("oc,bchw->bohw", fwd[kh * 3 + kw], xp[:, :, kh:kh + 5, kw:kw + 6]) for kh in range(3) for kw in range(3))
    _close(y, want.detach())
    want.backward(dy)
    dyp = Fn.pad(dy, (1, 1, 1, 1))
    dx = sum(torch.einsum("co,bohw->bchw", dgr[kh * 3 + kw], dyp[:, :, kh:kh + 5, kw:kw + 6]) for kh in range(3) for kw in range(3))
    _close(dx, x.grad)
    assert torch.equal(dgr, W.detach().flip(2, 3).permute(2, 3, 1, 0).reshape(9, ci, co))


@pytest.mark.parametrize("B,T,d", [(1, 1, 4), (3, 37, 8)])
def test_mean_over_frames(B, T, d):
    x = _rand((B, T, d), 31).requires_grad_(True)
    dy = _rand((B, d), 32)
    want = x.mean(1)
    _close(refs.mean_rows(x.detach()), want.detach())
    want.backward(dy)
    _close(refs.mean_rows_bwd(dy, T), x.grad)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (5, 7, 20)])
def test_small_linear(M, N, K, act):
    x = _rand((M, K), 33).requires_grad_(True)
    W = _rand((N, K), 34).requires_grad_(True)
    b = _rand((N,), 35).requires_grad_(True)
    dy = _rand((M, N), 36)
    want = Fn.linear(x, W, b)
    if act == 1:
        want = torch.relu(want)
    y = refs.small_linear_fwd(x.detach(), W.detach(), b.detach(), act)
    _close(y, want.detach())
    want.backward(dy)
    dx, dW, db = refs.small_linear_bwd(dy, y, x.detach(), W.detach(), act)
    for got, ref in ((dx, x.grad), (dW, W.grad), (db, b.grad)):
        assert float((got - ref).abs().max()) <= TOL * max(1.0, float(ref.abs().max()))
    _close(refs.small_linear_fwd(x.detach(), W.detach(), None, 0), Fn.linear(x.detach(), W.detach()))
