"""f64 restatements of the row / elementwise kernels (csrc/elementwise.hip, csrc/dwconv.hip, csrc/head.hip and the small relayout /
affine kernels of csrc/stem.hip, csrc/conv3x3.hip), each written from the formula in the kernel's header comment.

Plain torch on the CPU; nothing here calls the library.  Every function takes f64 tensors holding the operands AS STORED (the caller
rounds to the storage dtype first and passes the f64 view of that) and returns f64.  tests/test_rowkernel_refs_cpu.py proves them
against torch autograd / torch.nn.functional before tests/test_gpu_rowkernels.py holds a kernel to them.
"""
import torch

DWK = 31          # depthwise-conv taps, padding 15


# ---- LayerNorm: y = (x - mean) * rstd * gamma + beta, statistics per row
def layernorm_fwd(x, gamma, beta, eps):
    """-> (y, mean [M], rstd [M])."""
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, resid=None):
    """dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)) (+ resid); dgamma = sum dy*xhat; dbeta = sum dy, with the SAVED mean and
    rstd of the forward pass -> (dx, dgamma, dbeta)."""
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if resid is not None:
        dx = dx + resid
    return dx, (dy * xhat).sum(0), dy.sum(0)


# ---- GLU over the last axis: h = [a | b] -> a * sigmoid(b)
def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def glu_fwd(h):
    d = h.shape[-1] // 2
    return h[..., :d] * sigmoid(h[..., d:])


def glu_bwd(dg, h):
    """dh = [dg * s | dg * a * s * (1 - s)], s = sigmoid(b)."""
    d = h.shape[-1] // 2
    a, s = h[..., :d], sigmoid(h[..., d:])
    return torch.cat([dg * s, dg * a * s * (1.0 - s)], -1)


# ---- depthwise conv over frames, k = 31, pad 15: x (B, T, d), w (d, 31)
def _windows(x):
    """(B, T, d) -> (B, T, d, 31): win[b][t][c][k] = x[b][t + k - 15][c], zero outside [0, T)."""
    xp = torch.nn.functional.pad(x, (0, 0, DWK // 2, DWK // 2))
    return xp.unfold(1, DWK, 1)


def dwconv_fwd(x, w):
    """y[b][t][c] = sum_k w[c][k] * x[b][t + k - 15][c]."""
    return (_windows(x) * w).sum(-1)


def dwconv_dgrad(dy, w):
    """dx[b][t][c] = sum_k w[c][30 - k] * dy[b][t + k - 15][c] (the same sum with flipped taps)."""
    return (_windows(dy) * w.flip(-1)).sum(-1)


def dwconv_wgrad(dy, x):
    """dw[c][k] = sum_{b,t} dy[b][t][c] * x[b][t + k - 15][c]."""
    return torch.einsum("btc,btck->ck", dy, _windows(x))


def _ident(t):
    return t


def dwglu_fwd(h, w, stored=_ident):
    """h (B, T, 2d) -> conv of g = GLU(h) `stored`: the fused kernels take g as the unfused path would read it back from storage
    (csrc/dwconv.hip as_stored), `stored` rounds an f64 tensor to that dtype and back (identity for f32)."""
    return dwconv_fwd(stored(glu_fwd(h)), w)


def dwglu_bwd(dc, h, w):
    """dh = GLU backward of the flipped-tap convolution of dc."""
    return glu_bwd(dwconv_dgrad(dc, w), h)


def dwglu_wgrad(dc, h, stored=_ident):
    return dwconv_wgrad(dc, stored(glu_fwd(h)))


# ---- relative shift (conformer/attention.py:105-113) on (..., T, T)
def shift(pos):
    """out[i][j] = pos[i][T-1-i+j] (j <= i), 0 (j == i+1), pos[i+1][j-i-2] (j >= i+2)."""
    T = pos.shape[-1]
    i = torch.arange(T)[:, None].expand(T, T)
    j = torch.arange(T)[None, :].expand(T, T)
    low = j <= i
    zero = j == i + 1
    row = torch.where(low, i, (i + 1).clamp(max=T - 1))
    col = torch.where(low, T - 1 - i + j, (j - i - 2).clamp(min=0))
    out = pos[..., row, col]
    return torch.where(zero, torch.zeros((), dtype=pos.dtype), out)


def shift_bwd(ds):
    """The adjoint: dpos[r][m] = ds[r][m-T+1+r] (m >= T-1-r), ds[r-1][m+r+1] (r >= 1 and m <= T-2-r), else 0 - the column j == i+1 of ds
    is never read."""
    T = ds.shape[-1]
    r = torch.arange(T)[:, None].expand(T, T)
    m = torch.arange(T)[None, :].expand(T, T)
    same = m >= T - 1 - r
    prev = (~same) & (r >= 1) & (m <= T - 2 - r)
    row = torch.where(same, r, (r - 1).clamp(min=0))
    col = torch.where(same, m - T + 1 + r, (m + r + 1).clamp(max=T - 1))
    out = ds[..., row, col]
    return torch.where(same | prev, out, torch.zeros((), dtype=ds.dtype))


# ---- softmax over the last axis of (content + shift(pos)) * scale
def softmax_relshift_fwd(content, pos, scale):
    s = (content + shift(pos)) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


def softmax_bwd(dp, p, scale):
    """dscore = scale * p * (dp - sum_j dp*p): the gradient w.r.t. content + shift(pos)."""
    return scale * p * (dp - (dp * p).sum(-1, keepdim=True))


# ---- activation derivatives
def swish_grad(h):
    """d/dh h * sigmoid(h) = s * (1 + h * (1 - s))."""
    s = sigmoid(h)
    return s * (1.0 + h * (1.0 - s))


def relu_grad(h):
    """1 where h > 0 (0 at +0 and -0)."""
    return (h > 0).to(h.dtype)


def colsum(x):
    return x.sum(0)


# ---- BatchNorm in eval mode as a per-channel affine map
def bn_eval_affine(gamma, beta, running_mean, running_var, eps):
    """-> (scale, shift, mean, rstd): y = x * scale + shift."""
    rstd = 1.0 / torch.sqrt(running_var + eps)
    return gamma * rstd, beta - running_mean * gamma * rstd, running_mean.clone(), rstd


# ---- weight relayouts (pure moves)
def patch_w(W):
    """(d, 4, F, 1) -> [d][f * 4 + c]."""
    d, C, F, _ = W.shape
    out = W.new_empty((d, F * C))
    for f in range(F):
        for c in range(C):
            out[:, f * C + c] = W[:, c, f, 0]
    return out


def conv_taps(W):
    """(co, ci, 3, 3) -> (fwd [9][co][ci] with tap = kh * 3 + kw, dgrad [9][ci][co] with flipped taps: dgrad[tap][ci][co] =
    W[co][ci][2 - kh][2 - kw])."""
    co, ci = W.shape[:2]
    fwd = W.new_empty((9, co, ci))
    dgr = W.new_empty((9, ci, co))
    for kh in range(3):
        for kw in range(3):
            fwd[kh * 3 + kw] = W[:, :, kh, kw]
            dgr[kh * 3 + kw] = W[:, :, 2 - kh, 2 - kw].t()
    return fwd, dgr


# ---- downstream heads
def mean_rows(x):
    """(B, T, d) -> (B, d)."""
    return x.sum(1) / x.shape[1]


def mean_rows_bwd(dy, T):
    return (dy / T)[:, None, :].expand(dy.shape[0], T, dy.shape[1])


def small_linear_fwd(x, W, bias, act):
    y = x @ W.t()
    if bias is not None:
        y = y + bias
    return y.clamp(min=0) if act == 1 else y


def small_linear_bwd(dy, y, x, W, act):
    """-> (dx, dW, db) with dz = dy (act 0) or dy * [y > 0] (act 1)."""
    dz = dy * (y > 0).to(dy.dtype) if act == 1 else dy
    return dz @ W, dz.t() @ x, dz.sum(0)
