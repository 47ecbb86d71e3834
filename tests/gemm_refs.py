"""f64 restatement of what ONE sarssl_gemm / sarssl_gemm_split call computes (csrc/gemm.hip, csrc/gemm_epilogue.h) on the operands AS
STORED: the operand staging (layout flags, the fp16 -> bf16 re-encoding of the mixed pairings, the bf16 rounding of the f32 fast mode, the
hi / lo parts of the f32 precise mode and of the fp16 pairs with the lo lo term left out), the epilogue in the order of epilogue8, the
split-K accumulate form and the relative shift.  Plain torch in float64, on whatever device the operands live on; tests/test_gemm_refs_cpu.py
checks it against torch.nn.functional and autograd, tests/test_gpu_gemm.py holds the kernels to it."""
import numpy as np
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def rows(T, kc):
    """An operand as laid out -> [..., rows, K]: kc = the contraction index is the contiguous one ([rows][K]), else [K][rows]."""
    return T if kc else T.transpose(-1, -2)


def split16(x, dtype):
    """f32 x -> (hi, lo) in f64: hi = dtype(x), lo = dtype(x - hi) (the difference is exact in f32)."""
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    return hi.double(), lo.double()


def _mm(a, b, outer):
    """a [.., M, K], b [.., N, K] -> a b^T; outer: every a against every b, [na, nb, M, N] (batch_inner = nb, sA = (s, 0), sB = (0, s))."""
    return torch.einsum("amk,bnk->abmn", a, b) if outer else a @ b.transpose(-1, -2)


def pair_product(Ah, Al, Bh, Bl, outer=False):
    """hi hi [+ hi lo_B] [+ lo_A hi]: the three (two, one) segments of sarssl_gemm_split and the three passes of the f32 precise mode."""
    y = _mm(Ah, Bh, outer)
    if Bl is not None:
        y = y + _mm(Ah, Bl, outer)
    if Al is not None:
        y = y + _mm(Al, Bh, outer)
    return y


def product(A, B, a_kc=True, b_kc=True, precise=False, outer=False):
    """sum_k opA(A)[m][k] opB(B)[n][k] as the matrix cores contract it, in f64."""
    A, B = rows(A, a_kc), rows(B, b_kc)
    if A.dtype == F32:
        assert B.dtype == F32
        if precise:
            (ah, al), (bh, bl) = split16(A, BF16), split16(B, BF16)
            return pair_product(ah, al, bh, bl, outer)
        return _mm(A.to(BF16).double(), B.to(BF16).double(), outer)
    if A.dtype != B.dtype:                           # a bf16 gradient against a saved fp16 activation: contracted in bf16
        A, B = A.to(BF16), B.to(BF16)
    return _mm(A.double(), B.double(), outer)


def swish_grad(h):
    s = torch.sigmoid(h)
    return s * (1.0 + h * (1.0 - s))


def inv_keep(p):
    """1 / (1 - p) as the kernel forms it: in f32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def epilogue(acc, alpha=1.0, bias=None, act=0, aux=None, aux_act=0, keep=None, p=0.0, out_scale=1.0, resid=None, res_scale=1.0):
    """-> (C, saved pre-activation), both f64 and unrounded.  acc [.., M, N]; bias [N]; aux / resid as stored, [.., M, N]; keep: bool keep
    mask of the dropout (keep_mask), p its probability.  act / aux_act: 0 none, 1 ReLU, 2 Swish."""
    h = float(np.float32(alpha)) * acc
    if bias is not None:
        h = h + bias.double()
    v = torch.relu(h) if act == 1 else h * torch.sigmoid(h) if act == 2 else h
    if aux is not None:
        a = aux.double()
        v = v * ((a > 0).double() if aux_act == 1 else swish_grad(a))
    if keep is not None:
        v = torch.where(keep, v * inv_keep(p), torch.zeros_like(v))
    v = v * float(np.float32(out_scale))
    if resid is not None:
        v = v + float(np.float32(res_scale)) * resid.double()
    return v, h


def accumulate(C0, acc, alpha=1.0):
    """The split-K form: C += alpha A B."""
    return C0.double() + float(np.float32(alpha)) * acc


def shift(R):
    """c_row_shift on [.., T, T]: element (m, n) is stored m + 1 - T elements further, what falls before its matrix is dropped.
    -> (result with zeros where nothing is stored, mask of the stored positions)."""
    T = R.shape[-1]
    flat = R.reshape(-1, T * T)
    m, n = torch.meshgrid(torch.arange(T, device=R.device), torch.arange(T, device=R.device), indexing="ij")
    dst = (m * T + n + m + 1 - T).reshape(-1)
    ok = dst >= 0
    out = torch.zeros_like(flat)
    written = torch.zeros(T * T, dtype=torch.bool, device=R.device)
    out[:, dst[ok]] = flat[:, ok]
    written[dst[ok]] = True
    return out.reshape(R.shape), written.reshape(T, T)


def _hash_u32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def keep_mask(seed, n, p):
    """Keep decisions of flat elements 0 .. n-1 (n < 2^33) of dropout stream `seed` (csrc/common.h dropout_scale): one 32-bit hash per
    element pair, 16 bits each, keep iff bits >= round(p 65536).  -> numpy bool [n]."""
    assert 0 < n < (1 << 33)
    with np.errstate(over="ignore"):
        key = _hash_u32(np.array([seed & 0xffffffff], dtype=np.uint32)) ^ (np.uint32((seed >> 32) & 0xffffffff) * np.uint32(0x9e3779b9))
        idx = np.arange(n, dtype=np.uint64)
        h = _hash_u32((idx >> np.uint64(1)).astype(np.uint32) ^ key)
    bits = np.where((idx & np.uint64(1)) == 1, h >> np.uint32(16), h & np.uint32(0xffff))
    thr = np.uint32(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return bits >= thr
