"""Per-phase cycle stamps of the GEMM K loops (workgroup (0,0,0), its 4 waves, first 16 K-tiles): a probe copy of the library built with
-DGEMM_STAMPS (never the shipped one) prints where a K-tile's cycles go for the hot shapes - the plain kernel's loop and the pair
products' (sarssl_gemm_split) at both K-tile depths.
    python tools/gemm_stamps.py --build-only [--lib PATH]     compile the probe library (no GPU needed; the other objects come from csrc/*.o)
    python tools/gemm_stamps.py [--lib PATH] [--pairs-only]   run it (builds first when PATH is missing)"""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = os.path.join(ROOT, "sar-ssl_amd", "csrc")
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "tmp_ab", "libgemmprobe.so"), help="the probe library (tmp_ab/, as tools/probe_lib.py)")
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--pairs-only", action="store_true")
args = ap.parse_args()
out = os.path.abspath(args.lib)
if args.build_only or not os.path.exists(out):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    sys.path.insert(0, C)
    import build as B  # noqa: E402  (the product build's compiler and flags)
    objs = [os.path.join(C, f) for f in os.listdir(C) if f.endswith(".o") and f != "gemm.o"]
    subprocess.check_call([B._hipcc()] + B.FLAGS + ["-DGEMM_STAMPS", "-c", os.path.join(C, "gemm.hip"), "-o", out + ".gemm.o"])
    subprocess.check_call([B._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, out + ".gemm.o"] + objs + ["-lpthread"])
    os.remove(out + ".gemm.o")
if args.build_only:
    print(out)
    sys.exit(0)
os.environ["SARSSL_HIP_LIB"] = out
sys.path.insert(0, ROOT)
import sarssl_boot  # noqa
import torch
from sar_ssl_amd import hip, _lib
dev = torch.device("cuda:0")
M = 16384
buf = torch.zeros((4, 16, 8), dtype=torch.int64, device=dev)
names = ["lds store", "barrier1", "issue loads", "mfma phase", "barrier2", "loop"]


def stamped(label, run, nk):
    for _ in range(3): run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record(); run(); e1.record(); torch.cuda.synchronize()
    buf.zero_()
    _lib.call("sarssl_gemm_stamp_buffer", _lib.c_void_p(buf.data_ptr()))
    run(); torch.cuda.synchronize()
    _lib.call("sarssl_gemm_stamp_buffer", _lib.c_void_p(0))
    t = buf.cpu().numpy().astype("int64")
    print("== %s: %.1f us; cycles per phase (s_memtime ticks = 100 MHz? see loop total), K-tiles 2..%d averaged" % (label, e0.elapsed_time(e1) * 1e3, nk - 2))
    for wv in range(4):
        d = (t[wv, 2:nk - 1, 1:6] - t[wv, 2:nk - 1, 0:5]).mean(axis=0)
        tot = (t[wv, 3:nk - 1, 0] - t[wv, 2:nk - 2, 0]).mean()
        print("  wave %d: " % wv + "  ".join("%s %6.0f" % (n, v) for n, v in zip(names, d)) + "  | K-tile %6.0f" % tot)


if not args.pairs_only:
    for label, N, K, b_kc in (("decoder2 NT", 1024, 3072, True), ("decoder1 NT", 3072, 768, True), ("ffn1 d512 NT", 2048, 512, True),
                              ("ffn2 d512 NT", 512, 2048, True), ("ffn1 dX NN d512", 512, 2048, False), ("ffn2 d256 NT", 256, 1024, True)):
        A = torch.randn((M, K), device=dev).bfloat16()
        B = (torch.randn((N, K) if b_kc else (K, N), device=dev) * 0.05).bfloat16()
        o = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        stamped("%s  M=%d N=%d K=%d" % (label, M, N, K),
                lambda: hip.gemm(A, B, a_kc=True, b_kc=b_kc, M=M, N=N, K=K, lda=K, ldb=B.shape[1], out=o), min(16, K // 64))
# the pair products' loop (NSEG = 2 | 3) at K-tile depth 64 and 32: a K-tile of depth 32 is half the work of one of depth 64
f16, f32 = torch.float16, torch.float32
for label, M_, N, K, nseg, odt in (("ffn1 d512 x3", M, 2048, 512, 3, f16), ("decoder1 x3", M // 2, 3072, 768, 3, f16),
                                   ("ffn2 d512 x2", M, 512, 2048, 2, f32), ("decoder2 x2", M // 2, 1024, 3072, 2, f32),
                                   ("qkv-like x3 f32", M, 768, 256, 3, f32)):
    xa = hip.split_pair(torch.randn((M_, K), device=dev))
    wp = hip.split_pair(torch.randn((N, K), device=dev) * K ** -0.5)
    A_ = xa if nseg == 3 else xa.hi
    o = torch.empty((M_, N), dtype=odt, device=dev)
    for depth in (64, 32):
        hip.pair_kdepth_override(depth)
        stamped("pair %s  M=%d N=%d K=%d depth %d" % (label, M_, N, K, depth),
                lambda: hip.gemm_split(A_, wp.hi, wp.lo, M=M_, N=N, K=K, out=o), min(16, K // depth))
    hip.pair_kdepth_override(0)
