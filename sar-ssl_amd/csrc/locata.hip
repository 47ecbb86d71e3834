// Device work of the LOCATA TDOA corpus generator (locatads.generate; the reference forms both per item on the host,
// code/data_generation/utils_LOCATA.py:80-130, 209-261):
//   sarssl_peak_scale    x / (max|x| + 1e-8) * 0.9 of every item of a batch, in place, the peaks stored for the generator's check
//   sarssl_interp_mean   the mean of np.interp over an item's 16 640 sample times, for every column of the item's annotation table:
//                        the `np.mean(TDOA)` label of a static source without the (nsample, nch - 1, nsource) table it is the mean of
// Both are bound by latency at these sizes (a batch is 16 items of 33 280 samples and 16 tables of ~130 rows): one workgroup per item,
// no atomics, every sum and maximum folded in a fixed order, so an item's result does not depend on its position in the batch.
#include "common.h"
#include <cmath>
#include <vector>

#define LC_THREADS 256

// ------------------------------------------------------------------------------------------------------------------- peak and scale
// one sample into a thread's running max|x|; a sample that is not finite sets `bad` (fmaxf would pass a NaN over)
__device__ __forceinline__ void peak_acc(float v, float& m, bool& bad) {
    const float a = fabsf(v);
    bad |= !(a < INFINITY);
    m = fmaxf(m, a);
}

__global__ __launch_bounds__(LC_THREADS) void peak_scale_kernel(float* __restrict__ x, long len, float* __restrict__ peak) {
    __shared__ float s_m[LC_THREADS / 64];
    __shared__ int s_bad[LC_THREADS / 64];
    __shared__ float s_scale;
    float* xi = x + (long)blockIdx.x * len;
    const int tid = threadIdx.x;
    const bool vec = (len & 3) == 0 && (((uintptr_t)x) & 15) == 0;     // every item then starts on a 16-byte boundary
    float m = 0.f;
    bool bad = false;
    if (vec) {
        const float4* x4 = (const float4*)xi;
        for (long i = tid; i < (len >> 2); i += LC_THREADS) {
            const float4 v = x4[i];
            peak_acc(v.x, m, bad); peak_acc(v.y, m, bad); peak_acc(v.z, m, bad); peak_acc(v.w, m, bad);
        }
    } else {
        for (long i = tid; i < len; i += LC_THREADS) peak_acc(xi[i], m, bad);
    }
    m = wave_max(m);
    const int anybad = __any(bad ? 1 : 0);
    if ((tid & 63) == 0) { s_m[tid >> 6] = m; s_bad[tid >> 6] = anybad; }
    __syncthreads();
    if (tid == 0) {
        float p = s_m[0];
        int b = s_bad[0];
        for (int w = 1; w < LC_THREADS / 64; ++w) { p = fmaxf(p, s_m[w]); b |= s_bad[w]; }
        if (b) p = __uint_as_float(0x7fc00000u);
        peak[blockIdx.x] = p;
        s_scale = 0.9f / (p + 1e-8f);
    }
    __syncthreads();
    const float sc = s_scale;
    if (vec) {
        float4* x4 = (float4*)xi;
        for (long i = tid; i < (len >> 2); i += LC_THREADS) {
            float4 v = x4[i];
            v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
            x4[i] = v;
        }
    } else {
        for (long i = tid; i < len; i += LC_THREADS) xi[i] *= sc;
    }
}

extern "C" int sarssl_peak_scale(float* x, int nb, long ns, int nch, float* peak, void* stream) {
    SARSSL_REQUIRE(x && peak && nb >= 1 && nb <= 65535 && ns >= 1 && nch >= 1 && nch <= 65535 && (double)ns * nch < 2147483648.0,
                   "sarssl_peak_scale(B 1..65535, ns nch < 2^31)");
    hipLaunchKernelGGL(peak_scale_kernel, dim3(nb), dim3(LC_THREADS), 0, (hipStream_t)stream, x, ns * (long)nch, peak);
    SARSSL_CHECK_LAUNCH("sarssl_peak_scale");
    return 0;
}

// ------------------------------------------------------------------------------------------------------------- mean of np.interp
struct InterpItem { int off, npoint, n, pad; double t0, dt; };          // 32 bytes: one row of the workspace

// One workgroup per item.  Thread t owns samples k in [t chunk, (t + 1) chunk), chunk = ceil(n / 256): it finds the interval of its
// first sample time by binary search, walks forward from there (dt >= 0: the times ascend) and sums np.interp's values in f64, the
// slope of an interval formed once, as numpy's `(fp[j+1] - fp[j]) / (xp[j+1] - xp[j])`, the value as `slope (x - xp[j]) + fp[j]`
// in separately rounded steps (__dmul_rn / __dadd_rn: no contraction into an fma, which numpy's build does not use either).
// numpy's end rules: fp[0] before the table, fp[-1] from the last node on; exactly at a node the product is 0 and the left node's value
// comes back unchanged.  The 256 partials of a column are folded by one thread in thread order.
__global__ __launch_bounds__(LC_THREADS) void interp_mean_kernel(const InterpItem* __restrict__ items, const double* __restrict__ ts,
                                                                 const double* __restrict__ val, int ncol, double* __restrict__ out) {
    __shared__ double s_part[LC_THREADS][8];
    const InterpItem it = items[blockIdx.x];
    const double* xp = ts + it.off;
    const double* fp = val + (long)it.off * ncol;
    const int np = it.npoint, tid = threadIdx.x;
    const long n = it.n;
    const long chunk = (n + LC_THREADS - 1) / LC_THREADS;
    const long k0 = tid * chunk < n ? tid * chunk : n;
    const long k1 = k0 + chunk < n ? k0 + chunk : n;
    double acc[8], slope[8], fj[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { acc[c] = 0.0; slope[c] = 0.0; fj[c] = 0.0; }
    if (k0 < k1) {
        double t = __dadd_rn(it.t0, __dmul_rn((double)k0, it.dt));
        int lo = 0, hi = np;                                            // -> lo = the number of nodes <= t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (xp[mid] <= t) lo = mid + 1; else hi = mid;
        }
        int j = lo - 1, jl = -2;                                        // jl: the interval `slope` and `fj` belong to
        double xj = 0.0;
        for (long k = k0; k < k1; ++k) {
            t = __dadd_rn(it.t0, __dmul_rn((double)k, it.dt));
            while (j + 1 < np && xp[j + 1] <= t) ++j;
            if (j != jl) {
                jl = j;
                if (j < 0 || j >= np - 1) {                             // outside the table, or on its last node: the end value
                    const long r = j < 0 ? 0 : np - 1;
#pragma unroll
                    for (int c = 0; c < 8; ++c) if (c < ncol) { slope[c] = 0.0; fj[c] = fp[r * ncol + c]; }
                    xj = t;
                } else {
                    xj = xp[j];
                    const double dx = xp[j + 1] - xj;
#pragma unroll
                    for (int c = 0; c < 8; ++c) if (c < ncol) {
                        fj[c] = fp[(long)j * ncol + c];
                        slope[c] = (fp[(long)(j + 1) * ncol + c] - fj[c]) / dx;
                    }
                }
            }
            const bool flat = j < 0 || j >= np - 1;
            const double d = flat ? 0.0 : t - xj;
#pragma unroll
            for (int c = 0; c < 8; ++c) if (c < ncol) acc[c] += flat ? fj[c] : __dadd_rn(__dmul_rn(slope[c], d), fj[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) s_part[tid][c] = acc[c];
    __syncthreads();
    if (tid < ncol) {
        double s = 0.0;
        for (int u = 0; u < LC_THREADS; ++u) s += s_part[u][tid];
        out[(long)blockIdx.x * ncol + tid] = s / (double)n;
    }
}

extern "C" long sarssl_interp_mean_workspace_bytes(int nb) { return nb >= 1 && nb <= 65535 ? (long)nb * (long)sizeof(InterpItem) : -1; }

extern "C" int sarssl_interp_mean(const int* offsets, const double* t0, const double* dt, const int* n, int nb, int ncol, long ntotal,
                                  const double* ts, const double* val, void* ws, double* out, void* stream) {
    SARSSL_REQUIRE(offsets && t0 && dt && n && ts && val && ws && out, "sarssl_interp_mean");
    SARSSL_REQUIRE(nb >= 1 && nb <= 65535, "sarssl_interp_mean(B 1..65535)");
    SARSSL_REQUIRE(ncol >= 1 && ncol <= 8, "sarssl_interp_mean(ncol 1..8)");
    SARSSL_REQUIRE(offsets[0] == 0 && (long)offsets[nb] == ntotal, "sarssl_interp_mean(offsets span the tables)");
    std::vector<InterpItem> items(nb);
    for (int b = 0; b < nb; ++b) {
        SARSSL_REQUIRE(offsets[b + 1] - offsets[b] >= 1, "sarssl_interp_mean(npoint >= 1)");
        SARSSL_REQUIRE(n[b] >= 1, "sarssl_interp_mean(n >= 1)");
        SARSSL_REQUIRE(std::isfinite(t0[b]) && std::isfinite(dt[b]) && dt[b] >= 0.0, "sarssl_interp_mean(t0 finite, dt finite and >= 0)");
        items[b] = InterpItem{offsets[b], offsets[b + 1] - offsets[b], n[b], 0, t0[b], dt[b]};
    }
    hipStream_t st = (hipStream_t)stream;
    // the rows come from this call's own host memory: the copy is waited for before the call returns
    if (hipMemcpyAsync(ws, items.data(), (size_t)nb * sizeof(InterpItem), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        sarssl_set_error("sarssl_interp_mean: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    hipLaunchKernelGGL(interp_mean_kernel, dim3(nb), dim3(LC_THREADS), 0, st, (const InterpItem*)ws, ts, val, ncol, out);
    SARSSL_CHECK_LAUNCH("sarssl_interp_mean");
    return 0;
}
