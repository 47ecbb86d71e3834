// The accept test and the annotations of simulated RIRs on the device (sarssl_rir_labels), and the float -> PCM-16 step of the signal
// generator (sarssl_pcm16_pack).
//
// sarssl_rir_labels restates roomsim.labels in f64 on the f32 values as stored - check_rir, check_rir_envelope, generate_annotation
// of code/data_generation/utils_simu_rir_sig.py:510-614, 863-994 - so that a RIR that is only rendered to be judged never leaves the
// device.  Two launches:
//
//   rirlabel_row_kernel, one 256-thread workgroup per (item, channel) row h[0..L), L = n_len[b]:
//     finite / non-zero flags of the row; max_idx = first index of the signed maximum (np.argmax);
//     S[n] = sum_{k >= n} h[k]^2 (the reverse cumulative sum), E[n] = 10 log10(S[n] / (S[max_idx] + 1e-10) + 1e-10);
//     nearest(v) = first index of min |E - v| for the 22 distinct targets v = -5, -7 .. -47;
//     the 80 stretches [nearest(st0), nearest(st0 + dur)), st0 = -5, -7 .. -19 outer, dur = -10, -12 .. -28 inner: |st - ed| <= 1 gives
//     t60 = NaN, r = 0; otherwise the least-squares line of E over n / fs as scipy.stats.linregress (1.15) computes it - r =
//     ssxym / sqrt(ssxm ssym) clipped to [-1, 1], r = 0 when ssxm or ssym is zero, slope = ssxym / ssxm - and t60 = -60 / (slope + 1e-10);
//     the winner is the first stretch of largest |r|.  As numpy's argmax does, A NaN |r| WINS over every number (the first NaN is taken).
//   rirlabel_item_kernel, one workgroup per item: the same flags of the direct path, rir_ok, the mean of the channels' t60, env_ok =
//     |mean t60 - t60_specify| < 0.05 and |r of the LAST channel| > 0.5 (the reference's quirk), nd = first signed maximum of the direct
//     path's channel 0 padded with zeros to max(L, Ld), DRR over +-int(fs 2.5 / 1000) samples around nd and C50 up to nd +
//     int(fs 50 / 1000), both of channel 0 with eps = 1e-8.  Without rir_ok the item's t60, corr and t60_edc are NaN, as the host never
//     runs the envelope test then; a non-finite value in channel 0 makes DRR and C50 NaN, as the host's masked sums do.
//
// The scan.  S is a suffix sum over contiguous per-thread chunks of ceil(L / 256) samples: S[n] = (sum of the chunk's samples from its
// end down to n, added one by one) + carry, and the carries are chained one rounded add per chunk from the row's end.  Where h is zero
// the sum is therefore EXACTLY constant, also across chunk borders, as it is in numpy's sequential cumsum - a plateau of E must stay a
// plateau, or "first index of the nearest value" lands somewhere else on it.  The chunk size depends on L alone, so an item's result
// depends neither on its batch position nor on lmax.  The fits are O(1) each from suffix sums of (E - E0), (E - E0)^2 and
// (n - L / 2)(E - E0) with E0 = -26 dB, the middle of the targets: centred so that the differences of the sums do not cancel; the x
// side of the fit is closed-form (variance of N consecutive integers).  A fit is a function of (st, ed) alone, so equal stretches give
// bit-equal r and the first-wins rule decides as on the host.  No atomics, plain C++.
#include "common.h"
#include <math.h>

#define RL_THREADS 256
#define RL_WAVES (RL_THREADS / 64)
#define RL_MAX_LEN (1 << 15)
#define RL_NTARGET 22            // -5, -7 .. -47 dB
#define RL_NFIT 80

struct RirLabelWs { double* E; double* Q0; double* Q1; double* Q2; int* rowflag; };

static bool rirlabel_shape_ok(int nb, int nch, int lmax, int ldmax) {
    return nb >= 1 && nch >= 1 && nch <= 8 && lmax >= 1 && lmax <= RL_MAX_LEN && ldmax >= 1 && ldmax <= RL_MAX_LEN;
}
static size_t rirlabel_rowflag_off(int nb, int nch, int lmax) { return (size_t)4 * nb * nch * lmax * sizeof(double); }
extern "C" long sarssl_rir_labels_workspace_bytes(int nb, int nch, int lmax, int ldmax) {
    if (!rirlabel_shape_ok(nb, nch, lmax, ldmax)) return -1;
    return (long)(rirlabel_rowflag_off(nb, nch, lmax) + (size_t)nb * nch * sizeof(int));
}

// ---- workgroup helpers (256 threads = 4 waves) -------------------------------------------------------------------------------------
__device__ __forceinline__ double rl_shfl_xor(double v, int o) {
    const unsigned long long u = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(u & 0xffffffffull), o, 64), hi = __shfl_xor((int)(u >> 32), o, 64);
    return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// sum over the workgroup in a fixed order (lanes by butterfly, then the waves one by one); every thread gets the result
__device__ double rl_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += rl_shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < RL_WAVES; ++w) s += sh[w];
    return s;
}
__device__ int rl_block_or(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = sh[0];
    for (int w = 1; w < RL_WAVES; ++w) s |= sh[w];
    return s;
}
// the smaller key wins, the smaller index among equal keys: (key, idx) of the workgroup's first minimum in every thread
__device__ void rl_block_argmin(double& key, int& idx, double* shk, int* shi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double k2 = rl_shfl_xor(key, o);
        const int i2 = __shfl_xor(idx, o, 64);
        if (k2 < key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shk[threadIdx.x >> 6] = key; shi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    key = shk[0]; idx = shi[0];
    for (int w = 1; w < RL_WAVES; ++w)
        if (shk[w] < key || (shk[w] == key && shi[w] < idx)) { key = shk[w]; idx = shi[w]; }
}
// first index of the signed maximum of x[0..n) as np.argmax finds it (a NaN is a maximum); n >= 1.  `val` gets the maximum.
__device__ int rl_first_argmax(const float* __restrict__ x, int n, float& val, double* shk, int* shi) {
    double key = INFINITY;          // -value, so that the argmin helper applies; NaN maps to -inf
    int idx = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += RL_THREADS) {
        const float v = x[i];
        const double k = (v != v) ? -INFINITY : -(double)v;
        if (idx == 0x7fffffff || k < key) { key = k; idx = i; }       // (ascending i: the first index of a thread's maximum stays)
    }
    rl_block_argmin(key, idx, shk, shi);
    idx = idx < n ? idx : 0;
    val = x[idx];
    return idx;
}

// out[n] = (f(hi-1) + ... + f(n), added from the chunk's end) + carry of the chunks behind, for the thread's chunk [lo, hi)
template <typename F>
__device__ void rl_suffix_scan(F f, double* __restrict__ out, int lo, int hi, double* tot, double* carry) {
    double t = 0.0;
    for (int n = hi - 1; n >= lo; --n) t += f(n);
    __syncthreads();
    tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0;
        carry[RL_THREADS - 1] = 0.0;
        for (int k = RL_THREADS - 2; k >= 0; --k) { c += tot[k + 1]; carry[k] = c; }
    }
    __syncthreads();
    const double c = carry[threadIdx.x];
    t = 0.0;
    for (int n = hi - 1; n >= lo; --n) { t += f(n); out[n] = t + c; }
    __syncthreads();
}

__global__ __launch_bounds__(RL_THREADS) void rirlabel_row_kernel(const float* __restrict__ rir, const int* __restrict__ n_len, double fs,
                                                                  int nch, int lmax, RirLabelWs w, double* __restrict__ t60_out,
                                                                  double* __restrict__ corr_out) {
    __shared__ double tot[RL_THREADS], carry[RL_THREADS];
    __shared__ double shk[RL_WAVES];
    __shared__ int shi[RL_WAVES];
    __shared__ int near_idx[RL_NTARGET];
    __shared__ double fit_r[RL_NFIT], fit_t60[RL_NFIT];
    const int row = blockIdx.x, b = row / nch, tid = threadIdx.x;
    const float* h = rir + (size_t)row * lmax;
    double* E = w.E + (size_t)row * lmax;
    double* Q0 = w.Q0 + (size_t)row * lmax;
    double* Q1 = w.Q1 + (size_t)row * lmax;
    double* Q2 = w.Q2 + (size_t)row * lmax;
    int L = n_len[b];
    L = L < 0 ? 0 : (L > lmax ? lmax : L);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (L < 1) {                                                     // (uniform over the workgroup)
        if (tid == 0) { w.rowflag[row] = 0; t60_out[row] = nan; corr_out[row] = nan; }
        return;
    }
    // flags: bit 0 every value finite, bit 1 some value non-zero
    int bad = 0, nz = 0;
    for (int i = tid; i < L; i += RL_THREADS) {
        const float v = h[i];
        bad |= !(fabsf(v) <= 3.402823466e38f);
        nz |= v != 0.f;
    }
    bad = rl_block_or(bad, shi);
    nz = rl_block_or(nz, shi);
    if (tid == 0) w.rowflag[row] = (bad ? 0 : 1) | (nz ? 2 : 0);
    float hmax;
    const int max_idx = rl_first_argmax(h, L, hmax, shk, shi);

    const int chunk = (L + RL_THREADS - 1) / RL_THREADS;
    int lo = tid * chunk, hi = lo + chunk;
    lo = lo > L ? L : lo;
    hi = hi > L ? L : hi;
    rl_suffix_scan([&](int n) { const double v = (double)h[n]; return v * v; }, E, lo, hi, tot, carry);
    const double den = E[max_idx] + 1e-10;
    __syncthreads();                                                 // (E[max_idx] is read by all before its owner overwrites it)
    for (int n = lo; n < hi; ++n) E[n] = 10.0 * log10(E[n] / den + 1e-10);
    __syncthreads();

    // nearest(v) for the 22 targets: first index of the smallest |E - v|
    double bk[RL_NTARGET];
    int bi[RL_NTARGET];
#pragma unroll
    for (int k = 0; k < RL_NTARGET; ++k) { bk[k] = INFINITY; bi[k] = 0x7fffffff; }
    for (int n = tid; n < L; n += RL_THREADS) {
        const double e = E[n];
#pragma unroll
        for (int k = 0; k < RL_NTARGET; ++k) {
            const double d = fabs(e - (double)(-5 - 2 * k));
            if (d < bk[k]) { bk[k] = d; bi[k] = n; }
        }
    }
#pragma unroll
    for (int k = 0; k < RL_NTARGET; ++k) {
        rl_block_argmin(bk[k], bi[k], shk, shi);
        if (tid == 0) near_idx[k] = bi[k] < L ? bi[k] : 0;            // (every |E - v| NaN: unreachable for a finite row; keeps the index in range)
    }
    __syncthreads();

    const double E0 = -26.0, xc = 0.5 * (double)L;
    rl_suffix_scan([&](int n) { return E[n] - E0; }, Q0, lo, hi, tot, carry);
    rl_suffix_scan([&](int n) { const double y = E[n] - E0; return y * y; }, Q1, lo, hi, tot, carry);
    rl_suffix_scan([&](int n) { return ((double)n - xc) * (E[n] - E0); }, Q2, lo, hi, tot, carry);

    if (tid < RL_NFIT) {
        const int a = tid / 10, d = tid % 10;                        // st0 = -5 - 2a, dur = -10 - 2d: targets a and a + 5 + d
        const int st = near_idx[a], ed = near_idx[a + 5 + d];
        double r = 0.0, t60 = nan;
        const int diff = st > ed ? st - ed : ed - st;
        if (diff > 1 && ed > st) {                                   // (E does not rise, so ed >= st; ed < st would be an empty slice)
            const double N = (double)(ed - st);
            const double sy = Q0[st] - Q0[ed], syy = Q1[st] - Q1[ed], sxy = Q2[st] - Q2[ed];
            const double xm = 0.5 * (double)(st + ed - 1) - xc;      // mean of n - xc over the stretch
            const double ssxm = (N * N - 1.0) / 12.0 / (fs * fs);
            const double ssym = (syy - sy * sy / N) / N;
            const double ssxym = (sxy - xm * sy) / N / fs;
            if (ssxm == 0.0 || ssym == 0.0) r = 0.0;
            else {
                r = ssxym / sqrt(ssxm * ssym);
                if (r > 1.0) r = 1.0;
                else if (r < -1.0) r = -1.0;
            }
            t60 = -60.0 / (ssxym / ssxm + 1e-10);
        }
        fit_r[tid] = r;
        fit_t60[tid] = t60;
    }
    __syncthreads();
    if (tid == 0) {
        int win = 0;
        double best = fabs(fit_r[0]);
        if (best == best)
            for (int i = 1; i < RL_NFIT; ++i) {
                const double a = fabs(fit_r[i]);
                if (a != a) { win = i; break; }
                if (a > best) { best = a; win = i; }
            }
        t60_out[row] = fit_t60[win];
        corr_out[row] = fit_r[win];
    }
}

__global__ __launch_bounds__(RL_THREADS) void rirlabel_item_kernel(const float* __restrict__ rir, const int* __restrict__ n_len,
                                                                   const float* __restrict__ rir_dp, const int* __restrict__ dp_len,
                                                                   const double* __restrict__ t60_specify, double fs, int nch, int lmax,
                                                                   int ldmax, const int* __restrict__ rowflag, double* __restrict__ t60,
                                                                   double* __restrict__ corr, double* __restrict__ t60_edc,
                                                                   double* __restrict__ drr, double* __restrict__ c50, int* __restrict__ nd_out,
                                                                   int* __restrict__ flags) {
    __shared__ double shk[RL_WAVES];
    __shared__ int shi[RL_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    int L = n_len[b], Ld = dp_len[b];
    L = L < 0 ? 0 : (L > lmax ? lmax : L);
    Ld = Ld < 0 ? 0 : (Ld > ldmax ? ldmax : Ld);
    const float* h = rir + (size_t)b * nch * lmax;                   // channel 0
    const float* dp = rir_dp + (size_t)b * nch * ldmax;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // the direct path's flags over all channels
    int bad = 0, nz = 0;
    for (int m = 0; m < nch; ++m)
        for (int i = tid; i < Ld; i += RL_THREADS) {
            const float v = dp[(size_t)m * ldmax + i];
            bad |= !(fabsf(v) <= 3.402823466e38f);
            nz |= v != 0.f;
        }
    bad = rl_block_or(bad, shi);
    nz = rl_block_or(nz, shi);
    int rf_and = 1, rf_nz = 0, h0_finite = 1;
    for (int m = 0; m < nch; ++m) {
        const int f = rowflag[b * nch + m];
        rf_and &= f & 1;
        rf_nz |= f & 2;
        if (m == 0) h0_finite = f & 1;
    }
    const bool rir_ok = L >= 1 && Ld >= 1 && rf_and && rf_nz && !bad && nz;
    // nd: np.argmax of the direct path's channel 0, padded with zeros to max(L, Ld)
    int nd = 0;
    if (Ld >= 1) {
        float v;
        nd = rl_first_argmax(dp, Ld, v, shk, shi);
        if (v < 0.f && L > Ld) nd = Ld;
    }
    const int n0 = (int)(fs * 2.5 / 1000.0), n1 = (int)(fs * 50.0 / 1000.0);
    double s_dp = 0.0, s_rev = 0.0, s_early = 0.0, s_late = 0.0;
    for (int n = tid; n < L; n += RL_THREADS) {
        const double v = (double)h[n], p = v * v;
        if (n >= nd - n0 && n <= nd + n0) s_dp += p; else s_rev += p;
        if (n <= nd + n1) s_early += p; else s_late += p;
    }
    s_dp = rl_block_sum(s_dp, shk);
    s_rev = rl_block_sum(s_rev, shk);
    s_early = rl_block_sum(s_early, shk);
    s_late = rl_block_sum(s_late, shk);
    if (tid == 0) {
        const double eps = 1e-8;
        drr[b] = h0_finite ? 10.0 * log10(s_dp / (s_rev + eps) + eps) : nan;
        c50[b] = h0_finite ? 10.0 * log10(s_early / (s_late + eps) + eps) : nan;
        nd_out[b] = nd;
        int env_ok = 0;
        double mean = nan;
        if (rir_ok) {
            double s = 0.0;
            for (int m = 0; m < nch; ++m) s += t60[b * nch + m];
            mean = s / (double)nch;
            env_ok = (fabs(mean - t60_specify[b]) < 0.05) && (fabs(corr[b * nch + nch - 1]) > 0.5);
        } else {
            for (int m = 0; m < nch; ++m) { t60[b * nch + m] = nan; corr[b * nch + m] = nan; }
        }
        t60_edc[b] = mean;
        flags[b] = (rir_ok ? 1 : 0) | (env_ok ? 2 : 0);
    }
}

extern "C" int sarssl_rir_labels(const float* rir, const int* n_len, const float* rir_dp, const int* dp_len, const double* t60_specify,
                                 double fs, int nb, int nch, int lmax, int ldmax, void* ws, double* t60, double* corr, double* t60_edc,
                                 double* drr, double* c50, int* nd, int* flags, void* stream) {
    SARSSL_REQUIRE(rir && n_len && rir_dp && dp_len && t60_specify && ws && t60 && corr && t60_edc && drr && c50 && nd && flags,
                   "sarssl_rir_labels");
    SARSSL_REQUIRE(rirlabel_shape_ok(nb, nch, lmax, ldmax), "sarssl_rir_labels(nch 1..8, lmax and ldmax 1..32768)");
    SARSSL_REQUIRE(fs > 0.0, "sarssl_rir_labels");
    hipStream_t st = (hipStream_t)stream;
    RirLabelWs w;
    const size_t n = (size_t)nb * nch * lmax;
    w.E = (double*)ws; w.Q0 = w.E + n; w.Q1 = w.Q0 + n; w.Q2 = w.Q1 + n;
    w.rowflag = (int*)((char*)ws + rirlabel_rowflag_off(nb, nch, lmax));
    rirlabel_row_kernel<<<nb * nch, RL_THREADS, 0, st>>>(rir, n_len, fs, nch, lmax, w, t60, corr);
    SARSSL_CHECK_LAUNCH("rirlabel_row_kernel");
    rirlabel_item_kernel<<<nb, RL_THREADS, 0, st>>>(rir, n_len, rir_dp, dp_len, t60_specify, fs, nch, lmax, ldmax, w.rowflag, t60, corr,
                                                    t60_edc, drr, c50, nd, flags);
    SARSSL_CHECK_LAUNCH("rirlabel_item_kernel");
    return 0;
}

// ---- float -> PCM-16 ----------------------------------------------------------------------------------------------------------------
// out = rint(double(x) 32767) with ties to even, saturated to +-32767: libsndfile's float -> PCM-16 conversion with normalisation on, AS
// THIS PROJECT READS IT - soundfile is not available to pin it against (UNPINNED).  A float times 32767 is exact in f64, so this is
// bit-equal to numpy's rint(x.astype(f64) * 32767).  NaN gives 0.
__device__ __forceinline__ short rl_pcm16(float x) {
    double v = rint((double)x * 32767.0);
    v = v > 32767.0 ? 32767.0 : (v < -32767.0 ? -32767.0 : v);
    return (v == v) ? (short)(int)v : (short)0;
}
__global__ __launch_bounds__(256) void pcm16_pack_kernel(const float* __restrict__ in, short* __restrict__ out, long n) {
    const long i4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 + 4 <= n) {
        const float4 v = *(const float4*)(in + i4);
        short4 o;
        o.x = rl_pcm16(v.x); o.y = rl_pcm16(v.y); o.z = rl_pcm16(v.z); o.w = rl_pcm16(v.w);
        *(short4*)(out + i4) = o;
    } else {
        for (long i = i4; i < n; ++i) out[i] = rl_pcm16(in[i]);
    }
}
extern "C" int sarssl_pcm16_pack(const float* in, long n, short* out, void* stream) {
    SARSSL_REQUIRE(in && out && n >= 0, "sarssl_pcm16_pack");
    SARSSL_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0, "sarssl_pcm16_pack(in 16-byte, out 8-byte aligned)");
    if (n == 0) return 0;
    const long nblk = (n + 1023) / 1024;
    SARSSL_REQUIRE(nblk <= 0x7fffffffl, "sarssl_pcm16_pack");
    pcm16_pack_kernel<<<(unsigned)nblk, 256, 0, (hipStream_t)stream>>>(in, out, n);
    SARSSL_CHECK_LAUNCH("pcm16_pack_kernel");
    return 0;
}
