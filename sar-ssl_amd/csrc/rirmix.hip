// Microphone signals from stored room impulse responses, rendered on the GPU (gfx950).
//
// Replaces the per-item CPU work of RandomMicSigFromRIRDataset (code/dataset.py:287-382): the two scipy.signal.fftconvolve calls and
// add_noise + peak normalisation of MicSigFromRIRDataset.__getitem__ (code/data_generation/utils_simu_rir_sig.py:1203-1237,
// gen_sig_from_real_rir.py:185-304), the diffuse noise field of NoiseDataset.generate_diffuse_noise (utils_noise.py:141-253) and the
// white-noise draw that feeds it.
//
// sarssl_rir_mix: uniformly partitioned overlap-save, 256-sample blocks, 512-point transforms (fft512_wave).  Source block spectra X_t
// (samples [(t-1)256, (t+1)256)) are formed once per item, RIR partition spectra H_p once per RIR.  Two channels share one complex
// transform and are NEVER separated: the source is real, so IFFT(X . FFT(h_a + i h_b)) = x*h_a + i x*h_b.  One workgroup forms 8
// consecutive output blocks of one (item, channel pair): a thread owns one bin, keeps the 8 sliding source spectra in registers and reads
// every H_p once.  The direct-path signal is needed for its power and peak only; sarssl_rir_mix_dp also stores it (out_dp, the layout and
// the scale of out), from the same kernels: out_dp == nullptr is sarssl_rir_mix.  A workgroup that leaves early because its stretch of
// the direct-path signal is exactly zero writes those zeros itself before it returns - out_dp is not cleared on the stream first.
#include "common.h"
#include "fft_wave.h"

#define RB 256          // block length
#define RN 512          // transform length
#define RZ 513          // float2 per wave buffer (padded)
#define TB 8            // output blocks per workgroup

struct RirWs {
    double* stats;          // [nb][2]: sum dp^2, sum noise^2
    float2* X;              // [nb][nT][512]
    float2* H;              // [nb][Q][P][512]
    unsigned* peak;         // [nb][2]: bits of max|dp|, max|mic|
    int* nd;                // [nb][nch]: first index of the signed maximum
    int* prange;            // [nb][Q][2]: first / last live partition
    int nT, Q, P, npair;
    long bytes;
};
static RirWs rir_ws_layout(void* base, int nb, long ns, int nch, int lmax, int ldmax) {
    RirWs w;
    w.nT = (int)((ns + RB - 1) / RB);
    w.npair = (nch + 1) / 2;
    w.Q = 2 * w.npair;
    const int lm = lmax > ldmax ? lmax : ldmax;
    w.P = (lm + RB - 1) / RB;
    char* p = (char*)base;
    long o = 0;
    w.stats = (double*)(p + o); o += (long)nb * 2 * sizeof(double);
    w.X = (float2*)(p + o); o += (long)nb * w.nT * RN * sizeof(float2);
    w.H = (float2*)(p + o); o += (long)nb * w.Q * w.P * RN * sizeof(float2);
    w.peak = (unsigned*)(p + o); o += (long)nb * 2 * sizeof(unsigned);
    w.nd = (int*)(p + o); o += ((long)nb * nch * sizeof(int) + 7) / 8 * 8;
    w.prange = (int*)(p + o); o += (long)nb * w.Q * 2 * sizeof(int);
    w.bytes = o;
    return w;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// per item: nd[c] (window mode) and the live partition range of every packed filter
__global__ __launch_bounds__(256) void rir_plan_kernel(const float* __restrict__ rir, const int* __restrict__ rir_len,
                                                       const int* __restrict__ dp_len, int explicit_dp, int n0, int nch, int lmax,
                                                       int ldmax, int npair, int* __restrict__ nd, int* __restrict__ prange) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ int snd[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = clampi(rir_len[b], 1, lmax);
    if (!explicit_dp) {
        for (int c = 0; c < nch; ++c) {
            const float* h = rir + ((long)b * nch + c) * lmax;
            float bv = -INFINITY; int bi = 0x7fffffff;
            for (int n = tid; n < len; n += 256) {
                const float x = h[n];
                if (x > bv || bi == 0x7fffffff) { bv = x; bi = n; }     // strictly greater: the first index wins inside a thread
            }
            sv[tid] = bv; si[tid] = bi;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) {
                if (tid < s) {
                    const float ov = sv[tid + s]; const int oi = si[tid + s];
                    if (oi != 0x7fffffff && (si[tid] == 0x7fffffff || ov > sv[tid] || (ov == sv[tid] && oi < si[tid]))) { sv[tid] = ov; si[tid] = oi; }
                }
                __syncthreads();
            }
            if (tid == 0) { snd[c] = si[0]; nd[b * nch + c] = si[0]; }
            __syncthreads();
        }
    }
    if (tid < 2 * npair) {
        const int q = tid, pr = q % npair;
        int lo = 0, hi = (len - 1) / RB;
        if (q >= npair) {
            if (explicit_dp) hi = (clampi(dp_len[b], 1, ldmax) - 1) / RB;
            else {
                lo = 0x7fffffff; hi = 0;
                for (int c = 2 * pr; c < 2 * pr + 2 && c < nch; ++c) {
                    const int a = clampi(snd[c] - n0, 0, len - 1), e = clampi(snd[c] + n0, 0, len - 1);
                    lo = min(lo, a / RB); hi = max(hi, e / RB);
                }
            }
        }
        prange[(b * 2 * npair + q) * 2 + 0] = lo;
        prange[(b * 2 * npair + q) * 2 + 1] = hi;
    }
}

// X[b][t] = FFT512(src[(t-1)256 .. (t+1)256)), zero outside [0, ns)
__global__ __launch_bounds__(512) void rir_src_spec_kernel(const float* __restrict__ src, long ns, int nT, float2* __restrict__ X) {
    __shared__ float2 Z[TB * RZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x * TB + wave, b = blockIdx.y;
    const bool live = t < nT;
    float2* zb = Z + wave * RZ;
    cpx v[8];
    if (live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long n = (long)(t - 1) * RB + lane + 64 * j;
            v[j] = {(n >= 0 && n < ns) ? src[(long)b * ns + n] : 0.f, 0.f};
        }
    }
    fft512_wave(v, zb, lane, live);
    if (live) {
        float2* o = X + ((long)b * nT + t) * RN;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[lane + 64 * j] = zb[lane + 64 * j];
    }
}

// H[b][q][p] = FFT512(h_c0[p 256 .. (p+1)256) + i h_c1[..], zero-padded); q < npair: the RIR, q >= npair: the direct-path RIR
__global__ __launch_bounds__(512) void rir_spec_kernel(const float* __restrict__ rir, const int* __restrict__ rir_len,
                                                       const float* __restrict__ rir_dp, const int* __restrict__ dp_len, int n0, int nch,
                                                       int lmax, int ldmax, int npair, int P, const int* __restrict__ nd,
                                                       const int* __restrict__ prange, float2* __restrict__ H) {
    __shared__ float2 Z[TB * RZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x * TB + wave, q = blockIdx.y, b = blockIdx.z, Q = 2 * npair;
    const int lo = prange[(b * Q + q) * 2], hi = prange[(b * Q + q) * 2 + 1];
    const bool live = p >= lo && p <= hi && p < P;
    float2* zb = Z + wave * RZ;
    cpx v[8];
    if (live) {
        const bool isdp = q >= npair, expl = rir_dp != nullptr;
        const int c0 = 2 * (q % npair);
        const float* base = (isdp && expl) ? rir_dp : rir;
        const int stride = (isdp && expl) ? ldmax : lmax;
        const int len = (isdp && expl) ? clampi(dp_len[b], 1, ldmax) : clampi(rir_len[b], 1, lmax);
        float hv[2][4];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int c = c0 + e;
            int wl = 0, wh = len - 1;
            if (c < nch && isdp && !expl) { wl = nd[b * nch + c] - n0; wh = min(wh, nd[b * nch + c] + n0); }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = p * RB + lane + 64 * j;
                hv[e][j] = (c < nch && n >= wl && n <= wh) ? base[((long)b * nch + c) * stride + n] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = {hv[0][j], hv[1][j]}; v[j + 4] = {0.f, 0.f}; }
    }
    fft512_wave(v, zb, lane, live);
    if (live) {
        float2* o = H + (((long)b * Q + q) * P + p) * RN;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[lane + 64 * j] = zb[lane + 64 * j];
    }
}

// Y_t = sum_p X_{t-p} H_p for TB consecutive t, inverse transform, last 256 samples.  q < npair: clean -> out (and the noise power of these
// samples), q >= npair: direct path -> power and peak, and out_dp where it is given.
__global__ __launch_bounds__(512) void rir_conv_kernel(const float2* __restrict__ X, const float2* __restrict__ H,
                                                       const int* __restrict__ prange, const float* __restrict__ noise, long ns, int nch,
                                                       int nT, int npair, int P, float* __restrict__ out, float* __restrict__ out_dp,
                                                       double* __restrict__ stats, unsigned* __restrict__ peak) {
    __shared__ float2 Z[TB * RZ];
    __shared__ float rsum[TB], rmax[TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T0 = blockIdx.x * TB, q = blockIdx.y, b = blockIdx.z, Q = 2 * npair;
    const int lo = prange[(b * Q + q) * 2];
    const int upper = min(min(prange[(b * Q + q) * 2 + 1], P - 1), T0 + TB - 1);      // X_s is zero for s < 0
    const bool isdp = q >= npair;
    if (isdp && lo > upper) {                            // this stretch of the direct-path signal is exactly zero (uniform: before any barrier)
        if (out_dp) {
            const int c0 = 2 * (q % npair), c1 = c0 + 1;
            for (int i = tid; i < TB * RB; i += 512) {
                const long n = (long)T0 * RB + i;
                if (n < ns) {
                    const long o = ((long)b * ns + n) * nch;
                    out_dp[o + c0] = 0.f;
                    if (c1 < nch) out_dp[o + c1] = 0.f;
                }
            }
        }
        return;
    }

    const float2* Xb = X + (long)b * nT * RN + tid;
    const float2* Hb = H + ((long)b * Q + q) * P * RN + tid;
    auto ldX = [&](int s) -> cpx {
        if (s < 0 || s >= nT) return cpx{0.f, 0.f};
        const float2 x = Xb[(long)s * RN];
        return cpx{x.x, x.y};
    };
    cpx W[TB], acc[TB];
    const int base = T0 - lo;
#pragma unroll
    for (int j = 0; j < TB; ++j) { W[j] = ldX(base + j); acc[j] = {0.f, 0.f}; }
    const int np = upper - lo + 1;
    for (int p0 = 0; p0 < np; p0 += TB) {
#pragma unroll
        for (int r = 0; r < TB; ++r) {
            const int pp = p0 + r;
            if (pp < np) {
                const float2 hq = Hb[(long)(lo + pp) * RN];
                const cpx h = {hq.x, hq.y};
#pragma unroll
                for (int j = 0; j < TB; ++j) {
                    const cpx x = W[(j - r) & (TB - 1)];
                    acc[j].x = fmaf(x.x, h.x, fmaf(-x.y, h.y, acc[j].x));
                    acc[j].y = fmaf(x.x, h.y, fmaf(x.y, h.x, acc[j].y));
                }
                W[(TB - 1 - r) & (TB - 1)] = ldX(base - pp - 1);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TB; ++j) Z[j * RZ + tid] = make_float2(acc[j].x, -acc[j].y);       // conj: inverse = conj(FFT(conj(.))) / N
    __syncthreads();

    const int t = T0 + wave;
    const bool live = t < nT;
    float2* zb = Z + wave * RZ;
    cpx v[8];
    if (live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float2 z = zb[lane + 64 * j]; v[j] = {z.x, z.y}; }
    }
    fft512_wave(v, zb, lane, live);

    const int c0 = 2 * (q % npair), c1 = c0 + 1;
    float s = 0.f, m = 0.f;
    if (live) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long n = (long)t * RB + lane + 64 * j;
            if (n < ns) {
                const float2 z = zb[RB + lane + 64 * j];
                const float y0 = z.x * (1.0f / RN), y1 = -z.y * (1.0f / RN);
                const long o = ((long)b * ns + n) * nch;
                if (isdp) {
                    s = fmaf(y0, y0, s); m = fmaxf(m, fabsf(y0));
                    if (c1 < nch) { s = fmaf(y1, y1, s); m = fmaxf(m, fabsf(y1)); }
                    if (out_dp) {
                        out_dp[o + c0] = y0;
                        if (c1 < nch) out_dp[o + c1] = y1;
                    }
                } else {
                    out[o + c0] = y0;
                    if (c1 < nch) out[o + c1] = y1;
                    if (noise) {
                        const float a = noise[o + c0];
                        s = fmaf(a, a, s);
                        if (c1 < nch) { const float e = noise[o + c1]; s = fmaf(e, e, s); }
                    }
                }
            }
        }
    }
    s = wave_sum(s); m = wave_max(m);
    if (lane == 0) { rsum[wave] = s; rmax[wave] = m; }
    __syncthreads();
    if (tid == 0) {
        double ss = 0.0; float mm = 0.f;
        for (int i = 0; i < TB; ++i) { ss += (double)rsum[i]; mm = fmaxf(mm, rmax[i]); }
        if (isdp) {
            atomicAdd(&stats[b * 2 + 0], ss);
            atomicMax(&peak[b * 2 + 0], __float_as_uint(mm));
        } else if (noise) atomicAdd(&stats[b * 2 + 1], ss);
    }
}

// g = sqrt(P_dp / 10^(snr/10)) / (sqrt(P_n) + 1e-10), in f64 from the f64 sums (add_noise, utils_noise.py:157-176)
__device__ __forceinline__ float noise_gain(const double* stats, int b, float snr_db, long ns, int nch, bool has_noise) {
    if (!has_noise) return 0.f;
    const double cnt = (double)ns * nch;
    const double pdp = stats[b * 2] / cnt, pn = stats[b * 2 + 1] / cnt;
    return (float)(sqrt(pdp / pow(10.0, (double)snr_db / 10.0)) / (sqrt(pn) + 1e-10));
}
__global__ __launch_bounds__(256) void rir_mic_peak_kernel(const float* __restrict__ out, const float* __restrict__ noise,
                                                           const float* __restrict__ snr_db, const double* __restrict__ stats, long ns,
                                                           int nch, unsigned* __restrict__ peak) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float g = noise_gain(stats, b, snr_db[b], ns, nch, noise != nullptr);
    const long per = ns * nch, o = (long)b * per;
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + tid; i < per; i += (long)gridDim.x * 256) {
        const float v = noise ? fmaf(g, noise[o + i], out[o + i]) : out[o + i];
        m = fmaxf(m, fabsf(v));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) atomicMax(&peak[b * 2 + 1], __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}
__global__ __launch_bounds__(256) void rir_mix_final_kernel(float* __restrict__ out, float* __restrict__ out_dp, const float* __restrict__ noise,
                                                            const float* __restrict__ snr_db, const float* __restrict__ gain,
                                                            const double* __restrict__ stats, const unsigned* __restrict__ peak, long ns,
                                                            int nch) {
    const int b = blockIdx.y;
    const float g = noise_gain(stats, b, snr_db[b], ns, nch, noise != nullptr);
    const float value = fmaxf(__uint_as_float(peak[b * 2]), __uint_as_float(peak[b * 2 + 1])), gn = gain[b];
    const long per = ns * nch, o = (long)b * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const float v = noise ? fmaf(g, noise[o + i], out[o + i]) : out[o + i];
        out[o + i] = v / value * gn;
        if (out_dp) out_dp[o + i] = out_dp[o + i] / value * gn;
    }
}

extern "C" long sarssl_rir_mix_workspace_bytes(int nb, long ns, int nch, int lmax, int ldmax) {
    if (nb <= 0 || ns <= 0 || nch < 1 || nch > 8 || lmax < 1 || ldmax < 0) return -1;
    return rir_ws_layout(nullptr, nb, ns, nch, lmax, ldmax).bytes;
}

static int rir_mix_launch(const float* src, const float* rir, const int* rir_len, const float* rir_dp, const int* dp_len, int n0,
                          const float* noise, const float* snr_db, const float* gain, int nb, long ns, int nch, int lmax, int ldmax, void* ws,
                          float* out, float* out_dp, void* stream) {
    SARSSL_REQUIRE(src && rir && rir_len && snr_db && gain && ws && out, "sarssl_rir_mix");
    SARSSL_REQUIRE(nb > 0 && nb <= 65535 && ns > 0 && ns < (1L << 31) - 2 * RN && nch >= 1 && nch <= 8 && lmax >= 1, "sarssl_rir_mix");
    SARSSL_REQUIRE(rir_dp ? (dp_len && ldmax >= 1) : (n0 >= 0 && ldmax == 0), "sarssl_rir_mix(explicit rir_dp + dp_len + ldmax, or a window n0 with ldmax 0)");
    hipStream_t st = (hipStream_t)stream;
    const RirWs w = rir_ws_layout(ws, nb, ns, nch, lmax, ldmax);
    if (hipMemsetAsync(w.stats, 0, sizeof(double) * 2 * nb, st) != hipSuccess || hipMemsetAsync(w.peak, 0, sizeof(unsigned) * 2 * nb, st) != hipSuccess) {
        sarssl_set_error("sarssl_rir_mix: memset failed"); return -2;
    }
    rir_plan_kernel<<<nb, 256, 0, st>>>(rir, rir_len, dp_len, rir_dp ? 1 : 0, n0, nch, lmax, ldmax, w.npair, w.nd, w.prange);
    SARSSL_CHECK_LAUNCH("rir_plan_kernel");
    rir_src_spec_kernel<<<dim3((w.nT + TB - 1) / TB, nb), 512, 0, st>>>(src, ns, w.nT, w.X);
    SARSSL_CHECK_LAUNCH("rir_src_spec_kernel");
    rir_spec_kernel<<<dim3((w.P + TB - 1) / TB, w.Q, nb), 512, 0, st>>>(rir, rir_len, rir_dp, dp_len, n0, nch, lmax, ldmax, w.npair, w.P, w.nd,
                                                                      w.prange, w.H);
    SARSSL_CHECK_LAUNCH("rir_spec_kernel");
    rir_conv_kernel<<<dim3((w.nT + TB - 1) / TB, w.Q, nb), 512, 0, st>>>(w.X, w.H, w.prange, noise, ns, nch, w.nT, w.npair, w.P, out, out_dp, w.stats,
                                                                       w.peak);
    SARSSL_CHECK_LAUNCH("rir_conv_kernel");
    long nblk = (ns * nch + 256 * 8 - 1) / (256 * 8); if (nblk > 256) nblk = 256;
    rir_mic_peak_kernel<<<dim3((int)nblk, nb), 256, 0, st>>>(out, noise, snr_db, w.stats, ns, nch, w.peak);
    SARSSL_CHECK_LAUNCH("rir_mic_peak_kernel");
    rir_mix_final_kernel<<<dim3((int)nblk, nb), 256, 0, st>>>(out, out_dp, noise, snr_db, gain, w.stats, w.peak, ns, nch);
    SARSSL_CHECK_LAUNCH("rir_mix_final_kernel");
    return 0;
}

extern "C" int sarssl_rir_mix(const float* src, const float* rir, const int* rir_len, const float* rir_dp, const int* dp_len, int n0,
                              const float* noise, const float* snr_db, const float* gain, int nb, long ns, int nch, int lmax, int ldmax,
                              void* ws, float* out, void* stream) {
    return rir_mix_launch(src, rir, rir_len, rir_dp, dp_len, n0, noise, snr_db, gain, nb, ns, nch, lmax, ldmax, ws, out, nullptr, stream);
}

// the same launches with the direct-path signal stored: out_dp (B, ns, nch) f32 = dp / max(max|mic|, max|dp|) * gain
extern "C" int sarssl_rir_mix_dp(const float* src, const float* rir, const int* rir_len, const float* rir_dp, const int* dp_len, int n0,
                                 const float* noise, const float* snr_db, const float* gain, int nb, long ns, int nch, int lmax, int ldmax,
                                 void* ws, float* out, float* out_dp, void* stream) {
    SARSSL_REQUIRE(out_dp, "sarssl_rir_mix_dp(out_dp)");
    return rir_mix_launch(src, rir, rir_len, rir_dp, dp_len, n0, noise, snr_db, gain, nb, ns, nch, lmax, ldmax, ws, out, out_dp, stream);
}

// ------------------------------------------------------------------------------------------------ diffuse noise field
// NoiseDataset._diffuse_noise (utils_noise.py:234-253): scipy.signal.stft (periodic Hann 256, hop 64, 128 zeros on both sides), per-bin
// mix X_n = sum_m C[f,m,n] N_m, scipy.signal.istft.  The two spectrum scalings cancel.  C is real and the same at bins k and 256 - k, so
// the mix acts on real and imaginary parts alike: one complex transform carries frames t and t+1 of a channel, unseparated.
#define DN 256
#define DHOP 64
#define DZ 257
__device__ __forceinline__ float hann256(int i) { return 0.5f - 0.5f * cospif((float)i * (1.0f / 128.0f)); }

// frames: (B, M, nfr, 256) f32 = w . IFFT(mixed spectrum) of every frame
__global__ __launch_bounds__(512) void diffuse_frames_kernel(const float* __restrict__ white, const float* __restrict__ C, long ns, int M,
                                                             int nfr, float* __restrict__ frames) {
    __shared__ float2 Z[8 * DZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;      // wave = input channel, then output channel
    const int t0 = blockIdx.x * 2, t1 = t0 + 1, b = blockIdx.y;
    float2* zb = Z + wave * DZ;
    cpx v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        const long n0 = (long)t0 * DHOP - DN / 2 + i, n1 = n0 + DHOP;
        const float w = hann256(i);
        const float a = (n0 >= 0 && n0 < ns) ? white[((long)b * ns + n0) * M + wave] : 0.f;
        const float e = (t1 < nfr && n1 >= 0 && n1 < ns) ? white[((long)b * ns + n1) * M + wave] : 0.f;
        v[j] = {a * w, e * w};
    }
    fft256_wave(v, zb, lane, true);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j, f = k <= DN / 2 ? k : DN - k;
        const float* cf = C + (((long)b * (DN / 2 + 1) + f) * M) * M + wave;           // C[b][f][m][n = wave]
        float yr = 0.f, yi = 0.f;
        for (int m = 0; m < M; ++m) {
            const float c = cf[m * M];
            const float2 z = Z[m * DZ + k];
            yr = fmaf(c, z.x, yr); yi = fmaf(c, z.y, yi);
        }
        v[j] = {yr, -yi};
    }
    __syncthreads();
    fft256_wave(v, zb, lane, true);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = lane + 64 * j;
        const float2 z = zb[i];
        const float w = hann256(i) * (1.0f / DN);
        float* o = frames + (((long)b * M + wave) * nfr + t0) * DN + i;
        o[0] = z.x * w;
        if (t1 < nfr) o[DN] = -z.y * w;
    }
}

// signed maximum through an unsigned atomicMax: order-preserving key of a float (0 = below everything)
__device__ __forceinline__ unsigned fkey(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float funkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// overlap-add / actual window-square sum, boundary removed; signed maximum per item
__global__ __launch_bounds__(256) void diffuse_ola_kernel(const float* __restrict__ frames, long ns, int M, int nfr, float* __restrict__ out,
                                                          unsigned* __restrict__ mx) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const long per = ns * M;
    float m = -INFINITY;
    for (long e = (long)blockIdx.x * 256 + tid; e < per; e += (long)gridDim.x * 256) {
        const int c = (int)(e % M);
        const long i = e / M + DN / 2;
        const int tt = (int)(i / DHOP);
        const float* fb = frames + ((long)b * M + c) * nfr * DN;
        float acc = 0.f, norm = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tt - j;
            if (t >= 0 && t < nfr) {
                const int off = (int)(i - (long)t * DHOP);
                const float w = hann256(off);
                acc += fb[(long)t * DN + off];
                norm = fmaf(w, w, norm);
            }
        }
        const float y = acc / (norm > 1e-10f ? norm : 1.0f);
        out[(long)b * per + e] = y;
        m = fmaxf(m, y);
    }
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) atomicMax(&mx[b], fkey(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}
__global__ __launch_bounds__(256) void diffuse_scale_kernel(float* __restrict__ out, long per, const unsigned* __restrict__ mx) {
    const int b = blockIdx.y;
    const float d = funkey(mx[b]) + 1e-8f;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) out[(long)b * per + e] /= d;
}

extern "C" long sarssl_diffuse_noise_workspace_bytes(int nb, long ns, int m) {
    if (nb <= 0 || ns <= 0 || ns % DHOP != 0 || m < 1 || m > 8) return -1;
    return (long)nb * m * (ns / DHOP + 1) * DN * sizeof(float) + (long)nb * sizeof(unsigned);
}

// white: (B, ns, M) f32; C: (B, 129, M, M) f32 real mixing table (row 0 zero); out: (B, ns, M) f32 = noise / (max(noise) + 1e-8)
extern "C" int sarssl_diffuse_noise(const float* white, const float* C, int nb, long ns, int m, void* ws, float* out, void* stream) {
    SARSSL_REQUIRE(white && C && ws && out && nb > 0 && nb <= 65535 && m >= 1 && m <= 8 && ns > 0 && ns < (1L << 31) - DN, "sarssl_diffuse_noise");
    SARSSL_REQUIRE(ns % DHOP == 0, "sarssl_diffuse_noise(defined for ns % 64 == 0, as scipy's stft / istft round trip is)");
    hipStream_t st = (hipStream_t)stream;
    const int nfr = (int)(ns / DHOP) + 1;
    float* frames = (float*)ws;
    unsigned* mx = (unsigned*)(frames + (long)nb * m * nfr * DN);
    if (hipMemsetAsync(mx, 0, sizeof(unsigned) * nb, st) != hipSuccess) { sarssl_set_error("sarssl_diffuse_noise: memset failed"); return -2; }
    diffuse_frames_kernel<<<dim3((nfr + 1) / 2, nb), 64 * m, 0, st>>>(white, C, ns, m, nfr, frames);
    SARSSL_CHECK_LAUNCH("diffuse_frames_kernel");
    long nblk = (ns * m + 256 * 8 - 1) / (256 * 8); if (nblk > 256) nblk = 256;
    diffuse_ola_kernel<<<dim3((int)nblk, nb), 256, 0, st>>>(frames, ns, m, nfr, out, mx);
    SARSSL_CHECK_LAUNCH("diffuse_ola_kernel");
    diffuse_scale_kernel<<<dim3((int)nblk, nb), 256, 0, st>>>(out, ns * m, mx);
    SARSSL_CHECK_LAUNCH("diffuse_scale_kernel");
    return 0;
}

// ------------------------------------------------------------------------------------------------ white noise
// Standard normal f32 values, Box-Muller over the library's counter hash: element e = sample * M + channel of item (item0 + b) takes the
// cosine (e even) or sine (e odd) branch of pair e / 2.  A pure function of (seed, item, sample, channel) - NOT numpy's stream.
__global__ __launch_bounds__(256) void gauss_fill_kernel(float* __restrict__ out, long per, unsigned long long seed, int item0) {
    const int b = blockIdx.y;
    const uint32_t key = hash_u32((uint32_t)seed ^ hash_u32((uint32_t)(seed >> 32) + 0x9e3779b9u * (uint32_t)(item0 + b + 1)));
    const long npairs = (per + 1) / 2;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npairs; p += (long)gridDim.x * 256) {
        const uint32_t c = (uint32_t)p * 2u;
        const uint32_t h1 = hash_u32(hash_u32(c) ^ key), h2 = hash_u32(hash_u32(c + 1u) ^ key);
        const float u1 = (float)((h1 >> 8) + 1u) * (1.0f / 16777216.0f);          // (0, 1]
        const float u2 = (float)(h2 >> 8) * (1.0f / 16777216.0f);                 // [0, 1)
        const float r = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        float* o = out + (long)b * per + 2 * p;
        o[0] = r * cs;
        if (2 * p + 1 < per) o[1] = r * sn;
    }
}
extern "C" int sarssl_gauss_fill(float* out, int nb, long ns, int m, unsigned long long seed, int item0, void* stream) {
    SARSSL_REQUIRE(out && nb > 0 && nb <= 65535 && ns > 0 && m >= 1 && ns * m < (1L << 32), "sarssl_gauss_fill");
    const long per = ns * m;
    long nblk = (per / 2 + 256 * 4) / (256 * 4); if (nblk > 512) nblk = 512;
    gauss_fill_kernel<<<dim3((int)nblk, nb), 256, 0, (hipStream_t)stream>>>(out, per, seed, item0);
    SARSSL_CHECK_LAUNCH("gauss_fill_kernel");
    return 0;
}

// ------------------------------------------------------------------------------------------------ mixing table
// NoiseDataset._desired_spatial_coherence + _mix_matrix (utils_noise.py:178-232) as rirsynth.mixing_table states them: per (item, bin k)
// the upper Cholesky factor U (U^T U = G) of the spherical coherence G_pq = sinc(w_k d_pq / (c pi)), w_k = 2 pi fs k / 256, unit
// diagonal; bin 0 is zero.  One thread owns one (item, bin): G and then U live in registers (every index below is a compile-time
// constant after unrolling), all arithmetic is f64 and the M x M block is rounded to f32 at its contiguous store.  A pivot <= 0 (or NaN)
// makes the whole block NaN - LAPACK's dpotrf refuses at the same condition.
template <int M>
__global__ __launch_bounds__(64) void mixing_table_kernel(const double* __restrict__ mic, int total, double fs, double c, float* __restrict__ out) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= total) return;
    const int b = t / 129, k = t - b * 129;
    float* o = out + (long)t * (M * M);
    if (k == 0) {
#pragma unroll
        for (int e = 0; e < M * M; ++e) o[e] = 0.0f;
        return;
    }
    const double pi = 3.141592653589793;
    const double w = 2.0 * pi * fs * (double)k / 256.0;
    const double cpi = c * pi;
    double pos[M][3];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int a = 0; a < 3; ++a) pos[m][a] = mic[((long)b * M + m) * 3 + a];
    double U[M][M];
#pragma unroll
    for (int p = 0; p < M; ++p)
#pragma unroll
        for (int q = p; q < M; ++q) {
            if (q == p) { U[p][q] = 1.0; continue; }
            const double dx = pos[p][0] - pos[q][0], dy = pos[p][1] - pos[q][1], dz = pos[p][2] - pos[q][2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            const double x = w * d / cpi;
            const double y = pi * (x == 0.0 ? 1.0e-20 : x);               // numpy.sinc
            U[p][q] = sin(y) / y;
        }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double s = U[j][j];
#pragma unroll
        for (int r = 0; r < j; ++r) s -= U[r][j] * U[r][j];
        ok = ok && (s > 0.0);
        const double piv = sqrt(s);
        U[j][j] = piv;
#pragma unroll
        for (int i = j + 1; i < M; ++i) {
            double v = U[j][i];
#pragma unroll
            for (int r = 0; r < j; ++r) v -= U[r][j] * U[r][i];
            U[j][i] = v / piv;
        }
    }
    const float nanv = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int p = 0; p < M; ++p)
#pragma unroll
        for (int q = 0; q < M; ++q) o[p * M + q] = !ok ? nanv : q < p ? 0.0f : (float)U[p][q];
}

// mic: (B, M, 3) f64; out: (B, 129, M, M) f32
extern "C" int sarssl_mixing_table(const double* mic, int nb, int m, double fs, double c, float* out, void* stream) {
    SARSSL_REQUIRE(m >= 1 && m <= 8, "sarssl_mixing_table(1 to 8 microphones)");
    SARSSL_REQUIRE(mic && out && nb > 0 && nb <= (1 << 20), "sarssl_mixing_table");
    const int total = nb * 129, grid = (total + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    switch (m) {
        case 1: mixing_table_kernel<1><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        case 2: mixing_table_kernel<2><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        case 3: mixing_table_kernel<3><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        case 4: mixing_table_kernel<4><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        case 5: mixing_table_kernel<5><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        case 6: mixing_table_kernel<6><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        case 7: mixing_table_kernel<7><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
        default: mixing_table_kernel<8><<<grid, 64, 0, st>>>(mic, total, fs, c, out); break;
    }
    SARSSL_CHECK_LAUNCH("mixing_table_kernel");
    return 0;
}
