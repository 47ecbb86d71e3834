// Image-source room impulse responses, rendered on the GPU (gfx950): the hot part of the simulated-RIR generator (roomsim.py), i.e. what
// the reference asks a CUDA-only third-party library for in RoomImpulseResponse.generate_rir (code/data_generation/utils_simu_rir_sig.py:
// 475-508).  The arithmetic is DEFINED by roomsim.restate_ism (f64 numpy); see include/sarssl_hip.h.
//
// sarssl_ism_rir, four launches, no float atomics and nothing read back:
//   ism_image_kernel   one thread per image: Allen-Berkley position and wall factor in f64, then per microphone ONE f64 square root ->
//                      integer delay, f32 fraction, f32 amplitude (SoA in the workspace)
//   ism_accum_kernel   output-stationary: a workgroup owns 256 output samples of one (item, microphone), sweeps the item's image list 256
//                      at a time, keeps by ballot compaction (in image order) those whose 8 ms window overlaps its samples, and every thread
//                      adds the kept images' taps to its own sample in that order - the same bits run to run and at any batch position
//   ism_level_kernel   per (item, microphone): absolute peak, mean power of the 128-sample frames behind it, intercept at the given slope
//   ism_tail_kernel    samples [n_ism, n_len): noise * 10^((slope n / fs + level) / 20); [n_len, lmax): zero
// Taps without per-sample transcendentals: sin(pi (j - f)) = -(-1)^j sin(pi f); cos(2 pi (j - f) / W) from a W-entry table and two
// per-image values by angle addition; the x = 0 tap is the limit 1.
#include "common.h"

#define IW 128              // window length in samples (8 ms at 16 kHz), also the frame length of the level fit
#define IH 64               // half window
#define IB 256              // output samples per workgroup = threads = images per sweep step
#define ISM_MAX_IMAGES (1 << 20)
#define ISM_DEAD 0x3fffffff // delay of an image that contributes nowhere

struct IsmWs {
    int* n0;                // [nb][nch][nimg_max] integer part of the delay
    float* fr;              // fraction in [0, 1]
    float* amp;             // wall factors / (4 pi d)
    float* level;           // [nb][nch] dB
    long bytes;
};
static IsmWs ism_ws_layout(void* base, int nb, int nch, int nimg_max) {
    IsmWs w;
    char* p = (char*)base;
    const long n = (long)nb * nch * nimg_max;
    long o = 0;
    w.n0 = (int*)(p + o); o += n * sizeof(int);
    w.fr = (float*)(p + o); o += n * sizeof(float);
    w.amp = (float*)(p + o); o += n * sizeof(float);
    w.level = (float*)(p + o); o += ((long)nb * nch * sizeof(float) + 15) / 16 * 16;
    w.bytes = o;
    return w;
}

__device__ __forceinline__ int ism_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ double ism_powi(double b, int e) {
    double r = 1.0;
    for (; e > 0; e >>= 1, b *= b) if (e & 1) r *= b;
    return r;
}
// image index i of N along one axis -> coordinate (1 - 2q) s + 2 k L and wall factor beta0^|k - q| beta1^|k|
__device__ __forceinline__ void ism_axis(int i, int N, double s, double L, float b0, float b1, double& pos, double& g) {
    const int n = i - N / 2, q = n & 1, k = (n + q) / 2;
    pos = (1 - 2 * q) * s + 2.0 * k * L;
    g = ism_powi((double)b0, abs(k - q)) * ism_powi((double)b1, abs(k));
}

__global__ __launch_bounds__(256) void ism_image_kernel(const double* __restrict__ room, const float* __restrict__ beta,
                                                        const double* __restrict__ src, const double* __restrict__ mic,
                                                        const int* __restrict__ nb_img, const int* __restrict__ n_ism, double fs, double c,
                                                        int nch, int nism_max, int nimg_max, int* __restrict__ n0, float* __restrict__ fr,
                                                        float* __restrict__ amp) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nimg_max) return;
    const int Nx = max(nb_img[b * 3], 1), Ny = max(nb_img[b * 3 + 1], 1), Nz = max(nb_img[b * 3 + 2], 1);
    const long nimg = (long)Nx * Ny * Nz;
    const int nism = ism_clampi(n_ism[b], 1, nism_max);
    const bool live = i < nimg;
    double px = 0, py = 0, pz = 0, g = 0;
    if (live) {
        const int iz = i % Nz, iy = (i / Nz) % Ny, ix = i / (Nz * Ny);
        double gx, gy, gz;
        ism_axis(ix, Nx, src[b * 3], room[b * 3], beta[b * 6], beta[b * 6 + 1], px, gx);
        ism_axis(iy, Ny, src[b * 3 + 1], room[b * 3 + 1], beta[b * 6 + 2], beta[b * 6 + 3], py, gy);
        ism_axis(iz, Nz, src[b * 3 + 2], room[b * 3 + 2], beta[b * 6 + 4], beta[b * 6 + 5], pz, gz);
        g = gx * gy * gz;
    }
    for (int m = 0; m < nch; ++m) {
        const long o = ((long)b * nch + m) * nimg_max + i;
        int d0 = ISM_DEAD; float f = 0.f, a = 0.f;
        if (live) {
            const double* mp = mic + ((long)b * nch + m) * 3;
            const double dx = px - mp[0], dy = py - mp[1], dz = pz - mp[2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            const double tau = d / c * fs, fl = floor(tau);
            if (d > 0.0 && fl - IH < (double)nism) {                 // (an image on top of a microphone has no finite amplitude: left out)
                d0 = (int)fl; f = (float)(tau - fl); a = (float)(g / (4.0 * 3.14159265358979323846 * d));
            }
        }
        n0[o] = d0; fr[o] = f; amp[o] = a;
    }
}

__global__ __launch_bounds__(IB) void ism_accum_kernel(const int* __restrict__ n0, const float* __restrict__ fr, const float* __restrict__ amp,
                                                       const int* __restrict__ nb_img, const int* __restrict__ n_ism, int nch, int lmax,
                                                       int nism_max, int nimg_max, float* __restrict__ out) {
    __shared__ float tc[IW], ts[IW];
    __shared__ int ld0[IB];
    __shared__ float lf[IB], la[IB], lq[IB], lcw[IB], lsw[IB];
    __shared__ int cnt[IB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x, m = blockIdx.y, b = blockIdx.z;
    const int nism = ism_clampi(n_ism[b], 1, nism_max);
    const int lo = blk * IB;
    if (lo >= nism) return;                                          // uniform: before any barrier
    const int hi = min(lo + IB, nism) - 1;                           // last sample of this block inside the image part
    if (tid < IW) { float s, cc; sincospif((float)tid * (2.0f / IW), &s, &cc); tc[tid] = cc; ts[tid] = s; }
    long nimg = (long)max(nb_img[b * 3], 1) * max(nb_img[b * 3 + 1], 1) * max(nb_img[b * 3 + 2], 1);
    if (nimg > nimg_max) nimg = nimg_max;
    const long base = ((long)b * nch + m) * nimg_max;
    const int n = lo + tid;
    float acc = 0.f;
    __syncthreads();
    for (long i0 = 0; i0 < nimg; i0 += IB) {
        const long i = i0 + tid;
        int d0 = ISM_DEAD; float f = 0.f, a = 0.f;
        if (i < nimg) { d0 = n0[base + i]; f = fr[base + i]; a = amp[base + i]; }
        // samples d0 - 63 .. d0 + 64 (and d0 - 64 when f == 0, where the window is zero) can be touched
        const bool hit = d0 != ISM_DEAD && d0 + IH >= lo && d0 - IH <= hi;
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) cnt[wave] = __popcll(mask);
        __syncthreads();
        int off = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < IB / 64; ++w) { if (w < wave) off += cnt[w]; total += cnt[w]; }
        if (hit) {
            float sw, cw;
            sincospif(f * (2.0f / IW), &sw, &cw);
            ld0[off] = d0; lf[off] = f; la[off] = a;
            lq[off] = -a * sinpif(f) * (0.5f / 3.14159265358979323846f);
            lcw[off] = cw; lsw[off] = sw;
        }
        __syncthreads();
        if (n <= hi) {
            for (int k = 0; k < total; ++k) {
                const int j = n - ld0[k];
                if (j >= -IH && j <= IH) {
                    const float x = (float)j - lf[k];
                    if (x >= -(float)IH) {
                        const float w = 1.0f + fmaf(tc[j & (IW - 1)], lcw[k], ts[j & (IW - 1)] * lsw[k]);
                        const float q = (j & 1) ? -lq[k] : lq[k];
                        acc += x == 0.f ? la[k] : q * w * __builtin_amdgcn_rcpf(x);
                    }
                }
            }
        }
    }
    if (n <= hi) out[((long)b * nch + m) * lmax + n] = acc;
}

// level[b][m]: least-squares intercept at fixed slope through 10 log10 of the mean power of the 128-sample frames of the image part that
// start at the first multiple of 128 at least 128 samples behind the first index of max |h| and lie inside n_ism; frame time = its centre
__global__ __launch_bounds__(256) void ism_level_kernel(const float* __restrict__ out, const int* __restrict__ n_ism,
                                                        const float* __restrict__ tail_slope, double fs, int nch, int lmax,
                                                        int nism_max, float* __restrict__ level) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ double sy[4];
    const int m = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nism = ism_clampi(n_ism[b], 1, nism_max);
    const float* h = out + ((long)b * nch + m) * lmax;
    float bv = -1.f; int bi = 0x7fffffff;
    for (int n = tid; n < nism; n += 256) {
        const float x = fabsf(h[n]);
        if (x > bv) { bv = x; bi = n; }                               // strictly greater: the first index wins inside a thread
    }
    sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float ov = sv[tid + s]; const int oi = si[tid + s];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        __syncthreads();
    }
    const int peak = si[0] == 0x7fffffff ? 0 : si[0];              // (all NaN)
    const int start = (peak + IW + IW - 1) / IW * IW;
    const int nfr = nism > start ? (nism - start) / IW : 0;
    double ysum = 0.0;
    for (int k = wave; k < nfr; k += 4) {                             // a wave per frame, two samples per lane
        const float a = h[start + k * IW + lane], e = h[start + k * IW + 64 + lane];
        double p = (double)a * (double)a + (double)e * (double)e;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
        ysum += 10.0 * log10(p / IW + 1e-30);
    }
    if (lane == 0) sy[wave] = ysum;
    __syncthreads();
    if (tid == 0) {
        float lv = -INFINITY;                                         // fewer than two frames: no tail (the host layer refuses the shape)
        if (nfr >= 2) {
            const double ymean = (sy[0] + sy[1] + sy[2] + sy[3]) / nfr;
            const double tmean = ((double)start + 0.5 * (IW - 1) + 0.5 * IW * (nfr - 1)) / fs;
            lv = (float)(ymean - (double)tail_slope[b] * tmean);
        }
        level[b * nch + m] = lv;
    }
}

__global__ __launch_bounds__(256) void ism_tail_kernel(const float* __restrict__ noise, const int* __restrict__ n_ism,
                                                       const int* __restrict__ n_len, const float* __restrict__ tail_slope,
                                                       const float* __restrict__ level, float fs, int nch, int lmax, int nism_max,
                                                       float* __restrict__ out) {
    const int m = blockIdx.y, b = blockIdx.z;
    const int nism = ism_clampi(n_ism[b], 1, nism_max), nlen = ism_clampi(n_len[b], nism, lmax);
    const int n = nism + blockIdx.x * 256 + threadIdx.x;
    if (n >= lmax) return;
    const long o = ((long)b * nch + m) * lmax + n;
    float v = 0.f;
    if (n < nlen && noise) {
        const float db = fmaf(tail_slope[b], (float)n / fs, level[b * nch + m]);
        v = noise[o] * exp2f(db * 0.16609640474436813f);             // 10^(db / 20), log2(10) / 20
    }
    out[o] = v;
}

static bool ism_shape_ok(int nb, int nch, int lmax, int nism_max, int nimg_max) {
    return nb > 0 && nb <= 65535 && nch >= 1 && nch <= 8 && lmax >= 1 && lmax <= (1 << 24) && nism_max >= 1 && nism_max <= lmax &&
           nimg_max >= 1 && nimg_max <= ISM_MAX_IMAGES;
}

extern "C" long sarssl_ism_workspace_bytes(int nb, int nch, int lmax, int nism_max, int nimg_max) {
    if (!ism_shape_ok(nb, nch, lmax, nism_max, nimg_max)) return -1;
    return ism_ws_layout(nullptr, nb, nch, nimg_max).bytes;
}

extern "C" int sarssl_ism_rir(const double* room, const float* beta, const double* src, const double* mic, const int* nb_img,
                              const int* n_ism, const int* n_len, const float* tail_slope, const float* noise, double fs, double c,
                              int nb, int nch, int lmax, int nism_max, int nimg_max, void* ws, float* out, void* stream) {
    SARSSL_REQUIRE(room && beta && src && mic && nb_img && n_ism && n_len && tail_slope && ws && out, "sarssl_ism_rir");
    SARSSL_REQUIRE(nch >= 1 && nch <= 8, "sarssl_ism_rir(1 to 8 microphones)");
    SARSSL_REQUIRE(nimg_max >= 1 && nimg_max <= ISM_MAX_IMAGES, "sarssl_ism_rir(at most 2^20 images per RIR)");
    SARSSL_REQUIRE(ism_shape_ok(nb, nch, lmax, nism_max, nimg_max), "sarssl_ism_rir");
    SARSSL_REQUIRE(noise || lmax == nism_max, "sarssl_ism_rir(n_len > n_ism needs the tail's noise)");
    SARSSL_REQUIRE(fs > 0.0 && c > 0.0, "sarssl_ism_rir");
    hipStream_t st = (hipStream_t)stream;
    const IsmWs w = ism_ws_layout(ws, nb, nch, nimg_max);
    ism_image_kernel<<<dim3((nimg_max + 255) / 256, nb), 256, 0, st>>>(room, beta, src, mic, nb_img, n_ism, fs, c, nch, nism_max, nimg_max, w.n0,
                                                                      w.fr, w.amp);
    SARSSL_CHECK_LAUNCH("ism_image_kernel");
    ism_accum_kernel<<<dim3((nism_max + IB - 1) / IB, nch, nb), IB, 0, st>>>(w.n0, w.fr, w.amp, nb_img, n_ism, nch, lmax, nism_max, nimg_max, out);
    SARSSL_CHECK_LAUNCH("ism_accum_kernel");
    if (noise) {
        ism_level_kernel<<<dim3(nch, nb), 256, 0, st>>>(out, n_ism, tail_slope, fs, nch, lmax, nism_max, w.level);
        SARSSL_CHECK_LAUNCH("ism_level_kernel");
    }
    if (lmax > 1) {                                                   // (n_ism >= 1: with lmax == 1 nothing lies behind the image part)
        ism_tail_kernel<<<dim3((lmax - 1 + 255) / 256, nch, nb), 256, 0, st>>>(noise, n_ism, n_len, tail_slope, w.level, (float)fs, nch, lmax,
                                                                             nism_max, out);
        SARSSL_CHECK_LAUNCH("ism_tail_kernel");
    }
    return 0;
}
