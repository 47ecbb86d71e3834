// Polyphase FIR resampling of measured recordings on the GPU (gfx950): what code/data_generation/gen_real_rir.py asks
// scipy.signal.resample_poly(x, up, down, axis=0) for (window ('kaiser', 5.0), padtype 'constant'), all channels of a file in one launch.
//
// With up / down reduced by their gcd, half = 10 max(up, down) and taps h[0 .. 2 half] = up firwin(2 half + 1, 1 / max(up, down)) (built
// on the host in f64, handed over as f32 - no window maths here):
//
//     y[m][c] = sum over n in [0, n_in) with |m down - n up| <= half of  x[n][c] h[m down - n up + half],   m in [0, ceil(n_in up / down))
//
// realrir.restate_resample is this in f64 numpy, and the authority.
//
// One workgroup owns RS_T consecutive outputs x all channels.  A (output, channel) item belongs to one thread and has ONE f32 accumulator
// that takes its terms in ascending n, one fmaf each; rows outside [0, n_in) are skipped, not added as zeros.  Nothing of that depends on
// the tile, on the staging below or on nch: channel c of a 32-channel call is bit-equal to the column resampled alone, and a file cut into
// chunks (rows [row0, row0 + nrows) present, outputs [m0, m1) asked for) is bit-equal to the one-shot call.  No atomics.
//
// The taps (at most 8821 floats), the input rows the tile needs and the tile's accumulators live in LDS.  The rows are staged RS_STAGE
// floats at a time with coalesced interleaved reads - a tile's span is (RS_T down + 2 half) / up rows, which no fixed buffer holds for
// every ratio; at 48 kHz -> 16 kHz and 32 channels it is two stages - and every item walks the part of its range that lies inside the
// stage, its partial sum parked in LDS in between.  Registers (39 - 50, no scratch) would allow eight waves per SIMD; the dynamic LDS
// of a workgroup - 8 KiB of accumulators, 16 KiB of rows and the whole tap table - decides: 24.2 KiB at 1 : 3 = six workgroups per CU
// (six waves per SIMD), 59 KiB at 160 : 441 = two (two waves per SIMD; a tile touches about 3 500 of those 8 821 taps, and staging only
// them would double that - not built: the corpus this serves is recorded at 48 kHz).  Consecutive lanes take
// consecutive channels of one output, so a 32-lane group reads 32 consecutive LDS words (nch = 32) and one tap (a broadcast); the
// sub-filter an output uses is the phase (m down + half) mod up, reached as the tap index m down - n up + half stepping down by `up`.
//
// sarssl_resample_poly_batch is the same tile body over B crops of a training batch in one launch (realsig.RealMixLoader: B recordings cut
// at random, each at most a few seconds): the batch index is the grid's y and changes no arithmetic, the crop lengths are read on the device.
#include "common.h"

#define RS_T 64                     // outputs per workgroup
#define RS_THREADS 256
#define RS_STAGE 4096               // floats of input per stage (16 KiB; with the accumulators and the largest tap table 59 KiB of LDS)
#define RS_MAXCH 32
#define RS_MAXRATIO 441

__device__ __forceinline__ float rs_load(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float rs_load(const short* p, long i) { return (float)p[i] * (1.0f / 32768.0f); }
__device__ __forceinline__ void rs_store(float* p, long i, float y) { p[i] = y; }
// roomsim.pcm16's rule (sarssl_pcm16_pack): rint(32767 y) in f64, ties to even, saturated to +-32767, NaN -> 0
__device__ __forceinline__ void rs_store(short* p, long i, float y) {
    double v = rint((double)y * 32767.0);
    v = v > 32767.0 ? 32767.0 : (v < -32767.0 ? -32767.0 : v);
    p[i] = (v == v) ? (short)(int)v : (short)0;
}

// first / last input row of output m, clipped to the signal
__device__ __host__ __forceinline__ long rs_first(long m, int up, int down, int half) {
    const long a = m * down - half;
    return a <= 0 ? 0 : (a + up - 1) / up;
}
__device__ __host__ __forceinline__ long rs_last(long m, int up, int down, int half, long n_in) {
    const long b = (m * down + half) / up;
    return b < n_in - 1 ? b : n_in - 1;
}

// Outputs [mt0, mt1) (at most RS_T of them) of a signal of n_in rows whose row row0 is x[0], written to out[0 ...]: the one body of the
// single-file and of the batched launch, so that an item of a batch cannot differ from the same signal resampled alone.
template <typename TI, typename TO>
__device__ __forceinline__ void rs_tile(const TI* __restrict__ x, long row0, long n_in, int nch, int up, int down, int half,
                                        const float* __restrict__ taps, long mt0, long mt1, TO* __restrict__ out) {
    extern __shared__ float rs_lds[];
    const int ntaps = 2 * half + 1;
    float* accs = rs_lds;                                   // [RS_T * RS_MAXCH]
    float* xs = accs + RS_T * RS_MAXCH;                     // [RS_STAGE]
    float* hs = xs + RS_STAGE;                              // [ntaps]
    const int tid = threadIdx.x;
    const int nitem = (int)(mt1 - mt0) * nch;
    for (int i = tid; i < ntaps; i += RS_THREADS) hs[i] = taps[i];
    for (int it = tid; it < nitem; it += RS_THREADS) accs[it] = 0.f;

    // output mt0 + ml: first row ceil((A0 + ml down) / up), last row floor((B0 + ml down) / up), both clipped; the 64-bit divisions are
    // done once for the tile and the per-item ones fit 32 bits (ml down < 64 * 441)
    const long A0 = mt0 * down - half, B0 = mt0 * down + half;
    const long qa = A0 >= 0 ? A0 / up : -((-A0 + up - 1) / up), qb = B0 / up;
    const int ra = (int)(A0 - qa * up), rb = (int)(B0 - qb * up);
    const long t_lo = rs_first(mt0, up, down, half), t_hi = rs_last(mt1 - 1, up, down, half, n_in);
    const int rows = RS_STAGE / nch;
    for (long s0 = t_lo; s0 <= t_hi; s0 += rows) {
        const long s1 = s0 + rows <= t_hi + 1 ? s0 + rows : t_hi + 1;
        const int nel = (int)(s1 - s0) * nch;
        const long g = (s0 - row0) * nch;
        __syncthreads();                                    // the previous stage is consumed (first pass: hs and accs are written)
        for (int i = tid; i < nel; i += RS_THREADS) xs[i] = rs_load(x, g + i);
        __syncthreads();
        for (int it = tid; it < nitem; it += RS_THREADS) {
            const int ml = it / nch, c = it - ml * nch;
            long a = qa + (ra + ml * down + up - 1) / up, b = qb + (rb + ml * down) / up;
            a = a < s0 ? s0 : a;                            // (s0 >= 0: the clip at row 0 is in t_lo)
            b = b < s1 - 1 ? b : s1 - 1;                    // (s1 - 1 <= t_hi <= n_in - 1)
            if (a <= b) {
                const float* xp = xs + (int)(a - s0) * nch + c;
                int ti = (int)(B0 + (long)ml * down - a * up);
                const int k = (int)(b - a) + 1;
                float acc = accs[it];
#pragma unroll 4
                for (int r = 0; r < k; ++r) { acc = fmaf(xp[0], hs[ti], acc); xp += nch; ti -= up; }
                accs[it] = acc;
            }
        }
    }
    __syncthreads();
    for (int it = tid; it < nitem; it += RS_THREADS) rs_store(out, it, accs[it]);
}

template <typename TI, typename TO>
__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(const TI* __restrict__ x, long row0, long n_in, int nch, int up, int down,
                                                                    int half, const float* __restrict__ taps, long m0, long m1,
                                                                    TO* __restrict__ out) {
    const long mt0 = m0 + (long)blockIdx.x * RS_T;
    const long mt1 = mt0 + RS_T < m1 ? mt0 + RS_T : m1;
    rs_tile(x, row0, n_in, nch, up, down, half, taps, mt0, mt1, out + (mt0 - m0) * nch);
}

// A batch of crops, one ratio: blockIdx.y is the item, blockIdx.x the tile of its (n_out_max, nch) slot.  Item b is n_in[b] rows (clamped to
// [0, n_max]: the lengths live on the device, nothing on the host has seen them) at x + b n_max nch; its ceil(n_in[b] up / down) outputs
// are rs_tile's, the rows of the slot behind them are written as zeros by the workgroup that owns their tile - the slot is never cleared.
template <typename TI, typename TO>
__global__ __launch_bounds__(RS_THREADS) void resample_poly_batch_kernel(const TI* __restrict__ x, const int* __restrict__ n_in, long n_max,
                                                                          int nch, int up, int down, int half,
                                                                          const float* __restrict__ taps, long n_out_max,
                                                                          TO* __restrict__ out) {
    const long b = blockIdx.y;
    long n = n_in[b];
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    const long n_out = (n * up + down - 1) / down;          // <= n_out_max, as n <= n_max
    const long mt0 = (long)blockIdx.x * RS_T;
    const long me = mt0 + RS_T < n_out_max ? mt0 + RS_T : n_out_max;        // the tile's end in the slot
    const long mt1 = me < n_out ? me : n_out;                               // ... and in the item
    TO* o = out + (b * n_out_max + mt0) * nch;
    if (mt0 < mt1) rs_tile(x + b * n_max * nch, 0, n, nch, up, down, half, taps, mt0, mt1, o);      // (uniform over the workgroup)
    const int z0 = mt0 < mt1 ? (int)(mt1 - mt0) * nch : 0, z1 = (int)(me - mt0) * nch;
    for (int it = z0 + (int)threadIdx.x; it < z1; it += RS_THREADS) rs_store(o, it, 0.f);
}

static bool rs_ratio_ok(int nch, int up, int down) {
    if (nch < 1 || nch > RS_MAXCH || up < 1 || down < 1 || up > RS_MAXRATIO || down > RS_MAXRATIO) return false;
    int a = up, b = down;
    while (b) { const int t = a % b; a = b; b = t; }
    return a == 1;                                          // reduced: the caller divides by the gcd
}

// 1: sarssl_resample_poly takes this (nch, up, down); 0: it refuses (nch outside 1..32, up or down outside 1..441 or not reduced)
extern "C" int sarssl_resample_poly_supported(int nch, int up, int down) { return rs_ratio_ok(nch, up, down) ? 1 : 0; }

extern "C" int sarssl_resample_poly(const void* x, int in_dtype, long row0, long nrows, long n_in, int nch, int up, int down,
                                    const float* taps, int ntaps, long n_out, long m0, long m1, void* out, int out_dtype, void* stream) {
    SARSSL_REQUIRE(x && taps && out, "sarssl_resample_poly");
    SARSSL_REQUIRE(rs_ratio_ok(nch, up, down), "sarssl_resample_poly(nch 1..32, up and down 1..441 and reduced by their gcd)");
    SARSSL_REQUIRE((in_dtype == SARSSL_F32 || in_dtype == SARSSL_I16) && (out_dtype == SARSSL_F32 || out_dtype == SARSSL_I16),
                   "sarssl_resample_poly(f32 or PCM-16 in and out)");
    SARSSL_REQUIRE(n_in > 0 && n_in <= (1L << 40) && nrows > 0 && row0 >= 0 && row0 + nrows <= n_in, "sarssl_resample_poly(empty input, or rows outside the signal)");
    const int half = 10 * (up > down ? up : down);
    SARSSL_REQUIRE(ntaps == 2 * half + 1, "sarssl_resample_poly(2 * 10 max(up, down) + 1 taps)");
    SARSSL_REQUIRE(n_out == (n_in * up + down - 1) / down, "sarssl_resample_poly(n_out = ceil(n_in up / down))");
    SARSSL_REQUIRE(m0 >= 0 && m0 < m1 && m1 <= n_out, "sarssl_resample_poly(0 <= m0 < m1 <= n_out)");
    SARSSL_REQUIRE(rs_first(m0, up, down, half) >= row0 && rs_last(m1 - 1, up, down, half, n_in) < row0 + nrows,
                   "sarssl_resample_poly(the rows present do not cover outputs [m0, m1): a chunk needs a halo of ceil(half / up) rows)");
    const long nblk = (m1 - m0 + RS_T - 1) / RS_T;
    SARSSL_REQUIRE(nblk <= 0x7fffffffl, "sarssl_resample_poly");
    const size_t lds = (size_t)(RS_T * RS_MAXCH + RS_STAGE + ntaps) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk);
    if (in_dtype == SARSSL_F32 && out_dtype == SARSSL_F32)
        resample_poly_kernel<float, float><<<grid, RS_THREADS, lds, st>>>((const float*)x, row0, n_in, nch, up, down, half, taps, m0, m1, (float*)out);
    else if (in_dtype == SARSSL_F32)
        resample_poly_kernel<float, short><<<grid, RS_THREADS, lds, st>>>((const float*)x, row0, n_in, nch, up, down, half, taps, m0, m1, (short*)out);
    else if (out_dtype == SARSSL_F32)
        resample_poly_kernel<short, float><<<grid, RS_THREADS, lds, st>>>((const short*)x, row0, n_in, nch, up, down, half, taps, m0, m1, (float*)out);
    else
        resample_poly_kernel<short, short><<<grid, RS_THREADS, lds, st>>>((const short*)x, row0, n_in, nch, up, down, half, taps, m0, m1, (short*)out);
    SARSSL_CHECK_LAUNCH("resample_poly_kernel");
    return 0;
}

// 1: sarssl_resample_poly_batch takes this (nb, nch, up, down); 0: it refuses (the single-file bounds, or nb outside 1..65535 = the grid's y)
extern "C" int sarssl_resample_poly_batch_supported(int nb, int nch, int up, int down) {
    return nb >= 1 && nb <= 65535 && rs_ratio_ok(nch, up, down) ? 1 : 0;
}

extern "C" int sarssl_resample_poly_batch(const void* x, int in_dtype, const int* n_in, int nb, long n_max, int nch, int up, int down,
                                          const float* taps, int ntaps, long n_out_max, void* out, int out_dtype, void* stream) {
    SARSSL_REQUIRE(x && n_in && taps && out, "sarssl_resample_poly_batch");
    SARSSL_REQUIRE(nb >= 1 && nb <= 65535, "sarssl_resample_poly_batch(1..65535 items)");
    SARSSL_REQUIRE(rs_ratio_ok(nch, up, down), "sarssl_resample_poly_batch(nch 1..32, up and down 1..441 and reduced by their gcd)");
    SARSSL_REQUIRE((in_dtype == SARSSL_F32 || in_dtype == SARSSL_I16) && (out_dtype == SARSSL_F32 || out_dtype == SARSSL_I16),
                   "sarssl_resample_poly_batch(f32 or PCM-16 in and out)");
    SARSSL_REQUIRE(n_max > 0 && n_max <= (1L << 40), "sarssl_resample_poly_batch(empty input)");
    const int half = 10 * (up > down ? up : down);
    SARSSL_REQUIRE(ntaps == 2 * half + 1, "sarssl_resample_poly_batch(2 * 10 max(up, down) + 1 taps)");
    SARSSL_REQUIRE(n_out_max == (n_max * up + down - 1) / down, "sarssl_resample_poly_batch(n_out_max = ceil(n_max up / down))");
    const long nblk = (n_out_max + RS_T - 1) / RS_T;
    SARSSL_REQUIRE(nblk <= 0x7fffffffl, "sarssl_resample_poly_batch");
    const size_t lds = (size_t)(RS_T * RS_MAXCH + RS_STAGE + ntaps) * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nblk, (unsigned)nb);
    if (in_dtype == SARSSL_F32 && out_dtype == SARSSL_F32)
        resample_poly_batch_kernel<float, float><<<grid, RS_THREADS, lds, st>>>((const float*)x, n_in, n_max, nch, up, down, half, taps, n_out_max, (float*)out);
    else if (in_dtype == SARSSL_F32)
        resample_poly_batch_kernel<float, short><<<grid, RS_THREADS, lds, st>>>((const float*)x, n_in, n_max, nch, up, down, half, taps, n_out_max, (short*)out);
    else if (out_dtype == SARSSL_F32)
        resample_poly_batch_kernel<short, float><<<grid, RS_THREADS, lds, st>>>((const short*)x, n_in, n_max, nch, up, down, half, taps, n_out_max, (float*)out);
    else
        resample_poly_batch_kernel<short, short><<<grid, RS_THREADS, lds, st>>>((const short*)x, n_in, n_max, nch, up, down, half, taps, n_out_max, (short*)out);
    SARSSL_CHECK_LAUNCH("resample_poly_batch_kernel");
    return 0;
}
