// The source crops of the online signal loader (onlinesig.OnlineSignalLoader) from a speech corpus that lives on the device as one flat
// PCM-16 array (rirsynth.DeviceSourceBank):
//   sarssl_src_gather   item b = samples [start, start + ns) of the concatenation of its segments (utterances of one speaker, wrapping to
//                       the speaker's first), as s / 32768 minus the crop's mean - what rirsynth.SourceBank.draw returns, without a file
//                       being opened or a sample crossing the bus.
// The crop's sum is a sum of int16 values: exact as a 64-bit integer, so every item is BIT-EQUAL to the host's f64 arithmetic whatever
// the fold order.  One workgroup per item, no atomics; an item's result does not depend on its position in the batch.
#include "common.h"
#include <vector>

#define SB_THREADS 256
#define SB_MAXSEG 32

struct SrcItem {
    long long off[SB_MAXSEG];    // where each segment starts in the bank
    int cum[SB_MAXSEG + 1];      // samples in front of each segment, counted from the crop's first: cum[0] = -start
    int nseg;
};

__global__ __launch_bounds__(SB_THREADS) void src_gather_kernel(const short* __restrict__ bank, const SrcItem* __restrict__ items, int ns,
                                                                float* __restrict__ out) {
    __shared__ long long s_off[SB_MAXSEG];
    __shared__ int s_cum[SB_MAXSEG + 1];
    __shared__ long long s_part[SB_THREADS / 64];
    const SrcItem* it = items + blockIdx.x;
    const int tid = threadIdx.x, nseg = it->nseg;
    if (tid < SB_MAXSEG) s_off[tid] = it->off[tid < nseg ? tid : 0];
    if (tid <= SB_MAXSEG) s_cum[tid] = it->cum[tid <= nseg ? tid : nseg];
    __syncthreads();
    // pass 1: the crop's sum.  A thread's samples ascend, so its segment index only moves forward.
    long long sum = 0;
    int j = 0;
    for (int i = tid; i < ns; i += SB_THREADS) {
        while (j + 1 < nseg && i >= s_cum[j + 1]) ++j;
        sum += (long long)bank[s_off[j] + (i - s_cum[j])];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = sum;
    __syncthreads();
    long long total = 0;
#pragma unroll
    for (int w = 0; w < SB_THREADS / 64; ++w) total += s_part[w];
    // numpy's s.mean(): the exact sum of the f64 samples (multiples of 2^-15 below 2^17), one division
    const double mean = ((double)total * (1.0 / 32768.0)) / (double)ns;
    float* o = out + (long)blockIdx.x * ns;
    j = 0;
    for (int i = tid; i < ns; i += SB_THREADS) {
        while (j + 1 < nseg && i >= s_cum[j + 1]) ++j;
        o[i] = (float)((double)bank[s_off[j] + (i - s_cum[j])] * (1.0 / 32768.0) - mean);
    }
}

extern "C" int sarssl_src_gather(const short* bank, long bank_len, const long* seg_off, const int* seg_len, const int* nseg,
                                 const long* crop_start, int nb, long ns, void* ws, long ws_bytes, float* out, void* stream) {
    SARSSL_REQUIRE(nb >= 1 && nb <= 65535, "sarssl_src_gather(B 1..65535)");
    SARSSL_REQUIRE(ns >= 1 && ns <= 0x3fffffffl, "sarssl_src_gather(Ns 1..2^30 - 1)");
    SARSSL_REQUIRE(bank && seg_off && seg_len && nseg && crop_start && ws && out, "sarssl_src_gather");
    SARSSL_REQUIRE(bank_len >= 1, "sarssl_src_gather(an empty bank)");
    SARSSL_REQUIRE(ws_bytes >= (long)nb * (long)sizeof(SrcItem), "sarssl_src_gather(ws holds 392 bytes per item)");
    std::vector<SrcItem> items(nb);
    for (int b = 0; b < nb; ++b) {
        SARSSL_REQUIRE(nseg[b] >= 1 && nseg[b] <= SB_MAXSEG, "sarssl_src_gather(nseg 1..32)");
        SARSSL_REQUIRE(crop_start[b] >= 0 && crop_start[b] <= 0x3fffffffl, "sarssl_src_gather(crop start 0..2^30 - 1)");
        SrcItem& it = items[b];
        long pos = -crop_start[b];
        for (int s = 0; s < SB_MAXSEG; ++s) {
            if (s < nseg[b]) {
                const long off = seg_off[(long)b * SB_MAXSEG + s], len = seg_len[(long)b * SB_MAXSEG + s];
                SARSSL_REQUIRE(off >= 0 && len >= 1 && off <= bank_len - len, "sarssl_src_gather(a segment lies inside the bank)");
                it.off[s] = off;
                it.cum[s] = (int)pos;
                pos += len;
                SARSSL_REQUIRE(pos <= 0x7fffffffl, "sarssl_src_gather(the segments of an item hold less than 2^31 samples)");
            } else {
                it.off[s] = 0;
                it.cum[s] = (int)pos;
            }
        }
        it.cum[SB_MAXSEG] = (int)pos;
        it.nseg = nseg[b];
        SARSSL_REQUIRE(pos >= ns, "sarssl_src_gather(the segments cover the crop)");     // pos: the samples from the crop's first on
    }
    hipStream_t st = (hipStream_t)stream;
    // the rows come from this call's own host memory: the copy is waited for before the call returns
    if (hipMemcpyAsync(ws, items.data(), (size_t)nb * sizeof(SrcItem), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        sarssl_set_error("sarssl_src_gather: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    hipLaunchKernelGGL(src_gather_kernel, dim3(nb), dim3(SB_THREADS), 0, st, bank, (const SrcItem*)ws, (int)ns, out);
    SARSSL_CHECK_LAUNCH("sarssl_src_gather");
    return 0;
}
