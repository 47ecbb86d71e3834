// One-wave FFTs of the RIR renderer (rirmix.hip): fft512_wave and its helpers as in the STFT front-end (stft.hip keeps its own copy,
// the front-end's object code stays what it was), and the 256-point companion.
#pragma once
#include "common.h"

struct cpx { float x, y; };
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cpx cmul(cpx a, cpx b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cpx mul_mi(cpx a) { return {a.y, -a.x}; }   // a * (-i)

__device__ __forceinline__ void dft8(cpx* x) {
    cpx a0 = cadd(x[0], x[4]), a4 = csub(x[0], x[4]), a2 = cadd(x[2], x[6]), a6 = mul_mi(csub(x[2], x[6]));
    cpx a1 = cadd(x[1], x[5]), a5 = csub(x[1], x[5]), a3 = cadd(x[3], x[7]), a7 = mul_mi(csub(x[3], x[7]));
    cpx b0 = cadd(a0, a2), b2 = csub(a0, a2), b4 = cadd(a4, a6), b6 = csub(a4, a6);
    cpx b1 = cadd(a1, a3), b3 = mul_mi(csub(a1, a3)), b5 = cadd(a5, a7), b7 = csub(a5, a7);
    const float s = 0.70710678118654752440f;
    b5 = cmul(b5, cpx{s, -s});
    b7 = cmul(b7, cpx{-s, -s});
    x[0] = cadd(b0, b1); x[1] = cadd(b4, b5); x[2] = cadd(b2, b3); x[3] = cadd(b6, b7);
    x[4] = csub(b0, b1); x[5] = csub(b4, b5); x[6] = csub(b2, b3); x[7] = csub(b6, b7);
}
// exp(-2*pi*i * num / den), den a power of two
__device__ __forceinline__ cpx twiddle(int num, int den) {
    float s, c;
    sincospif(-2.0f * (float)(num & (den - 1)) / (float)den, &s, &c);
    return {c, s};
}

// One wave transforms one 512-point frame: in v[j] = z[lane + 64 j], out zb[k] in natural order.  Three radix-8 passes with
// two in-LDS exchanges (n = 64 n1 + 8 n2 + n3, k = k1 + 8 k2 + 64 k3).  Every thread of the workgroup must call it (barriers).
__device__ __forceinline__ void fft512_wave(cpx (&v)[8], float2* zb, int lane, bool live) {
    if (live) {
        dft8(v);                                                                   // over n1
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) {
            cpx y = cmul(v[k1], twiddle(lane * k1, 512));
            zb[k1 * 64 + lane] = make_float2(y.x, y.y);
        }
    }
    __syncthreads();
    if (live) {
        const int k1 = lane >> 3, n3 = lane & 7;
#pragma unroll
        for (int n2 = 0; n2 < 8; ++n2) { float2 q = zb[k1 * 64 + n2 * 8 + n3]; v[n2] = {q.x, q.y}; }
        dft8(v);                                                                   // over n2
    }
    __syncthreads();
    if (live) {
        const int k1 = lane >> 3, n3 = lane & 7;
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            cpx y = cmul(v[k2], twiddle(n3 * k2, 64));
            zb[k1 * 64 + k2 * 8 + n3] = make_float2(y.x, y.y);
        }
    }
    __syncthreads();
    if (live) {
        const int k2 = lane >> 3, k1 = lane & 7;
#pragma unroll
        for (int n3 = 0; n3 < 8; ++n3) { float2 q = zb[k1 * 64 + k2 * 8 + n3]; v[n3] = {q.x, q.y}; }
        dft8(v);                                                                   // over n3
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k3 = 0; k3 < 8; ++k3) zb[lane + 64 * k3] = make_float2(v[k3].x, v[k3].y);
    }
    __syncthreads();
}

// The 256-point companion: in v[j] = z[lane + 64 j], out zb[k] (256 float2) in natural order.  One radix-4 pass on all 64 lanes, then two
// radix-8 passes on lanes 0..31 (n = 64 n1 + 8 n2 + n3, k = k1 + 4 k2 + 32 k3).  Every thread of the workgroup must call it (barriers).
__device__ __forceinline__ void fft256_wave(cpx (&v)[4], float2* zb, int lane, bool live) {
    cpx w[8];
    if (live) {
        const cpx a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), a2 = cadd(v[1], v[3]), a3 = mul_mi(csub(v[1], v[3]));
        v[0] = cadd(a0, a2); v[1] = cadd(a1, a3); v[2] = csub(a0, a2); v[3] = csub(a1, a3);      // over n1
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            cpx y = cmul(v[k1], twiddle(lane * k1, 256));
            zb[k1 * 64 + lane] = make_float2(y.x, y.y);
        }
    }
    __syncthreads();
    const bool half = live && lane < 32;
    if (half) {
        const int k1 = lane >> 3, n3 = lane & 7;
#pragma unroll
        for (int n2 = 0; n2 < 8; ++n2) { float2 q = zb[k1 * 64 + n2 * 8 + n3]; w[n2] = {q.x, q.y}; }
        dft8(w);                                                                   // over n2
    }
    __syncthreads();
    if (half) {
        const int k1 = lane >> 3, n3 = lane & 7;
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) {
            cpx y = cmul(w[k2], twiddle(n3 * k2, 64));
            zb[k1 * 64 + k2 * 8 + n3] = make_float2(y.x, y.y);
        }
    }
    __syncthreads();
    if (half) {
        const int k1 = lane & 3, k2 = lane >> 2;
#pragma unroll
        for (int n3 = 0; n3 < 8; ++n3) { float2 q = zb[k1 * 64 + k2 * 8 + n3]; w[n3] = {q.x, q.y}; }
        dft8(w);                                                                   // over n3
    }
    __syncthreads();
    if (half) {
#pragma unroll
        for (int k3 = 0; k3 < 8; ++k3) zb[lane + 32 * k3] = make_float2(w[k3].x, w[k3].y);
    }
    __syncthreads();
}
