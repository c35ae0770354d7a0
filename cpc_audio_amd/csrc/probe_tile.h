// The tile the linear classifiers on 256 frozen features are built from (probe.hip: the fused probe step; posterior.hip: phone
// posteriors): 32 rows of x and 64 rows of W in LDS, their logits as exact-f32 FMA chains (probe.hip; posterior.hip forms them
// with f32 MFMAs), and a row's softmax statistics (maximum, first index of the maximum, sum of exponentials) from one 64-class
// step and merged over steps.
// The loaders take any argument struct with the members they name: x, ldx, R and W, b, C.
// probe.hip's probe_wide_kernel (any feature width) has loaders and a logits loop of its own at its row pitch and shares
// probe_merge and probe_row_stats.
#pragma once
#include <climits>

#include "cpc_common.h"

namespace cpc {

constexpr int kPrMaxClasses = 8192;
constexpr int kPrRows = 32;                // rows per x tile
constexpr int kPrCls = 64;                 // classes per walk step
constexpr int kPrLd = kC + 4;              // LDS row pitch in floats: 16-byte reads of 16 rows apart hit 16 different bank quads

// Running softmax statistics of a row over the class steps met so far: maximum M at index ix (the first one on ties), S = sum
// exp(l - M).  A step comes in as its own maximum mx at mi and e = sum exp(l - mx); a later step wins only with a larger maximum.
__device__ __forceinline__ void probe_merge(float& M, float& S, int& ix, float mx, float e, int mi, bool first) {
    if (first) {
        M = mx; S = e; ix = mi;
    } else if (mx > M) {
        S = S * expf(M - mx) + e;
        M = mx; ix = mi;
    } else {
        S += e * expf(mx - M);
    }
}

// rows [r0, r0 + 32) of x -> xs (rows past R: zeros)
template <class Args>
__device__ __forceinline__ void probe_load_x(float (*xs)[kPrLd], const Args& p, int r0) {
    const int tid = threadIdx.x;
    const bool vec = (((uintptr_t)p.x & 15) == 0) && ((p.ldx & 3) == 0);
    if (vec) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q, r = e >> 6, k = (e & 63) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + r < p.R) v = *reinterpret_cast<const float4*>(p.x + (long)(r0 + r) * p.ldx + k);
            *reinterpret_cast<float4*>(&xs[r][k]) = v;
        }
    } else {
        for (int q = 0; q < 32; ++q) {
            const int e = tid + 256 * q, r = e >> 8, k = e & 255;
            xs[r][k] = r0 + r < p.R ? p.x[(long)(r0 + r) * p.ldx + k] : 0.f;
        }
    }
}

// classes [c0, c0 + 64) of W and b -> ws, bs (classes past C: zeros)
template <class Args>
__device__ __forceinline__ void probe_load_w(float (*ws)[kPrLd], float* bs, const Args& p, int c0) {
    const int tid = threadIdx.x;
    const bool vec = ((uintptr_t)p.W & 15) == 0;
    if (vec) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 256 * q, c = e >> 6, k = (e & 63) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c0 + c < p.C) v = *reinterpret_cast<const float4*>(p.W + (long)(c0 + c) * kC + k);
            *reinterpret_cast<float4*>(&ws[c][k]) = v;
        }
    } else {
        for (int q = 0; q < 64; ++q) {
            const int e = tid + 256 * q, c = e >> 8, k = e & 255;
            ws[c][k] = c0 + c < p.C ? p.W[(long)(c0 + c) * kC + k] : 0.f;
        }
    }
    if (tid < kPrCls) bs[tid] = c0 + tid < p.C ? p.b[c0 + tid] : 0.f;
}

// acc[i][j] = <x row ty + 16 i, W class tx + 16 j> + b: the k order is 0..255 for every element, in every walk
__device__ __forceinline__ void probe_logits(const float (*xs)[kPrLd], const float (*ws)[kPrLd], const float* bs, int tx, int ty,
                                             float (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k = 0; k < kC; k += 4) {
        float4 a[2], w[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const float4*>(&xs[ty + 16 * i][k]);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const float4*>(&ws[tx + 16 * j][k]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = acc[i][j];
                s = fmaf(a[i].x, w[j].x, s);
                s = fmaf(a[i].y, w[j].y, s);
                s = fmaf(a[i].z, w[j].z, s);
                s = fmaf(a[i].w, w[j].w, s);
                acc[i][j] = s;
            }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += bs[tx + 16 * j];
}

// One step's statistics of row sr of the tile's logits lt (the step's classes at columns col0 ..), by the row's 8 threads (sq =
// 0..7, neighbouring lanes; thread sq scans classes sq, sq + 8, .. below nc): mx = the maximum, mi = its first index within the
// step, e = sum exp(l - mx), in all 8 threads.
template <int LD>
__device__ __forceinline__ void probe_row_stats(const float (*lt)[LD], int sr, int sq, int nc, float& mx, int& mi, float& e,
                                                int col0 = 0) {
    mx = -INFINITY;
    mi = INT_MAX;
    for (int cc = sq; cc < nc; cc += 8) {
        const float v = lt[sr][col0 + cc];
        if (mi == INT_MAX || v > mx) { mx = v; mi = cc; }
    }
#pragma unroll
    for (int off = 1; off <= 4; off <<= 1) {
        const float om = __shfl_xor(mx, off);
        const int oi = __shfl_xor(mi, off);
        if (oi != INT_MAX && (mi == INT_MAX || om > mx || (om == mx && oi < mi))) { mx = om; mi = oi; }
    }
    e = 0.f;
    for (int cc = sq; cc < nc; cc += 8) e += expf(lt[sr][col0 + cc] - mx);
    e += __shfl_xor(e, 1);
    e += __shfl_xor(e, 2);
    e += __shfl_xor(e, 4);
}

}  // namespace cpc
