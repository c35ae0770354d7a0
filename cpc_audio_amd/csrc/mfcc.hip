// The MFCC front end (cpc/model.py:108-122, MFCCEncoder): torchaudio.transforms.MFCC(n_mfcc = D, melkwargs = {n_mels: M,
// n_fft: 321}), M = max(128, D), restated as three small dense products with two pointwise steps between them (the formula and
// the tables' layouts: include/cpc_hip.h).  Two launches, because the dB floor hangs on the maximum over the whole call:
//
//   meldb   a workgroup of 8 waves owns 32 frames of one row.  It stages their 160 * 31 + 321 samples once in LDS, reflection
//           resolved on the way in, with ONE PAD FLOAT BEHIND EVERY 160 SAMPLES: frame i, tap j sits at 161 i + j + j / 160, so
//           the 32 lanes of a half-wave that read one tap of 32 frames (the A operand of v_mfma_f32_32x32x2_f32, row = frame)
//           hit 32 different banks; at the plain frame stride of 160 floats they would all hit one.  re / im = frames x windowed
//           DFT basis (K = 321 + 1 zero): six waves take 32 bins each, cos and -sin of the same bins feed two accumulators of
//           one wave, so re^2 + im^2 is formed in registers.  The power tile (32 x 192, rows of 193 floats) goes to LDS and is
//           the A operand of the mel product (K = 161 + 1 zero, M columns, 32 per wave and pass); the epilogue takes
//           10 log10(max(., 1e-10)), stores db channels-last and keeps the maximum of what it stored: one float per workgroup.
//   dct     a workgroup owns 32 frames of one row again: it takes the maximum of the partial maxima (of the call, or of its row),
//           clamps db at top - 80 on its way into LDS (256 filters at a time, rows of 257 floats) and multiplies by dct (M, D).
// The tables (413 KB + 161 M + M D floats) are the B operands and come straight from L2, 32 consecutive floats per half-wave
// and contraction index: a workgroup is a chain of ~160 dependent MFMAs per product, so what decides its time is whether the
// loads run ahead of that chain.  They are issued without a branch (a row past the table re-reads its last row, the operand is
// zeroed in a register) a batch of 7 to 9 contraction steps ahead, into a second register set.  With masked, branching loads
// the same kernels took 140 us at N = 8 .. 64 (L = 20480, D = 256); so they take 61 .. 66 us.
// Columns and contraction indices beyond the tables (bins 161 .., tap 321, filters M .., coefficients D ..) are zeros formed in
// registers: no table is read past its end, and nothing is stored for them.  No atomics, no packed fp32; the inputs are only read.
#include <math.h>

#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kMfFft = 321, kMfHop = 160, kMfBins = 161, kMfBasisCols = 2 * kMfBins;
constexpr int kMfT = 32;                                        // frames of a workgroup = rows of the MFMA tile
constexpr int kMfThreads = 512, kMfWaves = 8;
constexpr int kMfSamples = kMfHop * (kMfT - 1) + kMfFft;        // 5281 samples under 32 frames
constexpr int kMfSeg = 5320;                                    // their padded image (5281 + 33 pads) and the zero tap 321 of frame 31
constexpr int kMfBinTiles = 6;                                  // 6 x 32 >= 161 bins
constexpr int kMfPowRow = 32 * kMfBinTiles + 1;                 // 193: odd, so a column read over 32 frames is conflict free
constexpr int kMfKc = 256, kMfDbRow = kMfKc + 1;                // filters per LDS pass of the DCT
constexpr int kMfMaxD = 512;

static_assert(kMfSamples - 1 + (kMfSamples - 1) / kMfHop + 2 <= kMfSeg, "the segment holds tap 321 of the last frame");

__device__ __forceinline__ int mf_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }   // row of accumulator register r

__device__ __forceinline__ f32x16 mf_zero() {
    f32x16 a;
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
    return a;
}

// B operands of SB contraction steps (rows k0 + 2 i + hi of a table whose rows are ld floats apart), loaded without a branch:
// a row past the table reads its last row instead, and mf_b makes the operand zero there and in lanes whose column lies past
// the table (bp then points at column 0)
template <int SB>
__device__ __forceinline__ void mf_load_b(float (&b)[SB], const float* __restrict__ bp, int ld, int k0, int hi, int K) {
#pragma unroll
    for (int i = 0; i < SB; ++i) {
        const int kk = k0 + 2 * i + hi;
        b[i] = bp[(long)(kk < K ? kk : K - 1) * ld];
    }
}
__device__ __forceinline__ float mf_b(float v, int kk, int K, bool cv) { return (cv && kk < K) ? v : 0.f; }

// acc += A (32 rows x 2 SB nb, the lane's row of an LDS tile at a[k]) x B (K rows of the table, the lane's column at bp).  The
// table comes from L2: the operands of the next SB steps are in flight while the MFMAs of this batch run (two register sets).
template <int SB>
__device__ __forceinline__ f32x16 mf_product(const float* a, const float* __restrict__ bp, int ld, int K, int nb, int hi, bool cv,
                                             f32x16 acc) {
    float b0[SB], b1[SB];
    mf_load_b<SB>(b0, bp, ld, 0, hi, K);
#pragma unroll 1
    for (int bt = 0; bt < nb; bt += 2) {
        mf_load_b<SB>(b1, bp, ld, 2 * SB * (bt + 1), hi, K);
#pragma unroll
        for (int i = 0; i < SB; ++i) {
            const int kk = 2 * SB * bt + 2 * i + hi;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], mf_b(b0[i], kk, K, cv), acc, 0, 0, 0);
        }
        if (bt + 1 < nb) {
            mf_load_b<SB>(b0, bp, ld, 2 * SB * (bt + 2), hi, K);
#pragma unroll
            for (int i = 0; i < SB; ++i) {
                const int kk = 2 * SB * (bt + 1) + 2 * i + hi;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], mf_b(b1[i], kk, K, cv), acc, 0, 0, 0);
            }
        }
    }
    return acc;
}

// position of tap jj of the lane's frame in the padded image, relative to the frame's first sample
__device__ __forceinline__ int mf_tap(int jj) { return jj + (jj >= kMfHop) + (jj >= 2 * kMfHop); }

constexpr int kMfSb1 = 7, kMfNb1 = 23;             // 161 = 7 x 23 steps of two taps: taps 0 .. 321 (321: a zero row)
constexpr int kMfSb2 = 9, kMfNb2 = 9;              // 81 = 9 x 9 steps of two bins: bins 0 .. 161 (161: a zero row)
constexpr int kMfSb3 = 8;                          // the DCT walks 16 filters per batch

__global__ __launch_bounds__(kMfThreads) void mfcc_meldb_kernel(const float* __restrict__ x, const float* __restrict__ basis,
                                                               const float* __restrict__ fb, float* __restrict__ db,
                                                               float* __restrict__ part, int L, int F, int M, int tiles) {
    __shared__ float seg[kMfSeg];
    __shared__ float pw[kMfT * kMfPowRow];
    __shared__ float red[kMfWaves];
    const int n = blockIdx.x / tiles, f0 = kMfT * (blockIdx.x % tiles);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, hi = lane >> 5;
    const float* xn = x + (long)n * L;
    // position q * 161 + u of the image is sample 160 q + u of the segment (u = 160: the pad), which starts 160 in front of frame f0
    const long t0 = (long)kMfHop * f0 - kMfHop;
    for (int i = threadIdx.x; i < kMfSeg; i += kMfThreads) {
        const int q = i / (kMfHop + 1), u = i - q * (kMfHop + 1), s = kMfHop * q + u;
        float v = 0.f;
        if (u < kMfHop && s < kMfSamples) {
            long t = t0 + s;
            if (t < 0) t = -t;
            if (t >= L) t = 2L * (L - 1) - t;
            if (t >= 0 && t < L) v = xn[t];                    // (frames behind the last one reach further than one reflection: zeros)
        }
        seg[i] = v;
    }
    __syncthreads();
    // ---- re, im and the power of 32 bins at a time: cos and -sin of the same bins feed two accumulators of one wave
    for (int bt = w; bt < kMfBinTiles; bt += kMfWaves) {
        const int c = 32 * bt + col;
        const bool cv = c < kMfBins;
        const float* bre = basis + (cv ? c : 0);
        const float* bim = bre + kMfBins;
        const float* xa = seg + (kMfHop + 1) * col;                           // frame = col
        f32x16 re = mf_zero(), im = mf_zero();
        float r0[kMfSb1], i0[kMfSb1], r1[kMfSb1], i1[kMfSb1];
        mf_load_b<kMfSb1>(r0, bre, kMfBasisCols, 0, hi, kMfFft);
        mf_load_b<kMfSb1>(i0, bim, kMfBasisCols, 0, hi, kMfFft);
#pragma unroll 1
        for (int b = 0; b < kMfNb1; b += 2) {
            mf_load_b<kMfSb1>(r1, bre, kMfBasisCols, 2 * kMfSb1 * (b + 1), hi, kMfFft);
            mf_load_b<kMfSb1>(i1, bim, kMfBasisCols, 2 * kMfSb1 * (b + 1), hi, kMfFft);
#pragma unroll
            for (int i = 0; i < kMfSb1; ++i) {
                const int jj = 2 * kMfSb1 * b + 2 * i + hi;
                const float a = xa[mf_tap(jj)];
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mf_b(r0[i], jj, kMfFft, cv), re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mf_b(i0[i], jj, kMfFft, cv), im, 0, 0, 0);
            }
            if (b + 1 < kMfNb1) {
                mf_load_b<kMfSb1>(r0, bre, kMfBasisCols, 2 * kMfSb1 * (b + 2), hi, kMfFft);
                mf_load_b<kMfSb1>(i0, bim, kMfBasisCols, 2 * kMfSb1 * (b + 2), hi, kMfFft);
#pragma unroll
                for (int i = 0; i < kMfSb1; ++i) {
                    const int jj = 2 * kMfSb1 * (b + 1) + 2 * i + hi;
                    const float a = xa[mf_tap(jj)];
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mf_b(r1[i], jj, kMfFft, cv), re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(a, mf_b(i1[i], jj, kMfFft, cv), im, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) pw[mf_row(r, hi) * kMfPowRow + c] = re[r] * re[r] + im[r] * im[r];
    }
    __syncthreads();
    // ---- the mel product and the decibels
    float mx = -INFINITY;
    const int ntm = (M + 31) / 32;
    for (int t = w; t < ntm; t += kMfWaves) {
        const int m = 32 * t + col;
        const bool mv = m < M;
        const f32x16 acc = mf_product<kMfSb2>(pw + col * kMfPowRow, fb + (mv ? m : 0), M, kMfBins, kMfNb2, hi, mv, mf_zero());
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = f0 + mf_row(r, hi);
            const float v = acc[r] > 1e-10f ? 10.0f * log10f(acc[r]) : -100.0f;       // (the floor exactly, whatever log10f rounds to)
            if (f < F && mv) {
                db[((long)n * F + f) * M + m] = v;
                mx = fmaxf(mx, v);
            }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float top = red[0];
#pragma unroll
        for (int i = 1; i < kMfWaves; ++i) top = fmaxf(top, red[i]);
        part[blockIdx.x] = top;
    }
}

__global__ __launch_bounds__(kMfThreads) void mfcc_dct_kernel(const float* __restrict__ db, const float* __restrict__ part,
                                                             const float* __restrict__ dct, float* __restrict__ y, int N, int F,
                                                             int M, int D, int tiles, int rowwise) {
    __shared__ float tile[kMfT * kMfDbRow];
    __shared__ float red[kMfWaves];
    constexpr int kAcc = kMfMaxD / 32 / kMfWaves;                 // column tiles of a wave
    const int n = blockIdx.x / tiles, f0 = kMfT * (blockIdx.x % tiles);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, hi = lane >> 5;
    const float* pp = rowwise ? part + (long)n * tiles : part;
    const long cnt = rowwise ? tiles : (long)N * tiles;
    float mx = -INFINITY;
    for (long i = threadIdx.x; i < cnt; i += kMfThreads) mx = fmaxf(mx, pp[i]);
    mx = wave_max(mx);
    if (lane == 0) red[w] = mx;
    __syncthreads();
    float top = red[0];
#pragma unroll
    for (int i = 1; i < kMfWaves; ++i) top = fmaxf(top, red[i]);
    const float floor_db = top - 80.0f;
    const float* dbn = db + (long)n * F * M;
    const int ntd = (D + 31) / 32;
    f32x16 acc[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; ++q) acc[q] = mf_zero();
    for (int k0 = 0; k0 < M; k0 += kMfKc) {
        const int kc = M - k0 < kMfKc ? M - k0 : kMfKc;
        __syncthreads();
        for (int i = threadIdx.x; i < kMfT * kMfKc; i += kMfThreads) {          // (the whole tile: zeros past kc and past F)
            const int r = i / kMfKc, k = i - r * kMfKc, f = f0 + r;
            tile[r * kMfDbRow + k] = (f < F && k < kc) ? fmaxf(dbn[(long)f * M + k0 + k], floor_db) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kAcc; ++q) {
            const int d = 32 * (w + kMfWaves * q) + col;
            const bool dv = d < D;
            if (w + kMfWaves * q < ntd)                                           // (wave-uniform)
                acc[q] = mf_product<kMfSb3>(tile + col * kMfDbRow, dct + (long)k0 * D + (dv ? d : 0), D, kc,
                                            (kc + 2 * kMfSb3 - 1) / (2 * kMfSb3), hi, dv, acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < kAcc; ++q) {
        const int d = 32 * (w + kMfWaves * q) + col;
        if (w + kMfWaves * q < ntd && d < D) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = f0 + mf_row(r, hi);
                if (f < F) y[((long)n * F + f) * D + d] = acc[q][r];
            }
        }
    }
}

// F >= 2 frames, M filters, one workgroup per 32 frames of a row
static int mfcc_shape(int N, long F, int D, int* M, int* tiles) {
    CPC_RETURN_IF(N < 1 || F < 2 || D < 1 || D > kMfMaxD, CPC_ERR_SHAPE);
    *M = D > 128 ? D : 128;
    CPC_RETURN_IF((long)N * F >= (1L << 31) || (long)N * F * *M >= (1L << 31), CPC_ERR_SHAPE);
    *tiles = cdiv(F, kMfT);
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_mfcc_layout(int N, int L, int D, long* sizes) {
    int M, tiles;
    CPC_RETURN_IF(L < kMfBins, CPC_ERR_SHAPE);
    const long F = (L - 1) / kMfHop + 1;
    const int rc = mfcc_shape(N, F, D, &M, &tiles);
    if (rc) return rc;
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = F;
    sizes[1] = M;
    sizes[2] = (long)N * tiles * (long)sizeof(float);
    return 0;
}

extern "C" int cpc_mfcc_meldb(const float* x, const float* basis, const float* fb, float* db, void* ws, int N, int L, int D,
                              void* stream) {
    int M, tiles;
    CPC_RETURN_IF(L < kMfBins, CPC_ERR_SHAPE);
    const long F = (L - 1) / kMfHop + 1;
    const int rc = mfcc_shape(N, F, D, &M, &tiles);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !basis || !fb || !db || !ws, CPC_ERR_ARG);
    hipLaunchKernelGGL(mfcc_meldb_kernel, dim3((unsigned)((long)N * tiles)), dim3(kMfThreads), 0, (hipStream_t)stream, x, basis, fb,
                       db, static_cast<float*>(ws), L, (int)F, M, tiles);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_mfcc_dct(const float* db, const void* ws, const float* dct, float* y, int N, int F, int D, int rowwise,
                            void* stream) {
    int M, tiles;
    const int rc = mfcc_shape(N, F, D, &M, &tiles);
    if (rc) return rc;
    CPC_RETURN_IF(!db || !ws || !dct || !y || db == y || rowwise < 0 || rowwise > 1, CPC_ERR_ARG);
    hipLaunchKernelGGL(mfcc_dct_kernel, dim3((unsigned)((long)N * tiles)), dim3(kMfThreads), 0, (hipStream_t)stream, db,
                       static_cast<const float*>(ws), dct, y, N, F, M, D, tiles, rowwise);
    CPC_LAUNCH_CHECK();
    return 0;
}
