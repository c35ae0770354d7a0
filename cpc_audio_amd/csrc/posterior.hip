// Phone posteriors for feature export (cpc/feature_loader.py:41-71, ModelPhoneCombined.forward behind getPrediction): the linear
// classifier of PhoneCriterion / CTCPhoneCriterion on R rows of 256 features followed by softmax -- or by argmax and one-hot --
// as ONE launch instead of torch's linear + softmax (+ argmax + zeros + scatter_) and their (R, C) logits tensor.
//
//   posterior_kernel   one workgroup per 32-row tile of x (probe_tile.h: the tile of probe.hip's first walk, its loaders and row
//                      statistics).  The x tile is loaded into LDS once; the classes are walked in steps of 64 rows of W.  A
//                      step's logits are exact-f32 MFMAs (v_mfma_f32_16x16x4_f32: wave w forms classes 16 w .. 16 w + 15 of the
//                      step for both halves of the tile, 16 bytes of LDS per lane and operand feeding four of them -- the FMA
//                      chains of probe_logits read 96 bytes of LDS per 32 FMAs and are bound by that) and go to LDS, where each
//                      row's maximum / first argmax / sum of exponentials are merged into registers step by step.
//                      <0> posteriors: up to kPoKeep classes all of the tile's logits stay in LDS and are written out once as
//                          exp(l - M) / S; beyond, a second walk forms the same logits again (same products in the same order,
//                          same bits) and writes them normalised.  <1> one-hot: one walk, then the tile's rows of 0 / 1.
//                      Every element of out is stored once, by one thread; nothing else is written but argmax.
//                      With one step a workgroup keeps its W in LDS and walks several tiles (grid capped at kPoMaxGroups).
// Fixed orders, no atomics: the same bits on every run.
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"
#include "probe_tile.h"

namespace cpc {

constexpr int kPoMaxGroups = 512;          // workgroups of a one-step call (two per CU; one is resident at a time: LDS)
constexpr int kPoKeep = 384;               // classes up to which a tile's logits all stay in LDS (32 x 385 floats)

struct PosteriorArgs {
    const float* x; long ldx;
    const float* W; const float* b;
    float* prob; long long* hot; int* argmax;
    int R, C;
};

// lt[r][col0 + c] = <x row r, W class c of the step> + b for the 32 x 64 tile.  Wave w: classes 16 w .. 16 w + 15, rows 0..15
// and 16..31.  Lane (i = lane & 15, kq = lane >> 4) reads k = 16 q + 4 kq .. + 3 of x rows i, 16 + i and of W class 16 w + i;
// MFMA jj of group q contracts k = 16 q + 4 g + jj over g = 0..3 (a permutation of k, the same for both operands).
__device__ __forceinline__ void posterior_logits(const float (*xs)[kPrLd], const float (*ws)[kPrLd], const float* bs,
                                                 float (*lt)[kPoKeep + 1], int col0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int q = 0; q < kC / 16; ++q) {
        const int k = 16 * q + 4 * kq;
        const float4 a0 = *reinterpret_cast<const float4*>(&xs[i][k]);
        const float4 a1 = *reinterpret_cast<const float4*>(&xs[16 + i][k]);
        const float4 bw = *reinterpret_cast<const float4*>(&ws[16 * w + i][k]);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a0, jj), f4c(bw, jj), acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a1, jj), f4c(bw, jj), acc1, 0, 0, 0);
        }
    }
    const float bias = bs[16 * w + i];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                        // acc[r]: row 4 kq + r, class 16 w + i
        lt[4 * kq + r][col0 + 16 * w + i] = acc0[r] + bias;
        lt[16 + 4 * kq + r][col0 + 16 * w + i] = acc1[r] + bias;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void posterior_kernel(PosteriorArgs p) {
    __shared__ float xs[kPrRows][kPrLd];
    __shared__ float ws[kPrCls][kPrLd];
    __shared__ float lt[kPrRows][kPoKeep + 1];           // the tile's logits: all classes (C <= kPoKeep) or the current step's
    __shared__ float bs[kPrCls];
    __shared__ float row_m[kPrRows], row_s[kPrRows];     // a row's maximum and sum exp(l - maximum) over all classes
    __shared__ int row_ix[kPrRows];
    const int tid = threadIdx.x;
    const int sr = tid >> 3, sq = tid & 7;               // statistics: thread (sr, sq) scans classes sq, sq + 8, .. of row sr
    const int ntiles = (p.R + kPrRows - 1) / kPrRows, nsteps = (p.C + kPrCls - 1) / kPrCls;
    const bool keep = p.C <= kPoKeep;
    const int nwalks = (MODE == 0 && !keep) ? 2 : 1;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int r0 = tile * kPrRows, nr = min(kPrRows, p.R - r0);
        __syncthreads();                                 // the readers of xs / lt / row_* of the tile before are done
        probe_load_x(xs, p, r0);
        float M = 0.f, S = 1.f;
        int ix = 0;
        for (int walk = 0; walk < nwalks; ++walk)
            for (int step = 0; step < nsteps; ++step) {
                const int c0 = step * kPrCls, nc = min(kPrCls, p.C - c0), col0 = keep ? c0 : 0;
                if (nsteps > 1 || tile == (int)blockIdx.x) {         // (one step: ws holds all of W from the first tile on)
                    if (nsteps > 1) __syncthreads();     // the readers of ws / bs of the step before are done
                    probe_load_w(ws, bs, p, c0);
                }
                __syncthreads();                         // xs, ws, bs are there; the readers of lt of the step before are done
                posterior_logits(xs, ws, bs, lt, col0);
                __syncthreads();
                if (walk == 0) {
                    float mx, e;
                    int mi;
                    probe_row_stats(lt, sr, sq, nc, mx, mi, e, col0);
                    probe_merge(M, S, ix, mx, e, c0 + mi, step == 0);
                    if (step == nsteps - 1 && sq == 0) {
                        row_m[sr] = M;
                        row_s[sr] = S;
                        row_ix[sr] = ix;
                        if (p.argmax && sr < nr) p.argmax[r0 + sr] = ix;
                    }
                }
                if (MODE == 0 && walk == 1) {            // (row_m / row_s: this walk's barriers are in between)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)   // (paired up, the subtractions become packed fp32: build.py's gate)
                    for (int q = 0; q < 8; ++q) {
                        const int e = tid + 256 * q, r = e >> 6, cc = e & 63;
                        if (r < nr && cc < nc) p.prob[(long)(r0 + r) * p.C + c0 + cc] = expf(lt[r][cc] - row_m[r]) / row_s[r];
                    }
                }
            }
        // the tile's rows of out are one contiguous run of nr * C elements
        if (MODE == 0 && keep) {
            __syncthreads();                             // row_m / row_s, and the last step's logits
            float* o = p.prob + (long)r0 * p.C;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)   // (as above)
            for (int e = tid; e < nr * p.C; e += 256) {
                const int r = e / p.C;
                o[e] = expf(lt[r][e - r * p.C] - row_m[r]) / row_s[r];
            }
        }
        if (MODE == 1) {
            __syncthreads();                             // row_ix
            long long* o = p.hot + (long)r0 * p.C;
            for (int e = tid; e < nr * p.C; e += 256) {
                const int r = e / p.C;
                o[e] = (e - r * p.C == row_ix[r]) ? 1 : 0;
            }
        }
    }
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_posterior_forward(const float* x, long ldx, const float* W, const float* b, int R, int C, int mode, void* out,
                                     int* argmax, void* stream) {
    CPC_RETURN_IF(R < 1 || C < 2 || C > kPrMaxClasses, CPC_ERR_SHAPE);
    CPC_RETURN_IF((long)R * C >= (1L << 31), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!x || ldx < kC || !W || !b || !out || (mode != 0 && mode != 1), CPC_ERR_ARG);
    CPC_RETURN_IF(((uintptr_t)x & 3) || ((uintptr_t)W & 3) || ((uintptr_t)b & 3) || ((uintptr_t)argmax & 3), CPC_ERR_ARG);
    CPC_RETURN_IF((uintptr_t)out & (mode == 1 ? 7 : 3), CPC_ERR_ARG);
    PosteriorArgs p;
    p.x = x; p.ldx = ldx; p.W = W; p.b = b;
    p.prob = mode == 0 ? static_cast<float*>(out) : nullptr;
    p.hot = mode == 1 ? static_cast<long long*>(out) : nullptr;
    p.argmax = argmax;
    p.R = R; p.C = C;
    const int ntiles = (R + kPrRows - 1) / kPrRows;
    const int groups = C <= kPrCls ? min(ntiles, kPoMaxGroups) : ntiles;
    const hipStream_t st = (hipStream_t)stream;
    if (mode == 0) hipLaunchKernelGGL(posterior_kernel<0>, dim3(groups), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(posterior_kernel<1>, dim3(groups), dim3(256), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}
