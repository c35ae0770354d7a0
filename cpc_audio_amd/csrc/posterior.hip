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
//
// Any feature width (cpc_posterior_forward_d, 1 <= D <= 512): the same kernel at the LDS row pitch LD and class step CLS the
// width asks for, as probe.hip's probe_wide_kernel is instantiated:
//   LD   CLS  keep  D           LDS rows hold D rounded up to 16 columns, the columns behind D zero: an MFMA group contracts
//   20   64   384   1 .. 16     16 k and 0 * 0 adds exactly 0, so D = 13 gives the bits of D = 16 with three zero columns.
//   68   64   384   17 .. 64    Global loads are 16 bytes wide where D % 4 == 0, the base is 16-byte aligned and (x) ldx % 4
//   260  64   384   65 .. 256   == 0, scalar otherwise.
//   516  32   192   257 .. 512  32 + 64 rows of 516 floats and 32 x 385 logits do not fit into a workgroup's 160 KB: the class
//                               step is halved (wave w: classes 16 (w & 1) .., rows 16 (w >> 1) .., one accumulator) AND the
//                               logits kept are halved, since 64 rows of 516 floats leave room for 32 x 247 only.
// FIXED (the cpc_posterior_forward entry point): LD 260, CLS 64 with probe_tile.h's 256 loaders and a constant q loop.  The
// wide instantiation of that pitch forms every sum in the same order: the _d call at 256 gives the same bits.
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"
#include "probe_tile.h"

namespace cpc {

constexpr int kPoMaxGroups = 512;          // workgroups of a one-step call (two per CU; one is resident at a time: LDS)
constexpr int kPoKeep = 384;               // classes up to which a tile's logits all stay in LDS (32 x 385 floats)
constexpr int kPoKeepWide = 192;           // ... at the 516 pitch (D > 256)
constexpr int kPoMaxD = 512;               // widest feature row of cpc_posterior_forward_d
template <int LD> constexpr int po_keep() { return LD > kPrLd ? kPoKeepWide : kPoKeep; }

struct PosteriorArgs {
    const float* x; long ldx;
    const float* W; const float* b;
    float* prob; long long* hot; int* argmax;
    int R, C;
    int D, D16, xvec, wvec;                // (the wide instantiations) the width, rounded up to 16, 16-byte loads of x / W
};

// rows [r0, r0 + 32) of x -> columns [0, D16) of xs (rows past R, columns past D: zeros); 8 threads per row
template <int LD>
__device__ __forceinline__ void posterior_load_x(float (*xs)[LD], const PosteriorArgs& p, int r0) {
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
    const bool live = r0 + r < p.R;
    const long row = live ? (long)(r0 + r) * p.ldx : 0;
    if (p.xvec) {
        for (int k = 4 * q; k < p.D16; k += 32) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && k < p.D) v = *reinterpret_cast<const float4*>(p.x + row + k);
            *reinterpret_cast<float4*>(&xs[r][k]) = v;
        }
    } else {
        for (int k = q; k < p.D16; k += 8) xs[r][k] = (live && k < p.D) ? p.x[row + k] : 0.f;
    }
}

// classes [c0, c0 + CLS) of W and b -> ws, bs (classes past C, columns past D: zeros); 256 / CLS threads per class
template <int LD, int CLS>
__device__ __forceinline__ void posterior_load_w(float (*ws)[LD], float* bs, const PosteriorArgs& p, int c0) {
    constexpr int kT = 256 / CLS;
    const int tid = threadIdx.x, c = tid / kT, q = tid % kT;
    const bool live = c0 + c < p.C;
    const long row = live ? (long)(c0 + c) * p.D : 0;
    if (p.wvec) {
        for (int k = 4 * q; k < p.D16; k += 4 * kT) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && k < p.D) v = *reinterpret_cast<const float4*>(p.W + row + k);
            *reinterpret_cast<float4*>(&ws[c][k]) = v;
        }
    } else {
        for (int k = q; k < p.D16; k += kT) ws[c][k] = (live && k < p.D) ? p.W[row + k] : 0.f;
    }
    if (tid < CLS) bs[tid] = c0 + tid < p.C ? p.b[c0 + tid] : 0.f;
}

// lt[r][col0 + c] = <x row r, W class c of the step> + b for the 32 x CLS tile.  CLS 64: wave w forms classes 16 w .. 16 w + 15
// for rows 0..15 and 16..31; CLS 32: classes 16 (w & 1) .. for rows 16 (w >> 1) ...  Lane (i = lane & 15, kq = lane >> 4) reads
// k = 16 q + 4 kq .. + 3 of its x rows and of its W class; MFMA jj of group q contracts k = 16 q + 4 g + jj over g = 0..3 (a
// permutation of k, the same for both operands).  nq groups of 16 k.
template <int LD, int CLS>
__device__ __forceinline__ void posterior_logits(const float (*xs)[LD], const float (*ws)[LD], const float* bs,
                                                 float (*lt)[po_keep<LD>() + 1], int col0, int nq) {
    static_assert(CLS == 64 || CLS == 32, "posterior_logits: four waves form 32 x 64 or 32 x 32 logits");
    constexpr int kHalves = CLS / 32;                    // 16-row accumulators of a wave
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
    const int cw = 16 * (CLS == 64 ? w : (w & 1)), rw = CLS == 64 ? 0 : 16 * (w >> 1);
    f32x4 acc[kHalves];
#pragma unroll
    for (int h = 0; h < kHalves; ++h) acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int q = 0; q < nq; ++q) {
        const int k = 16 * q + 4 * kq;
        float4 a[kHalves];
#pragma unroll
        for (int h = 0; h < kHalves; ++h) a[h] = *reinterpret_cast<const float4*>(&xs[rw + 16 * h + i][k]);
        const float4 bw = *reinterpret_cast<const float4*>(&ws[cw + i][k]);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int h = 0; h < kHalves; ++h)
                acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[h], jj), f4c(bw, jj), acc[h], 0, 0, 0);
    }
    const float bias = bs[cw + i];
#pragma unroll
    for (int r = 0; r < 4; ++r)                          // acc[h][r]: row rw + 16 h + 4 kq + r, class cw + i
#pragma unroll
        for (int h = 0; h < kHalves; ++h) lt[rw + 16 * h + 4 * kq + r][col0 + cw + i] = acc[h][r] + bias;
}

template <int MODE, int LD, int CLS, bool FIXED>
__global__ __launch_bounds__(256) void posterior_kernel(PosteriorArgs p) {
    constexpr int kKeep = po_keep<LD>();
    static_assert(!FIXED || (LD == kPrLd && CLS == kPrCls), "posterior_kernel: the 256 loaders fill 64 rows of kPrLd floats");
    static_assert(kKeep % CLS == 0, "posterior_kernel: the kept logits are whole class steps");
    __shared__ float xs[kPrRows][LD];
    __shared__ float ws[CLS][LD];
    __shared__ float lt[kPrRows][kKeep + 1];             // the tile's logits: all classes (C <= kKeep) or the current step's
    __shared__ float bs[CLS];
    __shared__ float row_m[kPrRows], row_s[kPrRows];     // a row's maximum and sum exp(l - maximum) over all classes
    __shared__ int row_ix[kPrRows];
    const int tid = threadIdx.x;
    const int sr = tid >> 3, sq = tid & 7;               // statistics: thread (sr, sq) scans classes sq, sq + 8, .. of row sr
    const int ntiles = (p.R + kPrRows - 1) / kPrRows, nsteps = (p.C + CLS - 1) / CLS;
    const int nq = FIXED ? kC / 16 : p.D16 / 16;
    const bool keep = p.C <= kKeep;
    const int nwalks = (MODE == 0 && !keep) ? 2 : 1;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int r0 = tile * kPrRows, nr = min(kPrRows, p.R - r0);
        __syncthreads();                                 // the readers of xs / lt / row_* of the tile before are done
        if constexpr (FIXED) probe_load_x(xs, p, r0);
        else posterior_load_x<LD>(xs, p, r0);
        float M = 0.f, S = 1.f;
        int ix = 0;
        for (int walk = 0; walk < nwalks; ++walk)
            for (int step = 0; step < nsteps; ++step) {
                const int c0 = step * CLS, nc = min(CLS, p.C - c0), col0 = keep ? c0 : 0;
                if (nsteps > 1 || tile == (int)blockIdx.x) {         // (one step: ws holds all of W from the first tile on)
                    if (nsteps > 1) __syncthreads();     // the readers of ws / bs of the step before are done
                    if constexpr (FIXED) probe_load_w(ws, bs, p, c0);
                    else posterior_load_w<LD, CLS>(ws, bs, p, c0);
                }
                __syncthreads();                         // xs, ws, bs are there; the readers of lt of the step before are done
                posterior_logits<LD, CLS>(xs, ws, bs, lt, col0, nq);
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
                    for (int q = 0; q < kPrRows * CLS / 256; ++q) {
                        const int e = tid + 256 * q, r = e / CLS, cc = e % CLS;
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

// D = 0: the 256 entry point and its instantiation
static int posterior_forward(const float* x, long ldx, const float* W, const float* b, int R, int C, int Dr, int mode, void* out,
                             int* argmax, void* stream) {
    const bool fixed = Dr == 0;
    const int D = fixed ? kC : Dr;
    CPC_RETURN_IF(D < 1 || D > kPoMaxD, CPC_ERR_SHAPE);
    CPC_RETURN_IF(R < 1 || C < 2 || C > kPrMaxClasses, CPC_ERR_SHAPE);
    CPC_RETURN_IF((long)R * C >= (1L << 31), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!x || ldx < D || !W || !b || !out || (mode != 0 && mode != 1), CPC_ERR_ARG);
    CPC_RETURN_IF(((uintptr_t)x & 3) || ((uintptr_t)W & 3) || ((uintptr_t)b & 3) || ((uintptr_t)argmax & 3), CPC_ERR_ARG);
    CPC_RETURN_IF((uintptr_t)out & (mode == 1 ? 7 : 3), CPC_ERR_ARG);
    PosteriorArgs p;
    p.x = x; p.ldx = ldx; p.W = W; p.b = b;
    p.prob = mode == 0 ? static_cast<float*>(out) : nullptr;
    p.hot = mode == 1 ? static_cast<long long*>(out) : nullptr;
    p.argmax = argmax;
    p.R = R; p.C = C;
    p.D = D; p.D16 = (D + 15) / 16 * 16;
    p.xvec = D % 4 == 0 && ((uintptr_t)x & 15) == 0 && ldx % 4 == 0;
    p.wvec = D % 4 == 0 && ((uintptr_t)W & 15) == 0;
    const int ntiles = (R + kPrRows - 1) / kPrRows;
    const int cls = D > kC ? kPrCls / 2 : kPrCls;
    const dim3 grid(C <= cls ? min(ntiles, kPoMaxGroups) : ntiles), block(256);
    const hipStream_t st = (hipStream_t)stream;
#define PO_LAUNCH(LD, CLS, FIXED)                                                                          \
    {                                                                                                      \
        if (mode == 0) hipLaunchKernelGGL((posterior_kernel<0, LD, CLS, FIXED>), grid, block, 0, st, p);   \
        else hipLaunchKernelGGL((posterior_kernel<1, LD, CLS, FIXED>), grid, block, 0, st, p);             \
    }
    if (fixed) PO_LAUNCH(kPrLd, kPrCls, true)
    else if (D <= 16) PO_LAUNCH(20, kPrCls, false)
    else if (D <= 64) PO_LAUNCH(68, kPrCls, false)
    else if (D <= kC) PO_LAUNCH(kPrLd, kPrCls, false)
    else PO_LAUNCH(kPoMaxD + 4, kPrCls / 2, false)
#undef PO_LAUNCH
    CPC_LAUNCH_CHECK();
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_posterior_forward(const float* x, long ldx, const float* W, const float* b, int R, int C, int mode, void* out,
                                     int* argmax, void* stream) {
    return posterior_forward(x, ldx, W, b, R, C, 0, mode, out, argmax, stream);
}

extern "C" int cpc_posterior_forward_d(const float* x, long ldx, const float* W, const float* b, int R, int C, int D, int mode,
                                       void* out, int* argmax, void* stream) {
    CPC_RETURN_IF(D < 1 || D > kPoMaxD, CPC_ERR_SHAPE);
    return posterior_forward(x, ldx, W, b, R, C, D, mode, out, argmax, stream);
}
