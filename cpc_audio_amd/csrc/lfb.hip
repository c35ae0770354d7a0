// The learned-filter-bank front end (cpc/model.py:125-152, LFBEnconder): Conv1d(1, 2D, 400, stride 1), squared modulus of
// adjacent channel pairs, a Hann low-pass of 400 taps at stride 160 (padding 350), log(1 + |.|) and an instance norm over the
// frames.  The conv output (N, 2D, L - 399) -- 41 MB per 1.28 s window at D = 256 -- never exists in memory:
//
//   energy forward   one launch.  A workgroup of 4 waves keeps the 32 conv channels (16 filters) of its channel block for all
//                    400 taps in LDS (transposed, rows padded to 33 floats) and walks over "hops": hop h is the 160 conv
//                    positions u = t + 350 in [160 h, 160 h + 160), five 32 x 32 tiles of the Toeplitz product
//                    y[t][c] = sum_j x[t + j] W[c][j] on exact-f32 MFMAs (v_mfma_f32_32x32x2_f32: A[i][k] = x[t_i + j + k] read
//                    32 bits at a time from the LDS copy of the waveform, B[k][c] = W[c][j + k]).  Frame f covers
//                    u in [160 f, 160 f + 400), so hop h feeds exactly the frames h, h - 1 and h - 2 with the Hann taps
//                    i, i + 160 and i + 320 (i = u - 160 h; the last only for i < 80).  The epilogue squares the accumulators
//                    in place, weights them, adds the two channels of a filter (neighbouring lanes) and the two row halves of
//                    the tile (lanes l and l + 32): three numbers per (hop, filter) go to LDS, and frame f of the workgroup's
//                    span is (p[f][0] + p[f+1][1]) + p[f+2][2].  A span of 4 g - 2 frames costs 4 g hops: 2 of them are
//                    computed by the neighbouring span as well.
//   energy backward  the same walk recomputes y one 32 x 32 tile at a time, turns it in place into gy = 2 y ge (ge from at most
//                    three gs values per lane and hop) and multiplies it into the wave's 32 x 416 partial of dW held in 13
//                    accumulator tiles: the accumulator layout of gy (lane = channel, register r = positions rho and rho + 4 of
//                    the two lane halves) IS the A operand of the 32x32x2 MFMA over the position pair (rho, rho + 4), so nothing
//                    is shuffled.  Tap column 400 of the B operand is the constant 1: dW[c][400] is db[c].  The four waves add
//                    their partials in LDS in wave order, every workgroup writes one 32 x 416 tile, and lfb_reduce_kernel sums
//                    the tiles of a channel block in slot order.  Work items (window, group of 4 hops) are dealt to the
//                    workgroups of a channel block round robin, so the order of every sum depends on the shapes only.
//   lognorm          one launch each way, two-pass statistics per (n, d) over the F frames, channels-last.
// No float atomics, no packed fp32 (component-wise arithmetic, see build.py); x, W, b, han and gs are only read.
#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kLfbTaps = 400, kLfbHop = 160, kLfbPad = 350;
constexpr int kLfbCh = 32;                         // conv channels of a workgroup = 16 filters
constexpr int kLfbThreads = 256, kLfbWaves = 4;
constexpr int kLfbWRow = 33;                       // floats per tap row of the transposed weights in LDS
constexpr int kLfbTapCols = 416;                   // 13 MFMA column blocks: taps 0..399, column 400 = ones (db), the rest unused
constexpr int kLfbWFloats = kLfbCh * kLfbTapCols;  // 13312 >= 400 * 33: the region holds Wt, later the workgroup's dW partial
constexpr int kLfbHan = 480;                       // han[0..399], zeros behind (tap i + 320 of positions i >= 80)
constexpr int kLfbTileF = 1040, kLfbTileB = 1056;  // waveform samples of a group of 4 hops: 640 + 399 (+ the ones column's reach)
constexpr int kLfbMaxGroups = 8;                   // hop groups of a forward workgroup
constexpr float kLfbEps = 1e-5f;

static_assert(kLfbWFloats >= kLfbTaps * kLfbWRow, "the dW partial reuses the weight region");

__device__ __forceinline__ int lfb_rho(int r) { return (r & 3) + 8 * (r >> 2); }   // row of accumulator register r (lane half 0)

// W rows c0 .. c0 + 31 -> wt[j * 33 + c]; han -> hn[0..479]
__device__ __forceinline__ void lfb_load_weights(const float* __restrict__ W, const float* __restrict__ han, int c0, float* wt,
                                                 float* hn) {
    for (int i = threadIdx.x; i < kLfbCh * kLfbTaps; i += kLfbThreads) {
        const int c = i / kLfbTaps, j = i - c * kLfbTaps;
        wt[j * kLfbWRow + c] = W[(long)(c0 + c) * kLfbTaps + j];
    }
    for (int i = threadIdx.x; i < kLfbHan; i += kLfbThreads) hn[i] = i < kLfbTaps ? han[i] : 0.f;
}

// samples t0 .. t0 + count - 1 of one window (zero outside [0, L))
__device__ __forceinline__ void lfb_load_wave(const float* __restrict__ xn, int t0, int L, float* xs, int count) {
    for (int i = threadIdx.x; i < count; i += kLfbThreads) {
        const int t = t0 + i;
        xs[i] = (t >= 0 && t < L) ? xn[t] : 0.f;
    }
}

// acc += the 32 positions at xs[xb ..] x the 32 channels, all 400 taps
__device__ __forceinline__ f32x16 lfb_tile(const float* xs, int xb, const float* wt, int col, int hi, f32x16 acc) {
    const float* xa = xs + xb + col + hi;
    const float* wb = wt + hi * kLfbWRow + col;
#pragma unroll 8
    for (int j = 0; j < kLfbTaps; j += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j], wb[j * kLfbWRow], acc, 0, 0, 0);
    return acc;
}

__global__ __launch_bounds__(kLfbThreads) void lfb_energy_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                     const float* __restrict__ bias,
                                                                     const float* __restrict__ han, float* __restrict__ s, int N,
                                                                     int L, int D, int F, int groups, int spans) {
    __shared__ float wt[kLfbTaps * kLfbWRow];
    __shared__ float hn[kLfbHan];
    __shared__ float xs[kLfbTileF];
    __shared__ float part[4 * kLfbMaxGroups][3][kLfbCh / 2];
    const int ncb = D / 16;
    const int cb = blockIdx.x % ncb, span = (blockIdx.x / ncb) % spans, n = blockIdx.x / (ncb * spans);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, hi = lane >> 5;
    const int fb = 4 * groups - 2, f0 = span * fb, c0 = cb * kLfbCh;
    const float* xn = x + (long)n * L;
    lfb_load_weights(W, han, c0, wt, hn);
    const float bc = bias[c0 + col];
    const int tmax = L - kLfbTaps;
    for (int q = 0; q < groups; ++q) {
        __syncthreads();
        lfb_load_wave(xn, kLfbHop * (f0 + 4 * q) - kLfbPad, L, xs, kLfbTileF);
        __syncthreads();
        const int h = f0 + 4 * q + w, u0 = kLfbHop * h;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        if (u0 + kLfbHop > kLfbPad && u0 - kLfbPad <= tmax && h <= F + 1) {      // the hop has a conv position at all
#pragma unroll 1
            for (int m = 0; m < 5; ++m) {
                const int ub = u0 + 32 * m;
                if (ub + 32 <= kLfbPad || ub - kLfbPad > tmax) continue;
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                acc = lfb_tile(xs, kLfbHop * w + 32 * m, wt, col, hi, acc);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = 32 * m + lfb_rho(r) + 4 * hi, t = u0 + i - kLfbPad;
                    const float y = acc[r] + bc;
                    const float e = (t >= 0 && t <= tmax) ? y * y : 0.f;
                    p0 += hn[i] * e;
                    p1 += hn[i + kLfbHop] * e;
                    p2 += hn[i + 2 * kLfbHop] * e;
                }
            }
            p0 += dpp_mov<0xB1>(p0);                    // the two channels of a filter sit in neighbouring lanes
            p1 += dpp_mov<0xB1>(p1);
            p2 += dpp_mov<0xB1>(p2);
            p0 += __shfl_xor(p0, 32);                   // the two row halves of the tiles
            p1 += __shfl_xor(p1, 32);
            p2 += __shfl_xor(p2, 32);
        }
        if (hi == 0 && (col & 1) == 0) {
            part[4 * q + w][0][col >> 1] = p0;
            part[4 * q + w][1][col >> 1] = p1;
            part[4 * q + w][2][col >> 1] = p2;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < fb * 16; i += kLfbThreads) {
        const int fl = i >> 4, d = i & 15, f = f0 + fl;
        if (f < F) s[((long)n * F + f) * D + cb * 16 + d] = (part[fl][0][d] + part[fl + 1][1][d]) + part[fl + 2][2][d];
    }
}

// grid: ncb * slots.  part: (ncb, slots, 32, 416)
__global__ __launch_bounds__(kLfbThreads) void lfb_energy_bwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                     const float* __restrict__ bias,
                                                                     const float* __restrict__ han, const float* __restrict__ gs,
                                                                     float* __restrict__ partial, int N, int L, int D, int F,
                                                                     int hop_groups, int slots) {
    __shared__ float wt[kLfbWFloats];
    __shared__ float hn[kLfbHan];
    __shared__ float xs[kLfbTileB];
    const int ncb = D / 16;
    const int cb = blockIdx.x % ncb, slot = blockIdx.x / ncb;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, hi = lane >> 5;
    const int c0 = cb * kLfbCh, d = cb * 16 + (col >> 1);
    lfb_load_weights(W, han, c0, wt, hn);
    const float bc = bias[c0 + col];
    const int tmax = L - kLfbTaps;
    f32x16 dw[13];
#pragma unroll
    for (int k = 0; k < 13; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) dw[k][r] = 0.f;
    const int items = N * hop_groups;
    for (int it = slot; it < items; it += slots) {
        const int n = it / hop_groups, q = it - n * hop_groups;
        __syncthreads();
        lfb_load_wave(x + (long)n * L, kLfbHop * (2 + 4 * q) - kLfbPad, L, xs, kLfbTileB);
        __syncthreads();
        const int h = 2 + 4 * q + w, u0 = kLfbHop * h;
        if (u0 - kLfbPad > tmax) continue;              // (wave-uniform; the barriers above are reached by every wave all the same)
        const float* gn = gs + (long)n * F * D + d;
        const float g0 = h < F ? gn[(long)h * D] : 0.f;
        const float g1 = (h - 1 < F) ? gn[(long)(h - 1) * D] : 0.f;
        const float g2 = (h - 2 < F) ? gn[(long)(h - 2) * D] : 0.f;
#pragma unroll 1
        for (int m = 0; m < 5; ++m) {
            const int ub = u0 + 32 * m;
            if (ub + 32 <= kLfbPad || ub - kLfbPad > tmax) continue;
            const int xb = kLfbHop * w + 32 * m;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            acc = lfb_tile(xs, xb, wt, col, hi, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = 32 * m + lfb_rho(r) + 4 * hi, t = u0 + i - kLfbPad;
                const float ge = (hn[i] * g0 + hn[i + kLfbHop] * g1) + hn[i + 2 * kLfbHop] * g2;
                const float y = acc[r] + bc;
                acc[r] = (t >= 0 && t <= tmax) ? (2.0f * y) * ge : 0.f;
            }
            // dW[c][j] += sum over the tile's positions gy[c][pos] x[pos + j]: k = the position pair (rho, rho + 4) of register r
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* xr = xs + xb + lfb_rho(r) + 4 * hi + col;
#pragma unroll
                for (int k = 0; k < 12; ++k) dw[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r], xr[32 * k], dw[k], 0, 0, 0);
                const float last = col < 16 ? xr[384] : (col == 16 ? 1.0f : 0.f);
                dw[12] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r], last, dw[12], 0, 0, 0);
            }
        }
    }
    // the four waves' partials, added in wave order in the weight region
    for (int ww = 0; ww < kLfbWaves; ++ww) {
        __syncthreads();
        if (w == ww) {
#pragma unroll
            for (int k = 0; k < 13; ++k)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float* p = wt + (lfb_rho(r) + 4 * hi) * kLfbTapCols + 32 * k + col;
                    *p = ww == 0 ? dw[k][r] : *p + dw[k][r];
                }
        }
    }
    __syncthreads();
    float* out = partial + ((long)cb * slots + slot) * kLfbWFloats;
    for (int i = threadIdx.x; i < kLfbWFloats; i += kLfbThreads) out[i] = wt[i];
}

// dW (2D, 400), db (2D) = the slots' tiles summed in slot order
__global__ void lfb_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dW, float* __restrict__ db, int D,
                                  int slots) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * D * (kLfbTaps + 1)) return;
    const int c = idx / (kLfbTaps + 1), j = idx - c * (kLfbTaps + 1);
    const float* p = partial + ((long)(c / kLfbCh) * slots * kLfbCh + (c % kLfbCh)) * kLfbTapCols + j;
    float a = 0.f;
    for (int sl = 0; sl < slots; ++sl) a += p[(long)sl * kLfbWFloats];
    if (j < kLfbTaps) dW[(long)c * kLfbTaps + j] = a;
    else db[c] = a;
}

// ---- log(1 + |s|) and the instance norm over the frames: a workgroup owns 32 channels of one window, 8 frame lanes.
// u = log(1 + |s|), its mean and its spread are formed in float64: a filter whose log energy sits 30 spreads above zero loses
// 30 ulp of the normalised value to the rounding of u alone in fp32, and the tensor is 128 x D numbers per window.
constexpr int kLnLanes = 8;

__device__ __forceinline__ double ln_u(float sv) { return log1p((double)fabsf(sv)); }

__device__ __forceinline__ double ln_sum(double (*red)[32], int q, int cl, double v) {
    __syncthreads();
    red[q][cl] = v;
    __syncthreads();
    double a = red[0][cl];
#pragma unroll
    for (int i = 1; i < kLnLanes; ++i) a += red[i][cl];
    return a;
}

__global__ __launch_bounds__(256) void lfb_lognorm_fwd_kernel(const float* __restrict__ s, float* __restrict__ y,
                                                              float* __restrict__ stats, int F, int D, int normalise) {
    __shared__ double red[kLnLanes][32];
    const int nblk = D / 32, n = blockIdx.x / nblk, c = (blockIdx.x % nblk) * 32 + (threadIdx.x & 31);
    const int q = threadIdx.x >> 5, cl = threadIdx.x & 31;
    const float* sp = s + (long)n * F * D + c;
    float* yp = y + (long)n * F * D + c;
    double m = 0.0, r = 1.0;
    if (normalise) {
        double a = 0.0;
        for (int f = q; f < F; f += kLnLanes) a += ln_u(sp[(long)f * D]);
        m = ln_sum(red, q, cl, a) / (double)F;
        a = 0.0;
        for (int f = q; f < F; f += kLnLanes) {
            const double dlt = ln_u(sp[(long)f * D]) - m;
            a += dlt * dlt;
        }
        r = 1.0 / sqrt(ln_sum(red, q, cl, a) / (double)F + (double)kLfbEps);
        if (stats && q == 0) {
            stats[((long)n * 2 + 0) * D + c] = (float)m;
            stats[((long)n * 2 + 1) * D + c] = (float)r;
        }
    }
    for (int f = q; f < F; f += kLnLanes) yp[(long)f * D] = (float)((ln_u(sp[(long)f * D]) - m) * r);
}

__global__ __launch_bounds__(256) void lfb_lognorm_bwd_kernel(const float* __restrict__ s, const float* __restrict__ stats,
                                                              const float* __restrict__ dy, float* __restrict__ ds, int F, int D,
                                                              int normalise) {
    __shared__ double red[kLnLanes][32];
    const int nblk = D / 32, n = blockIdx.x / nblk, c = (blockIdx.x % nblk) * 32 + (threadIdx.x & 31);
    const int q = threadIdx.x >> 5, cl = threadIdx.x & 31;
    const long off = (long)n * F * D + c;
    const float *sp = s + off, *gp = dy + off;
    float* dp = ds + off;
    double m = 0.0, r = 1.0, k1 = 0.0, k2 = 0.0;
    if (normalise) {
        m = (double)stats[((long)n * 2 + 0) * D + c];
        r = (double)stats[((long)n * 2 + 1) * D + c];
        double a1 = 0.0, a2 = 0.0;
        for (int f = q; f < F; f += kLnLanes) {
            const double g = (double)gp[(long)f * D], xh = (ln_u(sp[(long)f * D]) - m) * r;
            a1 += g;
            a2 += g * xh;
        }
        k1 = ln_sum(red, q, cl, a1) / (double)F;
        k2 = ln_sum(red, q, cl, a2) / (double)F;
    }
    for (int f = q; f < F; f += kLnLanes) {
        const float sv = sp[(long)f * D];
        double g = (double)gp[(long)f * D];
        if (normalise) g = r * (g - (k1 + ((ln_u(sv) - m) * r) * k2));
        const double sgn = sv > 0.f ? 1.0 : (sv < 0.f ? -1.0 : 0.0);
        dp[(long)f * D] = (float)(g * sgn / (1.0 + (double)fabsf(sv)));
    }
}

struct LfbPlan {
    int F;            // frames
    int groups;       // forward: groups of 4 hops per workgroup (a span of 4 groups - 2 frames)
    int spans;        // forward: workgroups per (window, channel block)
    int hop_groups;   // backward: groups of 4 hops that hold a conv position (hops 2 ..)
    int slots;        // backward: workgroups per channel block
};

static int lfb_plan(int N, int L, int D, LfbPlan* p) {
    CPC_RETURN_IF(N < 1 || L < kLfbTaps || D < 32 || D % 32 != 0 || D > 512, CPC_ERR_SHAPE);
    const long F = (L - 99) / kLfbHop + 1;
    CPC_RETURN_IF((long)N * F * D >= (1L << 31) || (long)N * (L - 399) >= (1L << 31), CPC_ERR_SHAPE);
    const int ncb = D / 16;
    p->F = (int)F;
    // long spans (2 recomputed hops in 32) once they still give every CU a few workgroups, shorter ones for small batches
    int g = kLfbMaxGroups;
    while (g > 1 && (long)N * ncb * cdiv(F, 4 * g - 2) < 1024) g >>= 1;
    p->groups = g;
    p->spans = cdiv(F, 4 * g - 2);
    CPC_RETURN_IF((long)N * ncb * p->spans >= (1L << 31), CPC_ERR_SHAPE);
    const int hmax = (L - 50) / kLfbHop;                 // the last hop with a conv position (u = L - 50)
    p->hop_groups = cdiv(hmax - 1, 4);
    const long items = (long)N * p->hop_groups;
    const long want = 512 / ncb > 1 ? 512 / ncb : 1;     // about two workgroups per CU over all channel blocks
    p->slots = (int)(items < want ? items : want);
    return 0;
}

static long lfb_bwd_bytes(int D, const LfbPlan& p) { return (long)(D / 16) * p.slots * kLfbWFloats * (long)sizeof(float); }

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_lfb_layout(int N, int L, int D, long* sizes) {
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    LfbPlan p;
    const int rc = lfb_plan(N, L, D, &p);
    if (rc) return rc;
    sizes[0] = p.F;
    sizes[1] = 0;
    sizes[2] = lfb_bwd_bytes(D, p);
    return 0;
}

extern "C" int cpc_lfb_energy_forward(const float* x, const float* W, const float* b, const float* han, float* s, void* ws, int N,
                                      int L, int D, void* stream) {
    (void)ws;
    LfbPlan p;
    const int rc = lfb_plan(N, L, D, &p);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !W || !b || !han || !s, CPC_ERR_ARG);
    const dim3 grid((unsigned)((long)N * (D / 16) * p.spans)), block(kLfbThreads);
    hipLaunchKernelGGL(lfb_energy_fwd_kernel, grid, block, 0, (hipStream_t)stream, x, W, b, han, s, N, L, D, p.F, p.groups, p.spans);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_lfb_energy_backward(const float* x, const float* W, const float* b, const float* han, const float* gs,
                                       float* dW, float* db, void* ws, int N, int L, int D, void* stream) {
    LfbPlan p;
    const int rc = lfb_plan(N, L, D, &p);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !W || !b || !han || !gs || !dW || !db || !ws, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    float* partial = static_cast<float*>(ws);
    hipLaunchKernelGGL(lfb_energy_bwd_kernel, dim3((unsigned)((D / 16) * p.slots)), dim3(kLfbThreads), 0, st, x, W, b, han, gs,
                       partial, N, L, D, p.F, p.hop_groups, p.slots);
    CPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(lfb_reduce_kernel, dim3((unsigned)cdiv(2L * D * (kLfbTaps + 1), 256)), dim3(256), 0, st, partial, dW, db, D,
                       p.slots);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int lfb_lognorm_shape(int N, int F, int D) {
    CPC_RETURN_IF(N < 1 || F < 2 || D < 32 || D % 32 != 0 || D > 512 || (long)N * F * D >= (1L << 31), CPC_ERR_SHAPE);
    return 0;
}

extern "C" int cpc_lfb_lognorm_forward(const float* s, float* y, float* stats, int N, int F, int D, int normalise, void* stream) {
    const int rc = lfb_lognorm_shape(N, F, D);
    if (rc) return rc;
    CPC_RETURN_IF(!s || !y || s == y || normalise < 0 || normalise > 1, CPC_ERR_ARG);
    hipLaunchKernelGGL(lfb_lognorm_fwd_kernel, dim3((unsigned)(N * (D / 32))), dim3(256), 0, (hipStream_t)stream, s, y, stats, F, D,
                       normalise);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_lfb_lognorm_backward(const float* s, const float* stats, const float* dy, float* ds, int N, int F, int D,
                                        int normalise, void* stream) {
    const int rc = lfb_lognorm_shape(N, F, D);
    if (rc) return rc;
    CPC_RETURN_IF(!s || !dy || !ds || s == ds || dy == ds || normalise < 0 || normalise > 1 || (normalise && !stats), CPC_ERR_ARG);
    hipLaunchKernelGGL(lfb_lognorm_bwd_kernel, dim3((unsigned)(N * (D / 32))), dim3(256), 0, (hipStream_t)stream, s, stats, dy, ds,
                       F, D, normalise);
    CPC_LAUNCH_CHECK();
    return 0;
}
