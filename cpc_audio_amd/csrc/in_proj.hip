// Layer 0's input projection of the recurrent cells at any input width D in 1..512 (gru.hip, lstm.hip, rnn.hip at D != 256):
//
//   forward          out[M,N] = x[M,D] . W[N,D]^T + bias         N = 3H / 4H / H gate rows (any multiple of 128)
//   backward data    dx[M,D]  = dG[M,N] . W[N,D]
//   backward weight  dW[N,D]  = dG[M,N]^T . x[M,D]
//
// on exact-f32 MFMAs (v_mfma_f32_16x16x4_f32, as nce_wide.hip and mfcc.hip): nothing is known about the size of x -- MFCC
// coefficients reach the hundreds -- so no fp16-piece split.
//
// x is read and dx written at their true width, rows `ldx` floats apart, straight from / to the (B,S,D) tensors; the padding
// to the MFMA's K granule (4) and to the tile happens in LDS, where every tile is zero-filled past D and past the last row.
// Rows of x and dx are only 4-byte aligned unless D, ldx and the base pointer say otherwise: the template parameter AL picks
// 16-byte accesses where they do and 4-byte accesses elsewhere.  out and dG (N % 128 == 0 floats per row, 16-byte aligned
// bases) always move 16 bytes per lane; their offsets are 64-bit.  The weight is copied once per call into a zero-padded
// (N, Dp) matrix in scratch, Dp = D rounded up to 32 (at most 1024 x 512 floats), so its tiles load 16 bytes per lane too.
//
// The kernels stage 32 (backward data: 64) contraction indices of both operands in LDS per round (pitches 36 / 68 / 144 / 80 floats: the four
// k-quarters of a wave's MFMA operand land in disjoint banks), 256 threads = 4 waves:
//   * forward: 64 rows x 128 gate columns per workgroup, a wave owns 16 rows x 128 columns (8 accumulators).  The product is
//     formed transposed (A = W, B = x), so a lane ends up with 4 consecutive gate columns of one row: one 16-byte store.
//     The kernel is bound by out (M x N floats against M x D read);
//   * backward data: 32 rows x 128 of dx's columns per workgroup (M / 32 workgroups: 256 at B S = 8192), K = N in rounds of 64
//     with the next round's tiles prefetched into registers; column tiles past D are skipped.  Bound by the one pass over dG;
//   * backward weight: 128 gate rows x 64 columns of dW per (workgroup, row split); every split writes its partial tile and
//     ip_dw_reduce_kernel sums the splits in index order -- no atomics, the same bits every run.
#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kIpKc = 32;          // contraction indices staged per round
constexpr int kIpLdK = 36;         // pitch of a [row][k] tile (k contiguous)
constexpr int kIpLdN = 144;        // pitch of a [k][128 columns] tile
constexpr int kIpLdD = 80;         // pitch of a [k][64 columns] tile
constexpr int kIpDwRows = 256;     // least rows of a weight-gradient split
constexpr int kIpDxKc = 64;        // backward data: gate columns per round
constexpr int kIpDxLdK = 68;       // ... and the pitch of its [row][k] tile

__device__ __forceinline__ f32x4 ip_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void ip_lds4(float* dst, float4 v) { *reinterpret_cast<float4*>(dst) = v; }

static inline int ip_dp(int D) { return (D + 31) & ~31; }
static inline int ip_dc(int D) { return (D + 63) & ~63; }

// Wp[n][0:Dp] = W[n][0:D], zeros behind
__global__ __launch_bounds__(256) void ip_pad_w_kernel(const float* __restrict__ W, float* __restrict__ Wp, int N, int D, int Dp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * Dp) return;
    const int n = (int)(idx / Dp), d = (int)(idx - (long)n * Dp);
    Wp[idx] = d < D ? W[(long)n * D + d] : 0.f;
}

// grid = (ceil(M / 64), N / 128)
template <bool AL>
__global__ __launch_bounds__(256) void ip_fwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ Wp, int Dp,
                                                     const float* __restrict__ bias, float* __restrict__ out, int M, int N, int D) {
    __shared__ float xs[64 * kIpLdK];
    __shared__ float ws[128 * kIpLdK];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 128;
    const int K4 = (D + 3) & ~3;
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K4; k0 += kIpKc) {
        if (AL) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int idx = tid + 256 * q, r = idx >> 3, c = (idx & 7) * 4, m = m0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (m < M && k0 + c < D) v = *reinterpret_cast<const float4*>(x + (long)m * ldx + k0 + c);
                ip_lds4(xs + r * kIpLdK + c, v);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int idx = tid + 256 * q, r = idx >> 5, c = idx & 31, m = m0 + r;
                xs[r * kIpLdK + c] = (m < M && k0 + c < D) ? x[(long)m * ldx + k0 + c] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, r = idx >> 3, c = (idx & 7) * 4;
            ip_lds4(ws + r * kIpLdK + c, *reinterpret_cast<const float4*>(Wp + (long)(n0 + r) * Dp + k0 + c));
        }
        __syncthreads();
        const int nk = (K4 - k0) >> 2 < 8 ? (K4 - k0) >> 2 : 8;
        for (int kk = 0; kk < nk; ++kk) {
            const float b = xs[(16 * w + i) * kIpLdK + 4 * kk + kq];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = ip_mfma(ws[(16 * j + i) * kIpLdK + 4 * kk + kq], b, acc[j]);
        }
        __syncthreads();
    }
    // acc[j][r] = out[m0 + 16 w + i][n0 + 16 j + 4 kq + r]
    const int m = m0 + 16 * w + i;
    if (m >= M) return;
    float* orow = out + (long)m * N + n0 + 4 * kq;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float4 o = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        if (bias) {
            const float* bp = bias + n0 + 16 * j + 4 * kq;
            o.x += bp[0]; o.y += bp[1]; o.z += bp[2]; o.w += bp[3];
        }
        *reinterpret_cast<float4*>(orow + 16 * j) = o;
    }
}

// One round's MFMAs of a wave with NJ live column tiles (a compile-time count: the LDS reads of a whole round are issued together,
// where a run-time `j < nj` test around every MFMA made each one wait for its own read).  gs_row / ws_col: the lane's operands at k = kq
template <int NJ>
__device__ __forceinline__ void ip_dx_round(f32x4 (&acc)[4], const float* gs_row, const float* ws_col) {
#pragma unroll
    for (int kk = 0; kk < kIpDxKc / 4; ++kk) {
        const float b = gs_row[4 * kk];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = ip_mfma(ws_col[4 * kk * kIpLdN + 32 * j], b, acc[j]);
    }
}

// grid = (ceil(M / 32), ceil(D / 128)).  K = N is walked 64 gate columns per round; the next round's tiles are fetched into
// registers in front of the MFMAs of the current one (one workgroup per CU at B S = 8192: nothing else hides the loads).
// The 2 x 8 (row tile, column tile) accumulators are dealt out so that a narrow D still uses all four waves: wave w owns row
// tile w & 1 and the column tiles (w >> 1) + 2 j.
template <bool AL>
__global__ __launch_bounds__(256) void ip_dx_kernel(const float* __restrict__ dG, const float* __restrict__ Wp, int Dp,
                                                    float* __restrict__ dx, long ldx, int M, int N, int D) {
    __shared__ float gs[32 * kIpDxLdK];        // [row][k = gate column]
    __shared__ float ws[kIpDxKc * kIpLdN];     // [k][d]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * 32, d0 = blockIdx.y * 128;
    const int mt = w & 1, dh = w >> 1;
    int nj = (D - d0 - 16 * dh + 31) >> 5;     // this wave's column tiles that start in front of D
    nj = nj > 4 ? 4 : nj;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 gv[2], wv[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + 256 * q, r = idx >> 4, c = (idx & 15) * 4, m = m0 + r;
            gv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < M) gv[q] = *reinterpret_cast<const float4*>(dG + (long)m * N + k0 + c);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int idx = tid + 256 * q, r = idx >> 5, c = (idx & 31) * 4;
            wv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (d0 + c < Dp) wv[q] = *reinterpret_cast<const float4*>(Wp + (long)(k0 + r) * Dp + d0 + c);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < N; k0 += kIpDxKc) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + 256 * q;
            ip_lds4(gs + (idx >> 4) * kIpDxLdK + (idx & 15) * 4, gv[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int idx = tid + 256 * q;
            ip_lds4(ws + (idx >> 5) * kIpLdN + (idx & 31) * 4, wv[q]);
        }
        __syncthreads();
        if (k0 + kIpDxKc < N) fetch(k0 + kIpDxKc);
        const float* gs_row = gs + (16 * mt + i) * kIpDxLdK + kq;
        const float* ws_col = ws + kq * kIpLdN + 16 * dh + i;
        switch (nj) {
            case 1: ip_dx_round<1>(acc, gs_row, ws_col); break;
            case 2: ip_dx_round<2>(acc, gs_row, ws_col); break;
            case 3: ip_dx_round<3>(acc, gs_row, ws_col); break;
            case 4: ip_dx_round<4>(acc, gs_row, ws_col); break;
            default: break;
        }
        __syncthreads();
    }
    // acc[j][r] = dx[m0 + 16 mt + i][d0 + 16 (dh + 2 j) + 4 kq + r]
    const int m = m0 + 16 * mt + i;
    if (m >= M) return;
    float* row = dx + (long)m * ldx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = d0 + 16 * (dh + 2 * j) + 4 * kq;
        if (AL) {
            if (d < D) *reinterpret_cast<float4*>(row + d) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (d + r < D) row[d + r] = acc[j][r];
        }
    }
}

template <int NJ>
__device__ __forceinline__ void ip_dw_round(f32x4 (&acc)[2][4], const float* ga, const float* xb) {
#pragma unroll
    for (int kk = 0; kk < kIpKc / 4; ++kk) {
        const float a0 = ga[4 * kk * kIpLdN], a1 = ga[4 * kk * kIpLdN + 16];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float b = xb[4 * kk * kIpLdD + 16 * j];
            acc[0][j] = ip_mfma(a0, b, acc[0][j]);
            acc[1][j] = ip_mfma(a1, b, acc[1][j]);
        }
    }
}

// grid = (N / 128, ceil(D / 64), splits); split z covers rows [z * rows, min(M, (z + 1) * rows)); part: [split][N][Dc]
template <bool AL>
__global__ __launch_bounds__(256) void ip_dw_kernel(const float* __restrict__ dG, const float* __restrict__ x, long ldx,
                                                    float* __restrict__ part, int M, int N, int D, int Dc, int rows) {
    __shared__ float gs[kIpKc * kIpLdN];       // [k = row][gate column]
    __shared__ float xs[kIpKc * kIpLdD];       // [k = row][d]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 128, d0 = blockIdx.y * 64;
    const long mb = (long)blockIdx.z * rows;
    const long me = mb + rows < M ? mb + rows : M;
    int nj = (D - d0 + 15) >> 4;               // column tiles that start in front of D
    nj = nj > 4 ? 4 : nj;
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long mm = mb; mm < me; mm += kIpKc) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + 256 * q, r = idx >> 5, c = (idx & 31) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (mm + r < me) v = *reinterpret_cast<const float4*>(dG + (mm + r) * N + n0 + c);
            ip_lds4(gs + r * kIpLdN + c, v);
        }
        if (AL) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int idx = tid + 256 * q, r = idx >> 4, c = (idx & 15) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (mm + r < me && d0 + c < D) v = *reinterpret_cast<const float4*>(x + (mm + r) * ldx + d0 + c);
                ip_lds4(xs + r * kIpLdD + c, v);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int idx = tid + 256 * q, r = idx >> 6, c = idx & 63;
                xs[r * kIpLdD + c] = (mm + r < me && d0 + c < D) ? x[(mm + r) * ldx + d0 + c] : 0.f;
            }
        }
        __syncthreads();
        const float* ga = gs + kq * kIpLdN + 32 * w + i;
        const float* xb = xs + kq * kIpLdD + i;
        switch (nj) {                              // (a compile-time tile count per round, as ip_dx_round)
            case 1: ip_dw_round<1>(acc, ga, xb); break;
            case 2: ip_dw_round<2>(acc, ga, xb); break;
            case 3: ip_dw_round<3>(acc, ga, xb); break;
            default: ip_dw_round<4>(acc, ga, xb); break;
        }
        __syncthreads();
    }
    // acc[t][j][r] = partial dW[n0 + 32 w + 16 t + 4 kq + r][d0 + 16 j + i]
    float* p = part + ((long)blockIdx.z * N + n0 + 32 * w + 4 * kq) * Dc + d0 + i;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nj) {
#pragma unroll
                for (int r = 0; r < 4; ++r) p[(long)(16 * t + r) * Dc + 16 * j] = acc[t][j][r];
            }
}

// dW[n][d] = the splits' partials summed in index order
__global__ __launch_bounds__(256) void ip_dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dW, int N, int D, int Dc,
                                                           int splits) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * D) return;
    const int n = (int)(idx / D), d = (int)(idx - (long)n * D);
    const float* p = part + (long)n * Dc + d;
    float v = p[0];
    for (int s = 1; s < splits; ++s) v += p[(long)s * N * Dc];
    dW[idx] = v;
}

// ------------------------------------------------------------------ host side
// Row splits of the weight gradient: kIpDwRows rows each, doubled until splits * ceil(D / 64) <= 64 (the partials stay below
// 64 * N * 64 floats: 16 MB at N = 1024) -- a function of the shape alone, so two runs sum in the same order.
static void ip_dw_plan(long M, int D, int* splits, int* rows) {
    const int cap = 64 / cdiv(D, 64) > 1 ? 64 / cdiv(D, 64) : 1;
    long r = kIpDwRows;
    while ((M + r - 1) / r > cap) r *= 2;
    *rows = (int)r;
    *splits = (int)((M + r - 1) / r);
}

bool in_proj_shape_ok(long M, int N, int D) {
    return M >= 1 && M <= (1L << 24) && N >= 128 && N <= (1 << 16) && N % 128 == 0 && D >= 1 && D <= kInProjMaxD;
}

long in_proj_w_floats(int N, int D) { return align64l((long)N * ip_dp(D)); }

long in_proj_scratch_floats(long M, int N, int D) {
    if (!in_proj_shape_ok(M, N, D)) return 0;
    int splits = 0, rows = 0;
    ip_dw_plan(M, D, &splits, &rows);
    return in_proj_w_floats(N, D) + align64l((long)splits * N * ip_dc(D));
}

static bool ip_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool ip_rows_aligned(const float* p, long ld, int D) { return D % 4 == 0 && ld % 4 == 0 && ip_aligned16(p); }

static int ip_pad_w(const float* W, float* Wp, int N, int D, hipStream_t st) {
    const int Dp = ip_dp(D);
    hipLaunchKernelGGL(ip_pad_w_kernel, dim3(cdiv((long)N * Dp, 256)), dim3(256), 0, st, W, Wp, N, D, Dp);
    CPC_LAUNCH_CHECK();
    return 0;
}

int in_proj_forward(const float* x, long ldx, const float* W, const float* bias, float* scratch, float* out, int M, int N, int D,
                    hipStream_t st) {
    CPC_RETURN_IF(!in_proj_shape_ok(M, N, D) || ldx < D, CPC_ERR_SHAPE);
    CPC_RETURN_IF(!x || !W || !scratch || !out || !ip_aligned16(scratch) || !ip_aligned16(out), CPC_ERR_ARG);
    int rc = ip_pad_w(W, scratch, N, D, st);
    if (rc) return rc;
    const dim3 grid(cdiv(M, 64), N / 128);
    if (ip_rows_aligned(x, ldx, D)) hipLaunchKernelGGL(ip_fwd_kernel<true>, grid, dim3(256), 0, st, x, ldx, scratch, ip_dp(D), bias, out, M, N, D);
    else hipLaunchKernelGGL(ip_fwd_kernel<false>, grid, dim3(256), 0, st, x, ldx, scratch, ip_dp(D), bias, out, M, N, D);
    CPC_LAUNCH_CHECK();
    return 0;
}

// dx and / or dW (either may be NULL: that product is not formed)
int in_proj_backward(const float* x, long ldx, const float* W, const float* dG, float* scratch, float* dx, float* dW, int M, int N,
                     int D, hipStream_t st) {
    CPC_RETURN_IF(!in_proj_shape_ok(M, N, D) || ldx < D, CPC_ERR_SHAPE);
    CPC_RETURN_IF(!x || !W || !dG || !scratch || (!dx && !dW) || !ip_aligned16(scratch) || !ip_aligned16(dG), CPC_ERR_ARG);
    if (dx) {
        int rc = ip_pad_w(W, scratch, N, D, st);
        if (rc) return rc;
        const dim3 grid(cdiv(M, 32), cdiv(D, 128));
        if (ip_rows_aligned(dx, ldx, D)) hipLaunchKernelGGL(ip_dx_kernel<true>, grid, dim3(256), 0, st, dG, scratch, ip_dp(D), dx, ldx, M, N, D);
        else hipLaunchKernelGGL(ip_dx_kernel<false>, grid, dim3(256), 0, st, dG, scratch, ip_dp(D), dx, ldx, M, N, D);
        CPC_LAUNCH_CHECK();
    }
    if (dW) {
        int splits = 0, rows = 0;
        ip_dw_plan(M, D, &splits, &rows);
        float* part = scratch + in_proj_w_floats(N, D);
        const int Dc = ip_dc(D);
        const dim3 grid(N / 128, cdiv(D, 64), splits);
        if (ip_rows_aligned(x, ldx, D)) hipLaunchKernelGGL(ip_dw_kernel<true>, grid, dim3(256), 0, st, dG, x, ldx, part, M, N, D, Dc, rows);
        else hipLaunchKernelGGL(ip_dw_kernel<false>, grid, dim3(256), 0, st, dG, x, ldx, part, M, N, D, Dc, rows);
        hipLaunchKernelGGL(ip_dw_reduce_kernel, dim3(cdiv((long)N * D, 256)), dim3(256), 0, st, part, dW, N, D, Dc, splits);
        CPC_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" long cpc_in_proj_scratch_floats(int M, int N, int D) { return in_proj_scratch_floats(M, N, D); }

extern "C" int cpc_in_proj_forward(const float* x, long ldx, const float* w, const float* bias, float* scratch, float* out, int M,
                                   int N, int D, void* stream) {
    return in_proj_forward(x, ldx, w, bias, scratch, out, M, N, D, (hipStream_t)stream);
}

extern "C" int cpc_in_proj_backward(const float* x, long ldx, const float* w, const float* dg, float* scratch, float* dx, float* dw,
                                    int M, int N, int D, void* stream) {
    return in_proj_backward(x, ldx, w, dg, scratch, dx, dw, M, N, D, (hipStream_t)stream);
}
