// The conv encoder at any hidden width C in 2..512 (C != 256: enc_conv0.hip / enc_conv.hip keep that width):
// five times relu(ChannelNorm(conv_i(x))) with the geometry k/s/p = 10/5/3, 8/4/2, 4/2/1 x 3, forward and backward, channels-last,
// fp32 storage, exact-f32 MFMAs (v_mfma_f32_16x16x4_f32, as in_proj.hip / nce_wide.hip / mfcc.hip); cpc_set_mfma_mode is not read.
//
// Padded storage.  Every internal activation and gradient has a row pitch Cp = 64 ceil(C / 64); the kernel that
// produces a tensor writes its pad columns as zeros.  conv1..4's weights are copied once per call into zero-padded GEMM layouts,
// so every tile load is 16 bytes per lane with no mask in the K loop.  z and the 20 gradients have their true shapes.
//
//   * conv1..4 forward: an overlapping-row NT GEMM.  The im2col row of output step t is the k Cp contiguous floats that start at
//     input row t s - p; a 32-wide K round lies inside one tap, whose row is either inside [0, L_in) or read as zeros.
//     ew_gemm_kernel owns 128 rows x 64 columns per workgroup and writes conv + bias; ChannelNorm and ReLU are a second pass
//     (ew_norm_fwd_kernel, one wave per row) -- a workgroup then need not own all Cp columns of its rows, so one tile shape fills
//     the chip at every width, and the pass costs one read and two writes of M x Cp floats beside a GEMM of K = k Cp.
//   * backward data gradient, gather form: with k = 2 s an input row u receives the pairs (t, j) = (v, r) and (v - 1, r + s),
//     v = (u + p) / s, r = (u + p) % s.  For a fixed phase r that is the same overlapping-row GEMM on dx with two taps, stride 1,
//     padding 1 and the weight slice Wd[r]; the s phases are the grid's z.  v runs far enough to reach every u < L_in, and a row no
//     window touches reads two rows outside dx: an exact zero.
//   * weight gradient: a TN product over the B L_i rows, 64 x 64 tiles of the (Cp, k Cp) matrix per (workgroup, row split); the
//     splits' partial tiles are summed in index order by ew_dw_reduce_kernel.
//   * the column sums (norm weight, norm bias, conv bias) leave ew_norm_bwd_kernel as per-workgroup partials, summed in index order.
// No float atomics, no hand-over between workgroups: two runs give the same bits.  Offsets into activations are 64-bit.
#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kEwMaxC = 512;
constexpr int kEwMinC = 2;
constexpr int kEwLdK = 36;        // pitch of a [row][32 k] tile: a lane's 8 consecutive k are two 16-byte reads
constexpr int kEwLdN = 80;        // pitch of a [32 k][64 columns] tile
constexpr int kEwNormRows = 16;   // rows per workgroup of the forward norm pass and of conv0 (4 per wave)

struct EwGeom { int k, s, p; };
static const EwGeom kEwGeom[5] = {{10, 5, 3}, {8, 4, 2}, {4, 2, 1}, {4, 2, 1}, {4, 2, 1}};

__device__ __forceinline__ f32x4 ew_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void ew_lds4(float* dst, float4 v) { *reinterpret_cast<float4*>(dst) = v; }
__device__ __forceinline__ float ew_elem(const float4& lo, const float4& hi, int kk) {
    switch (kk) {
        case 0: return lo.x; case 1: return lo.y; case 2: return lo.z; case 3: return lo.w;
        case 4: return hi.x; case 5: return hi.y; case 6: return hi.z; default: return hi.w;
    }
}

// conv weight (C, C, k) -> the forward GEMM's B operand Wp[n][j Cp + c] = W[n][c][j], zeros in the padding
__global__ __launch_bounds__(256) void ew_pad_w_kernel(const float* __restrict__ W, float* __restrict__ Wp, int C, int Cp, int k) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long K = (long)k * Cp;
    if (idx >= (long)Cp * K) return;
    const int n = (int)(idx / K), kc = (int)(idx - n * K), j = kc / Cp, c = kc - j * Cp;
    Wp[idx] = (n < C && c < C) ? W[((long)n * C + c) * k + j] : 0.f;
}

// conv weight (C, C, 2 s) -> the data gradient's operands Wd[r][c][q Cp + n], q = 0: W[n][c][r + s] (the window one step back),
// q = 1: W[n][c][r]
__global__ __launch_bounds__(256) void ew_pad_wd_kernel(const float* __restrict__ W, float* __restrict__ Wd, int C, int Cp, int s) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)Cp * 2 * Cp;
    if (idx >= per * s) return;
    const int r = (int)(idx / per);
    const long rem = idx - r * per;
    const int c = (int)(rem / (2 * Cp)), qn = (int)(rem - (long)c * 2 * Cp), q = qn / Cp, n = qn - q * Cp;
    Wd[idx] = (n < C && c < C) ? W[((long)n * C + c) * (2 * s) + r + (q ? 0 : s)] : 0.f;
}

// The overlapping-row NT GEMM.  GEMM row m = (b, v), v < V; its A row is the taps * Cp floats of X that start at row v s - p of
// sequence b (Lx rows per sequence; rows outside are zeros); B = Wp + z wz, (Cp, taps Cp) row-major; the result (+ bias) goes to row
// u = v os + oo + z of sequence b of `out` (Lo rows per sequence) when 0 <= u < Lo.  grid = (ceil(M / 128), Cp / 64, phases)
__global__ __launch_bounds__(256) void ew_gemm_kernel(const float* __restrict__ X, int Lx, int taps, int s, int p,
                                                      const float* __restrict__ Wp, long wz, const float* __restrict__ bias,
                                                      float* __restrict__ out, int Lo, int os, int oo, int V, long M, int Cp, int C) {
    __shared__ float xs[128 * kEwLdK];
    __shared__ float ws[64 * kEwLdK];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const long m0 = (long)blockIdx.x * 128;
    const int n0 = blockIdx.y * 64;
    const int K = taps * Cp;
    const float* Wz = Wp + (long)blockIdx.z * wz;
    const int c4 = (tid & 7) * 4;
    // the four A rows this thread stages: where tap 0 starts, and which input row that is
    long xoff[4];
    int vin[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long m = m0 + (tid >> 3) + 32 * q;
        if (m < M) {
            const long b = m / V;
            const int v = (int)(m - b * V);
            vin[q] = v * s - p;
            xoff[q] = (b * Lx + vin[q]) * Cp;
        } else {
            vin[q] = -(1 << 28);                // never a row of X
            xoff[q] = 0;
        }
    }
    float4 xv[4], wv[2];
    auto fetch = [&](int k0) {
        const int j = k0 / Cp;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = vin[q] + j;
            xv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row >= 0 && row < Lx) xv[q] = *reinterpret_cast<const float4*>(X + xoff[q] + k0 + c4);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
            wv[q] = *reinterpret_cast<const float4*>(Wz + (long)(n0 + (tid >> 3) + 32 * q) * K + k0 + c4);
    };
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ew_lds4(xs + ((tid >> 3) + 32 * q) * kEwLdK + c4, xv[q]);
#pragma unroll
        for (int q = 0; q < 2; ++q) ew_lds4(ws + ((tid >> 3) + 32 * q) * kEwLdK + c4, wv[q]);
        __syncthreads();
        if (k0 + 32 < K) fetch(k0 + 32);
        // MFMA round kk contracts the round's index 8 kq + kk: both operands use the same order, and a lane's eight are contiguous
        float4 bl[2], bh[2], al[4], ah[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float* src = xs + (32 * w + 16 * t + i) * kEwLdK + 8 * kq;
            bl[t] = *reinterpret_cast<const float4*>(src);
            bh[t] = *reinterpret_cast<const float4*>(src + 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* src = ws + (16 * j + i) * kEwLdK + 8 * kq;
            al[j] = *reinterpret_cast<const float4*>(src);
            ah[j] = *reinterpret_cast<const float4*>(src + 4);
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float b = ew_elem(bl[t], bh[t], kk);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t][j] = ew_mfma(ew_elem(al[j], ah[j], kk), b, acc[t][j]);
            }
        __syncthreads();
    }
    // acc[t][j][r] = result[m0 + 32 w + 16 t + i][n0 + 16 j + 4 kq + r]
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long m = m0 + 32 * w + 16 * t + i;
        if (m >= M) continue;
        const long b = m / V;
        const int v = (int)(m - b * V);
        const int u = v * os + oo + (int)blockIdx.z;
        if (u < 0 || u >= Lo) continue;
        float* orow = out + (b * Lo + u) * Cp + n0 + 4 * kq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4 o = make_float4(acc[t][j][0], acc[t][j][1], acc[t][j][2], acc[t][j][3]);
            if (bias) {
                const int n = n0 + 16 * j + 4 * kq;
                o.x += n < C ? bias[n] : 0.f;
                o.y += n + 1 < C ? bias[n + 1] : 0.f;
                o.z += n + 2 < C ? bias[n + 2] : 0.f;
                o.w += n + 3 < C ? bias[n + 3] : 0.f;
            }
            *reinterpret_cast<float4*>(orow + 16 * j) = o;
        }
    }
}

// One row's ChannelNorm statistics over the C true channels; v[q] = channel lane + 64 q (zero beyond C)
__device__ __forceinline__ void ew_row_stats(const float (&v)[8], int lane, int C, float& mean, float& rstd) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += v[q];
    mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float d = lane + 64 * q < C ? v[q] - mean : 0.f;
        sq += d * d;
    }
    const float var = wave_sum(sq) / (float)(C - 1);       // unbiased, as the reference's x.var
    rstd = 1.0f / sqrtf(var + kNormEps);
}

// ChannelNorm + ReLU over conv + bias (in place: xh holds the conv output on entry and xhat on return); y at pitch ldy (Cp: its pad
// columns are zeroed; C: z).  One wave per row, kEwNormRows rows per workgroup.
__global__ __launch_bounds__(256) void ew_norm_fwd_kernel(float* __restrict__ xh, const float* __restrict__ nw,
                                                          const float* __restrict__ nb, float* __restrict__ y, int ldy,
                                                          float* __restrict__ rstd_out, long M, int C, int Cp) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    float gw[8], gb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q;
        gw[q] = c < C ? nw[c] : 0.f;
        gb[q] = c < C ? nb[c] : 0.f;
    }
    for (int rr = 0; rr < kEwNormRows / 4; ++rr) {
        const long m = (long)blockIdx.x * kEwNormRows + 4 * rr + w;
        if (m >= M) break;                                  // wave-uniform
        float* row = xh + m * Cp;
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (q < nq && lane + 64 * q < C) ? row[lane + 64 * q] : 0.f;
        float mean, rstd;
        ew_row_stats(v, lane, C, mean, rstd);
        if (lane == 0) rstd_out[m] = rstd;
        float* yrow = y + m * ldy;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            if (q < nq) {
                const bool live = c < C;
                const float h = live ? (v[q] - mean) * rstd : 0.f;
                row[c] = h;
                if (c < ldy) yrow[c] = live ? fmaxf(relu_in(h * gw[q] + gb[q]), 0.f) : 0.f;
            }
        }
    }
}

// conv0 (one input channel, ten taps, stride 5, padding 3) + ChannelNorm + ReLU: y0 (pitch Cp, zero pad columns), rstd0, mean0.
// The weights sit transposed in LDS ([tap][channel]); one wave per row.
__global__ __launch_bounds__(256) void ew_conv0_fwd_kernel(const float* __restrict__ wave, const float* __restrict__ w0,
                                                           const float* __restrict__ b0, const float* __restrict__ nw,
                                                           const float* __restrict__ nb, float* __restrict__ y,
                                                           float* __restrict__ rstd_out, float* __restrict__ mean_out, int L,
                                                           int L0, long M, int C, int Cp) {
    __shared__ float wt[10 * kEwMaxC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    for (int idx = threadIdx.x; idx < 10 * Cp; idx += 256) {
        const int j = idx / Cp, c = idx - j * Cp;
        wt[j * kEwMaxC + c] = c < C ? w0[c * 10 + j] : 0.f;
    }
    __syncthreads();
    float gw[8], gb[8], cb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q;
        gw[q] = c < C ? nw[c] : 0.f;
        gb[q] = c < C ? nb[c] : 0.f;
        cb[q] = c < C ? b0[c] : 0.f;
    }
    for (int rr = 0; rr < kEwNormRows / 4; ++rr) {
        const long m = (long)blockIdx.x * kEwNormRows + 4 * rr + w;
        if (m >= M) break;
        const long b = m / L0;
        const int t = (int)(m - b * L0);
        float x[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int pos = 5 * t - 3 + j;
            x[j] = (pos >= 0 && pos < L) ? wave[b * L + pos] : 0.f;
        }
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float a = cb[q];
            if (q < nq) {
#pragma unroll
                for (int j = 0; j < 10; ++j) a = fmaf(wt[j * kEwMaxC + lane + 64 * q], x[j], a);
            }
            v[q] = a;                                       // zero beyond C: zero weights and bias
        }
        float mean, rstd;
        ew_row_stats(v, lane, C, mean, rstd);
        if (lane == 0) { rstd_out[m] = rstd; mean_out[m] = mean; }
        float* yrow = y + m * Cp;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            if (q < nq) yrow[c] = c < C ? fmaxf(relu_in((v[q] - mean) * rstd * gw[q] + gb[q]), 0.f) : 0.f;
        }
    }
}

// ReLU and ChannelNorm backward of one row held one channel per (lane, q): g = dy [y > 0]; returns dx (the gradient of the conv
// output; zero beyond C) and adds the row's terms to the three column sums
__device__ __forceinline__ void ew_row_norm_bwd(const float (&g)[8], const float (&h)[8], const float (&gw)[8], float rstd, int lane,
                                                int C, float (&dx)[8], float (&s_nw)[8], float (&s_nb)[8], float (&s_cb)[8]) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float dh = g[q] * gw[q];
        s1 += dh;
        s2 += dh * h[q];
    }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)(C - 1);                     // the unbiased variance's divisor
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float dh = g[q] * gw[q];
        dx[q] = lane + 64 * q < C ? rstd * (dh - s1 - h[q] * s2) : 0.f;
        s_nw[q] += g[q] * h[q];
        s_nb[q] += g[q];
        s_cb[q] += dx[q];
    }
}

// the four waves' column sums -> part[blockIdx.x][which][Cp], waves added in index order
__device__ __forceinline__ void ew_store_colsums(float* red, const float (&s)[8], int which, int nwhich, float* __restrict__ part,
                                                 int Cp) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) red[w * kEwMaxC + lane + 64 * q] = s[q];
    __syncthreads();
#pragma clang loop vectorize(disable) interleave(disable)       // (paired up, the adds become packed fp32: build.py's gate)
    for (int c = threadIdx.x; c < Cp; c += 256)
        part[((long)blockIdx.x * nwhich + which) * Cp + c] = ((red[c] + red[kEwMaxC + c]) + red[2 * kEwMaxC + c]) + red[3 * kEwMaxC + c];
}

// Layers 1..4: dx = ChannelNorm'(ReLU'(dy)) at pitch Cp (zero pad columns) and the workgroup's partial column sums
// part[block][0..2][Cp] = norm weight, norm bias, conv bias.  dy at pitch lddy, y (the ReLU's output: its mask) at pitch ldy.
__global__ __launch_bounds__(256) void ew_norm_bwd_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                          const float* __restrict__ xh, const float* __restrict__ rstd,
                                                          const float* __restrict__ nw, float* __restrict__ dx,
                                                          float* __restrict__ part, long M, int C, int Cp, int rows) {
    __shared__ float red[4 * kEwMaxC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    float gw[8], s_nw[8], s_nb[8], s_cb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        gw[q] = lane + 64 * q < C ? nw[lane + 64 * q] : 0.f;
        s_nw[q] = s_nb[q] = s_cb[q] = 0.f;
    }
    const long mb = (long)blockIdx.x * rows;
    const long me = mb + rows < M ? mb + rows : M;
    for (long m = mb + w; m < me; m += 4) {
        float g[8], h[8], d[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            const bool live = q < nq && c < C;
            h[q] = live ? xh[m * Cp + c] : 0.f;
            g[q] = (live && y[m * ldy + c] > 0.f) ? dy[m * lddy + c] : 0.f;
        }
        ew_row_norm_bwd(g, h, gw, rstd[m], lane, C, d, s_nw, s_nb, s_cb);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (q < nq) dx[m * Cp + lane + 64 * q] = d[q];
    }
    ew_store_colsums(red, s_nw, 0, 3, part, Cp);
    ew_store_colsums(red, s_nb, 1, 3, part, Cp);
    ew_store_colsums(red, s_cb, 2, 3, part, Cp);
}

// out[which][c] = sum over the workgroups' partials in index order, c < C; dst[which] may be NULL
struct EwColDst { float* p[13]; int stride[13]; };
__global__ __launch_bounds__(256) void ew_colsum_reduce_kernel(const float* __restrict__ part, int nblk, int nwhich, int Cp, int C,
                                                               EwColDst dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= nwhich * Cp) return;
    const int which = idx / Cp, c = idx - which * Cp;
    if (c >= C || !dst.p[which]) return;
    const float* p = part + (long)which * Cp + c;
    float v = p[0];
    for (int b = 1; b < nblk; ++b) v += p[(long)b * nwhich * Cp];
    dst.p[which][(long)c * dst.stride[which]] = v;
}

// Layer 0 backward: conv0 is formed again from the wave (xhat0 is not stored), then ReLU' / ChannelNorm', and the workgroup's partial
// sums part[block][0..12][Cp]: 0..9 = the ten taps of conv0's weight gradient, 10 = norm weight, 11 = norm bias, 12 = conv bias
__global__ __launch_bounds__(256) void ew_conv0_bwd_kernel(const float* __restrict__ wave, const float* __restrict__ w0,
                                                           const float* __restrict__ b0, const float* __restrict__ nw,
                                                           const float* __restrict__ y, const float* __restrict__ dy,
                                                           const float* __restrict__ rstd, const float* __restrict__ mean,
                                                           float* __restrict__ part, int L, int L0, long M, int C, int Cp, int rows) {
    __shared__ float wt[10 * kEwMaxC];
    float* red = wt;                                        // reused for the column sums once the rows are done
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    for (int idx = threadIdx.x; idx < 10 * Cp; idx += 256) {
        const int j = idx / Cp, c = idx - j * Cp;
        wt[j * kEwMaxC + c] = c < C ? w0[c * 10 + j] : 0.f;
    }
    __syncthreads();
    float gw[8], cb[8], s_nw[8], s_nb[8], s_cb[8], s_w[10][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q;
        gw[q] = c < C ? nw[c] : 0.f;
        cb[q] = c < C ? b0[c] : 0.f;
        s_nw[q] = s_nb[q] = s_cb[q] = 0.f;
#pragma unroll
        for (int j = 0; j < 10; ++j) s_w[j][q] = 0.f;
    }
    const long mb = (long)blockIdx.x * rows;
    const long me = mb + rows < M ? mb + rows : M;
    for (long m = mb + w; m < me; m += 4) {
        const long b = m / L0;
        const int t = (int)(m - b * L0);
        float x[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int pos = 5 * t - 3 + j;
            x[j] = (pos >= 0 && pos < L) ? wave[b * L + pos] : 0.f;
        }
        const float mu = mean[m], rs = rstd[m];
        float g[8], h[8], d[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            const bool live = q < nq && c < C;
            float a = cb[q];
            if (live) {
#pragma unroll
                for (int j = 0; j < 10; ++j) a = fmaf(wt[j * kEwMaxC + c], x[j], a);
            }
            h[q] = live ? (a - mu) * rs : 0.f;
            g[q] = (live && y[m * Cp + c] > 0.f) ? dy[m * Cp + c] : 0.f;
        }
        ew_row_norm_bwd(g, h, gw, rs, lane, C, d, s_nw, s_nb, s_cb);
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int j = 0; j < 10; ++j) s_w[j][q] = fmaf(d[q], x[j], s_w[j][q]);
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) ew_store_colsums(red, s_w[j], j, 13, part, Cp);
    ew_store_colsums(red, s_nw, 10, 13, part, Cp);
    ew_store_colsums(red, s_nb, 11, 13, part, Cp);
    ew_store_colsums(red, s_cb, 12, 13, part, Cp);
}

// Weight gradient, TN: part[z][n][j Cp + c] = sum over the split's rows m = (b, t) of dx[m][n] X[b][t s - p + j][c].
// grid = (Cp / 64, k Cp / 64, splits); a 64-column tile lies inside one tap
__global__ __launch_bounds__(256) void ew_wgrad_kernel(const float* __restrict__ dx, const float* __restrict__ X, int Lx, int Lo, int s,
                                                       int p, float* __restrict__ part, long M, int Cp, int K, int rows) {
    __shared__ float gs[32 * kEwLdN];       // [k = row][n]
    __shared__ float xs[32 * kEwLdN];       // [k = row][column]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * 64, kc0 = blockIdx.y * 64;
    const int j = kc0 / Cp, c0 = kc0 - j * Cp;
    const long mb = (long)blockIdx.z * rows;
    const long me = mb + rows < M ? mb + rows : M;
    const int nh = w & 1, ch = w >> 1;
    f32x4 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c4 = (tid & 15) * 4;
    for (long mm = mb; mm < me; mm += 32) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int r = (tid >> 4) + 16 * q;
            const long m = mm + r;
            float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), xv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < me) {
                gv = *reinterpret_cast<const float4*>(dx + m * Cp + n0 + c4);
                const long b = m / Lo;
                const int row = (int)(m - b * Lo) * s - p + j;
                if (row >= 0 && row < Lx) xv = *reinterpret_cast<const float4*>(X + (b * Lx + row) * Cp + c0 + c4);
            }
            ew_lds4(gs + r * kEwLdN + c4, gv);
            ew_lds4(xs + r * kEwLdN + c4, xv);
        }
        __syncthreads();
        const float* ga = gs + kq * kEwLdN + 32 * nh + i;
        const float* xb = xs + kq * kEwLdN + 32 * ch + i;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const float a0 = ga[4 * kk * kEwLdN], a1 = ga[4 * kk * kEwLdN + 16];
            const float b0 = xb[4 * kk * kEwLdN], b1 = xb[4 * kk * kEwLdN + 16];
            acc[0][0] = ew_mfma(a0, b0, acc[0][0]);
            acc[0][1] = ew_mfma(a0, b1, acc[0][1]);
            acc[1][0] = ew_mfma(a1, b0, acc[1][0]);
            acc[1][1] = ew_mfma(a1, b1, acc[1][1]);
        }
        __syncthreads();
    }
    // acc[t][u][r] = partial dWp[n0 + 32 nh + 16 t + 4 kq + r][kc0 + 32 ch + 16 u + i]
    float* pp = part + ((long)blockIdx.z * Cp + n0 + 32 * nh + 4 * kq) * K + kc0 + 32 * ch + i;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) pp[(long)(16 * t + r) * K + 16 * u] = acc[t][u][r];
}

// dW[n][c][j] = the splits' partials summed in index order
__global__ __launch_bounds__(256) void ew_dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dW, int C, int Cp, int k,
                                                           int splits) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * C * k) return;
    const int n = (int)(idx / ((long)C * k));
    const int rem = (int)(idx - (long)n * C * k), c = rem / k, j = rem - c * k;
    const long K = (long)k * Cp;
    const float* p = part + (long)n * K + (long)j * Cp + c;
    float v = p[0];
    for (int z = 1; z < splits; ++z) v += p[(long)z * Cp * K];
    dW[idx] = v;
}

// dst (rows, C) = src (rows, Cp)[:, :C]
__global__ __launch_bounds__(256) void ew_unpad_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, int C, int Cp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C) return;
    const long m = idx / C;
    dst[idx] = src[m * Cp + (idx - m * C)];
}

// ------------------------------------------------------------------ host side
static inline long ew_align(long v) { return (v + 63) & ~63L; }

struct EwLayout {
    int L[5], Cp;
    long y[4], xhat[5], rstd[5], mean0, saved_total;       // offsets (floats) into `saved`
    long wp[5], fwd_total;                                  // forward scratch: the padded weights of conv1..4
    long wd, dxb, dyb, part, bwd_total;                     // backward scratch
    int dw_splits[5], dw_rows[5], nb_rows[5], nb_blocks[5];
};

// rows per workgroup of the column-sum kernels: at most 512 partial rows per layer
static void ew_rows_plan(long M, int* rows, int* blocks) {
    long r = 64;
    while ((M + r - 1) / r > 512) r *= 2;
    *rows = (int)r;
    *blocks = (int)((M + r - 1) / r);
}

// row splits of a weight gradient: 256 rows each, doubled until splits * tiles <= 1024 (the partials stay below 4 M floats) -- a
// function of the shape alone, so two runs sum in the same order
static void ew_dw_plan(long M, int Cp, int k, int* splits, int* rows) {
    const long tiles = (long)(Cp / 64) * (k * Cp / 64);
    long r = 256;
    while ((M + r - 1) / r > 1 && (M + r - 1) / r * tiles > 1024) r *= 2;
    *rows = (int)r;
    *splits = (int)((M + r - 1) / r);
}

static bool ew_layout(int B, int Lw, int C, EwLayout& e) {
    if (B < 1 || C < kEwMinC || C > kEwMaxC || Lw < 1) return false;
    // every row count below stays under 2^28 and every kernel forms its offsets in 64 bits: B = 256, L = 20480, C = 512 (2^29
    // floats per layer-0 tensor) is inside
    if ((long)B * ((long)Lw + 16) >= (1L << 30)) return false;
    int lin = Lw;
    for (int i = 0; i < 5; ++i) {
        if (lin + 2 * kEwGeom[i].p < kEwGeom[i].k) return false;
        e.L[i] = conv_out_len(lin, kEwGeom[i].k, kEwGeom[i].s, kEwGeom[i].p);
        if (e.L[i] <= 0) return false;
        lin = e.L[i];
    }
    const int Cp = e.Cp = (C + 63) & ~63;
    long o = 0;
    for (int i = 0; i < 4; ++i) { e.y[i] = o; o += ew_align((long)B * e.L[i] * Cp); }
    e.xhat[0] = -1;
    for (int i = 1; i < 5; ++i) { e.xhat[i] = o; o += ew_align((long)B * e.L[i] * Cp); }
    for (int i = 0; i < 5; ++i) { e.rstd[i] = o; o += ew_align((long)B * e.L[i]); }
    e.mean0 = o; o += ew_align((long)B * e.L[0]);
    e.saved_total = o;

    o = 0;
    e.wp[0] = -1;
    for (int i = 1; i < 5; ++i) { e.wp[i] = o; o += ew_align((long)Cp * kEwGeom[i].k * Cp); }
    e.fwd_total = o;

    o = 0;
    e.wd = o; o += ew_align((long)Cp * 8 * Cp);
    e.dxb = o; o += ew_align((long)B * e.L[1] * Cp);        // dx_i, the gradient of conv i's output (i = 1..4, one at a time)
    e.dyb = o; o += ew_align((long)B * e.L[0] * Cp);        // dy_{i-1}, the data gradient (dy3 .. dy0, one at a time)
    long part = 0;
    for (int i = 0; i < 5; ++i) {
        const long M = (long)B * e.L[i];
        ew_rows_plan(M, &e.nb_rows[i], &e.nb_blocks[i]);
        const long cols = (long)e.nb_blocks[i] * (i ? 3 : 13) * Cp;
        part = cols > part ? cols : part;
        e.dw_splits[i] = e.dw_rows[i] = 0;
        if (i) {
            ew_dw_plan(M, Cp, kEwGeom[i].k, &e.dw_splits[i], &e.dw_rows[i]);
            const long dw = (long)e.dw_splits[i] * Cp * kEwGeom[i].k * Cp;
            part = dw > part ? dw : part;
        }
    }
    e.part = o; o += ew_align(part);
    e.bwd_total = o;
    return true;
}

static bool ew_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int ew_forward(const float* wave, const float* const* P, float* saved, float* scratch, float* z, int B, int L, int C,
                      hipStream_t st) {
    EwLayout e;
    CPC_RETURN_IF(!ew_layout(B, L, C, e), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!wave || !P || !saved || !scratch || !z || !ew_aligned16(saved) || !ew_aligned16(scratch), CPC_ERR_ARG);
    for (int q = 0; q < 20; ++q) CPC_RETURN_IF(!P[q], CPC_ERR_ARG);
    const int Cp = e.Cp;
    const long M0 = (long)B * e.L[0];
    hipLaunchKernelGGL(ew_conv0_fwd_kernel, dim3(cdiv(M0, kEwNormRows)), dim3(256), 0, st, wave, P[0], P[1], P[2], P[3],
                       saved + e.y[0], saved + e.rstd[0], saved + e.mean0, L, e.L[0], M0, C, Cp);
    CPC_LAUNCH_CHECK();
    for (int i = 1; i < 5; ++i) {
        const EwGeom g = kEwGeom[i];
        const long M = (long)B * e.L[i];
        float* wp = scratch + e.wp[i];
        hipLaunchKernelGGL(ew_pad_w_kernel, dim3(cdiv((long)Cp * g.k * Cp, 256)), dim3(256), 0, st, P[4 * i], wp, C, Cp, g.k);
        float* xh = saved + e.xhat[i];
        hipLaunchKernelGGL(ew_gemm_kernel, dim3(cdiv(M, 128), Cp / 64, 1), dim3(256), 0, st, saved + e.y[i - 1], e.L[i - 1], g.k, g.s,
                           g.p, wp, 0L, P[4 * i + 1], xh, e.L[i], 1, 0, e.L[i], M, Cp, C);
        hipLaunchKernelGGL(ew_norm_fwd_kernel, dim3(cdiv(M, kEwNormRows)), dim3(256), 0, st, xh, P[4 * i + 2], P[4 * i + 3],
                           i < 4 ? saved + e.y[i] : z, i < 4 ? Cp : C, saved + e.rstd[i], M, C, Cp);
        CPC_LAUNCH_CHECK();
    }
    return 0;
}

static int ew_backward(const float* wave, const float* const* P, const float* saved, const float* z, const float* dz, float* scratch,
                       float* const* G, int B, int L, int C, hipStream_t st) {
    EwLayout e;
    CPC_RETURN_IF(!ew_layout(B, L, C, e), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!wave || !P || !saved || !z || !dz || !scratch || !G || !ew_aligned16(saved) || !ew_aligned16(scratch), CPC_ERR_ARG);
    for (int q = 0; q < 20; ++q) CPC_RETURN_IF(!P[q] || !G[q], CPC_ERR_ARG);
    const int Cp = e.Cp;
    float* wd = scratch + e.wd;
    float* dxb = scratch + e.dxb;
    float* dyb = scratch + e.dyb;
    float* part = scratch + e.part;
    for (int i = 4; i >= 1; --i) {
        const EwGeom g = kEwGeom[i];
        const long M = (long)B * e.L[i];
        // ReLU' and ChannelNorm' -> dx_i, and the three column sums
        hipLaunchKernelGGL(ew_norm_bwd_kernel, dim3(e.nb_blocks[i]), dim3(256), 0, st, i == 4 ? dz : dyb, i == 4 ? C : Cp,
                           i == 4 ? z : saved + e.y[i], i == 4 ? C : Cp, saved + e.xhat[i], saved + e.rstd[i], P[4 * i + 2], dxb, part, M,
                           C, Cp, e.nb_rows[i]);
        EwColDst dst = {};
        dst.p[0] = G[4 * i + 2]; dst.p[1] = G[4 * i + 3]; dst.p[2] = G[4 * i + 1];
        dst.stride[0] = dst.stride[1] = dst.stride[2] = 1;
        hipLaunchKernelGGL(ew_colsum_reduce_kernel, dim3(cdiv(3 * Cp, 256)), dim3(256), 0, st, part, e.nb_blocks[i], 3, Cp, C, dst);
        CPC_LAUNCH_CHECK();
        // the weight gradient
        const int K = g.k * Cp;
        hipLaunchKernelGGL(ew_wgrad_kernel, dim3(Cp / 64, K / 64, e.dw_splits[i]), dim3(256), 0, st, dxb, saved + e.y[i - 1], e.L[i - 1],
                           e.L[i], g.s, g.p, part, M, Cp, K, e.dw_rows[i]);
        hipLaunchKernelGGL(ew_dw_reduce_kernel, dim3(cdiv((long)C * C * g.k, 256)), dim3(256), 0, st, part, G[4 * i], C, Cp, g.k,
                           e.dw_splits[i]);
        CPC_LAUNCH_CHECK();
        // the data gradient dy_{i-1}: one phase of input rows per z, every row u < L_{i-1} written
        const int V = (e.L[i - 1] + g.p + g.s - 1) / g.s;
        hipLaunchKernelGGL(ew_pad_wd_kernel, dim3(cdiv((long)g.s * Cp * 2 * Cp, 256)), dim3(256), 0, st, P[4 * i], wd, C, Cp, g.s);
        hipLaunchKernelGGL(ew_gemm_kernel, dim3(cdiv((long)B * V, 128), Cp / 64, g.s), dim3(256), 0, st, dxb, e.L[i], 2, 1, 1, wd,
                           (long)Cp * 2 * Cp, (const float*)nullptr, dyb, e.L[i - 1], g.s, -g.p, V, (long)B * V, Cp, C);
        CPC_LAUNCH_CHECK();
    }
    const long M0 = (long)B * e.L[0];
    hipLaunchKernelGGL(ew_conv0_bwd_kernel, dim3(e.nb_blocks[0]), dim3(256), 0, st, wave, P[0], P[1], P[2], saved + e.y[0], dyb,
                       saved + e.rstd[0], saved + e.mean0, part, L, e.L[0], M0, C, Cp, e.nb_rows[0]);
    EwColDst dst = {};
    for (int j = 0; j < 10; ++j) { dst.p[j] = G[0] + j; dst.stride[j] = 10; }
    dst.p[10] = G[2]; dst.p[11] = G[3]; dst.p[12] = G[1];
    dst.stride[10] = dst.stride[11] = dst.stride[12] = 1;
    hipLaunchKernelGGL(ew_colsum_reduce_kernel, dim3(cdiv(13 * Cp, 256)), dim3(256), 0, st, part, e.nb_blocks[0], 13, Cp, C, dst);
    CPC_LAUNCH_CHECK();
    return 0;
}

}  // namespace cpc

using namespace cpc;

// C == 256 forwards to the 256-wide entry points: those kernels, layouts and bits stay what they are
extern "C" int cpc_encoder_layout_c(int B, int L, int C, long* sizes) {
    CPC_RETURN_IF(C < kEwMinC || C > kEwMaxC, CPC_ERR_SHAPE);
    if (C == kC) return cpc_encoder_layout(B, L, sizes);
    EwLayout e;
    CPC_RETURN_IF(!ew_layout(B, L, C, e), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = e.saved_total; sizes[1] = e.fwd_total; sizes[2] = e.bwd_total;
    for (int i = 0; i < 5; ++i) sizes[3 + i] = e.L[i];
    for (int i = 0; i < 4; ++i) sizes[8 + i] = e.y[i];
    for (int i = 1; i < 5; ++i) sizes[11 + i] = e.xhat[i];
    for (int i = 0; i < 5; ++i) sizes[16 + i] = e.rstd[i];
    sizes[21] = e.mean0;
    return 0;
}

extern "C" int cpc_encoder_forward_c(const float* wave, const float* const* params, float* saved, float* scratch, float* z, int B,
                                     int L, int C, void* stream) {
    CPC_RETURN_IF(C < kEwMinC || C > kEwMaxC, CPC_ERR_SHAPE);
    if (C == kC) return cpc_encoder_forward(wave, params, saved, scratch, z, B, L, stream);
    return ew_forward(wave, params, saved, scratch, z, B, L, C, (hipStream_t)stream);
}

extern "C" int cpc_encoder_backward_c(const float* wave, const float* const* params, const float* saved, const float* z,
                                      const float* dz, float* scratch, float* const* grads, int B, int L, int C, void* stream) {
    CPC_RETURN_IF(C < kEwMinC || C > kEwMaxC, CPC_ERR_SHAPE);
    if (C == kC) return cpc_encoder_backward(wave, params, saved, z, dz, scratch, grads, B, L, stream);
    return ew_backward(wave, params, saved, z, dz, scratch, grads, B, L, C, (hipStream_t)stream);
}

extern "C" int cpc_encoder_saved_activation_c(const float* saved, int layer, float* dst, int B, int L, int C, void* stream) {
    CPC_RETURN_IF(C < kEwMinC || C > kEwMaxC, CPC_ERR_SHAPE);
    if (C == kC) return cpc_encoder_saved_activation(saved, layer, dst, B, L, stream);
    EwLayout e;
    CPC_RETURN_IF(!ew_layout(B, L, C, e), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!saved || !dst || layer < 0 || layer > 3, CPC_ERR_ARG);
    const long rows = (long)B * e.L[layer];
    hipLaunchKernelGGL(ew_unpad_kernel, dim3(cdiv(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, saved + e.y[layer], dst, rows, C,
                       e.Cp);
    CPC_LAUNCH_CHECK();
    return 0;
}
