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
// The second half of the file runs the reference's other normModes -- batchNorm, instanceNorm, ID -- on the same storage and
// GEMMs at every C in 2..512, 256 included (cpc_encoder_*_n).
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
// u = v os + oo + z of sequence b of `out` (Lo rows per sequence) when 0 <= u < Lo.  grid = (ceil(M / 128), Cp / 64, phases).
// kSplitK (the forward convs of batchNorm / instanceNorm / ID): every 128 k the accumulators are folded into a second
// set, so a rounding error grows with sqrt(128) + sqrt(K / 128) steps instead of sqrt(K) -- a statistic over as few as four rows
// multiplies the conv's error by up to rstd.  Without it the kernel is what it was, to the bit.
template <bool kSplitK>
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
    f32x4 tot[kSplitK ? 2 : 1][kSplitK ? 4 : 1];
    if (kSplitK) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[kSplitK ? t : 0][kSplitK ? j : 0] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
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
        if (kSplitK && ((k0 & 96) == 96 || k0 + 32 >= K)) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4& o = tot[kSplitK ? t : 0][kSplitK ? j : 0];
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] += acc[t][j][r];      // (component by component: build.py's packed-fp32 gate)
                    acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
        }
        __syncthreads();
    }
    if (kSplitK) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] = tot[kSplitK ? t : 0][kSplitK ? j : 0];
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
        hipLaunchKernelGGL(ew_gemm_kernel<false>, dim3(cdiv(M, 128), Cp / 64, 1), dim3(256), 0, st, saved + e.y[i - 1], e.L[i - 1], g.k, g.s,
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
        hipLaunchKernelGGL(ew_gemm_kernel<false>, dim3(cdiv((long)B * V, 128), Cp / 64, g.s), dim3(256), 0, st, dxb, e.L[i], 2, 1, 1, wd,
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

// ------------------------------------------------------------------ normMode batchNorm / instanceNorm / ID
// The same padded storage, GEMM, weight gradient and gather-form data gradient; the normalisation is per (group, channel), a group
// being one utterance (instanceNorm: L_i rows) or the whole batch (batchNorm: B L_i rows).  A statistics pass writes centred
// partials (mean, M2) per workgroup -- a workgroup's rows lie inside one group -- which a reduce combines in index order with
// Chan's formula (never E[x^2] - E[x]^2); an apply pass writes xhat in place and y = relu(xhat w + b).  batchNorm in eval mode
// takes mean and rstd from the running buffers and reduces nothing; ID has no statistics, no xhat and one elementwise ReLU pass.
// conv0's output is never stored: the statistics, the apply pass and both backward passes form it again from the wave's ten taps.
enum { kEnLayerNorm = 0, kEnBatchNorm = 1, kEnInstanceNorm = 2, kEnId = 3 };
constexpr int kEnMaxBlocks = 1024;   // workgroups (= partial rows) of a column pass, at most, while a group has more than 64 rows

// conv0's weights transposed into LDS: wt[tap][channel], zeros beyond C
__device__ __forceinline__ void en_stage_w0(float* wt, const float* __restrict__ w0, int C, int Cp) {
    for (int idx = threadIdx.x; idx < 10 * Cp; idx += 256) {
        const int j = idx / Cp, c = idx - j * Cp;
        wt[j * kEwMaxC + c] = c < C ? w0[c * 10 + j] : 0.f;
    }
    __syncthreads();
}

// Row m of a layer's conv + bias, channel lane + 64 q in v[q] (zero beyond C): formed from the wave's ten taps (kConv0; x keeps the
// taps) or read from xin at pitch Cp
template <bool kConv0>
__device__ __forceinline__ void en_row(float (&v)[8], float (&x)[10], long m, const float* xin,
                                       const float* __restrict__ wave, const float* wt, const float (&cb)[8], int L, int L0, int lane,
                                       int nq, int C, int Cp) {
    if (kConv0) {
        const long b = m / L0;
        const int t = (int)(m - b * L0);
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const int pos = 5 * t - 3 + j;
            x[j] = (pos >= 0 && pos < L) ? wave[b * L + pos] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float a = 0.f;
            if (q < nq) {
#pragma unroll
                for (int j = 0; j < 10; ++j) a = fmaf(wt[j * kEwMaxC + lane + 64 * q], x[j], a);
            }
            // the bias last: one rounding at its magnitude, not ten -- a statistic's rstd (25 at layer 0) multiplies each of them
            v[q] = a + cb[q];                               // zero beyond C: zero weights and bias
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (q < nq && lane + 64 * q < C) ? xin[m * Cp + lane + 64 * q] : 0.f;
    }
}

// the four waves' column sums -> part[slot][Cp], waves added in index order
__device__ __forceinline__ void en_store_colsums(float* red, const float (&s)[8], long slot, float* __restrict__ part, int Cp) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) red[w * kEwMaxC + lane + 64 * q] = s[q];
    __syncthreads();
#pragma clang loop vectorize(disable) interleave(disable)
    for (int c = threadIdx.x; c < Cp; c += 256)
        part[slot * Cp + c] = ((red[c] + red[kEwMaxC + c]) + red[2 * kEwMaxC + c]) + red[3 * kEwMaxC + c];
}

// Statistics pass.  grid = (chunks, groups); the workgroup owns rows [blockIdx.x rows, + rows) of group blockIdx.y (Lg rows per
// group).  Each wave runs Welford's update over its rows (every fourth), one channel per (lane, q); the four waves' (n, mean, M2) are
// combined in index order with Chan's formula -> part[(group chunks + chunk) 2 + {0: mean, 1: M2}][Cp].  The count is the chunk's
// row count, which the reduce knows from the shape.
template <bool kConv0>
__global__ __launch_bounds__(256) void en_stats_kernel(const float* __restrict__ xin, const float* __restrict__ wave,
                                                       const float* __restrict__ w0, const float* __restrict__ b0,
                                                       float* __restrict__ part, int L, int L0, int Lg, int rows, int C, int Cp) {
    __shared__ float wt[10 * kEwMaxC];
    float* red = wt;                                        // [wave][mean, M2][channel], once the rows are done
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    float cb[8], mu[8], m2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        cb[q] = (kConv0 && lane + 64 * q < C) ? b0[lane + 64 * q] : 0.f;
        mu[q] = m2[q] = 0.f;
    }
    if (kConv0) en_stage_w0(wt, w0, C, Cp);
    const int rb = blockIdx.x * rows;
    const int re = rb + rows < Lg ? rb + rows : Lg;
    const long base = (long)blockIdx.y * Lg;
    int cnt = 0;
    for (int r = rb + w; r < re; r += 4) {
        float v[8], x[10];
        en_row<kConv0>(v, x, base + r, xin, wave, wt, cb, L, L0, lane, nq, C, Cp);
        const float inv = 1.0f / (float)(++cnt);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float d = v[q] - mu[q];
            mu[q] += d * inv;
            m2[q] += d * (v[q] - mu[q]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        red[(2 * w) * kEwMaxC + lane + 64 * q] = mu[q];
        red[(2 * w + 1) * kEwMaxC + lane + 64 * q] = m2[q];
    }
    __syncthreads();
    const int n = re - rb;                                  // >= 1; wave w saw (n - w + 3) / 4 rows
    const long slot = ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
#pragma clang loop vectorize(disable) interleave(disable)
    for (int c = threadIdx.x; c < Cp; c += 256) {
        float na = (float)((n + 3) / 4), mean = red[c], M2 = red[kEwMaxC + c];
        for (int ww = 1; ww < 4; ++ww) {
            const int nw_ = (n - ww + 3) / 4;
            if (nw_ <= 0) break;
            const float nb = (float)nw_, nn = na + nb;
            const float d = red[(2 * ww) * kEwMaxC + c] - mean;
            mean += d * (nb / nn);
            M2 += red[(2 * ww + 1) * kEwMaxC + c] + d * d * (na * nb / nn);
            na = nn;
        }
        part[slot * Cp + c] = mean;
        part[(slot + 1) * Cp + c] = M2;
    }
}

// mean[g][c], rstd[g][c] (all Cp columns) from the chunks' partials, combined in index order with Chan's formula.  With run_mean
// (batchNorm in training; one group) the running buffers are updated in place: the unbiased variance M2 / (n - 1) for running_var.
__global__ __launch_bounds__(256) void en_stats_reduce_kernel(const float* __restrict__ part, float* __restrict__ mean_out,
                                                              float* __restrict__ rstd_out, float* __restrict__ run_mean,
                                                              float* __restrict__ run_var, float momentum, float eps, int groups,
                                                              int chunks, int rows, int Lg, int C, int Cp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= groups * Cp) return;
    const int g = idx / Cp, c = idx - g * Cp;
    const float* p = part + (long)g * chunks * 2 * Cp + c;
    float na = (float)(rows < Lg ? rows : Lg), mean = p[0], M2 = p[Cp];
    for (int k = 1; k < chunks; ++k) {
        const int left = Lg - k * rows;
        const float nb = (float)(left < rows ? left : rows), nn = na + nb;
        const float d = p[(long)k * 2 * Cp] - mean;
        mean += d * (nb / nn);
        M2 += p[(long)k * 2 * Cp + Cp] + d * d * (na * nb / nn);
        na = nn;
    }
    mean_out[idx] = mean;
    rstd_out[idx] = 1.0f / sqrtf(M2 / (float)Lg + eps);
    if (run_mean && c < C) {
        run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * mean;
        run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (M2 / (float)(Lg - 1));
    }
}

// batchNorm in eval mode: the statistics are the running buffers
__global__ __launch_bounds__(256) void en_eval_stats_kernel(const float* __restrict__ run_mean, const float* __restrict__ run_var,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out, float eps,
                                                            int C, int Cp) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cp) return;
    mean_out[c] = c < C ? run_mean[c] : 0.f;
    rstd_out[c] = c < C ? 1.0f / sqrtf(run_var[c] + eps) : 0.f;
}

// Apply pass: xhat = (x - mean[g]) rstd[g] written in place over x (layers 1..4; conv0 stores none), y = relu(xhat w + b) at pitch
// ldy (Cp: zero pad columns; C: z).  mean == NULL is normMode ID: y = relu(x), x is left as it is.  One wave per row, the row's
// group is m / Lg.
template <bool kConv0>
__global__ __launch_bounds__(256) void en_apply_kernel(float* __restrict__ xh, const float* __restrict__ wave,
                                                       const float* __restrict__ w0, const float* __restrict__ b0,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ nw, const float* __restrict__ nb,
                                                       float* __restrict__ y, int ldy, int L, int L0, int Lg, long M, int C, int Cp) {
    __shared__ float wt[kConv0 ? 10 * kEwMaxC : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    float gw[8], gb[8], cb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q;
        gw[q] = (mean && c < C) ? nw[c] : 1.f;
        gb[q] = (mean && c < C) ? nb[c] : 0.f;
        cb[q] = (kConv0 && c < C) ? b0[c] : 0.f;
    }
    if (kConv0) en_stage_w0(wt, w0, C, Cp);
    for (int rr = 0; rr < kEwNormRows / 4; ++rr) {
        const long m = (long)blockIdx.x * kEwNormRows + 4 * rr + w;
        if (m >= M) break;                                  // wave-uniform
        float v[8], x[10];
        en_row<kConv0>(v, x, m, xh, wave, wt, cb, L, L0, lane, nq, C, Cp);
        const long go = (m / Lg) * Cp;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            if (q < nq) {
                const bool live = c < C;
                float h = v[q];
                if (mean) {
                    h = live ? (v[q] - mean[go + c]) * rstd[go + c] : 0.f;
                    if (!kConv0) xh[m * Cp + c] = h;
                }
                if (c < ldy) y[m * ldy + c] = live ? fmaxf(relu_in(h * gw[q] + gb[q]), 0.f) : 0.f;
            }
        }
    }
}

// Backward, first pass: with g = dy [y > 0], the chunk's sums of g and of g xhat -> part[(group chunks + chunk) 2 + {0, 1}][Cp].
// Summed over a group they are the two means the normalisation's gradient subtracts; summed over everything, the norm bias and
// norm weight gradients.  grid = (chunks, groups), as the statistics pass.
template <bool kConv0>
__global__ __launch_bounds__(256) void en_bwd_sums_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                          const float* __restrict__ xh, const float* __restrict__ wave,
                                                          const float* __restrict__ w0, const float* __restrict__ b0,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ part, int L, int L0, int Lg, int rows, int C, int Cp) {
    __shared__ float wt[kConv0 ? 10 * kEwMaxC : 4 * kEwMaxC];
    float* red = wt;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    const long go = (long)blockIdx.y * Cp;
    float cb[8], mu[8], rs[8], s1[8], s2[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q;
        cb[q] = (kConv0 && c < C) ? b0[c] : 0.f;
        mu[q] = (kConv0 && c < C) ? mean[go + c] : 0.f;
        rs[q] = (kConv0 && c < C) ? rstd[go + c] : 0.f;
        s1[q] = s2[q] = 0.f;
    }
    if (kConv0) en_stage_w0(wt, w0, C, Cp);
    const int rb = blockIdx.x * rows;
    const int re = rb + rows < Lg ? rb + rows : Lg;
    const long base = (long)blockIdx.y * Lg;
    for (int r = rb + w; r < re; r += 4) {
        const long m = base + r;
        float h[8], x[10];
        en_row<kConv0>(h, x, m, xh, wave, wt, cb, L, L0, lane, nq, C, Cp);       // layers 1..4: xh holds xhat
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            const bool live = q < nq && c < C;
            const float g = (live && y[m * ldy + c] > 0.f) ? dy[m * lddy + c] : 0.f;
            const float hh = kConv0 ? (h[q] - mu[q]) * rs[q] : h[q];
            s1[q] += g;
            s2[q] += g * hh;
        }
    }
    const long slot = ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    en_store_colsums(red, s1, slot, part, Cp);
    en_store_colsums(red, s2, slot + 1, part, Cp);
}

// sums[g][which][c] = the group's chunks in index order; the groups in index order are the norm bias (which 0) and norm weight
// (which 1) gradients
__global__ __launch_bounds__(256) void en_bwd_sums_reduce_kernel(const float* __restrict__ part, float* __restrict__ sums,
                                                                 float* __restrict__ g_nb, float* __restrict__ g_nw, int groups,
                                                                 int chunks, int C, int Cp) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * Cp) return;
    const int which = idx / Cp, c = idx - which * Cp;
    float total = 0.f;
    for (int g = 0; g < groups; ++g) {
        const float* p = part + ((long)g * chunks * 2 + which) * Cp + c;
        float v = p[0];
        for (int k = 1; k < chunks; ++k) v += p[(long)k * 2 * Cp];
        sums[((long)g * 2 + which) * Cp + c] = v;
        total = g ? total + v : v;
    }
    if (c < C) (which ? g_nw : g_nb)[c] = total;
}

// Backward, second pass: dx = a (g - s1 / n - xhat s2 / n), a = w rstd.  `subtract` == 0 (batchNorm in eval mode: an affine map)
// drops the two means; mean == NULL (ID) is dx = g.  Layers 1..4 write dx at pitch Cp (zero pad columns) and the chunk's column sum
// of dx -> part[block][Cp] (the conv bias gradient); conv0 writes no dx but part[block][0..9] = the ten taps of its weight
// gradient and [10] = the conv bias.  grid = (chunks, groups).
template <bool kConv0>
__global__ __launch_bounds__(256) void en_bwd_dx_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                        const float* __restrict__ xh, const float* __restrict__ wave,
                                                        const float* __restrict__ w0, const float* __restrict__ b0,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ nw, const float* __restrict__ sums,
                                                        float* __restrict__ dx, float* __restrict__ part, int L, int L0, int Lg,
                                                        int rows, int C, int Cp, int subtract) {
    __shared__ float wt[kConv0 ? 10 * kEwMaxC : 4 * kEwMaxC];
    float* red = wt;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = Cp >> 6;
    const long go = (long)blockIdx.y * Cp;
    const float invn = 1.0f / (float)Lg;
    float cb[8], mu[8], rs[8], a[8], s1n[8], s2n[8], s_cb[8], s_w[kConv0 ? 10 : 1][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = lane + 64 * q;
        const bool live = c < C;
        cb[q] = (kConv0 && live) ? b0[c] : 0.f;
        mu[q] = (mean && live) ? mean[go + c] : 0.f;
        rs[q] = (mean && live) ? rstd[go + c] : 0.f;
        a[q] = live ? (mean ? nw[c] * rs[q] : 1.f) : 0.f;
        s1n[q] = (subtract && live) ? sums[2 * go + c] * invn : 0.f;
        s2n[q] = (subtract && live) ? sums[2 * go + Cp + c] * invn : 0.f;
        s_cb[q] = 0.f;
#pragma unroll
        for (int j = 0; j < (kConv0 ? 10 : 1); ++j) s_w[j][q] = 0.f;
    }
    if (kConv0) en_stage_w0(wt, w0, C, Cp);
    const int rb = blockIdx.x * rows;
    const int re = rb + rows < Lg ? rb + rows : Lg;
    const long base = (long)blockIdx.y * Lg;
    for (int r = rb + w; r < re; r += 4) {
        const long m = base + r;
        float h[8], x[10];
        if (kConv0 || (mean && xh)) en_row<kConv0>(h, x, m, xh, wave, wt, cb, L, L0, lane, nq, C, Cp);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = lane + 64 * q;
            const bool live = q < nq && c < C;
            const float g = (live && y[m * ldy + c] > 0.f) ? dy[m * lddy + c] : 0.f;
            const float hh = !mean ? 0.f : (kConv0 ? (h[q] - mu[q]) * rs[q] : h[q]);
            const float d = live ? a[q] * (g - s1n[q] - hh * s2n[q]) : 0.f;
            s_cb[q] += d;
            if (kConv0) {
#pragma unroll
                for (int j = 0; j < 10; ++j) s_w[j][q] = fmaf(d, x[j], s_w[j][q]);
            } else if (q < nq) {
                dx[m * Cp + c] = d;
            }
        }
    }
    const long blk = (long)blockIdx.y * gridDim.x + blockIdx.x;
    if (kConv0) {
#pragma unroll
        for (int j = 0; j < 10; ++j) en_store_colsums(red, s_w[j], blk * 11 + j, part, Cp);
        en_store_colsums(red, s_cb, blk * 11 + 10, part, Cp);
    } else {
        en_store_colsums(red, s_cb, blk, part, Cp);
    }
}

// ------------------------------------------------------------------ host side of the other normModes
struct EnLayout {
    EwLayout e;                                             // lengths, Cp, the weight gradients' row splits
    int groups;                                             // statistic groups: B under instanceNorm, 1 otherwise
    int Lg[5], rows[5], chunks[5];                          // rows per group, rows per workgroup, workgroups per group
    long y[4], xhat[5], mean[5], rstd[5], saved_total;      // offsets (floats) into `saved`; ID keeps y0..y3 only
    long wp[5], fpart, xtmp, fwd_total;                     // forward scratch
    long wd, dxb, dyb, part, sums, bwd_total;               // backward scratch
};

static int en_layout(int B, int Lw, int C, int norm, int training, EnLayout& n) {
    CPC_RETURN_IF(!ew_layout(B, Lw, C, n.e), CPC_ERR_SHAPE);
    const EwLayout& e = n.e;
    // the biased variance of one value is zero and torch refuses it: one utterance's last layer, the whole batch's in training
    CPC_RETURN_IF(norm == kEnInstanceNorm && e.L[4] < 2, CPC_ERR_SHAPE);
    CPC_RETURN_IF(norm == kEnBatchNorm && training && (long)B * e.L[4] < 2, CPC_ERR_SHAPE);
    CPC_RETURN_IF(norm == kEnInstanceNorm && B > 65535, CPC_ERR_SHAPE);      // the groups are the grid's y
    const int Cp = e.Cp;
    const bool id = norm == kEnId;
    n.groups = norm == kEnInstanceNorm ? B : 1;
    long fpart = 0, part = 0;
    for (int i = 0; i < 5; ++i) {
        const long lg = norm == kEnInstanceNorm ? e.L[i] : (long)B * e.L[i];
        long r = 64;
        while (r < lg && n.groups * ((lg + r - 1) / r) > kEnMaxBlocks) r *= 2;
        n.Lg[i] = (int)lg; n.rows[i] = (int)r; n.chunks[i] = (int)((lg + r - 1) / r);
        const long blocks = (long)n.groups * n.chunks[i];
        fpart = blocks * 2 * Cp > fpart ? blocks * 2 * Cp : fpart;
        const long cols = blocks * (i ? 2 : 11) * Cp;
        part = cols > part ? cols : part;
        if (i) {
            const long dw = (long)e.dw_splits[i] * Cp * kEwGeom[i].k * Cp;
            part = dw > part ? dw : part;
        }
    }
    long o = 0;
    for (int i = 0; i < 4; ++i) { n.y[i] = o; o += ew_align((long)B * e.L[i] * Cp); }
    n.xhat[0] = -1;
    for (int i = 1; i < 5; ++i) { n.xhat[i] = id ? -1 : o; if (!id) o += ew_align((long)B * e.L[i] * Cp); }
    for (int i = 0; i < 5; ++i) { n.mean[i] = id ? -1 : o; if (!id) o += ew_align((long)n.groups * Cp); }
    for (int i = 0; i < 5; ++i) { n.rstd[i] = id ? -1 : o; if (!id) o += ew_align((long)n.groups * Cp); }
    n.saved_total = o;

    o = 0;
    n.wp[0] = -1;
    for (int i = 1; i < 5; ++i) { n.wp[i] = o; o += ew_align((long)Cp * kEwGeom[i].k * Cp); }
    n.fpart = o; o += id ? 0 : ew_align(fpart);
    n.xtmp = o; o += id ? ew_align((long)B * e.L[1] * Cp) : 0;      // ID: conv + bias of one layer, before its ReLU pass
    n.fwd_total = o;

    o = 0;
    n.wd = o; o += ew_align((long)Cp * 8 * Cp);
    n.dxb = o; o += ew_align((long)B * e.L[1] * Cp);
    n.dyb = o; o += ew_align((long)B * e.L[0] * Cp);
    n.part = o; o += ew_align(part);
    n.sums = o; o += ew_align((long)n.groups * 2 * Cp);
    n.bwd_total = o;
    return 0;
}

static int en_check_params(const float* const* P, int norm) {
    CPC_RETURN_IF(!P, CPC_ERR_ARG);
    for (int q = 0; q < 20; ++q) CPC_RETURN_IF(!P[q] && !(norm == kEnId && (q & 2)), CPC_ERR_ARG);
    return 0;
}

static int en_forward(const float* wave, const float* const* P, float* const* R, float* saved, float* scratch, float* z, int B, int L,
                      int C, int norm, int training, float momentum, float eps, hipStream_t st) {
    EnLayout n;
    if (int rc = en_layout(B, L, C, norm, training, n)) return rc;
    CPC_RETURN_IF(!wave || !saved || !scratch || !z || !ew_aligned16(saved) || !ew_aligned16(scratch), CPC_ERR_ARG);
    if (int rc = en_check_params(P, norm)) return rc;
    const bool bn = norm == kEnBatchNorm, id = norm == kEnId;
    if (bn) {
        CPC_RETURN_IF(!R, CPC_ERR_ARG);
        for (int q = 0; q < 10; ++q) CPC_RETURN_IF(!R[q], CPC_ERR_ARG);
    }
    const EwLayout& e = n.e;
    const int Cp = e.Cp;
    const bool reduce = !id && !(bn && !training);          // batch statistics of this call
    for (int i = 0; i < 5; ++i) {
        const EwGeom g = kEwGeom[i];
        const long M = (long)B * e.L[i];
        float* xh = nullptr;
        if (i) {
            float* wp = scratch + n.wp[i];
            xh = id ? scratch + n.xtmp : saved + n.xhat[i];
            hipLaunchKernelGGL(ew_pad_w_kernel, dim3(cdiv((long)Cp * g.k * Cp, 256)), dim3(256), 0, st, P[4 * i], wp, C, Cp, g.k);
            hipLaunchKernelGGL(ew_gemm_kernel<true>, dim3(cdiv(M, 128), Cp / 64, 1), dim3(256), 0, st, saved + n.y[i - 1], e.L[i - 1], g.k, g.s,
                               g.p, wp, 0L, P[4 * i + 1], xh, e.L[i], 1, 0, e.L[i], M, Cp, C);
            CPC_LAUNCH_CHECK();
        }
        float* mean = id ? nullptr : saved + n.mean[i];
        float* rstd = id ? nullptr : saved + n.rstd[i];
        if (reduce) {
            float* part = scratch + n.fpart;
            const dim3 grid(n.chunks[i], n.groups);
            if (i) hipLaunchKernelGGL(en_stats_kernel<false>, grid, dim3(256), 0, st, xh, wave, P[0], P[1], part, L, e.L[0], n.Lg[i],
                                      n.rows[i], C, Cp);
            else hipLaunchKernelGGL(en_stats_kernel<true>, grid, dim3(256), 0, st, xh, wave, P[0], P[1], part, L, e.L[0], n.Lg[i],
                                    n.rows[i], C, Cp);
            hipLaunchKernelGGL(en_stats_reduce_kernel, dim3(cdiv((long)n.groups * Cp, 256)), dim3(256), 0, st, part, mean, rstd,
                               bn ? R[2 * i] : (float*)nullptr, bn ? R[2 * i + 1] : (float*)nullptr, momentum, eps, n.groups,
                               n.chunks[i], n.rows[i], n.Lg[i], C, Cp);
        } else if (bn) {
            hipLaunchKernelGGL(en_eval_stats_kernel, dim3(cdiv(Cp, 256)), dim3(256), 0, st, R[2 * i], R[2 * i + 1], mean, rstd, eps, C,
                               Cp);
        }
        float* y = i < 4 ? saved + n.y[i] : z;
        const int ldy = i < 4 ? Cp : C;
        const float* nw = id ? nullptr : P[4 * i + 2];
        const float* nb = id ? nullptr : P[4 * i + 3];
        if (i) hipLaunchKernelGGL(en_apply_kernel<false>, dim3(cdiv(M, kEwNormRows)), dim3(256), 0, st, xh, wave, P[0], P[1], mean, rstd,
                                  nw, nb, y, ldy, L, e.L[0], n.Lg[i], M, C, Cp);
        else hipLaunchKernelGGL(en_apply_kernel<true>, dim3(cdiv(M, kEwNormRows)), dim3(256), 0, st, xh, wave, P[0], P[1], mean, rstd,
                                nw, nb, y, ldy, L, e.L[0], n.Lg[i], M, C, Cp);
        CPC_LAUNCH_CHECK();
    }
    return 0;
}

static int en_backward(const float* wave, const float* const* P, const float* saved, const float* z, const float* dz, float* scratch,
                       float* const* G, int B, int L, int C, int norm, int training, hipStream_t st) {
    EnLayout n;
    if (int rc = en_layout(B, L, C, norm, training, n)) return rc;
    CPC_RETURN_IF(!wave || !saved || !z || !dz || !scratch || !ew_aligned16(saved) || !ew_aligned16(scratch), CPC_ERR_ARG);
    if (int rc = en_check_params(P, norm)) return rc;
    if (int rc = en_check_params(G, norm)) return rc;
    const bool id = norm == kEnId;
    const int subtract = !id && !(norm == kEnBatchNorm && !training);
    const EwLayout& e = n.e;
    const int Cp = e.Cp;
    float* wd = scratch + n.wd;
    float* dxb = scratch + n.dxb;
    float* dyb = scratch + n.dyb;
    float* part = scratch + n.part;
    float* sums = scratch + n.sums;
    for (int i = 4; i >= 0; --i) {
        const EwGeom g = kEwGeom[i];
        const long M = (long)B * e.L[i];
        const float* dy = i == 4 ? dz : dyb;
        const float* y = i == 4 ? z : saved + n.y[i];
        const int ld = i == 4 ? C : Cp;
        const float* xh = (id || !i) ? nullptr : saved + n.xhat[i];
        const float* mean = id ? nullptr : saved + n.mean[i];
        const float* rstd = id ? nullptr : saved + n.rstd[i];
        const dim3 grid(n.chunks[i], n.groups);
        const int blocks = n.chunks[i] * n.groups;
        if (!id) {
            if (i) hipLaunchKernelGGL(en_bwd_sums_kernel<false>, grid, dim3(256), 0, st, dy, ld, y, ld, xh, wave, P[0], P[1], mean, rstd,
                                      part, L, e.L[0], n.Lg[i], n.rows[i], C, Cp);
            else hipLaunchKernelGGL(en_bwd_sums_kernel<true>, grid, dim3(256), 0, st, dy, ld, y, ld, xh, wave, P[0], P[1], mean, rstd,
                                    part, L, e.L[0], n.Lg[i], n.rows[i], C, Cp);
            hipLaunchKernelGGL(en_bwd_sums_reduce_kernel, dim3(cdiv(2 * Cp, 256)), dim3(256), 0, st, part, sums, G[4 * i + 3],
                               G[4 * i + 2], n.groups, n.chunks[i], C, Cp);
            CPC_LAUNCH_CHECK();
        }
        const float* nw = id ? nullptr : P[4 * i + 2];
        EwColDst dst = {};
        if (!i) {
            hipLaunchKernelGGL(en_bwd_dx_kernel<true>, grid, dim3(256), 0, st, dy, ld, y, ld, xh, wave, P[0], P[1], mean, rstd, nw, sums,
                               dxb, part, L, e.L[0], n.Lg[i], n.rows[i], C, Cp, subtract);
            for (int j = 0; j < 10; ++j) { dst.p[j] = G[0] + j; dst.stride[j] = 10; }
            dst.p[10] = G[1]; dst.stride[10] = 1;
            hipLaunchKernelGGL(ew_colsum_reduce_kernel, dim3(cdiv(11 * Cp, 256)), dim3(256), 0, st, part, blocks, 11, Cp, C, dst);
            CPC_LAUNCH_CHECK();
            break;
        }
        hipLaunchKernelGGL(en_bwd_dx_kernel<false>, grid, dim3(256), 0, st, dy, ld, y, ld, xh, wave, P[0], P[1], mean, rstd, nw, sums,
                           dxb, part, L, e.L[0], n.Lg[i], n.rows[i], C, Cp, subtract);
        dst.p[0] = G[4 * i + 1]; dst.stride[0] = 1;
        hipLaunchKernelGGL(ew_colsum_reduce_kernel, dim3(cdiv(Cp, 256)), dim3(256), 0, st, part, blocks, 1, Cp, C, dst);
        CPC_LAUNCH_CHECK();
        // the weight gradient and the data gradient dy_{i-1}, as under layerNorm
        const int K = g.k * Cp;
        hipLaunchKernelGGL(ew_wgrad_kernel, dim3(Cp / 64, K / 64, e.dw_splits[i]), dim3(256), 0, st, dxb, saved + n.y[i - 1], e.L[i - 1],
                           e.L[i], g.s, g.p, part, M, Cp, K, e.dw_rows[i]);
        hipLaunchKernelGGL(ew_dw_reduce_kernel, dim3(cdiv((long)C * C * g.k, 256)), dim3(256), 0, st, part, G[4 * i], C, Cp, g.k,
                           e.dw_splits[i]);
        CPC_LAUNCH_CHECK();
        const int V = (e.L[i - 1] + g.p + g.s - 1) / g.s;
        hipLaunchKernelGGL(ew_pad_wd_kernel, dim3(cdiv((long)g.s * Cp * 2 * Cp, 256)), dim3(256), 0, st, P[4 * i], wd, C, Cp, g.s);
        hipLaunchKernelGGL(ew_gemm_kernel<false>, dim3(cdiv((long)B * V, 128), Cp / 64, g.s), dim3(256), 0, st, dxb, e.L[i], 2, 1, 1, wd,
                           (long)Cp * 2 * Cp, (const float*)nullptr, dyb, e.L[i - 1], g.s, -g.p, V, (long)B * V, Cp, C);
        CPC_LAUNCH_CHECK();
    }
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

// The encoder under any normMode: 0 layerNorm (the _c entries above: their kernels, launches and bits), 1 batchNorm,
// 2 instanceNorm, 3 ID.  2 <= C <= 512 with 256 included: the 256-only kernels fuse ChannelNorm, so the other modes run 256 on the
// padded path.  sizes has 32 slots: the first 22 as cpc_encoder_layout_c under layerNorm; otherwise 0..2 the totals, 3..7 L_i,
// 8..11 y0..y3, 12..15 xhat1..4, 16..20 mean_i, 21..25 rstd_i (-1: not kept), 26 the row pitch, 27 the statistic groups.
extern "C" int cpc_encoder_layout_n(int B, int L, int C, int norm, int training, long* sizes) {
    CPC_RETURN_IF(norm < kEnLayerNorm || norm > kEnId, CPC_ERR_ARG);
    if (norm == kEnLayerNorm) {
        const int rc = cpc_encoder_layout_c(B, L, C, sizes);
        if (rc == 0)
            for (int i = 22; i < 32; ++i) sizes[i] = 0;
        return rc;
    }
    EnLayout n;
    if (int rc = en_layout(B, L, C, norm, training, n)) return rc;
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    for (int i = 0; i < 32; ++i) sizes[i] = 0;
    sizes[0] = n.saved_total; sizes[1] = n.fwd_total; sizes[2] = n.bwd_total;
    for (int i = 0; i < 5; ++i) sizes[3 + i] = n.e.L[i];
    for (int i = 0; i < 4; ++i) sizes[8 + i] = n.y[i];
    for (int i = 1; i < 5; ++i) sizes[11 + i] = n.xhat[i];
    for (int i = 0; i < 5; ++i) { sizes[16 + i] = n.mean[i]; sizes[21 + i] = n.rstd[i]; }
    sizes[26] = n.e.Cp; sizes[27] = n.groups;
    return 0;
}

extern "C" int cpc_encoder_forward_n(const float* wave, const float* const* params, float* const* running, float* saved,
                                     float* scratch, float* z, int B, int L, int C, int norm, int training, float momentum, float eps,
                                     void* stream) {
    CPC_RETURN_IF(norm < kEnLayerNorm || norm > kEnId, CPC_ERR_ARG);
    if (norm == kEnLayerNorm) return cpc_encoder_forward_c(wave, params, saved, scratch, z, B, L, C, stream);
    return en_forward(wave, params, running, saved, scratch, z, B, L, C, norm, training, momentum, eps, (hipStream_t)stream);
}

extern "C" int cpc_encoder_backward_n(const float* wave, const float* const* params, const float* saved, const float* z,
                                      const float* dz, float* scratch, float* const* grads, int B, int L, int C, int norm,
                                      int training, void* stream) {
    CPC_RETURN_IF(norm < kEnLayerNorm || norm > kEnId, CPC_ERR_ARG);
    if (norm == kEnLayerNorm) return cpc_encoder_backward_c(wave, params, saved, z, dz, scratch, grads, B, L, C, stream);
    return en_backward(wave, params, saved, z, dz, scratch, grads, B, L, C, norm, training, (hipStream_t)stream);
}

extern "C" int cpc_encoder_saved_activation_n(const float* saved, int layer, float* dst, int B, int L, int C, int norm,
                                              void* stream) {
    CPC_RETURN_IF(norm < kEnLayerNorm || norm > kEnId, CPC_ERR_ARG);
    if (norm == kEnLayerNorm) return cpc_encoder_saved_activation_c(saved, layer, dst, B, L, C, stream);
    EnLayout n;
    if (int rc = en_layout(B, L, C, norm, 0, n)) return rc;
    CPC_RETURN_IF(!saved || !dst || layer < 0 || layer > 3, CPC_ERR_ARG);
    const long rows = (long)B * n.e.L[layer];
    hipLaunchKernelGGL(ew_unpad_kernel, dim3(cdiv(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, saved + n.y[layer], dst, rows, C,
                       n.e.Cp);
    CPC_LAUNCH_CHECK();
    return 0;
}
