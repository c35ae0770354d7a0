// The PER phone classifier of the reference (cpc/eval/common_voices_eval.py, CTCphone_criterion): the windowed head
// nn.Conv1d(256, C, 8, stride 4) on channels-last features, and log_softmax + nn.CTCLoss(blank, reduction, zero_infinity = True)
// with per-utterance input lengths and padded targets -- what `common_voices_eval train` trains.
//
// Head (cpc_phone_head_forward / _backward), x (B, S, 256), W (C, 256, 8) in torch's layout, T = (S - 8) / 4 + 1 windows:
//   wr[o][j 256 + c] = W[o][c][j]                  ph_relayout_kernel: the weight in the order of a window's 2048 floats
//   logits = windows wr^T + b                      frames 4t .. 4t+7 are 2048 contiguous floats, so window (b, t) is the row
//                                                  x + (b S + 4t) 256 of a K = 2048 product: ph_tile_kernel<kPhFwd>, 64 x 64
//                                                  tiles, exact-f32 FMA, eight K slabs of 256 (one per tap) for parallelism,
//                                                  added in slab order with the bias by ph_logits_kernel
//   dW = dlogits^T windows, db = sum dlogits       ph_tile_kernel<kPhDw> per row slab, ph_colsum_kernel; ph_wsum_kernel adds the
//                                                  slabs in slab order and writes torch's (C, 256, 8) layout
//   dX[b, s] = sum over the <= 2 windows of s      ph_tile_kernel<kPhDx>, gather form: frames of one phase s & 3 share their
//                                                  weight taps (s & 3 for window s / 4, (s & 3) + 4 for window s / 4 - 1), so each
//                                                  phase is one product over K = 2 C; frames no window covers get exactly 0
// CTC (cpc_ctc_seq_forward / _backward): per-row log-sum-exp (ph_lse_kernel), then one workgroup per sequence runs the
// log-space alpha recursion over its in_len[b] frames and 2 tgt_len[b] + 1 states in float64 (ph_alpha_kernel), and the beta
// recursion with the per-class occupancy sums (ph_beta_kernel).  Lengths and targets are read on the device as int64.
// No float atomics, fixed summation orders: identical calls give identical bits, and a sequence's results do not depend on
// the batch around it.
#include <climits>

#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kPhTaps = 8, kPhStride = 4;
constexpr int kPhWin = kPhTaps * kC;                 // floats of one window
constexpr int kPhMaxT = 2048, kPhMaxL = 512, kPhMaxC = 256;
constexpr int kPhMaxStates = 2 * kPhMaxL + 1;
constexpr int kPhPer = (kPhMaxStates + 255) / 256;   // CTC states per thread
constexpr int kPhFwdSlabs = kPhTaps;                 // K slabs of the forward product
constexpr int kPhSlabRows = 256;                     // windows per dW / db partial slab
constexpr int kPhMaxSlabs = 32;
constexpr int kHT = 64, kHK = 16;                    // product tile (rows = columns) and k-step
constexpr int kPhNone = 0, kPhMean = 1, kPhSum = 2;  // reductions

// bit 0: a target outside [0, C) or equal to the blank (CPC_DEVERR_LABEL_RANGE); bit 1: a length outside its range
// (CPC_DEVERR_LENGTH_RANGE).  Read and cleared by cpc_device_error_flags() (capi.hip).
static __device__ unsigned g_ph_error = 0;

__device__ __forceinline__ float ph_nan() { return __builtin_nanf(""); }

// log(exp(a) + exp(b) + exp(c)) in float64 (see supervised.hip on why the recursions are not float)
__device__ __forceinline__ double ph_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + log((exp(a - m) + exp(b - m)) + exp(c - m));
}

// window r = b T + t starts at frame b S + 4 t
__device__ __forceinline__ long ph_row_off(int r, int T, int S) {
    const int b = r / T, t = r - b * T;
    return ((long)b * S + (long)kPhStride * t) * kC;
}

// ------------------------------------------------------------------ products
constexpr int kPhFwd = 0, kPhDw = 1, kPhDx = 2;
struct PhTile {
    const float* A; const float* B; float* out;
    int S, T, C;
    int M, N, K, kchunk;
    long slab;
};

// out(m, n) = sum_k A(m, k) B(n, k), blockIdx.x the row tile, blockIdx.y the column tile.
//   kPhFwd  m window, n class, k in [2048 z', 2048 z' + kchunk) of slab z = blockIdx.z: A = x windows, B = wr
//   kPhDw   m class, n one of a window's 2048 floats, k a window of row slab z: A = dlogits^T, B = x windows
//   kPhDx   phase = blockIdx.z, m = b Q + q the frame s = 4 q + phase (Q = ceil(S / 4)), n channel, k = half C + o:
//           A = dlogits[b, q - half, o] (0 where that window does not exist), B = wr[o][(phase + 4 half) 256 + n]
template <int MODE>
__global__ __launch_bounds__(256) void ph_tile_kernel(PhTile p) {
    __shared__ float As[kHK][kHT + 4];
    __shared__ float Bs[kHK][kHT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.x * kHT, n0 = blockIdx.y * kHT, z = blockIdx.z;
    const int k0 = MODE == kPhDx ? 0 : z * p.kchunk, k1 = MODE == kPhDx ? p.K : min(p.K, k0 + p.kchunk);
    const int Q = (p.S + kPhStride - 1) / kPhStride;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kb = k0; kb < k1; kb += kHK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;               // 1024 elements of each 64 x 16 operand tile
            // the unit-stride index runs fastest across the threads: k (rk, kk) or the row (rr, kr)
            const int rk = e >> 4, kk = kb + (e & 15);
            const int rr = e & 63, kr = kb + (e >> 6);
            if (MODE == kPhFwd) {
                const int gm = m0 + rk, gn = n0 + rk;
                As[e & 15][rk] = (gm < p.M && kk < k1) ? p.A[ph_row_off(gm, p.T, p.S) + kk] : 0.f;
                Bs[e & 15][rk] = (gn < p.N && kk < k1) ? p.B[(long)gn * kPhWin + kk] : 0.f;
            } else if (MODE == kPhDw) {
                const int gm = m0 + rr, gn = n0 + rr;
                As[e >> 6][rr] = (gm < p.M && kr < k1) ? p.A[(long)kr * p.C + gm] : 0.f;
                Bs[e >> 6][rr] = (gn < p.N && kr < k1) ? p.B[ph_row_off(kr, p.T, p.S) + gn] : 0.f;
            } else {
                const int gm = m0 + rk, gn = n0 + rr;
                const int b = gm / Q, fq = gm - b * Q;
                const int ha = kk >= p.C ? 1 : 0, t = fq - ha;
                const bool va = gm < p.M && kk < k1 && kPhStride * fq + z < p.S && t >= 0 && t < p.T;
                As[e & 15][rk] = va ? p.A[((long)b * p.T + t) * p.C + (kk - ha * p.C)] : 0.f;
                const int hb = kr >= p.C ? 1 : 0;
                Bs[e >> 6][rr] = (gn < p.N && kr < k1) ? p.B[(long)(kr - hb * p.C) * kPhWin + (z + kPhStride * hb) * kC + gn] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kHK; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[k][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[k][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty + 16 * i;
        if (gm >= p.M) continue;
        float* row;
        if (MODE == kPhDx) {
            const int b = gm / Q, s = kPhStride * (gm - b * Q) + z;
            if (s >= p.S) continue;
            row = p.out + ((long)b * p.S + s) * kC;
        } else {
            row = p.out + (long)z * p.slab + (long)gm * p.N;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx + 16 * j;
            if (gn < p.N) row[gn] = acc[i][j];
        }
    }
}

template <int MODE>
static int ph_tile(const PhTile& p, int nz, hipStream_t st) {
    const dim3 grid((p.M + kHT - 1) / kHT, (p.N + kHT - 1) / kHT, nz);
    hipLaunchKernelGGL(ph_tile_kernel<MODE>, grid, dim3(256), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}

// wr[o][j 256 + c] = W[o][c][j]
__global__ __launch_bounds__(256) void ph_relayout_kernel(const float* __restrict__ W, float* __restrict__ wr, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int o = i / kPhWin, rem = i - o * kPhWin, j = rem >> kCLog2, c = rem & (kC - 1);
    wr[i] = W[(long)o * kPhWin + c * kPhTaps + j];
}

// logits = bias + the K slabs in slab order
__global__ __launch_bounds__(256) void ph_logits_kernel(const float* __restrict__ part, const float* __restrict__ bias,
                                                        float* __restrict__ logits, long n, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int z = 1; z < kPhFwdSlabs; ++z) s += part[(long)z * n + i];
    logits[i] = s + bias[(int)(i % C)];
}

// dbp[z][c] = sum over the windows of slab z of dl[r][c], windows in order
__global__ __launch_bounds__(256) void ph_colsum_kernel(const float* __restrict__ dl, float* __restrict__ dbp, int R, int C,
                                                        int kchunk) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const int r0 = blockIdx.x * kchunk, r1 = min(R, r0 + kchunk);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += dl[(long)r * C + c];
    dbp[(long)blockIdx.x * C + c] = s;
}

// dW[o][c][j] = sum_z part[z][o][j 256 + c], db = sum_z dbp[z], slabs in order
__global__ __launch_bounds__(256) void ph_wsum_kernel(const float* __restrict__ part, const float* __restrict__ dbp,
                                                      float* __restrict__ dW, float* __restrict__ db, int C, int Z) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int nw = C * kPhWin;
    if (i < nw) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += part[(long)z * nw + i];
        const int o = i / kPhWin, rem = i - o * kPhWin, j = rem >> kCLog2, c = rem & (kC - 1);
        dW[(long)o * kPhWin + c * kPhTaps + j] = s;
    } else if (i < nw + C) {
        const int c = i - nw;
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += dbp[(long)z * C + c];
        db[c] = s;
    }
}

// ------------------------------------------------------------------ CTC with lengths
// lse[r] = log sum_c exp(logits[r][c]): one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void ph_lse_kernel(const float* __restrict__ logits, float* __restrict__ lse, int R, int C) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                    // wave-uniform; no barrier below
    const float* l = logits + (long)r * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, l[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(l[c] - mx);
    s = wave_sum(s);
    if (lane == 0) lse[r] = mx + logf(s);
}

struct PhCtc {
    float* lse; double* alpha; int* lab; int* L; int* Tn; double* ll; float* term;
};

// Forward.  State s of the 2 L + 1: the blank for even s, target (s - 1) / 2 for odd s.
//   alpha_t(s) = log(exp alpha_{t-1}(s) + exp alpha_{t-1}(s-1) + [skip] exp alpha_{t-1}(s-2)) + logp(t, l'_s),  t < in_len
// every alpha kept for the backward (float64, row stride 2 Lmax + 1); ll[b] = -log(exp alpha(2L) + exp alpha(2L-1)) at the last
// frame (+inf: zero_infinity; in_len = 0: 0 for an empty target, +inf otherwise), term[b] = ll[b] with infinite losses as 0.
// A thread keeps its states' classes in registers and loads the next frame's emissions before it works on this one.
__global__ __launch_bounds__(256) void ph_alpha_kernel(const float* __restrict__ logits, const long long* __restrict__ in_len,
                                                       const long long* __restrict__ targets, long tgt_stride,
                                                       const long long* __restrict__ tgt_len, PhCtc sv, int T, int C, int Lmax,
                                                       int blank) {
    __shared__ int lab[kPhMaxL];
    __shared__ double buf[2][kPhMaxStates];
    __shared__ int flag;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) flag = 0;
    __syncthreads();
    const long long tl = in_len[b], ql = tgt_len[b];
    const int Tn = tl < 0 ? 0 : (tl > T ? T : (int)tl), L = ql < 0 ? 0 : (ql > Lmax ? Lmax : (int)ql);
    if (tid == 0 && (tl != Tn || ql != L)) { atomicOr(&g_ph_error, 2u); flag = 1; }
    for (int i = tid; i < L; i += 256) {
        const long long y = targets[(long)b * tgt_stride + i];
        const bool bad = y < 0 || y >= C || y == blank;
        if (bad) { atomicOr(&g_ph_error, 1u); flag = 1; }
        const int v = y < 0 ? 0 : (y >= C ? C - 1 : (int)y);
        lab[i] = v;
        sv.lab[(long)b * Lmax + i] = v;
    }
    __syncthreads();
    const int ns = 2 * L + 1, stride = 2 * Lmax + 1;
    const long row0 = (long)b * T;
    int cls[kPhPer];
    bool skip[kPhPer];
    float ecur[kPhPer], enext[kPhPer];
#pragma unroll
    for (int i = 0; i < kPhPer; ++i) {
        const int s = tid + 256 * i;
        const bool on = s < ns;
        cls[i] = (on && (s & 1)) ? lab[s >> 1] : blank;
        skip[i] = on && (s & 1) && s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1];
        ecur[i] = (on && Tn > 0) ? logits[row0 * C + cls[i]] : 0.f;
        enext[i] = 0.f;
    }
    float zcur = Tn > 0 ? sv.lse[row0] : 0.f, znext = 0.f;
    for (int t = 0; t < Tn; ++t) {
        const long row = row0 + t;
        if (t + 1 < Tn) {
            const float* lg = logits + (row + 1) * C;
#pragma unroll
            for (int i = 0; i < kPhPer; ++i)
                if (tid + 256 * i < ns) enext[i] = lg[cls[i]];
            znext = sv.lse[row + 1];
        }
        double* cur = buf[t & 1];
        const double* prev = buf[(t & 1) ^ 1];
#pragma unroll
        for (int i = 0; i < kPhPer; ++i) {
            const int s = tid + 256 * i;
            if (s < ns) {
                const double e = (double)ecur[i] - (double)zcur;
                double a;
                if (t == 0) a = s < 2 ? e : -INFINITY;
                else a = ph_lse3(prev[s], s >= 1 ? prev[s - 1] : -INFINITY, skip[i] ? prev[s - 2] : -INFINITY) + e;
                cur[s] = a;
                sv.alpha[row * stride + s] = a;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPhPer; ++i) ecur[i] = enext[i];
        zcur = znext;
    }
    if (tid == 0) {
        double loss;
        if (Tn == 0) {
            loss = L == 0 ? 0. : INFINITY;
        } else {
            const double* last = buf[(Tn - 1) & 1];
            loss = -ph_lse3(last[2 * L], L > 0 ? last[2 * L - 1] : -INFINITY, -INFINITY);
        }
        if (flag) loss = (double)ph_nan();
        const bool inf = __builtin_isinf((float)loss);        // (what float holds: as nn.CTCLoss in fp32)
        sv.L[b] = L;
        sv.Tn[b] = Tn;
        sv.ll[b] = inf ? INFINITY : loss;
        sv.term[b] = inf ? 0.f : (float)loss;
    }
}

// none: loss[b] = term[b]; sum: sum_b term[b]; mean: (sum_b term[b] / max(L_b, 1)) / B.  One workgroup, float64, each thread
// adds its strided share in index order, then a fixed tree.
__global__ __launch_bounds__(256) void ph_reduce_kernel(const float* __restrict__ term, const int* __restrict__ L, int B,
                                                        int reduction, float* __restrict__ loss) {
    __shared__ double sv[256];
    const int tid = threadIdx.x;
    if (reduction == kPhNone) {
        for (int i = tid; i < B; i += 256) loss[i] = term[i];
        return;
    }
    double a = 0.;
    for (int i = tid; i < B; i += 256) a += reduction == kPhMean ? (double)term[i] / (double)max(L[i], 1) : (double)term[i];
    sv[tid] = a;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) sv[tid] += sv[tid + s];
        __syncthreads();
    }
    if (tid == 0) loss[0] = (float)(reduction == kPhMean ? sv[0] / (double)B : sv[0]);
}

// Backward: beta_t(s) (without the emission at t) = log sum over s' in {s, s+1, [skip] s+2} of exp(beta_{t+1}(s') + logp(t+1, s')),
// occupancy gamma_t(s) = exp(alpha_t(s) + beta_t(s) + loss_b), and for t < in_len
//   dlogits[t, k] = g_b (p[t, k] - sum_{s: l'_s = k} gamma_t(s)),  g_b = dloss[b] (none), dloss (sum), dloss / (B max(L_b, 1)) (mean)
// Frames t >= in_len and sequences with an infinite loss get exactly 0.  The blank's sum is a fixed-order block reduction, every
// other class walks its states in increasing s (chains built in LDS): no sum depends on arrival order.
__global__ __launch_bounds__(256) void ph_beta_kernel(const float* __restrict__ logits, PhCtc sv, const float* __restrict__ dloss,
                                                      float* __restrict__ dlogits, int B, int T, int C, int Lmax, int blank,
                                                      int reduction) {
    __shared__ int lab[kPhMaxL];
    __shared__ int nxt[kPhMaxL];
    __shared__ int head[kPhMaxC];
    __shared__ double buf[2][kPhMaxStates];
    __shared__ float occ[kPhMaxStates];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = sv.L[b], Tn = sv.Tn[b];
    const int ns = 2 * L + 1, stride = 2 * Lmax + 1;
    const long row0 = (long)b * T;
    const double loss = sv.ll[b];
    const bool zero = __builtin_isinf((float)loss);
    const int tz = zero ? 0 : Tn;                          // frames from tz on carry no gradient
    for (long i = (long)tz * C + tid; i < (long)T * C; i += 256) dlogits[row0 * C + i] = 0.f;
    if (zero || Tn == 0) return;                           // block-uniform, before the first barrier
    const float gb = reduction == kPhNone ? dloss[b] : (reduction == kPhMean ? dloss[0] / ((float)B * (float)max(L, 1)) : dloss[0]);
    for (int i = tid; i < L; i += 256) lab[i] = sv.lab[(long)b * Lmax + i];
    for (int c = tid; c < C; c += 256) head[c] = -1;
    __syncthreads();
    if (tid == 0)
        for (int i = L - 1; i >= 0; --i) { nxt[i] = head[lab[i]]; head[lab[i]] = i; }
    __syncthreads();
    int cls[kPhPer];
    bool skip[kPhPer];
    float ecur[kPhPer], enext[kPhPer];
    double acur[kPhPer], anext[kPhPer];
#pragma unroll
    for (int i = 0; i < kPhPer; ++i) {
        const int s = tid + 256 * i;
        const bool on = s < ns;
        cls[i] = (on && (s & 1)) ? lab[s >> 1] : blank;
        skip[i] = on && (s & 1) && s + 2 < ns && lab[(s >> 1) + 1] != lab[s >> 1];
        ecur[i] = on ? logits[(row0 + Tn - 1) * C + cls[i]] : 0.f;
        acur[i] = on ? sv.alpha[(row0 + Tn - 1) * stride + s] : 0.;
        enext[i] = 0.f;
        anext[i] = 0.;
    }
    for (int t = Tn - 1; t >= 0; --t) {
        const long row = row0 + t;
        const float* lg = logits + row * C;
        const float z = sv.lse[row];
        if (t > 0) {
#pragma unroll
            for (int i = 0; i < kPhPer; ++i) {
                const int s = tid + 256 * i;
                if (s < ns) {
                    enext[i] = (lg - C)[cls[i]];
                    anext[i] = sv.alpha[(row - 1) * stride + s];
                }
            }
        }
        double* cur = buf[t & 1];
        const double* prev = buf[(t & 1) ^ 1];
#pragma unroll
        for (int i = 0; i < kPhPer; ++i) {
            const int s = tid + 256 * i;
            if (s < ns) {
                double be;
                if (t == Tn - 1) be = s >= ns - 2 ? 0. : -INFINITY;
                else be = ph_lse3(prev[s], s + 1 < ns ? prev[s + 1] : -INFINITY, skip[i] ? prev[s + 2] : -INFINITY);
                occ[s] = (float)exp(acur[i] + be + loss);
                cur[s] = be + ((double)ecur[i] - (double)z);
            }
        }
        __syncthreads();
        float part = 0.f;
        for (int s = 2 * tid; s < ns; s += 512) part += occ[s];
        part = wave_sum(part);
        if ((tid & 63) == 0) red[tid >> 6] = part;
        __syncthreads();
        const float bsum = (red[0] + red[1]) + (red[2] + red[3]);
        float* d = dlogits + row * C;
        for (int c = tid; c < C; c += 256) {
            float q = 0.f;
            if (c == blank) q = bsum;
            else
                for (int i = head[c]; i >= 0; i = nxt[i]) q += occ[2 * i + 1];
            d[c] = gb * (expf(lg[c] - z) - q);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPhPer; ++i) { ecur[i] = enext[i]; acur[i] = anext[i]; }
    }
}

// ------------------------------------------------------------------ layouts
struct PhLayout {
    int T, Z, kchunk;
    long R, wr, part, dbp, scratch;
};

static int ph_layout(int B, int S, int C, PhLayout* o) {
    CPC_RETURN_IF(B < 1 || S < kPhTaps || C < 2 || C > kPhMaxC, CPC_ERR_SHAPE);
    const int T = (S - kPhTaps) / kPhStride + 1;
    CPC_RETURN_IF(T > kPhMaxT, CPC_ERR_SHAPE);
    const long R = (long)B * T;
    CPC_RETURN_IF(R * C >= (1L << 28), CPC_ERR_SHAPE);         // (eight forward slabs stay below 2^31 floats)
    o->T = T;
    o->R = R;
    o->wr = (long)C * kPhWin;
    int Z = (int)((R + kPhSlabRows - 1) / kPhSlabRows);
    Z = min(Z, kPhMaxSlabs);
    int kchunk = (int)((R + Z - 1) / Z);
    kchunk = (kchunk + kHK - 1) / kHK * kHK;
    o->kchunk = kchunk;
    o->Z = (int)((R + kchunk - 1) / kchunk);
    o->part = 0;
    o->dbp = align64l((long)o->Z * C * kPhWin);
    const long bwd = o->dbp + align64l((long)o->Z * C), fwd = align64l(kPhFwdSlabs * R * C);
    o->scratch = bwd > fwd ? bwd : fwd;
    return 0;
}

struct PhCtcLayout {
    long lse, alpha, lab, L, Tn, ll, term, saved;
};

static int ph_ctc_layout(int B, int T, int C, int Lmax, PhCtcLayout* o) {
    CPC_RETURN_IF(B < 1 || T < 1 || T > kPhMaxT || C < 2 || C > kPhMaxC || Lmax < 0 || Lmax > kPhMaxL, CPC_ERR_SHAPE);
    const long R = (long)B * T, b64 = align64l(B);
    CPC_RETURN_IF(R * C >= (1L << 28), CPC_ERR_SHAPE);
    o->lse = 0;
    o->alpha = align64l(R);                                    // float64: two floats per state
    o->lab = o->alpha + align64l(2 * R * (2L * Lmax + 1));
    o->L = o->lab + align64l((long)B * Lmax);
    o->Tn = o->L + b64;
    o->ll = o->Tn + b64;
    o->term = o->ll + 2 * b64;
    o->saved = o->term + b64;
    return 0;
}

static PhCtc ph_ctc_saved(float* saved, const PhCtcLayout& ly) {
    PhCtc sv;
    sv.lse = saved + ly.lse;
    sv.alpha = reinterpret_cast<double*>(saved + ly.alpha);
    sv.lab = reinterpret_cast<int*>(saved + ly.lab);
    sv.L = reinterpret_cast<int*>(saved + ly.L);
    sv.Tn = reinterpret_cast<int*>(saved + ly.Tn);
    sv.ll = reinterpret_cast<double*>(saved + ly.ll);
    sv.term = saved + ly.term;
    return sv;
}

int phone_head_error_flag_fetch(int clear, unsigned* out) {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_ph_error), sizeof(v)) != hipSuccess) return CPC_ERR_ARG;
    if (clear && v) {
        const unsigned zero = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_ph_error), &zero, sizeof(zero)) != hipSuccess) return CPC_ERR_ARG;
    }
    *out = v;
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_phone_head_layout(int B, int S, int C, int Lmax, long* sizes) {
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    PhLayout ly;
    PhCtcLayout cl;
    int rc = ph_layout(B, S, C, &ly);
    if (rc) return rc;
    rc = ph_ctc_layout(B, ly.T, C, Lmax, &cl);
    if (rc) return rc;
    sizes[0] = ly.T;
    sizes[1] = ly.wr;
    sizes[2] = ly.scratch;
    sizes[3] = ly.R * C;
    sizes[4] = cl.saved;
    return 0;
}

extern "C" int cpc_phone_head_forward(const float* x, const float* W, const float* b, float* wr, float* scratch, float* logits,
                                      int B, int S, int C, void* stream) {
    PhLayout ly;
    const int rc = ph_layout(B, S, C, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !W || !b || !wr || !scratch || !logits, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const int nw = C * kPhWin;
    hipLaunchKernelGGL(ph_relayout_kernel, dim3((nw + 255) / 256), dim3(256), 0, st, W, wr, nw);
    CPC_LAUNCH_CHECK();
    PhTile p{};
    p.A = x; p.B = wr; p.out = scratch + ly.part;
    p.S = S; p.T = ly.T; p.C = C;
    p.M = (int)ly.R; p.N = C; p.K = kPhWin; p.kchunk = kPhWin / kPhFwdSlabs;
    p.slab = ly.R * C;
    const int r2 = ph_tile<kPhFwd>(p, kPhFwdSlabs, st);
    if (r2) return r2;
    const long n = ly.R * C;
    hipLaunchKernelGGL(ph_logits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scratch + ly.part, b, logits, n, C);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_phone_head_backward(const float* x, const float* wr, const float* dlogits, float* scratch, float* dW,
                                       float* db, float* dX, int B, int S, int C, void* stream) {
    PhLayout ly;
    const int rc = ph_layout(B, S, C, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !wr || !dlogits || !scratch || !dW || !db, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const int R = (int)ly.R;
    PhTile p{};                                    // partial dW of each row slab: (C x 2048) = dlogits^T windows
    p.A = dlogits; p.B = x; p.out = scratch + ly.part;
    p.S = S; p.T = ly.T; p.C = C;
    p.M = C; p.N = kPhWin; p.K = R; p.kchunk = ly.kchunk;
    p.slab = (long)C * kPhWin;
    int r2 = ph_tile<kPhDw>(p, ly.Z, st);
    if (r2) return r2;
    hipLaunchKernelGGL(ph_colsum_kernel, dim3(ly.Z), dim3(256), 0, st, dlogits, scratch + ly.dbp, R, C, ly.kchunk);
    CPC_LAUNCH_CHECK();
    const int n = C * kPhWin + C;
    hipLaunchKernelGGL(ph_wsum_kernel, dim3((n + 255) / 256), dim3(256), 0, st, scratch + ly.part, scratch + ly.dbp, dW, db, C,
                       ly.Z);
    CPC_LAUNCH_CHECK();
    if (dX) {                                      // one product per phase s & 3 over the frames of that phase
        PhTile q{};
        q.A = dlogits; q.B = wr; q.out = dX;
        q.S = S; q.T = ly.T; q.C = C;
        q.M = B * ((S + kPhStride - 1) / kPhStride); q.N = kC; q.K = 2 * C; q.kchunk = 2 * C;
        r2 = ph_tile<kPhDx>(q, kPhStride, st);
        if (r2) return r2;
    }
    return 0;
}

extern "C" int cpc_ctc_seq_forward(const float* logits, const long long* in_len, const long long* targets, long tgt_stride,
                                   const long long* tgt_len, float* saved, float* loss, int B, int T, int C, int Lmax, int blank,
                                   int reduction, void* stream) {
    PhCtcLayout ly;
    const int rc = ph_ctc_layout(B, T, C, Lmax, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!logits || !in_len || !tgt_len || !saved || !loss || (Lmax > 0 && (!targets || tgt_stride < Lmax)), CPC_ERR_ARG);
    CPC_RETURN_IF(blank < 0 || blank >= C || reduction < kPhNone || reduction > kPhSum, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const PhCtc sv = ph_ctc_saved(saved, ly);
    const int R = B * T;
    hipLaunchKernelGGL(ph_lse_kernel, dim3((R + 3) / 4), dim3(256), 0, st, logits, sv.lse, R, C);
    CPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ph_alpha_kernel, dim3(B), dim3(256), 0, st, logits, in_len, targets, tgt_stride, tgt_len, sv, T, C, Lmax,
                       blank);
    CPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ph_reduce_kernel, dim3(1), dim3(256), 0, st, sv.term, sv.L, B, reduction, loss);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_ctc_seq_backward(const float* logits, const float* saved, const float* dloss, float* dlogits, int B, int T,
                                    int C, int Lmax, int blank, int reduction, void* stream) {
    PhCtcLayout ly;
    const int rc = ph_ctc_layout(B, T, C, Lmax, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!logits || !saved || !dloss || !dlogits, CPC_ERR_ARG);
    CPC_RETURN_IF(blank < 0 || blank >= C || reduction < kPhNone || reduction > kPhSum, CPC_ERR_ARG);
    const PhCtc sv = ph_ctc_saved(const_cast<float*>(saved), ly);
    hipLaunchKernelGGL(ph_beta_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, sv, dloss, dlogits, B, T, C, Lmax,
                       blank, reduction);
    CPC_LAUNCH_CHECK();
    return 0;
}
