// Supervised criteria of the reference (cpc/criterion/criterion.py:128-355): the linear classifier with cross-entropy that
// SpeakerCriterion and PhoneCriterion are, and the CTC loss of CTCPhoneCriterion -- what cpc/eval/linear_separability.py and
// train.py --supervised train on top of CPC features.
//
// Classifier (cpc_classifier_forward / _backward), R rows of 256 features, C classes:
//   logits = x W^T + b                         sup_prod_kernel, 64 x 64 tiles, exact-f32 FMA, masked in rows and classes
//   lse, argmax, per-row loss / hit            sup_rows_kernel, one wave per row, max / sum-exp over 64-class tiles
//   loss = mean, acc = mean (float64)          sup_mean_kernel, one workgroup, fixed-order tree
//   dlogits = g (softmax - onehot) / R         sup_dlogits_kernel (or the caller's dlogits: the CTC path)
//   dW = dlogits^T x, db = sum dlogits         per-slab partial products over row slabs, then sup_slab_sum_kernel adds the
//                                              slabs in slab order: no float atomics, the same bits on every run
//   dX = dlogits W                             sup_prod_kernel (only when the caller passes dX)
// CTC (cpc_ctc_forward / _backward): log_softmax + nn.CTCLoss(blank = C-1, zero_infinity = True, reduction mean) with every
// input length S and the frame labels collapsed (cpc/criterion/seq_alignment.py:64-86) inside the kernel -- one workgroup per
// sequence runs the log-space alpha recursion (forward) and the beta recursion with the per-class occupancy sums (backward).
#include <climits>

#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kSupMaxClasses = 8192;
constexpr int kCtcMaxSeq = 512;
constexpr int kCtcMaxStates = 2 * kCtcMaxSeq + 1;
constexpr int kSupSlabRows = 256;          // rows per dW / db partial slab (before the caps below)
constexpr int kSupMaxSlabs = 32;
constexpr int kPT = 64, kPK = 16;          // product tile (rows = columns) and k-step

// Set (bit 0) by a kernel that met a label outside [0, C) (CTC: [0, C-1)); read and cleared by cpc_device_error_flags()
// (capi.hip) as CPC_DEVERR_LABEL_RANGE.  The label is clamped for addressing and the loss made NaN.
static __device__ unsigned g_sup_label_range = 0;

__device__ __forceinline__ float sup_nan() { return __builtin_nanf(""); }

// The CTC recursions run in float64: alpha and beta reach -|log p| of hundreds, where float's rounding (|x| 6e-8 per step,
// 128+ steps) would put 1e-4 into every occupancy exp(alpha + beta + loss).
__device__ __forceinline__ double log_add(double a, double b) {
    const double m = fmax(a, b);
    if (m == -INFINITY) return -INFINITY;
    return m + log1p(exp(-fabs(a - b)));
}

// ------------------------------------------------------------------ products
// out[z][m][n] = sum_{k in slab z} A(m, k) B(n, k) (+ bias[n]),  A(m, k) = A[m sam + k sak],  B(n, k) = B[n sbn + k sbk].
struct SupProd {
    const float* A; long sam, sak;
    const float* B; long sbn, sbk;
    const float* bias;
    float* out; long ldc, slab;
    int M, N, K, kchunk;
};

__global__ __launch_bounds__(256) void sup_prod_kernel(SupProd p) {
    __shared__ float As[kPK][kPT + 4];
    __shared__ float Bs[kPK][kPT + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * kPT, m0 = blockIdx.y * kPT;
    const int k0 = blockIdx.z * p.kchunk, k1 = min(p.K, k0 + p.kchunk);
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int kb = k0; kb < k1; kb += kPK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;               // 1024 elements of each 64 x 16 operand tile
            // the unit-stride index runs fastest across the threads
            const int am = p.sak == 1 ? e >> 4 : e & 63, ak = p.sak == 1 ? e & 15 : e >> 6;
            const int bn = p.sbk == 1 ? e >> 4 : e & 63, bk = p.sbk == 1 ? e & 15 : e >> 6;
            const int gm = m0 + am, gka = kb + ak, gn = n0 + bn, gkb = kb + bk;
            As[ak][am] = (gm < p.M && gka < k1) ? p.A[(long)gm * p.sam + (long)gka * p.sak] : 0.f;
            Bs[bk][bn] = (gn < p.N && gkb < k1) ? p.B[(long)gn * p.sbn + (long)gkb * p.sbk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPK; ++k) {
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
    float* out = p.out + (long)blockIdx.z * p.slab;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + ty + 16 * i;
        if (gm >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tx + 16 * j;
            if (gn < p.N) out[(long)gm * p.ldc + gn] = acc[i][j] + (p.bias ? p.bias[gn] : 0.f);
        }
    }
}

static int sup_prod(const SupProd& p, int slabs, hipStream_t st) {
    const dim3 grid((p.N + kPT - 1) / kPT, (p.M + kPT - 1) / kPT, slabs);
    hipLaunchKernelGGL(sup_prod_kernel, grid, dim3(256), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ per-row softmax statistics
// One wave per row (four rows per workgroup).  lse[r] always; with labels also the row's loss (NaN for a label outside
// [0, C)) and whether its argmax -- the first index of the maximum, as torch.max -- is the label.
__global__ __launch_bounds__(256) void sup_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                       float* __restrict__ lse, float* __restrict__ row_loss,
                                                       float* __restrict__ row_hit, int R, int C) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;                                    // wave-uniform; no barrier below
    const float* l = logits + (long)r * C;
    float mx = -INFINITY;
    int ix = INT_MAX;
    for (int c = lane; c < C; c += 64) {
        const float v = l[c];
        if (ix == INT_MAX || v > mx) { mx = v; ix = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float om = __shfl_xor(mx, off);
        const int oi = __shfl_xor(ix, off);
        if (om > mx || (om == mx && oi < ix)) { mx = om; ix = oi; }
    }
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(l[c] - mx);
    s = wave_sum(s);
    const float z = mx + logf(s);
    if (lane == 0) {
        lse[r] = z;
        if (labels) {
            const long long y = labels[r];
            const bool bad = y < 0 || y >= C;
            if (bad) atomicOr(&g_sup_label_range, 1u);
            const int yc = bad ? (y < 0 ? 0 : C - 1) : (int)y;
            row_loss[r] = bad ? sup_nan() : z - l[yc];
            row_hit[r] = (!bad && ix == yc) ? 1.f : 0.f;
        }
    }
}

// loss[0] = (sum v) / n, acc[0] = (sum h) / n (float64): one workgroup, each thread adds its strided share in index order,
// then a fixed tree.
__global__ __launch_bounds__(256) void sup_mean_kernel(const float* __restrict__ v, const float* __restrict__ h, int n,
                                                       float* __restrict__ loss, double* __restrict__ acc) {
    __shared__ double sv[256], sh[256];
    const int tid = threadIdx.x;
    double a = 0., b = 0.;
    for (int i = tid; i < n; i += 256) {
        a += (double)v[i];
        if (h) b += (double)h[i];
    }
    sv[tid] = a;
    sh[tid] = b;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) { sv[tid] += sv[tid + s]; sh[tid] += sh[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        loss[0] = (float)(sv[0] / (double)n);
        if (acc) acc[0] = sh[0] / (double)n;
    }
}

// ------------------------------------------------------------------ classifier backward pieces
__global__ __launch_bounds__(256) void sup_dlogits_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                          const long long* __restrict__ labels, const float* __restrict__ dloss,
                                                          float* __restrict__ dl, int R, int C) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float g = dloss[0] / (float)R;
    const long long y = labels[r];
    const int yc = y < 0 ? 0 : (y >= C ? C - 1 : (int)y);
    const float z = lse[r];
    const float* l = logits + (long)r * C;
    float* d = dl + (long)r * C;
    // (the loop vectorizer would pair these products into v_pk_mul_f32: the library carries no packed fp32, build.py)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int c = lane; c < C; c += 64) d[c] = g * (expf(l[c] - z) - (c == yc ? 1.f : 0.f));
}

// dbp[z][c] = sum over the rows of slab z of dl[r][c], rows in order
__global__ __launch_bounds__(256) void sup_colsum_kernel(const float* __restrict__ dl, float* __restrict__ dbp, int R, int C,
                                                         int kchunk) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int r0 = blockIdx.y * kchunk, r1 = min(R, r0 + kchunk);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += dl[(long)r * C + c];
    dbp[(long)blockIdx.y * C + c] = s;
}

// dW = sum_z part[z], db = sum_z dbp[z], slabs in order
__global__ __launch_bounds__(256) void sup_slab_sum_kernel(const float* __restrict__ part, const float* __restrict__ dbp,
                                                           float* __restrict__ dW, float* __restrict__ db, int C, int Z) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nw = (long)C * kC;
    if (i < nw) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += part[(long)z * nw + i];
        dW[i] = s;
    } else if (i < nw + C) {
        const long c = i - nw;
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += dbp[(long)z * C + c];
        db[c] = s;
    }
}

// ------------------------------------------------------------------ CTC
__device__ __forceinline__ int ctc_state_label(const int* lab, int s, int blank) { return (s & 1) ? lab[s >> 1] : blank; }

// Reads one sequence's S labels, flags and clamps those outside [0, C-1), and collapses runs: position 0 and every position
// whose label differs from the one before.  -> lab[0..L), returns L (block-uniform), *bad set if any label was out of range.
__device__ int ctc_collapse(const long long* __restrict__ labels, int S, int C, int* raw, int* lab, int* flag) {
    const int tid = threadIdx.x;
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int t = tid; t < S; t += blockDim.x) {
        const long long y = labels[t];
        const bool bad = y < 0 || y >= C - 1;
        if (bad) { atomicOr(&g_sup_label_range, 1u); *flag = 1; }
        raw[t] = bad ? (y < 0 ? 0 : C - 2) : (int)y;
    }
    __syncthreads();
    if (tid == 0) {
        int L = 0;
        for (int t = 0; t < S; ++t)
            if (t == 0 || raw[t] != raw[t - 1]) lab[L++] = raw[t];
        raw[0] = L;                                        // raw[] is done with: hand L over through it
    }
    __syncthreads();
    return raw[0];
}

// Forward: alpha_t(s) = log_add(alpha_{t-1}(s), alpha_{t-1}(s-1), [skip] alpha_{t-1}(s-2)) + logp(t, l'_s), every alpha kept
// for the backward (float64); ll[b] = -log_add(alpha_{S-1}(2L), alpha_{S-1}(2L-1)) (+inf: zero_infinity), term[b] = ll[b] / max(L, 1)
// with infinite losses counted as 0.
struct CtcSaved {
    float* logits; float* lse; double* alpha; int* lprime; int* L; double* ll; float* term;
};

__global__ __launch_bounds__(256) void ctc_alpha_kernel(const long long* __restrict__ labels, CtcSaved sv, int S, int C) {
    __shared__ int raw[kCtcMaxSeq];
    __shared__ int lab[kCtcMaxSeq];
    __shared__ double buf[2][kCtcMaxStates];
    __shared__ int flag;
    const int b = blockIdx.x, tid = threadIdx.x, blank = C - 1;
    const int L = ctc_collapse(labels + (long)b * S, S, C, raw, lab, &flag);
    const int ns = 2 * L + 1, stride = 2 * S + 1;
    for (int i = tid; i < L; i += 256) sv.lprime[(long)b * S + i] = lab[i];
    for (int t = 0; t < S; ++t) {
        const long row = (long)b * S + t;
        const float* lg = sv.logits + row * C;
        const float z = sv.lse[row];
        double* cur = buf[t & 1];
        const double* prev = buf[(t & 1) ^ 1];
        for (int s = tid; s < ns; s += 256) {
            const double e = (double)lg[ctc_state_label(lab, s, blank)] - (double)z;
            double a;
            if (t == 0) {
                a = s < 2 ? e : -INFINITY;
            } else {
                a = prev[s];
                if (s >= 1) a = log_add(a, prev[s - 1]);
                if (s >= 2 && (s & 1) && lab[s >> 1] != lab[(s >> 1) - 1]) a = log_add(a, prev[s - 2]);
                a += e;
            }
            cur[s] = a;
            sv.alpha[row * stride + s] = a;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double* last = buf[(S - 1) & 1];
        double loss = -log_add(last[2 * L], last[2 * L - 1]);
        if (flag) loss = (double)sup_nan();
        const bool inf = __builtin_isinf((float)loss);        // (what float holds: as nn.CTCLoss in fp32)
        sv.L[b] = L;
        sv.ll[b] = inf ? INFINITY : loss;
        sv.term[b] = inf ? 0.f : (float)loss / (float)max(L, 1);
    }
}

// Backward: beta_t(s) (without the emission at t) = log_add over s' in {s, s+1, [skip] s+2} of beta_{t+1}(s') + logp(t+1, s'),
// occupancy gamma_t(s) = exp(alpha_t(s) + beta_t(s) + loss_b), and
//   dlogits[t, k] = g_b (p[t, k] - sum_{s: l'_s = k} gamma_t(s)),   g_b = g / (B max(L_b, 1))
// The blank's sum is a fixed-order block reduction, every other class walks its states in increasing s (chains built in
// LDS): no sum depends on arrival order.  A sequence with an infinite loss gets dlogits 0 (zero_infinity).
__global__ __launch_bounds__(256) void ctc_beta_kernel(CtcSaved sv, const float* __restrict__ dloss, float* __restrict__ dlogits,
                                                       int B, int S, int C) {
    __shared__ int lab[kCtcMaxSeq];
    __shared__ int nxt[kCtcMaxSeq];
    __shared__ int head[kSupMaxClasses];
    __shared__ double buf[2][kCtcMaxStates];
    __shared__ float occ[kCtcMaxStates];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, blank = C - 1;
    const int L = sv.L[b];
    const int ns = 2 * L + 1, stride = 2 * S + 1;
    const double loss = sv.ll[b];
    const bool zero = __builtin_isinf((float)loss);
    const float gb = zero ? 0.f : dloss[0] / ((float)B * (float)max(L, 1));
    for (int i = tid; i < L; i += 256) lab[i] = sv.lprime[(long)b * S + i];
    for (int c = tid; c < C; c += 256) head[c] = -1;
    __syncthreads();
    if (tid == 0)
        for (int i = L - 1; i >= 0; --i) { nxt[i] = head[lab[i]]; head[lab[i]] = i; }
    __syncthreads();
    for (int t = S - 1; t >= 0; --t) {
        const long row = (long)b * S + t;
        const float* lg = sv.logits + row * C;
        const float z = sv.lse[row];
        double* cur = buf[t & 1];
        const double* prev = buf[(t & 1) ^ 1];
        for (int s = tid; s < ns; s += 256) {
            double be;
            if (t == S - 1) {
                be = s >= ns - 2 ? 0. : -INFINITY;
            } else {
                be = prev[s];
                if (s + 1 < ns) be = log_add(be, prev[s + 1]);
                if (s + 2 < ns && (s & 1) && lab[(s >> 1) + 1] != lab[s >> 1]) be = log_add(be, prev[s + 2]);
            }
            occ[s] = zero ? 0.f : (float)exp(sv.alpha[row * stride + s] + be + loss);
            cur[s] = be + ((double)lg[ctc_state_label(lab, s, blank)] - (double)z);
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
            float g = 0.f;
            if (!zero) {
                float q = 0.f;
                if (c == blank) q = bsum;
                else
                    for (int i = head[c]; i >= 0; i = nxt[i]) q += occ[2 * i + 1];
                g = gb * (expf(lg[c] - z) - q);
            }
            d[c] = g;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ layouts
struct SupLayout {
    long logits, lse, row_loss, row_hit, saved;                // classifier forward (saved)
    long alpha, lprime, L, ll, term;                           // CTC forward (saved, after the classifier's four)
    long dl, part, dbp, scratch;                               // classifier backward (scratch)
    long dlogits;                                              // CTC backward output
    int Z, kchunk;
};

static int sup_layout(int B, int S, int C, int ctc, SupLayout* o) {
    CPC_RETURN_IF(B < 1 || S < 1 || C < 2 || C > kSupMaxClasses, CPC_ERR_SHAPE);
    CPC_RETURN_IF(ctc && S > kCtcMaxSeq, CPC_ERR_SHAPE);
    const long R = (long)B * S;
    CPC_RETURN_IF(R * C >= (1L << 31), CPC_ERR_SHAPE);
    const long rc = align64l(R * C), r64 = align64l(R), b64 = align64l(B);
    o->logits = 0;
    o->lse = rc;
    o->row_loss = o->lse + r64;
    o->row_hit = o->row_loss + r64;
    long end = o->row_hit + r64;
    o->alpha = o->lprime = o->L = o->ll = o->term = 0;
    if (ctc) {
        o->alpha = end;                                        // float64: two floats per state
        o->lprime = o->alpha + align64l(2 * R * (2L * S + 1));
        o->L = o->lprime + r64;
        o->ll = o->L + b64;
        o->term = o->ll + 2 * b64;
        end = o->term + b64;
    }
    o->saved = end;
    int Z = (int)((R + kSupSlabRows - 1) / kSupSlabRows);
    Z = min(Z, kSupMaxSlabs);
    Z = min(Z, max(1, (1 << 17) / C));                        // partial slabs stay <= 2^17 x 256 floats
    int kchunk = (int)((R + Z - 1) / Z);
    kchunk = (kchunk + kPK - 1) / kPK * kPK;
    o->kchunk = kchunk;
    o->Z = (int)((R + kchunk - 1) / kchunk);
    o->dl = 0;
    o->part = rc;
    o->dbp = o->part + align64l((long)o->Z * C * kC);
    o->scratch = o->dbp + align64l((long)o->Z * C);
    o->dlogits = ctc ? R * C : 0;
    return 0;
}

static int sup_forward_rows(const float* x, long ldx, const float* W, const float* b, const long long* labels, float* saved,
                            const SupLayout& ly, int R, int C, hipStream_t st) {
    SupProd p{};
    p.A = x; p.sam = ldx; p.sak = 1;
    p.B = W; p.sbn = kC; p.sbk = 1;
    p.bias = b;
    p.out = saved + ly.logits; p.ldc = C; p.slab = 0;
    p.M = R; p.N = C; p.K = kC; p.kchunk = kC;
    int rc = sup_prod(p, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(sup_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, st, saved + ly.logits, labels, saved + ly.lse,
                       saved + ly.row_loss, saved + ly.row_hit, R, C);
    CPC_LAUNCH_CHECK();
    return 0;
}

int sup_error_flag_fetch(int clear, unsigned* out) {
    unsigned v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_sup_label_range), sizeof(v)) != hipSuccess) return CPC_ERR_ARG;
    if (clear && v) {
        const unsigned zero = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_sup_label_range), &zero, sizeof(zero)) != hipSuccess) return CPC_ERR_ARG;
    }
    *out = v;
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_supervised_layout(int B, int S, int C, int ctc, long* sizes) {
    CPC_RETURN_IF(!sizes || (ctc != 0 && ctc != 1), CPC_ERR_ARG);
    SupLayout ly;
    const int rc = sup_layout(B, S, C, ctc, &ly);
    if (rc) return rc;
    sizes[0] = ly.saved;
    sizes[1] = ly.scratch;
    sizes[2] = ly.dlogits;
    return 0;
}

extern "C" int cpc_classifier_forward(const float* x, long ldx, const float* W, const float* b, const long long* labels,
                                      float* saved, float* loss, double* acc, int R, int C, void* stream) {
    SupLayout ly;
    const int rc = sup_layout(R, 1, C, 0, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || ldx < kC || !W || !b || !labels || !saved || !loss || !acc, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const int r2 = sup_forward_rows(x, ldx, W, b, labels, saved, ly, R, C, st);
    if (r2) return r2;
    hipLaunchKernelGGL(sup_mean_kernel, dim3(1), dim3(256), 0, st, saved + ly.row_loss, saved + ly.row_hit, R, loss, acc);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_classifier_backward(const float* x, long ldx, const float* W, const long long* labels, const float* saved,
                                       const float* dloss, const float* dlogits, float* scratch, float* dW, float* db,
                                       float* dX, int R, int C, void* stream) {
    SupLayout ly;
    const int rc = sup_layout(R, 1, C, 0, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || ldx < kC || !W || !scratch || !dW || !db, CPC_ERR_ARG);
    CPC_RETURN_IF(!dlogits && (!labels || !saved || !dloss), CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const float* dl = dlogits;
    if (!dl) {
        hipLaunchKernelGGL(sup_dlogits_kernel, dim3((R + 3) / 4), dim3(256), 0, st, saved + ly.logits, saved + ly.lse, labels,
                           dloss, scratch + ly.dl, R, C);
        CPC_LAUNCH_CHECK();
        dl = scratch + ly.dl;
    }
    SupProd p{};                                   // partial dW of each row slab: (C x 256) = dl^T x
    p.A = dl; p.sam = 1; p.sak = C;
    p.B = x; p.sbn = 1; p.sbk = ldx;
    p.out = scratch + ly.part; p.ldc = kC; p.slab = (long)C * kC;
    p.M = C; p.N = kC; p.K = R; p.kchunk = ly.kchunk;
    int r2 = sup_prod(p, ly.Z, st);
    if (r2) return r2;
    hipLaunchKernelGGL(sup_colsum_kernel, dim3((C + 255) / 256, ly.Z), dim3(256), 0, st, dl, scratch + ly.dbp, R, C, ly.kchunk);
    CPC_LAUNCH_CHECK();
    const long n = (long)C * kC + C;
    hipLaunchKernelGGL(sup_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scratch + ly.part,
                       scratch + ly.dbp, dW, db, C, ly.Z);
    CPC_LAUNCH_CHECK();
    if (dX) {                                      // dX (R x 256) = dl W
        SupProd q{};
        q.A = dl; q.sam = C; q.sak = 1;
        q.B = W; q.sbn = 1; q.sbk = kC;
        q.out = dX; q.ldc = kC; q.slab = 0;
        q.M = R; q.N = kC; q.K = C; q.kchunk = C;
        r2 = sup_prod(q, 1, st);
        if (r2) return r2;
    }
    return 0;
}

static CtcSaved ctc_saved(float* saved, const SupLayout& ly) {
    CtcSaved sv;
    sv.logits = saved + ly.logits;
    sv.lse = saved + ly.lse;
    sv.alpha = reinterpret_cast<double*>(saved + ly.alpha);
    sv.lprime = reinterpret_cast<int*>(saved + ly.lprime);
    sv.L = reinterpret_cast<int*>(saved + ly.L);
    sv.ll = reinterpret_cast<double*>(saved + ly.ll);
    sv.term = saved + ly.term;
    return sv;
}

extern "C" int cpc_ctc_forward(const float* x, const float* W, const float* b, const long long* labels, float* saved,
                               float* loss, int B, int S, int C, void* stream) {
    SupLayout ly;
    const int rc = sup_layout(B, S, C, 1, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !W || !b || !labels || !saved || !loss, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const int R = B * S;
    const int r2 = sup_forward_rows(x, kC, W, b, nullptr, saved, ly, R, C, st);
    if (r2) return r2;
    const CtcSaved sv = ctc_saved(saved, ly);
    hipLaunchKernelGGL(ctc_alpha_kernel, dim3(B), dim3(256), 0, st, labels, sv, S, C);
    CPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sup_mean_kernel, dim3(1), dim3(256), 0, st, sv.term, (const float*)nullptr, B, loss, (double*)nullptr);
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_ctc_backward(const float* saved, const float* dloss, float* dlogits, int B, int S, int C, void* stream) {
    SupLayout ly;
    const int rc = sup_layout(B, S, C, 1, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!saved || !dloss || !dlogits, CPC_ERR_ARG);
    const CtcSaved sv = ctc_saved(const_cast<float*>(saved), ly);
    hipLaunchKernelGGL(ctc_beta_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sv, dloss, dlogits, B, S, C);
    CPC_LAUNCH_CHECK();
    return 0;
}
