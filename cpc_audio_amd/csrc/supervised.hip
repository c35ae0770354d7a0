// Supervised criteria of the reference (cpc/criterion/criterion.py:128-355): the linear classifier with cross-entropy that
// SpeakerCriterion and PhoneCriterion are, and the CTC loss of CTCPhoneCriterion -- what cpc/eval/linear_separability.py and
// train.py --supervised train on top of CPC features.
//
// Classifier (cpc_classifier_forward / _backward: R rows of 256 features; cpc_classifier_forward_d / _backward_d: of D features,
// 1 <= D <= 512 -- the same host functions, which take D, on the same kernels), C classes:
//   logits = x W^T + b                         sup_prod_kernel, 64 x 64 tiles, exact-f32 FMA, masked in rows and classes
//   lse, argmax, per-row loss / hit            sup_rows_kernel, one wave per row, max / sum-exp over 64-class tiles
//   loss = mean, acc = mean (float64)          sup_mean_kernel, one workgroup, fixed-order tree
//   dlogits = g (softmax - onehot) / R         sup_dlogits_kernel (or the caller's dlogits: the CTC path)
//   dW = dlogits^T x, db = sum dlogits         per-slab partial products over row slabs, then sup_slab_sum_kernel adds the
//                                              slabs in slab order: no float atomics, the same bits on every run
//   dX = dlogits W                             sup_prod_kernel (only when the caller passes dX)
// CTC (cpc_ctc_forward / cpc_ctc_forward_d / cpc_ctc_backward, which works on the logits and serves every width): log_softmax + nn.CTCLoss(blank = C-1, zero_infinity = True, reduction mean) with every
// input length S.  ctc_collapse_kernel collapses the frame labels (cpc/criterion/seq_alignment.py:64-86) into padded targets
// with their lengths, and the loss itself is the library's one CTC loss (ctc_loss.hip) on the product's logits.
#include <climits>

#include "cpc_common.h"
#include "cpc_internal.h"
#include "head_tile.h"

namespace cpc {

constexpr int kSupMaxClasses = 8192;
constexpr int kCtcMaxSeq = 512;
constexpr int kSupSlabRows = 256;          // rows per dW / db partial slab (before the caps below)
constexpr int kSupMaxSlabs = 32;
constexpr int kSupMaxDim = 512;            // widest feature row of the _d entry points

// Set (bit 0) by a kernel that met a label outside [0, C) (CTC: [0, C-1)); read and cleared by cpc_device_error_flags()
// (capi.hip) as CPC_DEVERR_LABEL_RANGE.  The label is clamped for addressing and the loss made NaN.
static __device__ unsigned g_sup_label_range = 0;

__device__ __forceinline__ float sup_nan() { return __builtin_nanf(""); }

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
    __shared__ float As[kHK][kHLd];
    __shared__ float Bs[kHK][kHLd];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * kHT, m0 = blockIdx.y * kHT;
    const int k0 = blockIdx.z * p.kchunk, k1 = min(p.K, k0 + p.kchunk);
    float acc[4][4];
    head_tile_zero(acc);
    for (int kb = k0; kb < k1; kb += kHK) {
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
        head_tile_step(As, Bs, tx, ty, acc);
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
    const dim3 grid((p.N + kHT - 1) / kHT, (p.M + kHT - 1) / kHT, slabs);
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

int head_row_lse(const float* logits, float* lse, int R, int C, hipStream_t st) {
    hipLaunchKernelGGL(sup_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, st, logits, (const long long*)nullptr, lse,
                       (float*)nullptr, (float*)nullptr, R, C);
    CPC_LAUNCH_CHECK();
    return 0;
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

int head_colsum(const float* dl, float* dbp, int R, int C, int kchunk, int Z, hipStream_t st) {
    hipLaunchKernelGGL(sup_colsum_kernel, dim3((C + 255) / 256, Z), dim3(256), 0, st, dl, dbp, R, C, kchunk);
    CPC_LAUNCH_CHECK();
    return 0;
}

// dW = sum_z part[z], db = sum_z dbp[z], slabs in order
__global__ __launch_bounds__(256) void sup_slab_sum_kernel(const float* __restrict__ part, const float* __restrict__ dbp,
                                                           float* __restrict__ dW, float* __restrict__ db, int C, int D, int Z) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nw = (long)C * D;
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

// ------------------------------------------------------------------ CTC: frame labels -> targets
// One workgroup per sequence: reads its S labels, flags and clamps those outside [0, C-1), and collapses runs (position 0 and
// every position whose label differs from the one before) into targets[b][0..L), tgt_len[b] = L, in_len[b] = S.  A sequence
// with a label out of range gets the blank as its first target, which the loss rejects: its loss is NaN, as the flag says.
__global__ __launch_bounds__(256) void ctc_collapse_kernel(const long long* __restrict__ labels, long long* __restrict__ targets,
                                                           long long* __restrict__ tgt_len, long long* __restrict__ in_len, int S,
                                                           int C) {
    __shared__ int raw[kCtcMaxSeq];
    __shared__ int flag;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) flag = 0;
    __syncthreads();
    for (int t = tid; t < S; t += 256) {
        const long long y = labels[(long)b * S + t];
        const bool bad = y < 0 || y >= C - 1;
        if (bad) { atomicOr(&g_sup_label_range, 1u); flag = 1; }
        raw[t] = bad ? (y < 0 ? 0 : C - 2) : (int)y;
    }
    __syncthreads();
    if (tid == 0) {
        long long* tg = targets + (long)b * S;
        int L = 0;
        for (int t = 0; t < S; ++t)
            if (t == 0 || raw[t] != raw[t - 1]) tg[L++] = raw[t];
        if (flag) tg[0] = C - 1;
        tgt_len[b] = L;
        in_len[b] = S;
    }
}

// ------------------------------------------------------------------ layouts
struct SupLayout {
    long logits, lse, row_loss, row_hit, saved;                // classifier forward (saved)
    long targets, tgt_len, in_len, ctc;                        // CTC forward (saved): logits, the int64 targets and lengths, the loss's own
    long dl, part, dbp, scratch;                               // classifier backward (scratch)
    long dlogits;                                              // CTC backward output
    int Z, kchunk;
};

// D features per row, 1 <= D <= kSupMaxDim (the 256 entry points: kC)
static int sup_layout(int B, int S, int C, int D, int ctc, SupLayout* o) {
    CPC_RETURN_IF(D < 1 || D > kSupMaxDim, CPC_ERR_SHAPE);
    CPC_RETURN_IF(B < 1 || S < 1 || C < 2 || C > kSupMaxClasses, CPC_ERR_SHAPE);
    CPC_RETURN_IF(ctc && S > kCtcMaxSeq, CPC_ERR_SHAPE);
    const long R = (long)B * S;
    CPC_RETURN_IF(R * C >= (1L << 31), CPC_ERR_SHAPE);
    const long rc = align64l(R * C), r64 = align64l(R), b64 = align64l(B);
    o->logits = 0;
    o->lse = rc;
    o->row_loss = o->lse + r64;
    o->row_hit = o->row_loss + r64;
    o->saved = o->row_hit + r64;
    o->targets = o->tgt_len = o->in_len = o->ctc = 0;
    if (ctc) {
        long loss_floats = 0;
        const int r2 = ctc_loss_saved_floats(B, S, C, S, &loss_floats);
        if (r2) return r2;
        o->targets = rc;                                       // int64: two floats each
        o->tgt_len = o->targets + 2 * r64;
        o->in_len = o->tgt_len + 2 * b64;
        o->ctc = o->in_len + 2 * b64;
        o->saved = o->ctc + loss_floats;
    }
    int Z = (int)((R + kSupSlabRows - 1) / kSupSlabRows);
    Z = min(Z, kSupMaxSlabs);
    Z = (int)min((long)Z, max(1L, (1L << 25) / ((long)C * D)));   // the partial slabs (Z x C x D) stay <= 2^25 floats: 2^17 / C slabs at D = 256
    int kchunk = (int)((R + Z - 1) / Z);
    kchunk = (kchunk + kHK - 1) / kHK * kHK;
    o->kchunk = kchunk;
    o->Z = (int)((R + kchunk - 1) / kchunk);
    o->dl = 0;
    o->part = rc;
    o->dbp = o->part + align64l((long)o->Z * C * D);
    o->scratch = o->dbp + align64l((long)o->Z * C);
    o->dlogits = ctc ? R * C : 0;
    return 0;
}

static int sup_logits(const float* x, long ldx, const float* W, const float* b, float* saved, const SupLayout& ly, int R, int C,
                      int D, hipStream_t st) {
    SupProd p{};
    p.A = x; p.sam = ldx; p.sak = 1;
    p.B = W; p.sbn = D; p.sbk = 1;
    p.bias = b;
    p.out = saved + ly.logits; p.ldc = C; p.slab = 0;
    p.M = R; p.N = C; p.K = D; p.kchunk = D;
    return sup_prod(p, 1, st);
}

int sup_error_flag_fetch(int clear, unsigned* out) { return device_flag_fetch(HIP_SYMBOL(g_sup_label_range), clear, out); }

static int sup_layout_sizes(int B, int S, int C, int D, int ctc, long* sizes) {
    CPC_RETURN_IF(!sizes || (ctc != 0 && ctc != 1), CPC_ERR_ARG);
    SupLayout ly;
    const int rc = sup_layout(B, S, C, D, ctc, &ly);
    if (rc) return rc;
    sizes[0] = ly.saved;
    sizes[1] = ly.scratch;
    sizes[2] = ly.dlogits;
    return 0;
}

static int classifier_forward(const float* x, long ldx, const float* W, const float* b, const long long* labels, float* saved,
                              float* loss, double* acc, int R, int C, int D, hipStream_t st) {
    SupLayout ly;
    const int rc = sup_layout(R, 1, C, D, 0, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || ldx < D || !W || !b || !labels || !saved || !loss || !acc, CPC_ERR_ARG);
    const int r2 = sup_logits(x, ldx, W, b, saved, ly, R, C, D, st);
    if (r2) return r2;
    hipLaunchKernelGGL(sup_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, st, saved + ly.logits, labels, saved + ly.lse,
                       saved + ly.row_loss, saved + ly.row_hit, R, C);
    CPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sup_mean_kernel, dim3(1), dim3(256), 0, st, saved + ly.row_loss, saved + ly.row_hit, R, loss, acc);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int classifier_backward(const float* x, long ldx, const float* W, const long long* labels, const float* saved,
                               const float* dloss, const float* dlogits, float* scratch, float* dW, float* db, float* dX, int R,
                               int C, int D, hipStream_t st) {
    SupLayout ly;
    const int rc = sup_layout(R, 1, C, D, 0, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || ldx < D || !W || !scratch || !dW || !db, CPC_ERR_ARG);
    CPC_RETURN_IF(!dlogits && (!labels || !saved || !dloss), CPC_ERR_ARG);
    const float* dl = dlogits;
    if (!dl) {
        hipLaunchKernelGGL(sup_dlogits_kernel, dim3((R + 3) / 4), dim3(256), 0, st, saved + ly.logits, saved + ly.lse, labels,
                           dloss, scratch + ly.dl, R, C);
        CPC_LAUNCH_CHECK();
        dl = scratch + ly.dl;
    }
    SupProd p{};                                   // partial dW of each row slab: (C x D) = dl^T x
    p.A = dl; p.sam = 1; p.sak = C;
    p.B = x; p.sbn = 1; p.sbk = ldx;
    p.out = scratch + ly.part; p.ldc = D; p.slab = (long)C * D;
    p.M = C; p.N = D; p.K = R; p.kchunk = ly.kchunk;
    int r2 = sup_prod(p, ly.Z, st);
    if (r2) return r2;
    r2 = head_colsum(dl, scratch + ly.dbp, R, C, ly.kchunk, ly.Z, st);
    if (r2) return r2;
    const long n = (long)C * D + C;
    hipLaunchKernelGGL(sup_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scratch + ly.part,
                       scratch + ly.dbp, dW, db, C, D, ly.Z);
    CPC_LAUNCH_CHECK();
    if (dX) {                                      // dX (R x D) = dl W
        SupProd q{};
        q.A = dl; q.sam = C; q.sak = 1;
        q.B = W; q.sbn = 1; q.sbk = D;
        q.out = dX; q.ldc = D; q.slab = 0;
        q.M = R; q.N = D; q.K = C; q.kchunk = C;
        r2 = sup_prod(q, 1, st);
        if (r2) return r2;
    }
    return 0;
}

static int ctc_forward(const float* x, const float* W, const float* b, const long long* labels, float* saved, float* loss, int B,
                       int S, int C, int D, hipStream_t st) {
    SupLayout ly;
    const int rc = sup_layout(B, S, C, D, 1, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !W || !b || !labels || !saved || !loss, CPC_ERR_ARG);
    const int r2 = sup_logits(x, D, W, b, saved, ly, B * S, C, D, st);
    if (r2) return r2;
    long long* targets = reinterpret_cast<long long*>(saved + ly.targets);
    long long* tgt_len = reinterpret_cast<long long*>(saved + ly.tgt_len);
    long long* in_len = reinterpret_cast<long long*>(saved + ly.in_len);
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(256), 0, st, labels, targets, tgt_len, in_len, S, C);
    CPC_LAUNCH_CHECK();
    return ctc_loss_forward(saved + ly.logits, in_len, targets, S, tgt_len, saved + ly.ctc, loss, B, S, C, S, C - 1, kCtcMean, st);
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_supervised_layout(int B, int S, int C, int ctc, long* sizes) { return sup_layout_sizes(B, S, C, kC, ctc, sizes); }

extern "C" int cpc_supervised_layout_d(int B, int S, int C, int D, int ctc, long* sizes) {
    return sup_layout_sizes(B, S, C, D, ctc, sizes);
}

extern "C" int cpc_classifier_forward(const float* x, long ldx, const float* W, const float* b, const long long* labels,
                                      float* saved, float* loss, double* acc, int R, int C, void* stream) {
    return classifier_forward(x, ldx, W, b, labels, saved, loss, acc, R, C, kC, (hipStream_t)stream);
}

extern "C" int cpc_classifier_forward_d(const float* x, long ldx, const float* W, const float* b, const long long* labels,
                                        float* saved, float* loss, double* acc, int R, int C, int D, void* stream) {
    return classifier_forward(x, ldx, W, b, labels, saved, loss, acc, R, C, D, (hipStream_t)stream);
}

extern "C" int cpc_classifier_backward(const float* x, long ldx, const float* W, const long long* labels, const float* saved,
                                       const float* dloss, const float* dlogits, float* scratch, float* dW, float* db,
                                       float* dX, int R, int C, void* stream) {
    return classifier_backward(x, ldx, W, labels, saved, dloss, dlogits, scratch, dW, db, dX, R, C, kC, (hipStream_t)stream);
}

extern "C" int cpc_classifier_backward_d(const float* x, long ldx, const float* W, const long long* labels, const float* saved,
                                         const float* dloss, const float* dlogits, float* scratch, float* dW, float* db,
                                         float* dX, int R, int C, int D, void* stream) {
    return classifier_backward(x, ldx, W, labels, saved, dloss, dlogits, scratch, dW, db, dX, R, C, D, (hipStream_t)stream);
}

extern "C" int cpc_ctc_forward(const float* x, const float* W, const float* b, const long long* labels, float* saved,
                               float* loss, int B, int S, int C, void* stream) {
    return ctc_forward(x, W, b, labels, saved, loss, B, S, C, kC, (hipStream_t)stream);
}

extern "C" int cpc_ctc_forward_d(const float* x, const float* W, const float* b, const long long* labels, float* saved,
                                 float* loss, int B, int S, int C, int D, void* stream) {
    return ctc_forward(x, W, b, labels, saved, loss, B, S, C, D, (hipStream_t)stream);
}

// (what it reads of ``saved`` -- the logits and the CTC loss's own block -- lies where it does at every feature width: no _d twin)
extern "C" int cpc_ctc_backward(const float* saved, const float* dloss, float* dlogits, int B, int S, int C, void* stream) {
    SupLayout ly;
    const int rc = sup_layout(B, S, C, kC, 1, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!saved || !dloss || !dlogits, CPC_ERR_ARG);
    return ctc_loss_backward(saved + ly.logits, saved + ly.ctc, dloss, dlogits, B, S, C, S, C - 1, kCtcMean, (hipStream_t)stream);
}
