// The PER phone classifier of the reference (cpc/eval/common_voices_eval.py, CTCphone_criterion): the windowed head
// nn.Conv1d(256, C, 8, stride 4) on channels-last features -- what `common_voices_eval train` trains, under the CTC loss with
// lengths of ctc_loss.hip.
//
// Head (cpc_phone_head_forward / _backward), x (B, S, 256), W (C, 256, 8) in torch's layout, T = (S - 8) / 4 + 1 windows:
//   wr[o][j 256 + c] = W[o][c][j]                  ph_relayout_kernel: the weight in the order of a window's 2048 floats
//   logits = windows wr^T + b                      frames 4t .. 4t+7 are 2048 contiguous floats, so window (b, t) is the row
//                                                  x + (b S + 4t) 256 of a K = 2048 product: ph_tile_kernel<kPhFwd>, 64 x 64
//                                                  tiles (head_tile.h), eight K slabs of 256 (one per tap) for parallelism,
//                                                  added in slab order with the bias by ph_logits_kernel
//   dW = dlogits^T windows, db = sum dlogits       ph_tile_kernel<kPhDw> per row slab, head_colsum; ph_wsum_kernel adds the
//                                                  slabs in slab order and writes torch's (C, 256, 8) layout
//   dX[b, s] = sum over the <= 2 windows of s      ph_tile_kernel<kPhDx>, gather form: frames of one phase s & 3 share their
//                                                  weight taps (s & 3 for window s / 4, (s & 3) + 4 for window s / 4 - 1), so each
//                                                  phase is one product over K = 2 C; frames no window covers get exactly 0
// No float atomics, fixed summation orders: identical calls give identical bits, and a window's results do not depend on
// the batch around it.
//
// Any feature width (cpc_phone_head_*_d, 1 <= D <= 512): the same kernels with the width as their template argument DC -- 256 for
// the entry points above, 0 for "read p.D" -- so a window is 8 D contiguous floats, wr[o][j D + c] = W[o][c][j], the forward's
// eight K slabs are D wide (ph_tile_kernel masks k inside a slab's last 16-step when D % 16 != 0) and dX has N = D columns.
// Orders of summation do not depend on DC: the _d calls at 256 give the bits of the 256 calls.
#include "cpc_common.h"
#include "cpc_internal.h"
#include "head_tile.h"

namespace cpc {

constexpr int kPhTaps = 8, kPhStride = 4;
constexpr int kPhMaxD = 512;                         // widest feature row of the _d entry points
constexpr int kPhMaxT = 2048, kPhMaxC = 256;
constexpr int kPhFwdSlabs = kPhTaps;                 // K slabs of the forward product
constexpr int kPhSlabRows = 256;                     // windows per dW / db partial slab
constexpr int kPhMaxSlabs = 32;

// window r = b T + t starts at frame b S + 4 t
__device__ __forceinline__ long ph_row_off(int r, int T, int S, int D) {
    const int b = r / T, t = r - b * T;
    return ((long)b * S + (long)kPhStride * t) * D;
}

// ------------------------------------------------------------------ products
constexpr int kPhFwd = 0, kPhDw = 1, kPhDx = 2;
struct PhTile {
    const float* A; const float* B; float* out;
    int S, T, C, D;
    int M, N, K, kchunk;
    long slab;
};

// out(m, n) = sum_k A(m, k) B(n, k), blockIdx.x the row tile, blockIdx.y the column tile.  D = DC, or p.D where DC is 0.
//   kPhFwd  m window, n class, k in [kchunk z, kchunk z + kchunk) of slab z = blockIdx.z (kchunk = D: tap z): A = x windows,
//           B = wr
//   kPhDw   m class, n one of a window's 8 D floats, k a window of row slab z: A = dlogits^T, B = x windows
//   kPhDx   phase = blockIdx.z, m = b Q + q the frame s = 4 q + phase (Q = ceil(S / 4)), n channel, k = half C + o:
//           A = dlogits[b, q - half, o] (0 where that window does not exist), B = wr[o][(phase + 4 half) D + n]
// Every operand element is masked by its row (gm, gn) and by k < k1, so M, N, K and kchunk need not be multiples of the tile.
template <int MODE, int DC>
__global__ __launch_bounds__(256) void ph_tile_kernel(PhTile p) {
    __shared__ float As[kHK][kHLd];
    __shared__ float Bs[kHK][kHLd];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.x * kHT, n0 = blockIdx.y * kHT, z = blockIdx.z;
    const int k0 = MODE == kPhDx ? 0 : z * p.kchunk, k1 = MODE == kPhDx ? p.K : min(p.K, k0 + p.kchunk);
    const int Q = (p.S + kPhStride - 1) / kPhStride;
    const int D = DC ? DC : p.D, win = kPhTaps * D;
    float acc[4][4];
    head_tile_zero(acc);
    for (int kb = k0; kb < k1; kb += kHK) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;               // 1024 elements of each 64 x 16 operand tile
            // the unit-stride index runs fastest across the threads: k (rk, kk) or the row (rr, kr)
            const int rk = e >> 4, kk = kb + (e & 15);
            const int rr = e & 63, kr = kb + (e >> 6);
            if (MODE == kPhFwd) {
                const int gm = m0 + rk, gn = n0 + rk;
                As[e & 15][rk] = (gm < p.M && kk < k1) ? p.A[ph_row_off(gm, p.T, p.S, D) + kk] : 0.f;
                Bs[e & 15][rk] = (gn < p.N && kk < k1) ? p.B[(long)gn * win + kk] : 0.f;
            } else if (MODE == kPhDw) {
                const int gm = m0 + rr, gn = n0 + rr;
                As[e >> 6][rr] = (gm < p.M && kr < k1) ? p.A[(long)kr * p.C + gm] : 0.f;
                Bs[e >> 6][rr] = (gn < p.N && kr < k1) ? p.B[ph_row_off(kr, p.T, p.S, D) + gn] : 0.f;
            } else {
                const int gm = m0 + rk, gn = n0 + rr;
                const int b = gm / Q, fq = gm - b * Q;
                const int ha = kk >= p.C ? 1 : 0, t = fq - ha;
                const bool va = gm < p.M && kk < k1 && kPhStride * fq + z < p.S && t >= 0 && t < p.T;
                As[e & 15][rk] = va ? p.A[((long)b * p.T + t) * p.C + (kk - ha * p.C)] : 0.f;
                const int hb = kr >= p.C ? 1 : 0;
                Bs[e >> 6][rr] = (gn < p.N && kr < k1) ? p.B[(long)(kr - hb * p.C) * win + (z + kPhStride * hb) * D + gn] : 0.f;
            }
        }
        __syncthreads();
        head_tile_step(As, Bs, tx, ty, acc);
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
            row = p.out + ((long)b * p.S + s) * D;
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

// fixed: the 256 instantiation (the cpc_phone_head_* entry points); otherwise the one that reads p.D
template <int MODE>
static int ph_tile(const PhTile& p, int nz, bool fixed, hipStream_t st) {
    const dim3 grid((p.M + kHT - 1) / kHT, (p.N + kHT - 1) / kHT, nz);
    if (fixed) hipLaunchKernelGGL((ph_tile_kernel<MODE, kC>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((ph_tile_kernel<MODE, 0>), grid, dim3(256), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}

// wr[o][j D + c] = W[o][c][j]
template <int DC>
__global__ __launch_bounds__(256) void ph_relayout_kernel(const float* __restrict__ W, float* __restrict__ wr, int n, int Dr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int D = DC ? DC : Dr, win = kPhTaps * D;
    const int o = i / win, rem = i - o * win, j = rem / D, c = rem - j * D;
    wr[i] = W[(long)o * win + c * kPhTaps + j];
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

// dW[o][c][j] = sum_z part[z][o][j D + c], db = sum_z dbp[z], slabs in order
template <int DC>
__global__ __launch_bounds__(256) void ph_wsum_kernel(const float* __restrict__ part, const float* __restrict__ dbp,
                                                      float* __restrict__ dW, float* __restrict__ db, int C, int Z, int Dr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int D = DC ? DC : Dr, win = kPhTaps * D;
    const int nw = C * win;
    if (i < nw) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += part[(long)z * nw + i];
        const int o = i / win, rem = i - o * win, j = rem / D, c = rem - j * D;
        dW[(long)o * win + c * kPhTaps + j] = s;
    } else if (i < nw + C) {
        const int c = i - nw;
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += dbp[(long)z * C + c];
        db[c] = s;
    }
}

// ------------------------------------------------------------------ layouts
struct PhLayout {
    int T, Z, kchunk, win;
    long R, wr, part, dbp, scratch;
};

// Sizes in floats.  With D <= 512 and C <= 256 a relaid weight (wr, and one dW slab) is at most 2^20 floats and the <= 32 dW
// slabs at most 2^25, so the kernels' int element counts hold at every width; x is indexed in long throughout.
static int ph_layout(int B, int S, int C, int D, PhLayout* o) {
    CPC_RETURN_IF(D < 1 || D > kPhMaxD, CPC_ERR_SHAPE);
    CPC_RETURN_IF(B < 1 || S < kPhTaps || C < 2 || C > kPhMaxC, CPC_ERR_SHAPE);
    const int T = (S - kPhTaps) / kPhStride + 1;
    CPC_RETURN_IF(T > kPhMaxT, CPC_ERR_SHAPE);
    const long R = (long)B * T;
    CPC_RETURN_IF(R * C >= (1L << 28), CPC_ERR_SHAPE);         // (eight forward slabs stay below 2^31 floats)
    o->T = T;
    o->R = R;
    o->win = kPhTaps * D;
    o->wr = (long)C * o->win;
    int Z = (int)((R + kPhSlabRows - 1) / kPhSlabRows);
    Z = min(Z, kPhMaxSlabs);
    int kchunk = (int)((R + Z - 1) / Z);
    kchunk = (kchunk + kHK - 1) / kHK * kHK;
    o->kchunk = kchunk;
    o->Z = (int)((R + kchunk - 1) / kchunk);
    o->part = 0;
    o->dbp = align64l((long)o->Z * C * o->win);
    const long bwd = o->dbp + align64l((long)o->Z * C), fwd = align64l(kPhFwdSlabs * R * C);
    o->scratch = bwd > fwd ? bwd : fwd;
    return 0;
}

static int ph_sizes(int B, int S, int C, int D, int Lmax, long* sizes) {
    PhLayout ly;
    long ctc_saved = 0;
    int rc = ph_layout(B, S, C, D, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    rc = ctc_loss_saved_floats(B, ly.T, C, Lmax, &ctc_saved);
    if (rc) return rc;
    sizes[0] = ly.T;
    sizes[1] = ly.wr;
    sizes[2] = ly.scratch;
    sizes[3] = ly.R * C;
    sizes[4] = ctc_saved;
    return 0;
}

static int ph_forward(const float* x, const float* W, const float* b, float* wr, float* scratch, float* logits, int B, int S,
                      int C, int D, bool fixed, void* stream) {
    PhLayout ly;
    const int rc = ph_layout(B, S, C, D, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !W || !b || !wr || !scratch || !logits, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const int nw = C * ly.win;
    if (fixed) hipLaunchKernelGGL(ph_relayout_kernel<kC>, dim3((nw + 255) / 256), dim3(256), 0, st, W, wr, nw, D);
    else hipLaunchKernelGGL(ph_relayout_kernel<0>, dim3((nw + 255) / 256), dim3(256), 0, st, W, wr, nw, D);
    CPC_LAUNCH_CHECK();
    PhTile p{};
    p.A = x; p.B = wr; p.out = scratch + ly.part;
    p.S = S; p.T = ly.T; p.C = C; p.D = D;
    p.M = (int)ly.R; p.N = C; p.K = ly.win; p.kchunk = D;   // one K slab per tap
    p.slab = ly.R * C;
    const int r2 = ph_tile<kPhFwd>(p, kPhFwdSlabs, fixed, st);
    if (r2) return r2;
    const long n = ly.R * C;
    hipLaunchKernelGGL(ph_logits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scratch + ly.part, b, logits, n, C);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int ph_backward(const float* x, const float* wr, const float* dlogits, float* scratch, float* dW, float* db, float* dX,
                       int B, int S, int C, int D, bool fixed, void* stream) {
    PhLayout ly;
    const int rc = ph_layout(B, S, C, D, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !wr || !dlogits || !scratch || !dW || !db, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const int R = (int)ly.R;
    PhTile p{};                                    // partial dW of each row slab: (C x 8 D) = dlogits^T windows
    p.A = dlogits; p.B = x; p.out = scratch + ly.part;
    p.S = S; p.T = ly.T; p.C = C; p.D = D;
    p.M = C; p.N = ly.win; p.K = R; p.kchunk = ly.kchunk;
    p.slab = (long)C * ly.win;
    int r2 = ph_tile<kPhDw>(p, ly.Z, fixed, st);
    if (r2) return r2;
    r2 = head_colsum(dlogits, scratch + ly.dbp, R, C, ly.kchunk, ly.Z, st);
    if (r2) return r2;
    const int n = C * ly.win + C;
    if (fixed)
        hipLaunchKernelGGL(ph_wsum_kernel<kC>, dim3((n + 255) / 256), dim3(256), 0, st, scratch + ly.part, scratch + ly.dbp, dW,
                           db, C, ly.Z, D);
    else
        hipLaunchKernelGGL(ph_wsum_kernel<0>, dim3((n + 255) / 256), dim3(256), 0, st, scratch + ly.part, scratch + ly.dbp, dW,
                           db, C, ly.Z, D);
    CPC_LAUNCH_CHECK();
    if (dX) {                                      // one product per phase s & 3 over the frames of that phase
        PhTile q{};
        q.A = dlogits; q.B = wr; q.out = dX;
        q.S = S; q.T = ly.T; q.C = C; q.D = D;
        q.M = B * ((S + kPhStride - 1) / kPhStride); q.N = D; q.K = 2 * C; q.kchunk = 2 * C;
        r2 = ph_tile<kPhDx>(q, kPhStride, fixed, st);
        if (r2) return r2;
    }
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_phone_head_layout(int B, int S, int C, int Lmax, long* sizes) {
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    return ph_sizes(B, S, C, kC, Lmax, sizes);
}

extern "C" int cpc_phone_head_layout_d(int B, int S, int C, int Lmax, int D, long* sizes) {
    return ph_sizes(B, S, C, D, Lmax, sizes);
}

extern "C" int cpc_phone_head_forward(const float* x, const float* W, const float* b, float* wr, float* scratch, float* logits,
                                      int B, int S, int C, void* stream) {
    return ph_forward(x, W, b, wr, scratch, logits, B, S, C, kC, true, stream);
}

extern "C" int cpc_phone_head_forward_d(const float* x, const float* W, const float* b, float* wr, float* scratch, float* logits,
                                        int B, int S, int C, int D, void* stream) {
    return ph_forward(x, W, b, wr, scratch, logits, B, S, C, D, false, stream);
}

extern "C" int cpc_phone_head_backward(const float* x, const float* wr, const float* dlogits, float* scratch, float* dW,
                                       float* db, float* dX, int B, int S, int C, void* stream) {
    return ph_backward(x, wr, dlogits, scratch, dW, db, dX, B, S, C, kC, true, stream);
}

extern "C" int cpc_phone_head_backward_d(const float* x, const float* wr, const float* dlogits, float* scratch, float* dW,
                                         float* db, float* dX, int B, int S, int C, int D, void* stream) {
    return ph_backward(x, wr, dlogits, scratch, dW, db, dX, B, S, C, D, false, stream);
}
