// The feed-forward prediction networks of the reference's criterion (cpc/criterion/criterion.py:11-41,69-81, --rnnMode ffd /
// conv4 / conv8 / conv12) as ONE kernel family: a grouped causal convolution over the time axis, G heads, 256 -> 256 channels,
// ks taps, with the equalized-layer constant (custom_layers.py: the wrapped module's OUTPUT, bias included, times
// sqrt(2 / fan_in)) and an optional ReLU in the epilogue.  ffd is the same operation with ks = 1, run twice.
//
//   y[b, t, g 256 + o] = act( scale * ( bias[g][o] + sum_{j<ks} sum_{i<256} x_g[b, t - (ks-1) + j, i] W[g][o][i][j] ) )
//
// x_g is x (B, W, 256) for every head (`shared`) or columns g 256 .. of x (B, W, G 256); frames in front of the window read as
// zero (gemm_tile.h: RowMap with tmul = 1, tadd = -(ks-1), Lin = W -- no pad buffer); y is written in the (B, W, G 256) layout
// the score kernels read: no transposes, no cat.
//
//   forward    wr[g][o][j 256 + i] = W[g][o][i][j]           pc_relayout_kernel<false>: the weight K-major over a window's floats
//              y  = windows wr^T                             pc_fwd_kernel: NT tile; shared input: one K = ks 256 walk over the
//                                                            contiguous window; per-head input: ks walks of 256
//   backward   dym[g][b, t, o] = dy[b, t, g 256 + o]         pc_dym_kernel: head-major, so that a head's frames are contiguous
//                                (0 where relu and y <= 0)   rows; the ReLU mask on the way
//              part[z][g][j][o][i] = dym_g^T x_g(tap j)      pc_dw_kernel: TN tile per (row slab z, head, tap, 128 x 128 tile)
//              dbp[z][g][o] = column sums of row slab z      pc_colsum_kernel (rows in order)
//              dW[g][o][i][j] = scale sum_z part, db likewise   pc_wsum_kernel: slabs in slab order, torch's Conv1d layout
//              wt[g][i][j' 256 + o] = W[g][o][i][ks-1-j']    pc_relayout_kernel<true>
//              dx[b, t, :] = scale sum_g sum_{j'} dym_g[b, t + j', :] wt[g][:, j', :]^T
//                                                            pc_dx_kernel: per head one K = ks 256 walk over the frames
//                                                            t .. t + ks-1 (frames behind the item read as zero); the shared
//                                                            input's sum over heads runs in ONE accumulator, head after head --
//                                                            where the row tiles alone cannot fill the chip, over `nsplit`
//                                                            groups of consecutive heads whose partial dx pc_dxsum_kernel adds
//                                                            in group order
// Arithmetic: the library's fp32 level.  cpc_set_mfma_mode(0): exact-f32 MFMA tiles (NtTile / TnTile); otherwise (the
// library's default) the same products on three bf16 pieces per operand, six MFMAs per product (NtTileX3 / TnTileX3,
// gemm_tile.h: no operand bounds needed), as cpc_gemm_nt / cpc_gemm_tn do.
// No float atomics, fixed summation orders: identical calls give identical bits, and a batch item's outputs do not depend on
// the items around it (rows never read across an item's first or last frame).
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"

namespace cpc {

constexpr int kPcMaxG = 64, kPcMaxTaps = 16;
constexpr int kPcW = kC * kC;                        // floats of one head's weight per tap
constexpr int kPcMaxSlabs = 16;                      // row slabs of the weight gradient
constexpr int kPcMinSlabRows = 64;
constexpr int kPcMaxBiasSlabs = 64;                  // row slabs of the bias gradient
constexpr int kPcFill = 192;                         // workgroups from which the large tile is taken instead of 64 x 64
constexpr int kPcMaxSplit = 8;                       // head groups of the shared input's dx

using PcBig = NtTile<128, 128, 2, 2>;                // exact-f32 MFMA
using PcSmall = NtTile<64, 64, 2, 2>;
using PcTn = TnTile<128, 128, 2, 2>;
using PcBigX3 = NtTileX3<128, 256, 2, 4, 16, 2, true, false, 3>;     // three bf16 pieces: the pipelined 128 x 256 tile
using PcSmallX3 = NtTileX3<64, 64, 2, 2>;
using PcTnX3 = TnTileX3<128, 128, 2, 2>;

struct PcLayout {
    int M, Z, rows, Zb, rows_b;
    int nsplit, hpg;         // shared dx: head groups and heads per group
    long y, wr, wt, dym, part, dbp, dxp, scratch;
};

static int pc_layout(int B, int W, int G, int ks, PcLayout* o) {
    CPC_RETURN_IF(B < 1 || W < 1 || G < 1 || G > kPcMaxG || ks < 1 || ks > kPcMaxTaps, CPC_ERR_SHAPE);
    const long M = (long)B * W;
    CPC_RETURN_IF(M * G * kC >= (1L << 31), CPC_ERR_SHAPE);
    o->M = (int)M;
    o->y = M * G * kC;
    o->wr = (long)G * ks * kPcW;
    // row slabs of dW: enough (slab, head, tap, tile) workgroups to fill the chip, never fewer than kPcMinSlabRows rows each
    const int tiles = G * ks * 4;
    int Z = cdiv(512, tiles);
    Z = Z > kPcMaxSlabs ? kPcMaxSlabs : Z;
    int rows = cdiv(cdiv(M, Z), 32) * 32;
    rows = rows < kPcMinSlabRows ? kPcMinSlabRows : rows;
    o->rows = rows;
    o->Z = cdiv(M, rows);
    // ... of db: a column sum walks its rows one after the other, so many short slabs
    int Zb = cdiv(M, 32);
    Zb = Zb > kPcMaxBiasSlabs ? kPcMaxBiasSlabs : Zb;
    o->rows_b = cdiv(M, Zb);
    o->Zb = cdiv(M, o->rows_b);
    // head groups of the shared input's dx: only where the large tile is taken (pc_large) and its row tiles leave CUs idle
    const int rt = cdiv(M, 128);
    int ns = 1;
    if ((long)rt * (G < kPcMaxSplit ? G : kPcMaxSplit) >= kPcFill) {
        ns = cdiv(256, rt);
        ns = ns > kPcMaxSplit ? kPcMaxSplit : ns;
        ns = ns > G ? G : ns;
    }
    o->hpg = cdiv(G, ns);
    o->nsplit = cdiv(G, o->hpg);
    o->wt = 0;
    o->dym = o->wt + align64l(o->wr);
    o->part = o->dym + align64l(o->y);
    o->dbp = o->part + align64l((long)o->Z * o->wr);
    o->dxp = o->dbp + align64l((long)o->Zb * G * kC);
    o->scratch = o->dxp + (o->nsplit > 1 ? align64l((long)o->nsplit * M * kC) : 0);
    return 0;
}

// does a product of `wgs128` 128-row tiles (x heads or head groups) take the large tile?
static inline bool pc_large(long wgs128, bool x3) { return wgs128 * (x3 ? 1 : 2) >= kPcFill; }

// FLIPPED false: wr[g][o][j 256 + i] = W[g][o][i][j];  true: wt[g][i][j' 256 + o] = W[g][o][i][ks-1-j']
template <bool FLIPPED>
__global__ __launch_bounds__(256) void pc_relayout_kernel(const float* __restrict__ w, float* __restrict__ out, int ks, long n) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int per = ks * kPcW;
    const int g = (int)(idx / per), rem = (int)(idx - (long)g * per);
    const int r = rem / (ks * kC), jc = rem - r * (ks * kC);        // output row, (tap, column)
    const int jj = jc >> kCLog2, c = jc & (kC - 1);
    const int o = FLIPPED ? c : r, i = FLIPPED ? r : c, j = FLIPPED ? ks - 1 - jj : jj;
    out[idx] = w[(long)g * per + ((long)o * kC + i) * ks + j];
}

struct PcArgs {
    const float* x;        // forward: the input; dx: dym
    const float* wk;       // wr (forward) / wt (dx)
    const float* bias;
    float* out;
    long out_zs;           // dx: floats between the outputs of blockIdx.z (a head's columns, or a head group's partial)
    int ldo;               // dx: row pitch of the output
    int B, W, G, ks, shared, relu, hpg;
    float scale;
};

// rows (b, t) over frames of `ldx` floats: element k of a row is column col0 + (k & 255) of frame t + shift + (k >> 8) of item
// b, zero outside the item's W frames
__device__ __forceinline__ RowMap pc_rows(const float* x, int B, int W, int ldx, int col0, int shift) {
    RowMap r;
    r.base = x; r.R = W; r.bstride = (long)W * ldx; r.rstride = ldx; r.off = shift * ldx + col0;
    r.tmul = 1; r.tadd = shift; r.Lin = W; r.M = B * W;
    return r;
}

// grid (row tiles, 256 / BN column tiles, G)
template <class Nt, int BM, int BN>
__global__ __launch_bounds__(Nt::NTHREADS) void pc_fwd_kernel(PcArgs p) {
    __shared__ float smem[Nt::SMEM_FLOATS];
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, g = blockIdx.z;
    const int M = p.B * p.W, K = p.ks * kC;
    const float* wg = p.wk + (long)g * p.ks * kPcW;
    f32x16 acc[Nt::TM][Nt::TN];
    zero_acc(acc);
    if (p.shared) {            // the ks frames of a window are contiguous: one walk over K = ks 256
        const RowMap am = pc_rows(p.x, p.B, p.W, kC, 0, -(p.ks - 1));
        Nt::run(acc, am, m0, wg, K, n0, K, smem);
    } else {
        for (int j = 0; j < p.ks; ++j) {
            const RowMap am = pc_rows(p.x, p.B, p.W, p.G * kC, g * kC, j - (p.ks - 1));
            Nt::run(acc, am, m0, wg + j * kC, K, n0, kC, smem);
        }
    }
    const long ldy = (long)p.G * kC;
#pragma unroll
    for (int tn = 0; tn < Nt::TN; ++tn) {
        const int col = n0 + Nt::c_col(tn);
        const float bv = p.bias[g * kC + col];
#pragma unroll
        for (int tm = 0; tm < Nt::TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + Nt::c_row(tm, r);
                if (m < M) {
                    float v = (acc[tm][tn][r] + bv) * p.scale;
                    if (p.relu) v = fmaxf(v, 0.f);
                    p.out[(long)m * ldy + g * kC + col] = v;
                }
            }
    }
}

// grid (row tiles, 256 / BN column tiles, shared ? head groups : G)
template <class Nt, int BM, int BN>
__global__ __launch_bounds__(Nt::NTHREADS) void pc_dx_kernel(PcArgs p) {
    __shared__ float smem[Nt::SMEM_FLOATS];
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, z = blockIdx.z;
    const int M = p.B * p.W, K = p.ks * kC;
    const int g0 = p.shared ? z * p.hpg : z, g1 = p.shared ? min(p.G, g0 + p.hpg) : g0 + 1;
    f32x16 acc[Nt::TM][Nt::TN];
    zero_acc(acc);
    for (int g = g0; g < g1; ++g) {                // frame t + j' saw frame t at tap ks-1-j': a window FORWARD in time
        const RowMap am = pc_rows(p.x + (long)g * M * kC, p.B, p.W, kC, 0, 0);
        Nt::run(acc, am, m0, p.wk + (long)g * p.ks * kPcW, K, n0, K, smem);
    }
    float* out = p.out + z * p.out_zs;
#pragma unroll
    for (int tn = 0; tn < Nt::TN; ++tn) {
        const int col = n0 + Nt::c_col(tn);
#pragma unroll
        for (int tm = 0; tm < Nt::TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + Nt::c_row(tm, r);
                if (m < M) out[(long)m * p.ldo + col] = acc[tm][tn][r] * p.scale;
            }
    }
}

// dx = the head groups' partials in group order
__global__ __launch_bounds__(256) void pc_dxsum_kernel(const float* __restrict__ dxp, float* __restrict__ dx, long n, int nsplit) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = dxp[i];
    for (int z = 1; z < nsplit; ++z) s += dxp[(long)z * n + i];
    dx[i] = s;
}

// dym[g][m][o] = dy[m][g 256 + o], 0 where relu and y <= 0
__global__ __launch_bounds__(256) void pc_dym_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                     float* __restrict__ dym, int M, int G, int relu) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)M * G * kC;
    if (i >= n) return;
    const int ld = G * kC;
    const int m = (int)(i / ld), rem = (int)(i - (long)m * ld);
    const int g = rem >> kCLog2, o = rem & (kC - 1);
    float v = dy[i];
    if (relu) v = y[i] > 0.f ? v : 0.f;
    dym[((long)g * M + m) * kC + o] = v;
}

// grid (G, Zb): dbp[z][g][o] = sum over the rows of slab z of dym[g][m][o], rows in order
__global__ __launch_bounds__(256) void pc_colsum_kernel(const float* __restrict__ dym, float* __restrict__ dbp, int M, int G,
                                                        int rows) {
    const int g = blockIdx.x, z = blockIdx.y, o = threadIdx.x;
    const int r0 = z * rows, r1 = min(M, r0 + rows);
    const float* p = dym + (long)g * M * kC + o;
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += p[(long)r * kC];
    dbp[((long)z * G + g) * kC + o] = s;
}

// grid (4 Z, ks, G): slab z = blockIdx.x / 4 of part[z][g][j] (256 x 256: o x i), 128 x 128 tile blockIdx.x % 4
template <class Tn>
__global__ __launch_bounds__(256) void pc_dw_kernel(const float* __restrict__ dym, const float* __restrict__ x,
                                                    float* __restrict__ part, int B, int W, int G, int ks, int shared, int rows) {
    __shared__ float smem[Tn::SMEM_FLOATS];
    const int tile = blockIdx.x & 3, z = blockIdx.x >> 2, j = blockIdx.y, g = blockIdx.z;
    const int c0 = (tile >> 1) * 128, n0 = (tile & 1) * 128;
    const int M = B * W, mbeg = z * rows, mend = min(M, mbeg + rows);
    RowMap am;
    am.base = dym + (long)g * M * kC; am.R = M; am.bstride = 0; am.rstride = kC; am.off = 0;
    am.tmul = 0; am.tadd = 0; am.Lin = 0x7fffffff; am.M = M;
    const RowMap bm = shared ? pc_rows(x, B, W, kC, 0, j - (ks - 1)) : pc_rows(x, B, W, G * kC, g * kC, j - (ks - 1));
    f32x16 acc[Tn::TM][Tn::TN];
    zero_acc(acc);
    Tn::run(acc, am, c0, bm, n0, mbeg, mend, smem);
    float* out = part + (((long)z * G + g) * ks + j) * kPcW;
#pragma unroll
    for (int tm = 0; tm < Tn::TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = c0 + Tn::c_row(tm, r);
#pragma unroll
            for (int tn = 0; tn < Tn::TN; ++tn) out[(long)row * kC + n0 + Tn::c_col(tn)] = acc[tm][tn][r];
        }
}

// dW[g][o][i][j] = scale sum_z part[z][g][j][o][i], db[g][o] = scale sum_z dbp[z][g][o]: slabs in slab order
__global__ __launch_bounds__(256) void pc_wsum_kernel(const float* __restrict__ part, const float* __restrict__ dbp,
                                                      float* __restrict__ dW, float* __restrict__ db, int G, int ks, int Z,
                                                      int Zb, float scale) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long nw = (long)G * ks * kPcW;
    if (idx < nw) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += part[(long)z * nw + idx];
        const int per = ks * kPcW;
        const int g = (int)(idx / per), rem = (int)(idx - (long)g * per);
        const int j = rem / kPcW, oi = rem - j * kPcW;
        dW[(long)g * per + (long)oi * ks + j] = s * scale;
    } else if (idx < nw + G * kC) {
        const int c = (int)(idx - nw);
        float s = 0.f;
        for (int z = 0; z < Zb; ++z) s += dbp[(long)z * G * kC + c];
        db[c] = s * scale;
    }
}

static int pc_launch_fwd(const PcArgs& p, int M, hipStream_t st) {
    const bool x3 = g_mfma_mode != 0;
    const bool large = pc_large((long)cdiv(M, 128) * p.G, x3);
    if (x3 && large)
        hipLaunchKernelGGL((pc_fwd_kernel<PcBigX3, 128, 256>), dim3(cdiv(M, 128), 1, p.G), dim3(PcBigX3::NTHREADS), 0, st, p);
    else if (x3)
        hipLaunchKernelGGL((pc_fwd_kernel<PcSmallX3, 64, 64>), dim3(cdiv(M, 64), 4, p.G), dim3(PcSmallX3::NTHREADS), 0, st, p);
    else if (large)
        hipLaunchKernelGGL((pc_fwd_kernel<PcBig, 128, 128>), dim3(cdiv(M, 128), 2, p.G), dim3(PcBig::NTHREADS), 0, st, p);
    else
        hipLaunchKernelGGL((pc_fwd_kernel<PcSmall, 64, 64>), dim3(cdiv(M, 64), 4, p.G), dim3(PcSmall::NTHREADS), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int pc_launch_dx(const PcArgs& p, int M, int nz, bool large, hipStream_t st) {
    const bool x3 = g_mfma_mode != 0;
    if (x3 && large)
        hipLaunchKernelGGL((pc_dx_kernel<PcBigX3, 128, 256>), dim3(cdiv(M, 128), 1, nz), dim3(PcBigX3::NTHREADS), 0, st, p);
    else if (x3)
        hipLaunchKernelGGL((pc_dx_kernel<PcSmallX3, 64, 64>), dim3(cdiv(M, 64), 4, nz), dim3(PcSmallX3::NTHREADS), 0, st, p);
    else if (large)
        hipLaunchKernelGGL((pc_dx_kernel<PcBig, 128, 128>), dim3(cdiv(M, 128), 2, nz), dim3(PcBig::NTHREADS), 0, st, p);
    else
        hipLaunchKernelGGL((pc_dx_kernel<PcSmall, 64, 64>), dim3(cdiv(M, 64), 4, nz), dim3(PcSmall::NTHREADS), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_pred_conv_layout(int B, int W, int G, int ks, long* sizes) {
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    PcLayout ly;
    const int rc = pc_layout(B, W, G, ks, &ly);
    if (rc) return rc;
    sizes[0] = ly.wr;
    sizes[1] = ly.scratch;
    sizes[2] = ly.y;
    return 0;
}

extern "C" int cpc_pred_conv_forward(const float* x, const float* w, const float* bias, float* wr, float* y, int B, int W, int G,
                                     int ks, int shared, float scale, int relu, void* stream) {
    PcLayout ly;
    const int rc = pc_layout(B, W, G, ks, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !w || !bias || !wr || !y, CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_relayout_kernel<false>, dim3((unsigned)((ly.wr + 255) / 256)), dim3(256), 0, st, w, wr, ks, ly.wr);
    CPC_LAUNCH_CHECK();
    PcArgs p{};
    p.x = x; p.wk = wr; p.bias = bias; p.out = y;
    p.B = B; p.W = W; p.G = G; p.ks = ks; p.shared = shared ? 1 : 0; p.relu = relu ? 1 : 0;
    p.scale = scale;
    return pc_launch_fwd(p, ly.M, st);
}

extern "C" int cpc_pred_conv_backward(const float* x, const float* w, const float* y, const float* dy, float* scratch, float* dw,
                                      float* db, float* dx, int B, int W, int G, int ks, int shared, float scale, int relu,
                                      void* stream) {
    PcLayout ly;
    const int rc = pc_layout(B, W, G, ks, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !w || !dy || !scratch || !dw || !db || (relu && !y), CPC_ERR_ARG);
    const hipStream_t st = (hipStream_t)stream;
    const bool x3 = g_mfma_mode != 0;
    float* dym = scratch + ly.dym;
    hipLaunchKernelGGL(pc_dym_kernel, dim3((unsigned)((ly.y + 255) / 256)), dim3(256), 0, st, dy, y, dym, ly.M, G, relu ? 1 : 0);
    CPC_LAUNCH_CHECK();
    if (x3)
        hipLaunchKernelGGL(pc_dw_kernel<PcTnX3>, dim3(4 * ly.Z, ks, G), dim3(256), 0, st, dym, x, scratch + ly.part, B, W, G, ks,
                           shared ? 1 : 0, ly.rows);
    else
        hipLaunchKernelGGL(pc_dw_kernel<PcTn>, dim3(4 * ly.Z, ks, G), dim3(256), 0, st, dym, x, scratch + ly.part, B, W, G, ks,
                           shared ? 1 : 0, ly.rows);
    CPC_LAUNCH_CHECK();
    hipLaunchKernelGGL(pc_colsum_kernel, dim3(G, ly.Zb), dim3(256), 0, st, dym, scratch + ly.dbp, ly.M, G, ly.rows_b);
    CPC_LAUNCH_CHECK();
    const long n = ly.wr + (long)G * kC;
    hipLaunchKernelGGL(pc_wsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scratch + ly.part, scratch + ly.dbp,
                       dw, db, G, ks, ly.Z, ly.Zb, scale);
    CPC_LAUNCH_CHECK();
    if (dx) {
        hipLaunchKernelGGL(pc_relayout_kernel<true>, dim3((unsigned)((ly.wr + 255) / 256)), dim3(256), 0, st, w, scratch + ly.wt,
                           ks, ly.wr);
        CPC_LAUNCH_CHECK();
        PcArgs p{};
        p.x = dym; p.wk = scratch + ly.wt;
        p.B = B; p.W = W; p.G = G; p.ks = ks; p.shared = shared ? 1 : 0;
        p.scale = scale;
        int r2;
        if (shared) {              // the sum over heads inside the call: one group, or nsplit partials added in group order
            const bool large = ly.nsplit > 1 || pc_large((long)cdiv(ly.M, 128), x3);
            const int ns = large ? ly.nsplit : 1;
            p.hpg = ns > 1 ? ly.hpg : G;
            p.out = ns > 1 ? scratch + ly.dxp : dx;
            p.out_zs = (long)ly.M * kC; p.ldo = kC;
            r2 = pc_launch_dx(p, ly.M, ns, large, st);
            if (r2) return r2;
            if (ns > 1) {
                const long nx = (long)ly.M * kC;
                hipLaunchKernelGGL(pc_dxsum_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, scratch + ly.dxp, dx, nx, ns);
                CPC_LAUNCH_CHECK();
            }
        } else {
            p.hpg = 1; p.out = dx; p.out_zs = kC; p.ldo = G * kC;
            r2 = pc_launch_dx(p, ly.M, G, pc_large((long)cdiv(ly.M, 128) * G, x3), st);
            if (r2) return r2;
        }
    }
    return 0;
}
