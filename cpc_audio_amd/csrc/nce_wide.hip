// InfoNCE scores at any encoder width: the plain (exact-f32) scores path of nce.hip -- nce_fwd_kernel, nce_bwd_dpred_kernel,
// nce_bwd_dz_rows_kernel, nce_gather_rows_kernel -- with the channel axis as a parameter.
//
// Reference: cpc/criterion/criterion.py
//   :89-95,108-116   pred_k from any prediction network of width C = dimOutputEncoder; score = mean over the C features
//   :174-219         negatives drawn once, shared by the heads; positive of head k is z[b, t+k]
//   :248-257         CE(target 0) averaged over the B*W rows; acc = [argmax == 0] averaged
//
// The kernels work on the PADDED width Cp = C rounded up to a multiple of 64 (one block = 16 lanes x float4): z is
// (B, S, Cp), pred (B*W, K*Cp), columns C .. Cp-1 zero.  Zero padding is self-consistent -- it adds nothing to any dot
// product, and dpred = dS . Cand and V = dS^T . P are exactly zero there because Cand and P are -- so no kernel masks columns.
// The true C enters as the divisor of the mean (inv_c) and in the gradient scale gloss / (B*W*C) only.
//
// One wavefront per window (b, t), as in nce.hip.  Forward: P[16 heads x Cp] . Cand^T[Cp x 16] on v_mfma_f32_16x16x4_f32 with
// the prediction fragments of the whole width in registers (4 NB float4 per lane, NB = Cp / 64 = 1 .. 8: one instantiation
// per NB); candidate rows are gathered four blocks at a time through the wave's 4 KB LDS transpose tile.  Backward: dPred and
// the per-candidate rows V are independent per column block, so both walk the blocks outermost (four per pass, a pass per
// launch: the accumulators of nce.hip's kernels) and their register count does not grow with the width.  dz = destination-sorted gather of
// the V rows (perm, row_ptr of cpc_nce_prepare): no float atomics, rank-sorted slot lists, bit-reproducible.
// Every offset into V, logits, pred and z is 64-bit (V holds B*W*(N+K)*Cp floats: 2.1e9 at B = 256, W = 116, N = 128, C = 512).
#include <algorithm>
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"

namespace cpc {

__device__ __forceinline__ float4 wld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Sixteen rows x up to four 64-float column blocks, loaded the coalesced way (lane (c = lane & 15, r4 = lane >> 4) reads
// piece c of rows 4 q + r4) and handed out as MFMA fragments whose non-contracted index is the row, through a 16 x 16
// transpose of 16-byte pieces in a 4 KB LDS tile per wave (slot row * 16 + (chunk ^ row): no bank conflicts) -- Gather16 of
// nce.hip with the first block and the block count as parameters.
template <int NB>
struct GatherW {
    float4 v[4][4];                                   // [q][g]: piece c of row 4 q + r4, column block g0 + g
    __device__ __forceinline__ void issue(const float* const (&rowp)[4], int g0) {     // rowp[q]: row 4 q + r4, + 4 c floats
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g0 + g < NB) v[q][g] = wld4(rowp[q] + 64 * (g0 + g));
    }
    // fragments of block g0 + g (e = 0..3: floats 16 e + 4 r4 .. of the block) of row c; convergent: the whole wave calls it
    __device__ __forceinline__ void block(int g, float4* tile, float4 (&out)[4]) const {
        const int lane = threadIdx.x & 63, c = lane & 15, r4 = lane >> 4;
        __builtin_amdgcn_wave_barrier();                // the previous block's reads are done
#pragma unroll
        for (int q = 0; q < 4; ++q) tile[(4 * q + r4) * 16 + (c ^ (4 * q + r4))] = v[q][g];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = tile[c * 16 + ((4 * e + r4) ^ c)];
    }
};

// ------------------------------------------------------------------ forward scores
// pred: [BW][K * Cp]; z: [B*S][Cp]; ext: [BW][N] row ids into z (N a multiple of 16, entries >= Nv are padding).
// NB <= 4 keeps nce_fwd_kernel's three waves per SIMD; above, the 4 NB fragments (up to 128 VGPRs) take two.
template <int NB>
__global__ __launch_bounds__(256, (NB <= 4 ? 3 : 2)) void nce_wide_fwd_kernel(
    const float* __restrict__ pred, const float* __restrict__ z, const int* __restrict__ ext,
    float* __restrict__ logits, float* __restrict__ lse_out, float* __restrict__ rowstat, int BW, int W,
    int S, int K, int N, int Nv, int koff, float inv, unsigned* __restrict__ ticket) {
    constexpr int Cp = 64 * NB;
    __shared__ float4 tiles[4][256];
    const int lane = threadIdx.x & 63;
    const int bt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;      // nce_wide_reduce_finalize_kernel, the next launch on this stream
    if (bt >= BW) return;                           // whole wave leaves together
    float4* tile = tiles[threadIdx.x >> 6];
    const int b = bt / W, t = bt - b * W;
    const int i = lane & 15, kq = lane >> 4;        // i: head (and candidate row of the A operand); kq: k group
    const bool hv = i < K;
    GatherW<NB> gt;
    const float* rowp[4];

    float4 pa[4 * NB];                              // pred[head i][16 ii + 4 kq ..]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int head = 4 * q + kq;
        rowp[q] = pred + ((long)bt * K + (head < K ? head : 0)) * Cp + 4 * i;
    }
#pragma unroll
    for (int g0 = 0; g0 < NB; g0 += 4) {
        gt.issue(rowp, g0);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g0 + g < NB) {
                float4 o[4];
                gt.block(g, tile, o);
#pragma unroll
                for (int e = 0; e < 4; ++e) pa[4 * (g0 + g) + e] = hv ? o[e] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
    }
    // scores of the 16 rows rowp names against the heads: ONE accumulator over all column blocks.  The positives go through the
    // same chain as the negatives (a tile whose row j is head j's positive; the diagonal is kept), so a negative that is the
    // positive row scores bit-identically and the arg-max tie resolves to class 0 as in the reference (criterion.py:253).
    auto score_tile = [&]() __attribute__((always_inline)) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g0 = 0; g0 < NB; g0 += 4) {
            gt.issue(rowp, g0);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g0 + g < NB) {
                    float4 zf[4];
                    gt.block(g, tile, zf);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(zf[e], jj), f4c(pa[4 * (g0 + g) + e], jj), acc, 0, 0, 0);
                }
        }
        return acc;
    };
    float posl;
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int head = 4 * q + kq;
            rowp[q] = z + ((long)b * S + t + koff + (head < K ? head : 0) + 1) * Cp + 4 * i;
        }
        const f32x4 acc = score_tile();
        // acc[r] on lane (i, q) = score(positive row of head 4q+r, head i); the diagonal sits on lane (i, i >> 2), reg i & 3
        const float mine = (i & 3) == 0 ? acc[0] : (i & 3) == 1 ? acc[1] : (i & 3) == 2 ? acc[2] : acc[3];
        posl = __shfl(mine, i + 16 * (i >> 2)) * inv;
    }
    float M = posl;                                 // reference of the softmax weights, common to the four lanes of a head
    float ssum = kq == 0 ? 1.0f : 0.0f;             // the positive enters the sum once (exp(posl - M) = 1)
    float mneg = -3.0e38f;
    for (int nt = 0; nt < N / 16; ++nt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rowp[q] = z + (long)ext[(long)bt * N + nt * 16 + 4 * q + kq] * Cp + 4 * i;
        const f32x4 acc = score_tile();
        // acc[r] = score of head i against negative nt*16 + 4 kq + r (padding candidates -- index >= Nv -- weigh nothing)
        float l[4], lmax = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            l[r] = nt * 16 + 4 * kq + r < Nv ? acc[r] * inv : -3.0e38f;
            if (hv) logits[((long)bt * K + i) * (N + 1) + 1 + nt * 16 + 4 * kq + r] = l[r];
            lmax = fmaxf(lmax, l[r]);
        }
        mneg = fmaxf(mneg, lmax);
        if (__any(lmax - M > 40.0f)) {              // (wave-uniform) move the reference: rare
            float tm = fmaxf(lmax, __shfl_xor(lmax, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const float Mn = fmaxf(M, tm), alpha = expf(M - Mn);
            ssum *= alpha;
            M = Mn;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ssum += expf(l[r] - M);
    }
    // fold the four k groups of a head
    ssum += __shfl_xor(ssum, 16);
    ssum += __shfl_xor(ssum, 32);
    mneg = fmaxf(mneg, __shfl_xor(mneg, 16));
    mneg = fmaxf(mneg, __shfl_xor(mneg, 32));
    const float lse = M + logf(ssum);
    if (kq == 0 && hv) {
        logits[((long)bt * K + i) * (N + 1)] = posl;
        lse_out[(long)bt * K + i] = lse;
        rowstat[(long)bt * 2 * K + i] = lse - posl;                       // CE(target 0)
        rowstat[(long)bt * 2 * K + K + i] = posl >= mneg ? 1.f : 0.f;     // argmax == 0
    }
}

// Column sums of rowstat [nrows][n <= 32] -> losses / accuracies in ONE launch (nce_reduce_finalize_kernel of nce.hip): block g
// sums its rows_per_group rows into tmp[g], takes a ticket, and the block that draws the last ticket folds the groups in a
// fixed order and scales.  `ticket` was cleared by the scoring kernel.  No spinning: a block that is not the last one leaves.
__global__ __launch_bounds__(256) void nce_wide_reduce_finalize_kernel(const float* __restrict__ rowstat, int nrows, int n,
                                                                      int rows_per_group, float* __restrict__ tmp,
                                                                      unsigned* __restrict__ ticket, float* __restrict__ losses,
                                                                      float* __restrict__ acc, int K, float inv_rows) {
    __shared__ float red[8][33];
    __shared__ unsigned drawn;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    auto fold = [&](auto load, int r0, int r1) __attribute__((always_inline)) {      // rows r0..r1-1 of one column
        float s0 = 0.f, s1 = 0.f;
        if (tx < n) {
            int r = r0 + ty;
            for (; r + 8 < r1; r += 16) {
                s0 += load(r);
                s1 += load(r + 8);
            }
            if (r < r1) s0 += load(r);
        }
        red[ty][tx] = s0 + s1;
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += red[q][tx];
        __syncthreads();
        return s;
    };
    const int r0 = blockIdx.x * rows_per_group;
    const float mine = fold([&](int r) { return rowstat[(long)r * n + tx]; }, r0, min(nrows, r0 + rows_per_group));
    if (ty == 0 && tx < n) tmp[(long)blockIdx.x * n + tx] = mine;
    __threadfence();                                    // my group's sums are visible device-wide before my ticket is
    __syncthreads();
    if (threadIdx.x == 0) drawn = atomicAdd(ticket, 1u);
    __syncthreads();
    if (drawn != gridDim.x - 1) return;
    __threadfence();
    const float total = fold([&](int g) { return __hip_atomic_load(tmp + (long)g * n + tx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
                             0, (int)gridDim.x);
    if (ty == 0 && tx < n) {
        if (tx < K) losses[tx] = total * inv_rows;
        else if (tx < 2 * K) acc[tx - K] = total * inv_rows;
    }
}

// gscale[k] = dL/dloss_k / (B*W) / C
__global__ __launch_bounds__(64) void nce_wide_gscale_kernel(const float* __restrict__ gloss, float* __restrict__ gscale, int K,
                                                             float f) {
    const int k = threadIdx.x;
    if (k < 16) gscale[k] = k < K ? gloss[k] * f : 0.f;
}

// ------------------------------------------------------------------ backward: dPred = dS . Cand
// nce_bwd_dpred_kernel with the column blocks outermost, four per pass (the same 16 accumulators whatever the width); the
// score gradients of a pass are recomputed from the saved logits.  A pass is a launch of its own: PB <= 4 blocks starting at
// column c0 of the Cp-wide rows (PB = 4, one pass, is nce_bwd_dpred_kernel's loop; 512 channels are two such launches, which
// write disjoint columns).
template <int PB>
__global__ __launch_bounds__(256, 3) void nce_wide_bwd_dpred_kernel(
    const float* __restrict__ z, const int* __restrict__ ext, const float* __restrict__ logits,
    const float* __restrict__ lse, const float* __restrict__ gscale, float* __restrict__ dpred, int BW,
    int W, int S, int K, int N, int koff, int Cp, int c0) {
    const int lane = threadIdx.x & 63;
    const int bt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bt >= BW) return;
    const int b = bt / W, t = bt - b * W;
    const int i = lane & 15, kq = lane >> 4;
    const bool hv = i < K;
    const float gs = hv ? gscale[i] : 0.f;
    const float ls = hv ? lse[(long)bt * K + i] : 0.f;
    const float* lp = logits + ((long)bt * K + (hv ? i : 0)) * (N + 1) + 1 + 4 * kq;
    const int* ep = ext + (long)bt * N + 4 * kq;
    {
        constexpr int nb = PB;
        f32x4 acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ii = 0; ii < N / 16; ++ii) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float a = hv ? gs * expf(lp[16 * ii + jj] - ls) : 0.f;   // d score[head i][n], n = 16 ii + 4 kq + jj
                const float* zr = z + (long)ep[16 * ii + jj] * Cp + c0 + 4 * i;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < nb) {
                        const float4 bv = wld4(zr + 64 * u);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[u * 4 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f4c(bv, e), acc[u * 4 + e], 0, 0, 0);
                    }
            }
        }
        // C layout: head = 4kq + r, channel = c0 + 64 u + 4i + e
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int head = 4 * kq + r;
            if (head < K) {
                const float d0 = gscale[head] * (expf(logits[((long)bt * K + head) * (N + 1)] - lse[(long)bt * K + head]) - 1.0f);
                const float* zp = z + ((long)b * S + t + koff + head + 1) * Cp + c0 + 4 * i;
                float* op = dpred + ((long)bt * K + head) * Cp + c0 + 4 * i;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < nb) {
                        const float4 zv = wld4(zp + 64 * u);
                        float4 o;
                        o.x = fmaf(d0, zv.x, acc[u * 4 + 0][r]);
                        o.y = fmaf(d0, zv.y, acc[u * 4 + 1][r]);
                        o.z = fmaf(d0, zv.z, acc[u * 4 + 2][r]);
                        o.w = fmaf(d0, zv.w, acc[u * 4 + 3][r]);
                        *reinterpret_cast<float4*>(op + 64 * u) = o;
                    }
            }
        }
    }
}

// ------------------------------------------------------------------ backward: the per-candidate rows V = dS^T . P
// nce_bwd_dz_rows_kernel, column blocks outermost: slot bt * (N + K) + j (j < N negative j, j >= N positive of head j - N)
// carries d score[.][j] * P[.] as one Cp-float row.  A pass (PB <= 4 blocks from column c0) per launch, as above; three waves
// per SIMD, as nce_bwd_dz_rows_kernel -- which the four-block pass reaches without spilling only with the row pitch a constant,
// hence the second template argument (NB <= 4: <NB, NB>; above: <4, NB> and <NB - 4, NB>).
template <int PB, int NB>
__global__ __launch_bounds__(256, 3) void nce_wide_bwd_dz_rows_kernel(
    const float* __restrict__ pred, const float* __restrict__ logits, const float* __restrict__ lse,
    const float* __restrict__ gscale, float* __restrict__ V, int BW, int K, int N, int c0) {
    constexpr int Cp = 64 * NB;
    const int lane = threadIdx.x & 63;
    const int bt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bt >= BW) return;
    const int i = lane & 15, kq = lane >> 4;
    float gs[4], ls[4];
    const float* lp[4];
#pragma unroll
    for (int sx = 0; sx < 4; ++sx) {
        const int head = 4 * sx + kq;
        const bool hv = head < K;
        gs[sx] = hv ? gscale[head] : 0.f;
        ls[sx] = hv ? lse[(long)bt * K + head] : 0.f;
        lp[sx] = logits + ((long)bt * K + (hv ? head : 0)) * (N + 1);
    }
    {
        constexpr int nb = PB;
        // B operand: P[head 4sx+kq][channels c0 + 64 u + 4i + e]
        float4 pb[4][4];
#pragma unroll
        for (int sx = 0; sx < 4; ++sx) {
            const int head = 4 * sx + kq;
            const bool hv = head < K;
            const float* pp = pred + ((long)bt * K + (hv ? head : 0)) * Cp + c0 + 4 * i;
#pragma unroll
            for (int u = 0; u < 4; ++u) pb[sx][u] = hv && u < nb ? wld4(pp + 64 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float* vrow = V + (long)bt * (N + K) * Cp + c0 + 4 * i;
        for (int nt = 0; nt < N / 16; ++nt) {
            f32x4 acc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) {
                // d score[head 4sx+kq][n = nt*16+i]; exactly 0 for the padding heads (0 * exp(.) would be NaN once a logit of
                // head 0, whose row they alias, exceeds 88)
                const float a = 4 * sx + kq < K ? gs[sx] * expf(lp[sx][1 + nt * 16 + i] - ls[sx]) : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < nb) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[u * 4 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, f4c(pb[sx][u], e), acc[u * 4 + e], 0, 0, 0);
                    }
            }
            // C layout: negative n = nt*16 + 4kq + r, channel = c0 + 64 u + 4i + e
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* dst = vrow + (long)(nt * 16 + 4 * kq + r) * Cp;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < nb) {
                        // streamed: written once and read once by the gather
                        __builtin_nontemporal_store(acc[u * 4 + 0][r], dst + 64 * u);
                        __builtin_nontemporal_store(acc[u * 4 + 1][r], dst + 64 * u + 1);
                        __builtin_nontemporal_store(acc[u * 4 + 2][r], dst + 64 * u + 2);
                        __builtin_nontemporal_store(acc[u * 4 + 3][r], dst + 64 * u + 3);
                    }
            }
        }
        // positives: candidate slot N + head carries d score[head][pos] * P[head]
#pragma unroll
        for (int sx = 0; sx < 4; ++sx) {
            const int head = 4 * sx + kq;
            if (head < K) {
                const float d0 = gs[sx] * (expf(lp[sx][0] - ls[sx]) - 1.0f);
                float* dst = vrow + (long)(N + head) * Cp;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < nb) {
                        float4 o;
                        o.x = d0 * pb[sx][u].x; o.y = d0 * pb[sx][u].y; o.z = d0 * pb[sx][u].z; o.w = d0 * pb[sx][u].w;
                        *reinterpret_cast<float4*>(dst + 64 * u) = o;
                    }
            }
        }
    }
}

// dz[j] = sum of the V rows whose destination is j: slots perm[row_ptr[j] .. row_ptr[j+1]), rank-sorted in LDS first so that
// the summation order is the ascending slot order whatever order the list was filled in (nce_gather_rows_kernel).  One
// workgroup of Cp / 4 threads (16 .. 128) per destination row, 4 channels per thread.
constexpr int kWideMaxSort = 1024;
__global__ __launch_bounds__(128) void nce_wide_gather_rows_kernel(const float* __restrict__ V, const int* __restrict__ perm,
                                                                   const int* __restrict__ row_ptr, float* __restrict__ dz,
                                                                   int Cp) {
    __shared__ int raw[kWideMaxSort];
    __shared__ int sorted[kWideMaxSort];
    const int tid = threadIdx.x, nth = blockDim.x;
    const int j = blockIdx.x;
    const int beg = row_ptr[j], len = row_ptr[j + 1] - beg;
    const bool do_sort = len <= kWideMaxSort;         // (uniform over the workgroup)
    if (do_sort) {
        for (int i = tid; i < len; i += nth) raw[i] = perm[beg + i];
        __syncthreads();
        for (int i = tid; i < len; i += nth) {
            const int e = raw[i];
            int rank = 0;
            for (int q = 0; q < len; ++q) rank += raw[q] < e ? 1 : 0;      // slots are unique
            sorted[rank] = e;
        }
        __syncthreads();
    }
    const int* list = do_sort ? sorted : perm + beg;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    int p = 0;
    auto ldv = [&](const float* q) __attribute__((always_inline)) {      // V is read exactly once: non-temporal
        const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q));
        return make_float4(t.x, t.y, t.z, t.w);
    };
    for (; p + 4 <= len; p += 4) {
        const float4 v0 = ldv(V + (long)list[p] * Cp + 4 * tid);
        const float4 v1 = ldv(V + (long)list[p + 1] * Cp + 4 * tid);
        const float4 v2 = ldv(V + (long)list[p + 2] * Cp + 4 * tid);
        const float4 v3 = ldv(V + (long)list[p + 3] * Cp + 4 * tid);
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
        a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
        a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
    }
    for (; p < len; ++p) {
        const float4 v0 = ldv(V + (long)list[p] * Cp + 4 * tid);
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    }
    float4 o;
    o.x = (a0.x + a1.x) + (a2.x + a3.x);
    o.y = (a0.y + a1.y) + (a2.y + a3.y);
    o.z = (a0.z + a1.z) + (a2.z + a3.z);
    o.w = (a0.w + a1.w) + (a2.w + a3.w);
    *reinterpret_cast<float4*>(dz + (long)j * Cp + 4 * tid) = o;
}

// ------------------------------------------------------------------ host side
struct WideLayout {
    int W, BW, koff, N, Nv, Cp;
    long logits, lse, saved_total;
    long rowstat, tmp, sums, fwd_total;
    long gscale, V, bwd_total;
};

static int padded_width(int C) { return C < 1 || C > 512 ? 0 : (C + 63) & ~63; }

// the shapes of nce_layout (nce.hip: K <= 16 per call, the calling thread's head group, S > the criterion's heads) + the width
static bool wide_layout(int B, int S, int K, int N, int C, WideLayout& n) {
    int k0 = 0, k_total = 0;
    nce_head_group_get(&k0, &k_total);
    const int Ktot = k_total > 0 ? k_total : K;
    if (B <= 0 || K <= 0 || K > 16 || k0 + K > Ktot || S <= Ktot || N <= 0 || padded_width(C) == 0) return false;
    n.Cp = padded_width(C);
    n.Nv = N;
    N = (N + 15) & ~15;
    n.N = N;
    n.koff = k_total > 0 ? k0 : 0;
    n.W = S - Ktot;
    if ((long)B * n.W * (N + K) > 0x7fffffffL || (long)B * S > 0x7fffffffL) return false;     // slots and rows are int32
    n.BW = B * n.W;
    long o = 0;
    n.logits = o; o += align64l((long)n.BW * K * (N + 1));
    n.lse = o; o += align64l((long)n.BW * K);
    n.saved_total = o;
    o = 0;
    n.rowstat = o; o += align64l((long)n.BW * 2 * K);
    n.tmp = o; o += align64l((long)kRowsSumGroups * 2 * K);
    n.sums = o; o += 64;
    n.fwd_total = o;
    o = 0;
    n.gscale = o; o += 64;
    n.V = o; o += align64l((long)n.BW * (N + K) * n.Cp);
    n.bwd_total = o;
    return true;
}

template <int NB>
static void launch_fwd(const WideLayout& n, const float* pred, const float* z, const int* ext, float* saved, float* scratch, int S, int K,
                       float inv_c, hipStream_t st) {
    hipLaunchKernelGGL((nce_wide_fwd_kernel<NB>), dim3(cdiv(n.BW, 4)), dim3(256), 0, st, pred, z, ext, saved + n.logits,
                       saved + n.lse, scratch + n.rowstat, n.BW, n.W, S, K, n.N, n.Nv, n.koff, inv_c,
                       reinterpret_cast<unsigned*>(scratch + n.sums + 32));
}

// one pass of PB column blocks from column c0 of either backward kernel
template <int PB>
static void launch_dpred(const WideLayout& n, const float* z, const int* ext, const float* saved, float* scratch, float* dpred, int S,
                         int K, int c0, hipStream_t st) {
    hipLaunchKernelGGL((nce_wide_bwd_dpred_kernel<PB>), dim3(cdiv(n.BW, 4)), dim3(256), 0, st, z, ext, saved + n.logits, saved + n.lse,
                       scratch + n.gscale, dpred, n.BW, n.W, S, K, n.N, n.koff, n.Cp, c0);
}
template <int PB, int NB>
static void launch_dz_rows_pass(const WideLayout& n, const float* pred, const float* saved, float* scratch, int K, int c0,
                                hipStream_t st) {
    hipLaunchKernelGGL((nce_wide_bwd_dz_rows_kernel<PB, NB>), dim3(cdiv(n.BW, 4)), dim3(256), 0, st, pred, saved + n.logits,
                       saved + n.lse, scratch + n.gscale, scratch + n.V, n.BW, K, n.N, c0);
}
template <int NB>
static void launch_dz_rows(const WideLayout& n, const float* pred, const float* saved, float* scratch, int K, hipStream_t st) {
    if constexpr (NB <= 4) {
        launch_dz_rows_pass<NB, NB>(n, pred, saved, scratch, K, 0, st);
    } else {
        launch_dz_rows_pass<4, NB>(n, pred, saved, scratch, K, 0, st);
        launch_dz_rows_pass<NB - 4, NB>(n, pred, saved, scratch, K, 256, st);
    }
}

// the backward passes: one instantiation per blocks of a pass, 1 .. 4
#define CPC_WIDE_DISPATCH4(pb, fn, ...)         \
    switch (pb) {                               \
        case 1: fn<1>(__VA_ARGS__); break;      \
        case 2: fn<2>(__VA_ARGS__); break;      \
        case 3: fn<3>(__VA_ARGS__); break;      \
        default: fn<4>(__VA_ARGS__); break;     \
    }
// the forward: one instantiation per block count NB = Cp / 64
#define CPC_WIDE_DISPATCH(nb, fn, ...)          \
    switch (nb) {                               \
        case 1: fn<1>(__VA_ARGS__); break;      \
        case 2: fn<2>(__VA_ARGS__); break;      \
        case 3: fn<3>(__VA_ARGS__); break;      \
        case 4: fn<4>(__VA_ARGS__); break;      \
        case 5: fn<5>(__VA_ARGS__); break;      \
        case 6: fn<6>(__VA_ARGS__); break;      \
        case 7: fn<7>(__VA_ARGS__); break;      \
        default: fn<8>(__VA_ARGS__); break;     \
    }

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_nce_wide_padded_width(int C) { return padded_width(C); }

extern "C" int cpc_nce_wide_layout(int B, int S, int K, int N, int C, long* sizes) {
    WideLayout n;
    CPC_RETURN_IF(!wide_layout(B, S, K, N, C, n), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = n.saved_total; sizes[1] = n.fwd_total; sizes[2] = n.bwd_total;
    sizes[3] = n.logits; sizes[4] = n.lse;
    return 0;
}

// pred (B*W, K*Cp), z (B, S, Cp) with Cp = cpc_nce_wide_padded_width(C) and zero columns C ..; ext (B*W, padded N) of
// cpc_nce_prepare.  `saved` keeps logits and lse.
extern "C" int cpc_nce_wide_forward(const float* pred, const float* z, const int* ext, float* saved, float* scratch,
                                    float* losses, float* acc, int B, int S, int K, int N, int C, void* stream) {
    WideLayout n;
    CPC_RETURN_IF(!wide_layout(B, S, K, N, C, n), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!pred || !z || !ext || !saved || !scratch || !losses || !acc, CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const float inv_c = 1.0f / (float)C;
    CPC_WIDE_DISPATCH(n.Cp / 64, launch_fwd, n, pred, z, ext, saved, scratch, S, K, inv_c, st);
    CPC_LAUNCH_CHECK();
    {                                                   // 2 K <= 32 columns: rows_sum's groups and order of additions
        int groups = n.BW > 64 ? kRowsSumGroups : 1;
        const int rpg = cdiv(n.BW, groups);
        groups = cdiv(n.BW, rpg);
        hipLaunchKernelGGL(nce_wide_reduce_finalize_kernel, dim3(groups), dim3(256), 0, st, scratch + n.rowstat, n.BW, 2 * K, rpg,
                           scratch + n.tmp, reinterpret_cast<unsigned*>(scratch + n.sums + 32), losses, acc, K,
                           1.0f / (float)n.BW);
    }
    CPC_LAUNCH_CHECK();
    return 0;
}

// dpred (B*W, K*Cp) and dz (B, S, Cp) are overwritten; their columns C .. come out exactly 0.
extern "C" int cpc_nce_wide_backward(const float* pred, const float* z, const int* ext, const int* perm, const int* row_ptr,
                                     const float* saved, const float* gloss, float* scratch, float* dpred, float* dz,
                                     int B, int S, int K, int N, int C, void* stream) {
    WideLayout n;
    CPC_RETURN_IF(!wide_layout(B, S, K, N, C, n), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!pred || !z || !ext || !perm || !row_ptr || !saved || !gloss || !scratch || !dpred || !dz, CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nce_wide_gscale_kernel, dim3(1), dim3(64), 0, st, gloss, scratch + n.gscale, K,
                       1.0f / ((float)n.BW * (float)C));
    const int NB = n.Cp / 64;
    for (int u0 = 0; u0 < NB; u0 += 4)
        CPC_WIDE_DISPATCH4(std::min(4, NB - u0), launch_dpred, n, z, ext, saved, scratch, dpred, S, K, 64 * u0, st);
    CPC_WIDE_DISPATCH(NB, launch_dz_rows, n, pred, saved, scratch, K, st);
    hipLaunchKernelGGL(nce_wide_gather_rows_kernel, dim3(B * S), dim3(n.Cp / 4), 0, st, scratch + n.V, perm, row_ptr, dz, n.Cp);
    CPC_LAUNCH_CHECK();
    return 0;
}
