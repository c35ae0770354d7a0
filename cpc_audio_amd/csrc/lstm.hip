// CPCAR with mode="LSTM": multi-layer LSTM autoregressor (torch.nn.LSTM semantics, batch_first, gate order i,f,g,o).
//
// Reference: cpc/model.py:167-169 (nn.LSTM(dimEncoded, dimOutput, num_layers, batch_first=True)), the argparse default
// --arMode LSTM --nLevelsGRU 1 (cpc/cpc_default_config.py:74-78); forward with an optional carried (h, c), :185-204.
//
//   i = sigmoid(W_ii x + b_ii + W_hi h + b_hi)    f = sigmoid(W_if x + b_if + W_hf h + b_hf)
//   g = tanh   (W_ig x + b_ig + W_hg h + b_hg)    o = sigmoid(W_io x + b_io + W_ho h + b_ho)
//   c' = f * c + i * g                            h' = o * tanh(c')
//
// Structure (the GRU's, gru.hip, with one recurrent product per step and no second layer in flight):
//   * the input projection of all S steps of a layer is ONE GEMM (nt_gemm, bias_ih folded in);
//   * the recurrence is one PERSISTENT launch per layer: workgroup = (16 sequences) x (16 hidden units) x 4 gates, 4 waves
//     splitting the K = 256 contraction; each wave keeps its 64 x 64 quarter of the workgroup's 64 x 256 W_hh slice in
//     registers for all S steps.  h_{t-1} is polled from y itself while other workgroups write it (persist.h: y pre-filled
//     with the not-ready pattern, agent-scope stores and loads).  The cell state c of (sequence, unit) belongs to one thread of
//     one workgroup for the whole launch, so it never leaves registers;
//   * layers run one after another (any nl in 1..8);
//   * the forward saves the four activated gates (B,S,4H) and c (B,S,H) per layer;
//   * backward (BPTT) mirrors it with K = 1024: dh_t = dy_t + dG_{t+1} . W_hh, the dc chain in registers, the pre-activation
//     gate gradients dG_t handed over through the fill pattern; dx, dW_ih, dW_hh and both bias gradients are batched GEMMs /
//     reductions over the B*S rows afterwards;
//   * per-step kernels (one launch per step, same MFMA and summation order -- bit-identical) serve grids that cannot be
//     co-resident and the CPC_LSTM_PER_STEP flag.
//   * G heads (cpc_lstm_group_*: the criterion's --rnnMode LSTM predictors, cpc/criterion/criterion.py:66-68 -- K one-layer
//     LSTMs reading the same context) lie side by side in the columns of every (B,S,.) array and ride in blockIdx.z of the same
//     four kernels: one GEMM projects the input for all heads, as many whole heads as can be resident share a persistent launch.
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"
#include "persist.h"

namespace cpc {

constexpr int kLH = kC;          // hidden size (256)
constexpr int kLG = 4 * kLH;     // gate rows
constexpr int kLstmSpinLimit = 1 << 20;   // polling budget per wave and launch (re-reads, ~1 us each)

// Set (bit 0) by a wave of the persistent LSTM recurrence that gave up polling; read and cleared by cpc_device_error_flags()
// (capi.hip) as CPC_DEVERR_LSTM_POLL_TIMEOUT.
static __device__ unsigned g_lstm_poll_timeout = 0;

// ------------------------------------------------------------------ forward
struct LstmFwd {
    const float* gx;      // (B,S,4H): W_ih x + b_ih of every step
    const float* whh;     // (4H,H)
    const float* bhh;     // (4H)
    const float* h0;      // (B,H) of this layer or NULL
    const float* c0;      // (B,H) of this layer or NULL
    float* y;             // (B,S,H) this layer's output (persistent launch: pre-filled with kNotReady)
    float* G;             // (B,S,4H) saved activated gates i, f, g, o
    float* C;             // (B,S,H) saved cell state
    float* hN;            // (B,H) of this layer
    float* cN;            // (B,H) of this layer
    int B, S;
    // Groups (heads): ng independent recurrences side by side in the columns of every (B,S,.) array -- head g at columns
    // g * H (g * 4H for gx and G) of rows hs = ng * H (gs = ng * 4H) floats long -- with their W_hh, b_hh one behind the other.
    // A launch runs the heads g0 + blockIdx.z.  One head: ng = 1, g0 = 0 and the strides are the plain H / 4H.
    int ng, g0;
    long hs, gs;
};

// The pointers of head g0 + blockIdx.z (carried and final state exist for ng == 1 only)
__device__ __forceinline__ void lstm_fwd_head(LstmFwd& p) {
    const long g = p.g0 + (int)blockIdx.z;
    p.gx += g * kLG; p.whh += g * kLG * kLH; p.bhh += g * kLG;
    p.y += g * kLH; p.G += g * kLG; p.C += g * kLH;
}

// Lane (i, kq) of wave w holds W_hh[gate * H + j0 + i][koff + 16 ii .. + 4] (koff = 64 w + 4 kq): the B operand of the
// 16 x 16 x 4 MFMAs for k = koff + 16 ii + jj, as the h fragments of the A operand.
__device__ __forceinline__ void lstm_load_whh(float4 (&bw)[4][4], const float* __restrict__ whh, int j0, int i, int koff) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
            bw[g][ii] = *reinterpret_cast<const float4*>(whh + (long)(g * kLH + j0 + i) * kLH + koff + 16 * ii);
}

// This wave's quarter of the recurrent product h_{t-1} . W_hh^T for the 16 x 16 (sequence, unit) tile of each gate, into part[w]
__device__ __forceinline__ void lstm_fwd_mfma(float (&part)[4][4][256], const float4 (&a)[4], const float4 (&bw)[4][4], int w,
                                              int i, int kq) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[ii], jj), f4c(bw[g][ii], jj), acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) part[w][g][(kq * 4 + r) * 16 + i] = acc[r];
    }
}

// Gate math of thread tid = (row, col) = (sequence b, unit j) at step t: c is updated in place, h returned, gates and c saved.
__device__ __forceinline__ float lstm_fwd_gates(const float (&part)[4][4][256], int tid, const LstmFwd& p, long bt, int j,
                                                float& c) {
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        pre[g] = (((part[0][g][tid] + part[1][g][tid]) + (part[2][g][tid] + part[3][g][tid])) + p.bhh[g * kLH + j]) +
                 p.gx[bt * p.gs + g * kLH + j];
    const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
    c = fmaf(fg, c, ig * gg);
    const float h = og * tanhf(c);
    float* gs = p.G + bt * p.gs + j;
    gs[0] = ig; gs[kLH] = fg; gs[2 * kLH] = gg; gs[3 * kLH] = og;
    p.C[bt * p.hs + j] = c;
    return h;
}

// h_{t-1} fragments of this lane's row from h0 (t == 0; zeros without it) or from y (plain loads: a finished earlier launch)
__device__ __forceinline__ void lstm_load_h(float4 (&a)[4], const LstmFwd& p, int b, bool ok, int koff, int t) {
    const float* src = t == 0 ? (p.h0 ? p.h0 + (long)b * kLH : nullptr) : p.y + ((long)b * p.S + t - 1) * p.hs;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
        a[ii] = ok && src ? *reinterpret_cast<const float4*>(src + koff + 16 * ii) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid = (H/16, ceil(B/16), heads), 256 threads; every workgroup resident at once (lstm_heads_per_launch)
__global__ __launch_bounds__(256) void lstm_persist_fwd_kernel(LstmFwd p, int spin_limit) {
    __shared__ float part[4][4][256];
    lstm_fwd_head(p);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int koff = 64 * w + 4 * kq;
    float4 bw[4][4];
    lstm_load_whh(bw, p.whh, j0, i, koff);
    const bool ok = (b0 + i) < p.B;                  // this lane's MFMA row is a sequence of the batch
    const int arow = ok ? b0 + i : b0;               // (rows past the batch poll row b0 -- inside y -- and are masked)
    const int b = b0 + (tid >> 4), j = j0 + (tid & 15);
    const bool live = b < p.B;
    float c = live && p.c0 ? p.c0[(long)b * kLH + j] : 0.f;
    int budget = spin_limit;
    PollPace pace(-1);
    for (int t = 0; t < p.S; ++t) {
        float4 a[4];
        if (t == 0) lstm_load_h(a, p, arow, ok, koff, 0);
        else poll_frags<4, 16>(p.y + ((long)arow * p.S + t - 1) * p.hs + koff, ok, a, budget, pace, &g_lstm_poll_timeout);
        lstm_fwd_mfma(part, a, bw, w, i, kq);
        __syncthreads();
        if (live) {
            const long bt = (long)b * p.S + t;
            const float h = lstm_fwd_gates(part, tid, p, bt, j, c);
            store_coherent(p.y + bt * p.hs + j, h);
            if (t == p.S - 1 && p.hN) {
                p.hN[(long)b * kLH + j] = h;
                p.cN[(long)b * kLH + j] = c;
            }
        }
        __syncthreads();                             // part is rewritten by the next step's MFMAs
    }
}

// One step per launch (grids that cannot be co-resident, CPC_LSTM_PER_STEP): same operands, products and gate math.
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(LstmFwd p, int t) {
    __shared__ float part[4][4][256];
    lstm_fwd_head(p);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int koff = 64 * w + 4 * kq;
    float4 bw[4][4];
    lstm_load_whh(bw, p.whh, j0, i, koff);
    const bool ok = (b0 + i) < p.B;
    float4 a[4];
    lstm_load_h(a, p, ok ? b0 + i : b0, ok, koff, t);
    lstm_fwd_mfma(part, a, bw, w, i, kq);
    __syncthreads();
    const int b = b0 + (tid >> 4), j = j0 + (tid & 15);
    if (b >= p.B) return;
    const long bt = (long)b * p.S + t;
    float c = t > 0 ? p.C[(bt - 1) * p.hs + j] : (p.c0 ? p.c0[(long)b * kLH + j] : 0.f);
    const float h = lstm_fwd_gates(part, tid, p, bt, j, c);
    p.y[bt * p.hs + j] = h;
    if (t == p.S - 1 && p.hN) {
        p.hN[(long)b * kLH + j] = h;
        p.cN[(long)b * kLH + j] = c;
    }
}

// ------------------------------------------------------------------ backward
struct LstmBwd {
    const float* whhT;    // (H,4H)
    const float* dY;      // (B,S,H) gradient of this layer's output
    const float* G;       // (B,S,4H) saved gates
    const float* C;       // (B,S,H) saved cell state
    const float* c0;      // (B,H) of this layer or NULL
    float* dG;            // (B,S,4H) pre-activation gate gradients (persistent launch: pre-filled with kNotReady)
    float* DC;            // (B,H) dc_{t+1} between the launches of the per-step path
    int B, S;
    int ng, g0;           // heads, as in LstmFwd: W_hh^T and DC of the heads one behind the other
    long hs, gs;
};

__device__ __forceinline__ void lstm_bwd_head(LstmBwd& p) {
    const long g = p.g0 + (int)blockIdx.z;
    p.whhT += g * kLH * kLG; p.dY += g * kLH; p.G += g * kLG; p.C += g * kLH;
    p.dG += g * kLG; p.DC += g * p.B * kLH;
}

// Lane (i, kq) of wave w holds W_hh^T[j0 + i][koff + 16 ii .. + 4], koff = 256 w + 4 kq: its quarter of K = 4H
__device__ __forceinline__ void lstm_load_whhT(float4 (&bw)[16], const float* __restrict__ whhT, int j0, int i, int koff) {
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) bw[ii] = *reinterpret_cast<const float4*>(whhT + (long)(j0 + i) * kLG + koff + 16 * ii);
}

__device__ __forceinline__ void lstm_bwd_mfma(float (&part)[4][256], const float4 (&a)[16], const float4 (&bw)[16], int w, int i,
                                              int kq) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ii = 0; ii < 16; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[ii], jj), f4c(bw[ii], jj), acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) part[w][(kq * 4 + r) * 16 + i] = acc[r];
}

// Thread (b, j) at step t: dh from the recurrent partials and dY, dc (carried in `dc`: dc_{t+1} in, dc_t out), and the four
// pre-activation gate gradients, returned in dg[] (order i, f, g, o).
__device__ __forceinline__ void lstm_bwd_gates(const float (&part)[4][256], int tid, const LstmBwd& p, int b, int j, int t,
                                               float& dc, float (&dg)[4]) {
    const long bt = (long)b * p.S + t;
    const float dh = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + p.dY[bt * p.hs + j];
    const float* gs = p.G + bt * p.gs + j;
    const float ig = gs[0], fg = gs[kLH], gg = gs[2 * kLH], og = gs[3 * kLH];
    const float c = p.C[bt * p.hs + j];
    const float cp = t > 0 ? p.C[(bt - 1) * p.hs + j] : (p.c0 ? p.c0[(long)b * kLH + j] : 0.f);
    const float tc = tanhf(c);
    float d = dh * og * (1.0f - tc * tc);
    if (t + 1 < p.S) d = fmaf(dc, p.G[(bt + 1) * p.gs + kLH + j], d);     // + dc_{t+1} * f_{t+1}
    dc = d;
    dg[0] = d * gg * ig * (1.0f - ig);
    dg[1] = d * cp * fg * (1.0f - fg);
    dg[2] = d * ig * (1.0f - gg * gg);
    dg[3] = dh * tc * og * (1.0f - og);
}

__global__ __launch_bounds__(256) void lstm_persist_bwd_kernel(LstmBwd p, int spin_limit) {
    __shared__ float part[4][256];
    lstm_bwd_head(p);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int koff = 256 * w + 4 * kq;
    float4 bw[16];
    lstm_load_whhT(bw, p.whhT, j0, i, koff);
    const bool ok = (b0 + i) < p.B;
    const int arow = ok ? b0 + i : b0;
    const int b = b0 + (tid >> 4), j = j0 + (tid & 15);
    const bool live = b < p.B;
    float dc = 0.f;
    int budget = spin_limit;
    PollPace pace(-1);
    for (int t = p.S - 1; t >= 0; --t) {
        float4 a[16];
        if (t == p.S - 1) {
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) a[ii] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            poll_frags<16, 16>(p.dG + ((long)arow * p.S + t + 1) * p.gs + koff, ok, a, budget, pace, &g_lstm_poll_timeout);
        }
        lstm_bwd_mfma(part, a, bw, w, i, kq);
        __syncthreads();
        if (live) {
            float dg[4];
            lstm_bwd_gates(part, tid, p, b, j, t, dc, dg);
            float* out = p.dG + ((long)b * p.S + t) * p.gs + j;
#pragma unroll
            for (int g = 0; g < 4; ++g) store_coherent(out + g * kLH, dg[g]);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(LstmBwd p, int t) {
    __shared__ float part[4][256];
    lstm_bwd_head(p);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int koff = 256 * w + 4 * kq;
    float4 bw[16];
    lstm_load_whhT(bw, p.whhT, j0, i, koff);
    const bool ok = (b0 + i) < p.B;
    float4 a[16];
    const float* src = t + 1 < p.S && ok ? p.dG + ((long)(b0 + i) * p.S + t + 1) * p.gs + koff : nullptr;
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) a[ii] = src ? *reinterpret_cast<const float4*>(src + 16 * ii) : make_float4(0.f, 0.f, 0.f, 0.f);
    lstm_bwd_mfma(part, a, bw, w, i, kq);
    __syncthreads();
    const int b = b0 + (tid >> 4), j = j0 + (tid & 15);
    if (b >= p.B) return;
    float dc = t + 1 < p.S ? p.DC[(long)b * kLH + j] : 0.f;
    float dg[4];
    lstm_bwd_gates(part, tid, p, b, j, t, dc, dg);
    float* out = p.dG + ((long)b * p.S + t) * p.gs + j;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[g * kLH] = dg[g];
    p.DC[(long)b * kLH + j] = dc;
}

// ------------------------------------------------------------------ host side
struct LstmLayout {
    long G[8], C[8], Y[8];
    long saved_total;
    long gx, fwd_total;
    long whhT, wihT, dG, DC, mid[2], part, tmp, bwd_total;
    long ipf, ipb;        // D != 256: in_proj.hip's scratch behind the forward's / the backward's (the totals include it)
};

// D: the input width of layer 0 (cpc_lstm_*_in); at 256 the layout is the one cpc_lstm_layout has always reported
static bool lstm_layout(int B, int S, int nl, LstmLayout& g, int D = kLH) {
    if (B <= 0 || S <= 0 || nl <= 0 || nl > 8) return false;
    if (D < 1 || D > kInProjMaxD) return false;
    if ((long)B * S > (1L << 21)) return false;          // B*S*4H floats stay below 2^31 (int GEMM rows and offsets)
    const long bsh = align64l((long)B * S * kLH), bsg = align64l((long)B * S * kLG);
    long o = 0;
    for (int l = 0; l < nl; ++l) {
        g.G[l] = o; o += bsg;
        g.C[l] = o; o += bsh;
        g.Y[l] = -1;
        if (l < nl - 1) { g.Y[l] = o; o += bsh; }
    }
    g.saved_total = o;
    g.gx = 0;
    g.fwd_total = bsg;
    o = 0;
    g.whhT = o; o += (long)kLH * kLG;
    g.wihT = o; o += (long)kLH * kLG;
    g.dG = o; o += bsg;
    g.DC = o; o += align64l((long)B * kLH);
    g.mid[0] = o; o += bsh;
    g.mid[1] = o; o += bsh;
    g.part = o; o += align64l(tn_gemm_part_floats(B * S, kLG, kLH));
    g.tmp = o; o += align64l((long)kRowsSumGroups * kLG);
    g.bwd_total = o;
    g.ipf = g.fwd_total; g.ipb = g.bwd_total;
    if (D != kLH) {
        g.fwd_total += in_proj_w_floats(kLG, D);
        g.bwd_total += in_proj_scratch_floats((long)B * S, kLG, D);
    }
    return true;
}

// How many whole heads (16 * ceil(B/16) workgroups each) of the persistent kernel can be resident at once?  0: not even one.
// The occupancy query is advisory and can over-report by one block, and more than 4 blocks of 256 threads per CU are not
// counted on: resident workgroups = CUs * max(1, min(query - 1, 4)).
template <class K>
static int lstm_heads_per_launch(K kernel, int B) {
    int dev = 0, cus = 0, occ = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 256, 0) != hipSuccess) return 0;
    const int per_cu = occ - 1 > 4 ? 4 : (occ - 1 < 1 ? 1 : occ - 1);
    const long fit = (long)cus * per_cu / (16L * cdiv(B, 16));
    return fit > 64 ? 64 : (int)fit;
}
template <class K>
static bool lstm_persist_fits(K kernel, int B) { return lstm_heads_per_launch(kernel, B) >= 1; }

// The grouped recurrence (cpc_lstm_group_*): every (B,S,.) array holds the G heads side by side
struct LstmGroupLayout {
    long G, C, saved_total;
    long gx, fwd_total;
    long whhT, wihT, dG, DC, part, tmp, bwd_total;
};

static bool lstm_group_layout(int B, int S, int G, LstmGroupLayout& g) {
    if (B <= 0 || S <= 0 || G <= 0 || G > 64) return false;
    if ((long)B * S > (1L << 21) || (long)B * S * G > (1L << 21)) return false;     // B*S*G*4H floats stay below 2^31
    const long M = (long)B * S;
    long o = 0;
    g.G = o; o += align64l(M * G * kLG);
    g.C = o; o += align64l(M * G * kLH);
    g.saved_total = o;
    g.gx = 0;
    g.fwd_total = align64l(M * G * kLG);
    o = 0;
    g.whhT = o; o += (long)G * kLH * kLG;
    g.wihT = o; o += (long)G * kLH * kLG;
    g.dG = o; o += align64l(M * G * kLG);
    g.DC = o; o += align64l((long)G * B * kLH);
    const long pa = tn_gemm_part_floats((int)M, G * kLG, kLH), pb = (long)G * tn_gemm_part_floats((int)M, kLG, kLH);
    g.part = o; o += align64l(pa > pb ? pa : pb);
    g.tmp = o; o += align64l((long)kRowsSumGroups * G * kLG);
    g.bwd_total = o;
    return true;
}

static bool lstm_ptrs_ok(const float* const* v, int n) {
    if (!v) return false;
    for (int k = 0; k < n; ++k)
        if (!v[k]) return false;
    return true;
}

int lstm_error_flag_fetch(int clear, unsigned* out) { return device_flag_fetch(HIP_SYMBOL(g_lstm_poll_timeout), clear, out); }

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_lstm_layout(int B, int S, int nl, long* sizes) {
    LstmLayout g;
    CPC_RETURN_IF(!lstm_layout(B, S, nl, g), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = g.saved_total; sizes[1] = g.fwd_total; sizes[2] = g.bwd_total;
    return 0;
}

extern "C" int cpc_lstm_layout_in(int B, int S, int nl, int D, long* sizes) {
    LstmLayout g;
    CPC_RETURN_IF(!lstm_layout(B, S, nl, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = g.saved_total; sizes[1] = g.fwd_total; sizes[2] = g.bwd_total;
    return 0;
}

// D: x is (B,S,D) and weight_ih_l0 (4H,D); D == 256 is cpc_lstm_forward itself
static int lstm_forward_impl(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                             float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int D, int flags, void* stream) {
    LstmLayout g;
    CPC_RETURN_IF(!lstm_layout(B, S, nl, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~CPC_LSTM_PER_STEP, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !lstm_ptrs_ok(params, 4 * nl) || !saved || !scratch || !y || !hN || !cN, CPC_ERR_ARG);
    CPC_RETURN_IF((h0 == nullptr) != (c0 == nullptr), CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const int M = B * S;
    const bool persist = !(flags & CPC_LSTM_PER_STEP) && lstm_persist_fits(lstm_persist_fwd_kernel, B);
    const dim3 grid(kLH / 16, cdiv(B, 16));
    float* gx = scratch + g.gx;
    const float* in = x;
    for (int l = 0; l < nl; ++l) {
        const float* wih = params[4 * l], *bih = params[4 * l + 2];
        float* out = l == nl - 1 ? y : saved + g.Y[l];
        int rc = l == 0 && D != kLH ? in_proj_forward(x, D, wih, bih, scratch + g.ipf, gx, M, kLG, D, st)
                                    : nt_gemm(plain_rows(in, M, kLH), wih, kLH, bih, gx, kLG, kLG, kLH, st);
        if (rc) return rc;
        LstmFwd p;
        p.gx = gx; p.whh = params[4 * l + 1]; p.bhh = params[4 * l + 3];
        p.h0 = h0 ? h0 + (long)l * B * kLH : nullptr;
        p.c0 = c0 ? c0 + (long)l * B * kLH : nullptr;
        p.y = out; p.G = saved + g.G[l]; p.C = saved + g.C[l];
        p.hN = hN + (long)l * B * kLH; p.cN = cN + (long)l * B * kLH;
        p.B = B; p.S = S; p.ng = 1; p.g0 = 0; p.hs = kLH; p.gs = kLG;
        if (persist) {
            if (hipMemsetAsync(out, 0xFF, (size_t)M * kLH * sizeof(float), st) != hipSuccess) return CPC_ERR_ARG;
            hipLaunchKernelGGL(lstm_persist_fwd_kernel, grid, dim3(256), 0, st, p, kLstmSpinLimit);
        } else {
            for (int t = 0; t < S; ++t) hipLaunchKernelGGL(lstm_step_fwd_kernel, grid, dim3(256), 0, st, p, t);
        }
        CPC_LAUNCH_CHECK();
        in = out;
    }
    return 0;
}

extern "C" int cpc_lstm_forward(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                                float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int flags, void* stream) {
    return lstm_forward_impl(x, h0, c0, params, saved, scratch, y, hN, cN, B, S, nl, kLH, flags, stream);
}

extern "C" int cpc_lstm_forward_in(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                                   float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int D, int flags,
                                   void* stream) {
    return lstm_forward_impl(x, h0, c0, params, saved, scratch, y, hN, cN, B, S, nl, D, flags, stream);
}

static int lstm_backward_impl(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                              const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S,
                              int nl, int D, int flags, void* stream) {
    LstmLayout g;
    CPC_RETURN_IF(!lstm_layout(B, S, nl, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~CPC_LSTM_PER_STEP, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !lstm_ptrs_ok(params, 4 * nl) || !saved || !y || !dy || !scratch || !dx ||
                  !lstm_ptrs_ok(const_cast<const float* const*>(grads), 4 * nl), CPC_ERR_ARG);
    CPC_RETURN_IF((h0 == nullptr) != (c0 == nullptr), CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const int M = B * S;
    const bool persist = !(flags & CPC_LSTM_PER_STEP) && lstm_persist_fits(lstm_persist_bwd_kernel, B);
    const dim3 grid(kLH / 16, cdiv(B, 16));
    float* whhT = scratch + g.whhT, *wihT = scratch + g.wihT, *dG = scratch + g.dG;
    const float* dYl = dy;
    for (int l = nl - 1; l >= 0; --l) {
        const float* in = l == 0 ? x : saved + g.Y[l - 1];
        const float* out = l == nl - 1 ? y : saved + g.Y[l];
        const float* h0l = h0 ? h0 + (long)l * B * kLH : nullptr;
        float* dXl = l == 0 ? dx : scratch + g.mid[l & 1];
        int rc = transpose(params[4 * l + 1], whhT, kLG, kLH, st);      // (4H,H) -> (H,4H)
        if (rc) return rc;
        const bool narrow = l == 0 && D != kLH;          // layer 0 at another input width: its three products in in_proj.hip
        rc = narrow ? 0 : transpose(params[4 * l], wihT, kLG, kLH, st);
        if (rc) return rc;
        LstmBwd p;
        p.whhT = whhT; p.dY = dYl; p.G = saved + g.G[l]; p.C = saved + g.C[l];
        p.c0 = c0 ? c0 + (long)l * B * kLH : nullptr;
        p.dG = dG; p.DC = scratch + g.DC; p.B = B; p.S = S; p.ng = 1; p.g0 = 0; p.hs = kLH; p.gs = kLG;
        if (persist) {
            if (hipMemsetAsync(dG, 0xFF, (size_t)M * kLG * sizeof(float), st) != hipSuccess) return CPC_ERR_ARG;
            hipLaunchKernelGGL(lstm_persist_bwd_kernel, grid, dim3(256), 0, st, p, kLstmSpinLimit);
        } else {
            for (int t = S - 1; t >= 0; --t) hipLaunchKernelGGL(lstm_step_bwd_kernel, grid, dim3(256), 0, st, p, t);
        }
        CPC_LAUNCH_CHECK();
        // weight / bias gradients over all B*S rows: dW_ih = dG^T . in, dW_hh = dG^T . h_{t-1}, db_ih = db_hh = sum dG
        const RowMap gm = plain_rows(dG, M, kLG);
        rc = narrow ? in_proj_backward(x, D, params[0], dG, scratch + g.ipb, nullptr, grads[0], M, kLG, D, st)
                    : tn_gemm(gm, kLG, plain_rows(in, M, kLH), kLH, scratch + g.part, grads[4 * l], 0, st);
        if (rc) return rc;
        RowMap hm;                                       // h_{t-1} rows: out[b, t-1] (zero row at t = 0; h0 term below)
        hm.base = out; hm.R = S; hm.bstride = (long)S * kLH; hm.rstride = kLH; hm.off = -kLH;
        hm.tmul = 1; hm.tadd = -1; hm.Lin = S; hm.M = M;
        rc = tn_gemm(gm, kLG, hm, kLH, scratch + g.part, grads[4 * l + 1], 0, st);
        if (rc) return rc;
        if (h0l) {                                       // + dG[:,0,:]^T . h0
            RowMap g0;
            g0.base = dG; g0.R = 1; g0.bstride = (long)S * kLG; g0.rstride = 0; g0.off = 0;
            g0.tmul = 0; g0.tadd = 0; g0.Lin = 0x7fffffff; g0.M = B;
            rc = tn_gemm(g0, kLG, plain_rows(h0l, B, kLH), kLH, scratch + g.part, grads[4 * l + 1], 1, st);
            if (rc) return rc;
        }
        rc = rows_sum(dG, M, kLG, scratch + g.tmp, grads[4 * l + 2], st);
        if (rc) return rc;
        rc = rows_sum(dG, M, kLG, scratch + g.tmp, grads[4 * l + 3], st);
        if (rc) return rc;
        rc = narrow ? in_proj_backward(x, D, params[0], dG, scratch + g.ipb, dx, nullptr, M, kLG, D, st)
                    : nt_gemm(gm, wihT, kLG, nullptr, dXl, kLH, kLH, kLG, st);   // dX = dG . W_ih (as NT against W_ih^T)
        if (rc) return rc;
        dYl = dXl;
    }
    return 0;
}

extern "C" int cpc_lstm_backward(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                                 const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S,
                                 int nl, int flags, void* stream) {
    return lstm_backward_impl(x, h0, c0, params, saved, y, dy, scratch, dx, grads, B, S, nl, kLH, flags, stream);
}

extern "C" int cpc_lstm_backward_in(const float* x, const float* h0, const float* c0, const float* const* params,
                                    const float* saved, const float* y, const float* dy, float* scratch, float* dx,
                                    float* const* grads, int B, int S, int nl, int D, int flags, void* stream) {
    return lstm_backward_impl(x, h0, c0, params, saved, y, dy, scratch, dx, grads, B, S, nl, D, flags, stream);
}

// ---- G heads side by side (the criterion's --rnnMode LSTM predictors): see include/cpc_hip.h
extern "C" int cpc_lstm_group_layout(int B, int S, int G, long* sizes) {
    LstmGroupLayout g;
    CPC_RETURN_IF(!lstm_group_layout(B, S, G, g), CPC_ERR_SHAPE);
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = g.saved_total; sizes[1] = g.fwd_total; sizes[2] = g.bwd_total;
    return 0;
}

extern "C" int cpc_lstm_group_forward(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                      float* saved, float* scratch, float* y, int B, int S, int G, int flags, void* stream) {
    LstmGroupLayout g;
    CPC_RETURN_IF(!lstm_group_layout(B, S, G, g), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~CPC_LSTM_PER_STEP, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !w_ih || !w_hh || !b_ih || !b_hh || !saved || !scratch || !y, CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const int M = B * S;
    const int fit = (flags & CPC_LSTM_PER_STEP) ? 0 : lstm_heads_per_launch(lstm_persist_fwd_kernel, B);
    float* gx = scratch + g.gx;
    int rc = nt_gemm(plain_rows(x, M, kLH), w_ih, kLH, b_ih, gx, (long)G * kLG, G * kLG, kLH, st);   // all heads' input projection
    if (rc) return rc;
    LstmFwd p;
    p.gx = gx; p.whh = w_hh; p.bhh = b_hh; p.h0 = nullptr; p.c0 = nullptr;
    p.y = y; p.G = saved + g.G; p.C = saved + g.C; p.hN = nullptr; p.cN = nullptr;
    p.B = B; p.S = S; p.ng = G; p.g0 = 0; p.hs = (long)G * kLH; p.gs = (long)G * kLG;
    if (fit >= 1) {
        if (hipMemsetAsync(y, 0xFF, (size_t)M * G * kLH * sizeof(float), st) != hipSuccess) return CPC_ERR_ARG;
        for (p.g0 = 0; p.g0 < G; p.g0 += fit)       // as many whole heads per launch as can be resident together
            hipLaunchKernelGGL(lstm_persist_fwd_kernel, dim3(kLH / 16, cdiv(B, 16), G - p.g0 < fit ? G - p.g0 : fit), dim3(256), 0,
                               st, p, kLstmSpinLimit);
    } else {
        for (int t = 0; t < S; ++t)
            hipLaunchKernelGGL(lstm_step_fwd_kernel, dim3(kLH / 16, cdiv(B, 16), G), dim3(256), 0, st, p, t);
    }
    CPC_LAUNCH_CHECK();
    return 0;
}

extern "C" int cpc_lstm_group_backward(const float* x, const float* w_ih, const float* w_hh, const float* saved, const float* y,
                                       const float* dy, float* scratch, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                                       float* db_hh, int B, int S, int G, int flags, void* stream) {
    LstmGroupLayout g;
    CPC_RETURN_IF(!lstm_group_layout(B, S, G, g), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~CPC_LSTM_PER_STEP, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !w_ih || !w_hh || !saved || !y || !dy || !scratch || !dx || !dw_ih || !dw_hh || !db_ih || !db_hh,
                  CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const int M = B * S;
    const int fit = (flags & CPC_LSTM_PER_STEP) ? 0 : lstm_heads_per_launch(lstm_persist_bwd_kernel, B);
    float* whhT = scratch + g.whhT, *wihT = scratch + g.wihT, *dG = scratch + g.dG;
    int rc = transpose(w_hh, whhT, kLG, kLH, st, G, (long)kLG * kLH, (long)kLG * kLH);      // per head (4H,H) -> (H,4H)
    if (rc) return rc;
    rc = transpose(w_ih, wihT, G * kLG, kLH, st);                                           // stacked (G 4H,H) -> (H,G 4H)
    if (rc) return rc;
    LstmBwd p;
    p.whhT = whhT; p.dY = dy; p.G = saved + g.G; p.C = saved + g.C; p.c0 = nullptr;
    p.dG = dG; p.DC = scratch + g.DC; p.B = B; p.S = S; p.ng = G; p.g0 = 0; p.hs = (long)G * kLH; p.gs = (long)G * kLG;
    if (fit >= 1) {
        if (hipMemsetAsync(dG, 0xFF, (size_t)M * G * kLG * sizeof(float), st) != hipSuccess) return CPC_ERR_ARG;
        for (p.g0 = 0; p.g0 < G; p.g0 += fit)
            hipLaunchKernelGGL(lstm_persist_bwd_kernel, dim3(kLH / 16, cdiv(B, 16), G - p.g0 < fit ? G - p.g0 : fit), dim3(256), 0,
                               st, p, kLstmSpinLimit);
    } else {
        for (int t = S - 1; t >= 0; --t)
            hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3(kLH / 16, cdiv(B, 16), G), dim3(256), 0, st, p, t);
    }
    CPC_LAUNCH_CHECK();
    // stacked dW_ih = dG^T . x and both bias gradients over all heads' gate columns at once; dW_hh head by head in one launch
    const RowMap gm = plain_rows(dG, M, G * kLG);
    rc = tn_gemm(gm, G * kLG, plain_rows(x, M, kLH), kLH, scratch + g.part, dw_ih, 0, st);
    if (rc) return rc;
    RowMap hm;                                           // h_{t-1} rows of head 0: y[b, t-1, 0:H] (zero row at t = 0)
    hm.base = y; hm.R = S; hm.bstride = (long)S * G * kLH; hm.rstride = G * kLH; hm.off = -G * kLH;
    hm.tmul = 1; hm.tadd = -1; hm.Lin = S; hm.M = M;
    GemmGroup grp;
    grp.G = G; grp.a = kLG; grp.b = kLH; grp.c = (long)kLG * kLH;
    rc = tn_gemm(gm, kLG, hm, kLH, scratch + g.part, dw_hh, 0, st, GemmBounds(), grp);
    if (rc) return rc;
    rc = rows_sum(dG, M, G * kLG, scratch + g.tmp, db_ih, st);
    if (rc) return rc;
    rc = rows_sum(dG, M, G * kLG, scratch + g.tmp, db_hh, st);
    if (rc) return rc;
    return nt_gemm(gm, wihT, G * kLG, nullptr, dx, kLH, kLH, G * kLG, st);     // dx = sum over heads of dG_g . W_ih,g
}
