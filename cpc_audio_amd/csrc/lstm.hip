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
//   * the host side is one layout and one forward / backward for both forms -- one head of nl layers, G heads of one layer
//     (`heads`, lstm_layout) -- and what stands around the kernels (input projection, the gradients behind the backward
//     recurrence, persistent or per-step launches) is recurrent_host.h's, shared with gru.hip and rnn.hip.
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"
#include "persist.h"
#include "recurrent_host.h"
#include "padded_cell.h"

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

// grid = (H/16, ceil(B/16), heads), 256 threads; every workgroup resident at once (recur_launch)
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

// G heads side by side in the columns of every (B,S,.) array.  heads: the grouped form (cpc_lstm_group_*) -- one layer at
// D = 256, no carried or final state, and no mid[] in its scratch; otherwise one head, nl layers, and D the input width of
// layer 0 (cpc_lstm_*_in; at 256 the layout is the one cpc_lstm_layout has always reported, mid[] at nl = 1 included).
static bool lstm_layout(int B, int S, int G, int nl, bool heads, LstmLayout& g, int D = kLH) {
    if (B <= 0 || S <= 0 || G <= 0 || G > 64 || nl <= 0 || nl > 8) return false;
    if (D < 1 || D > kInProjMaxD || (heads ? nl != 1 || D != kLH : G != 1)) return false;
    if ((long)B * S > (1L << 21) || (long)B * S * G > (1L << 21)) return false;     // B*S*G*4H floats stay below 2^31
    const long M = (long)B * S, mh = align64l(M * G * kLH), mg = align64l(M * G * kLG);
    long o = 0;
    for (int l = 0; l < nl; ++l) {
        g.G[l] = o; o += mg;
        g.C[l] = o; o += mh;
        g.Y[l] = -1;
        if (l < nl - 1) { g.Y[l] = o; o += mh; }
    }
    g.saved_total = o;
    g.gx = 0;
    g.fwd_total = mg;
    o = 0;
    g.whhT = o; o += (long)G * kLH * kLG;
    g.wihT = o; o += (long)G * kLH * kLG;
    g.dG = o; o += mg;
    g.DC = o; o += align64l((long)G * B * kLH);
    g.mid[0] = o; o += heads ? 0 : mh;
    g.mid[1] = o; o += heads ? 0 : mh;
    const long pa = tn_gemm_part_floats((int)M, G * kLG, kLH), pb = (long)G * tn_gemm_part_floats((int)M, kLG, kLH);
    g.part = o; o += align64l(pa > pb ? pa : pb);
    g.tmp = o; o += align64l((long)kRowsSumGroups * G * kLG);
    g.bwd_total = o;
    g.ipf = g.fwd_total; g.ipb = g.bwd_total;
    if (D != kLH) {
        g.fwd_total += in_proj_w_floats(kLG, D);
        g.bwd_total += in_proj_scratch_floats(M, kLG, D);
    }
    return true;
}

// The S steps of one layer's recurrence (all G heads, 16 * ceil(B/16) workgroups each)
static int lstm_recur(const LstmFwd& p, int per_step, hipStream_t st) {
    return recur_launch(lstm_persist_fwd_kernel, lstm_step_fwd_kernel, p, dim3(kLH / 16, cdiv(p.B, 16)), p.ng, p.S, false, per_step,
                        p.y, (size_t)p.B * p.S * p.hs, kLstmSpinLimit, st);
}
static int lstm_recur(const LstmBwd& p, int per_step, hipStream_t st) {
    return recur_launch(lstm_persist_bwd_kernel, lstm_step_bwd_kernel, p, dim3(kLH / 16, cdiv(p.B, 16)), p.ng, p.S, true, per_step,
                        p.dG, (size_t)p.B * p.S * p.gs, kLstmSpinLimit, st);
}

int lstm_error_flag_fetch(int clear, unsigned* out) { return device_flag_fetch(HIP_SYMBOL(g_lstm_poll_timeout), clear, out); }

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_lstm_layout_in(int B, int S, int nl, int D, long* sizes) {
    LstmLayout g;
    return layout_sizes(lstm_layout(B, S, 1, nl, false, g, D), g, sizes);
}

extern "C" int cpc_lstm_layout(int B, int S, int nl, long* sizes) { return cpc_lstm_layout_in(B, S, nl, kLH, sizes); }

// D: x is (B,S,D) and weight_ih_l0 (4H,D); D == 256 is cpc_lstm_forward itself.  heads: see lstm_layout.
static int lstm_forward_impl(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                             float* scratch, float* y, float* hN, float* cN, int B, int S, int G, int nl, bool heads, int D,
                             int flags, void* stream) {
    LstmLayout g;
    CPC_RETURN_IF(!lstm_layout(B, S, G, nl, heads, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~CPC_LSTM_PER_STEP, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !ptrs_ok(params, 4 * nl) || !saved || !scratch || !y || (!heads && (!hN || !cN)), CPC_ERR_ARG);
    CPC_RETURN_IF((h0 == nullptr) != (c0 == nullptr), CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    float* gx = scratch + g.gx;
    const float* in = x;
    for (int l = 0; l < nl; ++l) {
        float* out = l == nl - 1 ? y : saved + g.Y[l];
        int rc = layer_input_projection(l, D, in, params[4 * l], params[4 * l + 2], scratch + g.ipf, gx, B * S, G * kLG, st);
        if (rc) return rc;
        LstmFwd p;
        p.gx = gx; p.whh = params[4 * l + 1]; p.bhh = params[4 * l + 3];
        p.h0 = h0 ? h0 + (long)l * B * kLH : nullptr;
        p.c0 = c0 ? c0 + (long)l * B * kLH : nullptr;
        p.y = out; p.G = saved + g.G[l]; p.C = saved + g.C[l];
        p.hN = hN ? hN + (long)l * B * kLH : nullptr;
        p.cN = cN ? cN + (long)l * B * kLH : nullptr;
        p.B = B; p.S = S; p.ng = G; p.g0 = 0; p.hs = (long)G * kLH; p.gs = (long)G * kLG;
        rc = lstm_recur(p, flags & CPC_LSTM_PER_STEP, st);
        if (rc) return rc;
        in = out;
    }
    return 0;
}

extern "C" int cpc_lstm_forward(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                                float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int flags, void* stream) {
    return lstm_forward_impl(x, h0, c0, params, saved, scratch, y, hN, cN, B, S, 1, nl, false, kLH, flags, stream);
}

extern "C" int cpc_lstm_forward_in(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                                   float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int D, int flags,
                                   void* stream) {
    return lstm_forward_impl(x, h0, c0, params, saved, scratch, y, hN, cN, B, S, 1, nl, false, D, flags, stream);
}

static int lstm_backward_impl(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                              const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S,
                              int G, int nl, bool heads, int D, int flags, void* stream) {
    LstmLayout g;
    CPC_RETURN_IF(!lstm_layout(B, S, G, nl, heads, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~CPC_LSTM_PER_STEP, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !ptrs_ok(params, 4 * nl) || !saved || !y || !dy || !scratch || !dx ||
                  !ptrs_ok(const_cast<const float* const*>(grads), 4 * nl), CPC_ERR_ARG);
    CPC_RETURN_IF((h0 == nullptr) != (c0 == nullptr), CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    float* dG = scratch + g.dG;
    const float* dYl = dy;
    for (int l = nl - 1; l >= 0; --l) {
        GradTail t;
        t.N = kLG; t.G = G; t.T = S; t.R = B; t.D = l == 0 ? D : kLH; t.time_major = false;
        t.dGi = t.dGh = dG; t.in = l == 0 ? x : saved + g.Y[l - 1]; t.out = l == nl - 1 ? y : saved + g.Y[l];
        t.h0 = h0 ? h0 + (long)l * B * kLH : nullptr;
        t.w = params + 4 * l; t.dw = grads + 4 * l; t.dx = l == 0 ? dx : scratch + g.mid[l & 1];
        t.whhT = scratch + g.whhT; t.wihT = scratch + g.wihT; t.part = scratch + g.part; t.tmp = scratch + g.tmp;
        t.ip_scratch = scratch + g.ipb;
        int rc = tail_transposes(t, st);
        if (rc) return rc;
        LstmBwd p;
        p.whhT = t.whhT; p.dY = dYl; p.G = saved + g.G[l]; p.C = saved + g.C[l];
        p.c0 = c0 ? c0 + (long)l * B * kLH : nullptr;
        p.dG = dG; p.DC = scratch + g.DC; p.B = B; p.S = S; p.ng = G; p.g0 = 0; p.hs = (long)G * kLH; p.gs = (long)G * kLG;
        rc = lstm_recur(p, flags & CPC_LSTM_PER_STEP, st);
        if (rc) return rc;
        rc = tail_gradients(t, st);
        if (rc) return rc;
        dYl = t.dx;
    }
    return 0;
}

extern "C" int cpc_lstm_backward(const float* x, const float* h0, const float* c0, const float* const* params, const float* saved,
                                 const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S,
                                 int nl, int flags, void* stream) {
    return lstm_backward_impl(x, h0, c0, params, saved, y, dy, scratch, dx, grads, B, S, 1, nl, false, kLH, flags, stream);
}

extern "C" int cpc_lstm_backward_in(const float* x, const float* h0, const float* c0, const float* const* params,
                                    const float* saved, const float* y, const float* dy, float* scratch, float* dx,
                                    float* const* grads, int B, int S, int nl, int D, int flags, void* stream) {
    return lstm_backward_impl(x, h0, c0, params, saved, y, dy, scratch, dx, grads, B, S, 1, nl, false, D, flags, stream);
}

// ---- G heads side by side (the criterion's --rnnMode LSTM predictors): see include/cpc_hip.h
extern "C" int cpc_lstm_group_layout(int B, int S, int G, long* sizes) {
    LstmLayout g;
    return layout_sizes(lstm_layout(B, S, G, 1, true, g), g, sizes);
}

extern "C" int cpc_lstm_group_forward(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                      float* saved, float* scratch, float* y, int B, int S, int G, int flags, void* stream) {
    const float* params[4] = {w_ih, w_hh, b_ih, b_hh};
    return lstm_forward_impl(x, nullptr, nullptr, params, saved, scratch, y, nullptr, nullptr, B, S, G, 1, true, kLH, flags, stream);
}

extern "C" int cpc_lstm_group_backward(const float* x, const float* w_ih, const float* w_hh, const float* saved, const float* y,
                                       const float* dy, float* scratch, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                                       float* db_hh, int B, int S, int G, int flags, void* stream) {
    const float* params[4] = {w_ih, w_hh, w_ih, w_hh};      // (the backward reads no bias: the two slots only pass the NULL check)
    float* grads[4] = {dw_ih, dw_hh, db_ih, db_hh};
    return lstm_backward_impl(x, nullptr, nullptr, params, saved, y, dy, scratch, dx, grads, B, S, G, 1, true, kLH, flags, stream);
}

// ================================================================== any hidden width H in 1..512 (cpc_lstm_*_h)
// The same recurrence at a padded width Hp = 128 * ceil(H / 128) on zero-padded copies of the parameters, made once per layer
// and call in scratch.  A padded unit has zero W_ih and W_hh rows, a zero W_hh column and zero biases: its pre-activations are
// 0, so g = tanh(0) = 0, c stays 0 (c0 is padded with zeros) and h = o * tanh(0) = 0 at every step, exactly; in the backward its
// dG meets zero weights only, so nothing of it reaches a real unit.  Every internal (B,S,.) array is Hp or 4 Hp floats wide,
// gate g of unit j at column g * Hp + j; y, hN, cN and the gradients are narrowed to their true shapes by a copy at the end.
//   * Hp % 128 == 0 because the weight-gradient GEMM (tn_gemm) tiles both widths by 128; the four waves then split K = Hp
//     (forward) or 4 Hp (backward) evenly: KF = Hp / 64 fragments of 4 per lane forward, 4 KF backward.
//   * the grid covers all Hp / 16 unit tiles, so every column of the polled arrays (y: Hp, dG: 4 Hp) is written by some
//     workgroup and no pad column keeps the not-ready pattern.
//   * the backward polls its 4 KF fragments in pieces of at most 16 and multiplies each piece before it fetches the next: the
//     MFMA order is that of one pass, the live fragments stay at 64 registers beside the 16 KF of W_hh^T.
//   * the tail products are recurrent_host.h's at H = Hp: layer 0 at D != Hp in in_proj.hip, everything else on nt_gemm / tn_gemm.
// What does not depend on the cell is padded_cell.h's, shared with gru.hip: the kernels' index prologue (PadTile), operand loads
// and products, the layout, the width dispatch and the forward / backward drivers.  Here: the records, the gate math, the
// kernels and the cell's description for the drivers (LstmHCell).
namespace cpc {

struct LstmHFwd {
    const float* gx;      // (B,S,4Hp)
    const float* whh;     // (4Hp,Hp) padded
    const float* bhh;     // (4Hp) padded
    const float* h0;      // (B,Hp) padded, of this layer, or NULL
    const float* c0;
    float* y;             // (B,S,Hp) (persistent launch: pre-filled with kNotReady)
    float* G;             // (B,S,4Hp) saved activated gates
    float* C;             // (B,S,Hp) saved cell state
    float* hN;            // (B,Hp) of this layer
    float* cN;
    int B, S;
    int g0;               // (recur_launch's head offset: one head here, always 0)
};

struct LstmHBwd {
    const float* whhT;    // (Hp,4Hp)
    const float* dY;      // (B,S,Hp)
    const float* G;       // (B,S,4Hp)
    const float* C;       // (B,S,Hp)
    const float* c0;      // (B,Hp) padded or NULL
    float* dG;            // (B,S,4Hp) (persistent launch: pre-filled with kNotReady)
    float* DC;            // (B,Hp) dc_{t+1} between the launches of the per-step path
    int B, S;
    int g0;
};

template <int HP>
__device__ __forceinline__ float lstmh_fwd_gates(const float (&part)[4][4][256], int tid, const LstmHFwd& p, long bt, int j,
                                                 float& c) {
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        pre[g] = (((part[0][g][tid] + part[1][g][tid]) + (part[2][g][tid] + part[3][g][tid])) + p.bhh[g * HP + j]) +
                 p.gx[bt * (4 * HP) + g * HP + j];
    const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf(pre[2]), og = sigmoidf_(pre[3]);
    c = fmaf(fg, c, ig * gg);
    const float h = og * tanhf(c);
    float* gs = p.G + bt * (4 * HP) + j;
    gs[0] = ig; gs[HP] = fg; gs[2 * HP] = gg; gs[3 * HP] = og;
    p.C[bt * HP + j] = c;
    return h;
}

// grid = (Hp/16, ceil(B/16)), 256 threads; every workgroup resident at once (recur_launch)
template <int KF>
__global__ __launch_bounds__(256) void lstmh_persist_fwd_kernel(LstmHFwd p, int spin_limit) {
    constexpr int HP = 64 * KF;
    __shared__ float part[4][4][256];
    PadTile q;
    const int koff = 16 * KF * q.w + 4 * q.kq;
    float4 bw[4][KF];
    pad_load_whh<4, KF>(bw, p.whh, q.j0, q.i, koff);
    q.feed_row(p.B);
    q.gate_thread(p.B);
    float c = q.live && p.c0 ? p.c0[(long)q.b * HP + q.j] : 0.f;
    int budget = spin_limit;
    PollPace pace(-1);
    for (int t = 0; t < p.S; ++t) {
        float4 a[KF];
        if (t == 0) pad_load_h<KF>(a, p.h0, p.y, p.S, q.arow, q.ok, koff, 0);
        else poll_frags<KF, 16>(p.y + ((long)q.arow * p.S + t - 1) * HP + koff, q.ok, a, budget, pace, &g_lstm_poll_timeout);
        pad_fwd_mfma<4, KF>(part, a, bw, q.w, q.i, q.kq);
        __syncthreads();
        if (q.live) {
            const long bt = (long)q.b * p.S + t;
            const float h = lstmh_fwd_gates<HP>(part, q.tid, p, bt, q.j, c);
            store_coherent(p.y + bt * HP + q.j, h);
            if (t == p.S - 1) {
                p.hN[(long)q.b * HP + q.j] = h;
                p.cN[(long)q.b * HP + q.j] = c;
            }
        }
        __syncthreads();
    }
}

template <int KF>
__global__ __launch_bounds__(256) void lstmh_step_fwd_kernel(LstmHFwd p, int t) {
    constexpr int HP = 64 * KF;
    __shared__ float part[4][4][256];
    PadTile q;
    const int koff = 16 * KF * q.w + 4 * q.kq;
    float4 bw[4][KF];
    pad_load_whh<4, KF>(bw, p.whh, q.j0, q.i, koff);
    q.feed_row(p.B);
    float4 a[KF];
    pad_load_h<KF>(a, p.h0, p.y, p.S, q.arow, q.ok, koff, t);
    pad_fwd_mfma<4, KF>(part, a, bw, q.w, q.i, q.kq);
    __syncthreads();
    q.gate_thread(p.B);
    if (!q.live) return;
    const int b = q.b, j = q.j;
    const long bt = (long)b * p.S + t;
    float c = t > 0 ? p.C[(bt - 1) * HP + j] : (p.c0 ? p.c0[(long)b * HP + j] : 0.f);
    const float h = lstmh_fwd_gates<HP>(part, q.tid, p, bt, j, c);
    p.y[bt * HP + j] = h;
    if (t == p.S - 1) {
        p.hN[(long)b * HP + j] = h;
        p.cN[(long)b * HP + j] = c;
    }
}

template <int HP>
__device__ __forceinline__ void lstmh_bwd_gates(const float (&part)[4][256], int tid, const LstmHBwd& p, int b, int j, int t,
                                                float& dc, float (&dg)[4]) {
    constexpr int GP = 4 * HP;
    const long bt = (long)b * p.S + t;
    const float dh = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + p.dY[bt * HP + j];
    const float* gs = p.G + bt * GP + j;
    const float ig = gs[0], fg = gs[HP], gg = gs[2 * HP], og = gs[3 * HP];
    const float c = p.C[bt * HP + j];
    const float cp = t > 0 ? p.C[(bt - 1) * HP + j] : (p.c0 ? p.c0[(long)b * HP + j] : 0.f);
    const float tc = tanhf(c);
    float d = dh * og * (1.0f - tc * tc);
    if (t + 1 < p.S) d = fmaf(dc, p.G[(bt + 1) * GP + HP + j], d);     // + dc_{t+1} * f_{t+1}
    dc = d;
    dg[0] = d * gg * ig * (1.0f - ig);
    dg[1] = d * cp * fg * (1.0f - fg);
    dg[2] = d * ig * (1.0f - gg * gg);
    dg[3] = dh * tc * og * (1.0f - og);
}

template <int KF>
__global__ __launch_bounds__(256) void lstmh_persist_bwd_kernel(LstmHBwd p, int spin_limit) {
    using W = PadBwd<4, KF>;
    constexpr int HP = W::HP, GP = W::GP, CH = W::CH;
    __shared__ float part[4][256];
    PadTile q;
    const int koff = GP / 4 * q.w + 4 * q.kq;
    float4 bw[W::NF];
    pad_load_whhT<4, KF>(bw, p.whhT, q.j0, q.i, koff);
    q.feed_row(p.B);
    q.gate_thread(p.B);
    float dc = 0.f;
    int budget = spin_limit;
    PollPace pace(-1), nopace(0);                    // (the later pieces of a step follow the first at once)
    for (int t = p.S - 1; t >= 0; --t) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < p.S - 1) {                           // (t == S - 1: dG_{t+1} = 0, the product is 0)
            const float* row = p.dG + ((long)q.arow * p.S + t + 1) * GP + koff;
#pragma unroll
            for (int c = 0; c < W::NCH; ++c) {
                float4 a[CH];
                poll_frags<CH, 16>(row + 16 * CH * c, q.ok, a, budget, c == 0 ? pace : nopace, &g_lstm_poll_timeout);
                pad_bwd_piece<W::NF, CH>(acc, a, bw, CH * c);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[q.w][(q.kq * 4 + r) * 16 + q.i] = acc[r];
        __syncthreads();
        if (q.live) {
            float dg[4];
            lstmh_bwd_gates<HP>(part, q.tid, p, q.b, q.j, t, dc, dg);
            float* out = p.dG + ((long)q.b * p.S + t) * GP + q.j;
#pragma unroll
            for (int g = 0; g < 4; ++g) store_coherent(out + g * HP, dg[g]);
        }
        __syncthreads();
    }
}

template <int KF>
__global__ __launch_bounds__(256) void lstmh_step_bwd_kernel(LstmHBwd p, int t) {
    using W = PadBwd<4, KF>;
    constexpr int HP = W::HP, GP = W::GP, CH = W::CH;
    __shared__ float part[4][256];
    PadTile q;
    const int koff = GP / 4 * q.w + 4 * q.kq;
    float4 bw[W::NF];
    pad_load_whhT<4, KF>(bw, p.whhT, q.j0, q.i, koff);
    q.feed_row(p.B);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t + 1 < p.S) {
        const float* row = p.dG + ((long)q.arow * p.S + t + 1) * GP + koff;
#pragma unroll
        for (int c = 0; c < W::NCH; ++c) {
            float4 a[CH];
#pragma unroll
            for (int ii = 0; ii < CH; ++ii)
                a[ii] = q.ok ? *reinterpret_cast<const float4*>(row + 16 * (CH * c + ii)) : make_float4(0.f, 0.f, 0.f, 0.f);
            pad_bwd_piece<W::NF, CH>(acc, a, bw, CH * c);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[q.w][(q.kq * 4 + r) * 16 + q.i] = acc[r];
    __syncthreads();
    q.gate_thread(p.B);
    if (!q.live) return;
    const int b = q.b, j = q.j;
    float dc = t + 1 < p.S ? p.DC[(long)b * HP + j] : 0.f;
    float dg[4];
    lstmh_bwd_gates<HP>(part, q.tid, p, b, j, t, dc, dg);
    float* out = p.dG + ((long)b * p.S + t) * GP + j;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[g * HP] = dg[g];
    p.DC[(long)b * HP + j] = dc;
}

// ------------------------------------------------------------------ host side
// Which recurrence kernels the cpc_lstm_*_h calls of this process launched since the last cpc_lstm_paths_h(1)
static int g_lstmh_paths = 0;

// The cell as padded_cell.h's layout and drivers see it.  Saved per layer: G (B,S,4Hp), C, Y; carried: h0, c0; the backward's
// own: dG (B,S,4Hp, polled and read by the tail as both dGi and dGh), DC (B,Hp).
struct LstmHCell {
    static constexpr int NG = 4, NS = 2, kDGh = 0, kPerStep = CPC_LSTM_PER_STEP;
    static constexpr const char* kSaved = "ghh";
    static constexpr const char* kOwn = "gs";
    using Fwd = LstmHFwd;
    using Bwd = LstmHBwd;
    static void fill(Fwd& p, float* saved, const long* slot, const float* const* s0, float* const* sN) {
        p.G = saved + slot[0]; p.C = saved + slot[1];
        p.h0 = s0[0]; p.c0 = s0[1]; p.hN = sN[0]; p.cN = sN[1];
    }
    static void fill(Bwd& p, const float* saved, const long* slot, const float* const* s0, float* scratch, const long* own) {
        p.G = saved + slot[0]; p.C = saved + slot[1];
        p.c0 = s0[1];
        p.dG = scratch + own[0]; p.DC = scratch + own[1];
    }
    template <int KF>
    static int recur(const Fwd& p, int per_step, hipStream_t st) {
        return padded_recur_kf(lstmh_persist_fwd_kernel<KF>, lstmh_step_fwd_kernel<KF>, p, KF, false, p.y, 1, kLstmSpinLimit,
                               per_step, &g_lstmh_paths, st);
    }
    template <int KF>
    static int recur(const Bwd& p, int per_step, hipStream_t st) {
        return padded_recur_kf(lstmh_persist_bwd_kernel<KF>, lstmh_step_bwd_kernel<KF>, p, KF, true, p.dG, NG, kLstmSpinLimit,
                               per_step, &g_lstmh_paths, st);
    }
};

}  // namespace cpc

// ---- any hidden width: see include/cpc_hip.h.  H == 256 is cpc_lstm_*_in itself.
extern "C" int cpc_lstm_paths_h(int clear) {
    const int m = g_lstmh_paths;
    if (clear) g_lstmh_paths = 0;
    return m;
}

extern "C" int cpc_lstm_layout_h(int B, int S, int nl, int D, int H, long* sizes) {
    if (H == kLH) return cpc_lstm_layout_in(B, S, nl, D, sizes);
    PaddedLayout g;
    return layout_sizes(padded_layout<LstmHCell>(B, S, nl, D, H, g), g, sizes);
}

extern "C" int cpc_lstm_forward_h(const float* x, const float* h0, const float* c0, const float* const* params, float* saved,
                                  float* scratch, float* y, float* hN, float* cN, int B, int S, int nl, int D, int H, int flags,
                                  void* stream) {
    if (H == kLH) return cpc_lstm_forward_in(x, h0, c0, params, saved, scratch, y, hN, cN, B, S, nl, D, flags, stream);
    const float* st0[2] = {h0, c0};
    float* stN[2] = {hN, cN};
    return padded_forward<LstmHCell>(x, st0, params, saved, scratch, y, stN, B, S, nl, D, H, flags, stream);
}

extern "C" int cpc_lstm_backward_h(const float* x, const float* h0, const float* c0, const float* const* params,
                                   const float* saved, const float* y, const float* dy, float* scratch, float* dx,
                                   float* const* grads, int B, int S, int nl, int D, int H, int flags, void* stream) {
    if (H == kLH) return cpc_lstm_backward_in(x, h0, c0, params, saved, y, dy, scratch, dx, grads, B, S, nl, D, flags, stream);
    const float* st0[2] = {h0, c0};
    return padded_backward<LstmHCell>(x, st0, params, saved, y, dy, scratch, dx, grads, B, S, nl, D, H, flags, stream);
}

