// Elman recurrences (torch.nn.RNN semantics, nonlinearity tanh): h_t = tanh(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh).
//
// Two callers (include/cpc_hip.h, cpc_rnn_*):
//   * the criterion's --rnnMode RNN predictors (cpc/criterion/criterion.py:62-64): K nn.RNN(256, 256) built WITHOUT batch_first,
//     so the recurrence walks the batch axis of the (B, W, 256) context -- T = B steps over R = W rows, time-major, G = K heads
//     side by side in the columns of y (B, W, K * 256);
//   * CPCAR with mode "RNN" (cpc/model.py:177-180): nn.RNN(256, 256, nl, batch_first=True) with an optional carried h0.
//
// Structure (lstm.hip's, with one gate):
//   * the input projection of all T steps of a layer (and of all G heads) is ONE GEMM (nt_gemm, b_ih folded in);
//   * the recurrence is one PERSISTENT launch: workgroup = (16 rows) x (64 hidden units), 4 waves splitting the K = 256
//     contraction on exact-f32 16 x 16 x 4 MFMAs; each wave keeps its 64 x 64 quarter of the workgroup's 64 x 256 W_hh slice in
//     registers for all T steps -- the register budget of the LSTM's four 16-unit gate tiles spent on four 16-unit column tiles of
//     the one gate, so a head needs 4 * ceil(R/16) workgroups, a quarter of what 16-unit tiles would take.  h_{t-1} is polled from
//     y itself (persist.h: y pre-filled with the not-ready pattern, agent-scope stores and loads);
//   * G heads ride in blockIdx.z; as many whole heads per launch as can be resident together, the launches one after another;
//   * backward (BPTT): dpre_t = (dy_t + dpre_{t+1} . W_hh) * (1 - y_t^2) -- the same product against W_hh^T, dpre handed over
//     through the fill pattern; y is the only saved state (plus the lower layers' outputs).  dx, dW_ih, dW_hh and both bias
//     gradients are batched GEMMs / reductions over the T * R rows afterwards;
//   * per-step kernels (one launch per step for all heads, same MFMAs and summation order -- bit-identical) serve grids of which
//     not even one head can be resident, and the CPC_RNN_PER_STEP flag;
//   * the host code around the kernels -- input projection, launch choice, the gradients behind the backward recurrence -- is
//     recurrent_host.h's, shared with gru.hip and lstm.hip.
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"
#include "persist.h"
#include "recurrent_host.h"

namespace cpc {

constexpr int kRH = kC;                  // hidden size (256)
constexpr int kRU = 64;                  // hidden units per workgroup
constexpr int kRnnSpinLimit = 1 << 20;   // polling budget per wave and launch

// Set (bit 0) by a wave of a persistent RNN recurrence that gave up polling; read and cleared by cpc_device_error_flags()
// (capi.hip) as CPC_DEVERR_RNN_POLL_TIMEOUT.
static __device__ unsigned g_rnn_poll_timeout = 0;

// One direction of the recurrence over rows (t, r) -> m = t * tsr + r * rsr of arrays whose rows are hs = ng * H floats long, head g
// at columns g * H (time-major: tsr = R, rsr = 1; batch-first: tsr = 1, rsr = T).
//   forward:  w = W_hh (H,H) per head, add = gx = W_ih x + b_ih, bias = b_hh, out = y, first = h0 (R,H) or NULL, last = hN or NULL
//   backward: w = W_hh^T per head, add = dy, yv = y, out = dpre; walks t = T-1 .. 0
struct RnnRec {
    const float* w;
    const float* add;
    const float* bias;    // forward only
    const float* first;   // forward only: h0 of this layer
    const float* yv;      // backward only
    float* out;           // handed over step to step (persistent launch: pre-filled with kNotReady)
    float* last;          // forward only: hN of this layer
    int T, R, tsr, rsr;
    int g0;               // a launch runs the heads g0 + blockIdx.z
    long hs;
};

__device__ __forceinline__ void rnn_head(RnnRec& p) {
    const long g = p.g0 + (int)blockIdx.z;
    p.w += g * kRH * kRH; p.add += g * kRH; p.out += g * kRH;
    if (p.bias) p.bias += g * kRH;
    if (p.yv) p.yv += g * kRH;
}
__device__ __forceinline__ long rnn_row(const RnnRec& p, int t, int r) { return (long)t * p.tsr + (long)r * p.rsr; }

// Lane (i, kq) of wave w holds W[j0 + 16 u + i][koff + 16 ii .. + 4] (koff = 64 w + 4 kq): the B operand of the 16 x 16 x 4 MFMAs
// of column tile u for k = koff + 16 ii + jj, as the fragments of the A operand.
__device__ __forceinline__ void rnn_load_w(float4 (&bw)[4][4], const float* __restrict__ wm, int j0, int i, int koff) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
            bw[u][ii] = *reinterpret_cast<const float4*>(wm + (long)(j0 + 16 * u + i) * kRH + koff + 16 * ii);
}

// This wave's quarter of the product (16 rows x 256) . W^T for the workgroup's four 16 x 16 (row, unit) tiles, into part[w]
__device__ __forceinline__ void rnn_mfma(float (&part)[4][4][256], const float4 (&a)[4], const float4 (&bw)[4][4], int w, int i,
                                         int kq) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[ii], jj), f4c(bw[u][ii], jj), acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) part[w][u][(kq * 4 + r) * 16 + i] = acc[r];
    }
}

// Value of thread tid = (row, col) in column tile u at row m of the arrays, unit j
template <bool BWD>
__device__ __forceinline__ float rnn_cell(const float (&part)[4][4][256], int tid, int u, const RnnRec& p, long m, int j) {
    const float s = (part[0][u][tid] + part[1][u][tid]) + (part[2][u][tid] + part[3][u][tid]);
    if (BWD) {
        const float yv = p.yv[m * p.hs + j];
        return (s + p.add[m * p.hs + j]) * (1.0f - yv * yv);
    }
    return tanhf((s + p.bias[j]) + p.add[m * p.hs + j]);
}

// Fragments of the previous step's values of this lane's row by plain loads: h0 (zeros without it) or a finished launch's output
template <bool BWD>
__device__ __forceinline__ void rnn_load_prev(float4 (&a)[4], const RnnRec& p, int r, bool ok, int koff, int t) {
    const bool start = BWD ? t == p.T - 1 : t == 0;
    const float* src = start ? (!BWD && p.first ? p.first + (long)r * kRH : nullptr)
                             : p.out + rnn_row(p, BWD ? t + 1 : t - 1, r) * p.hs;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
        a[ii] = ok && src ? *reinterpret_cast<const float4*>(src + koff + 16 * ii) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid = (H/64, ceil(R/16), heads), 256 threads; every workgroup resident at once (recur_launch)
template <bool BWD>
__global__ __launch_bounds__(256) void rnn_persist_kernel(RnnRec p, int spin_limit) {
    __shared__ float part[4][4][256];
    rnn_head(p);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * kRU, r0 = blockIdx.y * 16;
    const int koff = 64 * w + 4 * kq;
    float4 bw[4][4];
    rnn_load_w(bw, p.w, j0, i, koff);
    const bool ok = (r0 + i) < p.R;                  // this lane's MFMA row is a row of the problem
    const int arow = ok ? r0 + i : r0;               // (rows past the end poll row r0 -- inside the array -- and are masked)
    const int r = r0 + (tid >> 4), c = tid & 15;
    const bool live = r < p.R;
    int budget = spin_limit;
    PollPace pace(-1);
    for (int q = 0; q < p.T; ++q) {
        const int t = BWD ? p.T - 1 - q : q;
        float4 a[4];
        if (q == 0) rnn_load_prev<BWD>(a, p, arow, ok, koff, t);
        else poll_frags<4, 16>(p.out + rnn_row(p, BWD ? t + 1 : t - 1, arow) * p.hs + koff, ok, a, budget, pace, &g_rnn_poll_timeout);
        rnn_mfma(part, a, bw, w, i, kq);
        __syncthreads();
        if (live) {
            const long m = rnn_row(p, t, r);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + 16 * u + c;
                const float v = rnn_cell<BWD>(part, tid, u, p, m, j);
                store_coherent(p.out + m * p.hs + j, v);
                if (!BWD && q == p.T - 1 && p.last) p.last[(long)r * kRH + j] = v;
            }
        }
        __syncthreads();                             // part is rewritten by the next step's MFMAs
    }
}

// One step per launch: same operands, products and cell math.
template <bool BWD>
__global__ __launch_bounds__(256) void rnn_step_kernel(RnnRec p, int t) {
    __shared__ float part[4][4][256];
    rnn_head(p);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int j0 = blockIdx.x * kRU, r0 = blockIdx.y * 16;
    const int koff = 64 * w + 4 * kq;
    float4 bw[4][4];
    rnn_load_w(bw, p.w, j0, i, koff);
    const bool ok = (r0 + i) < p.R;
    float4 a[4];
    rnn_load_prev<BWD>(a, p, ok ? r0 + i : r0, ok, koff, t);
    rnn_mfma(part, a, bw, w, i, kq);
    __syncthreads();
    const int r = r0 + (tid >> 4), c = tid & 15;
    if (r >= p.R) return;
    const long m = rnn_row(p, t, r);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = j0 + 16 * u + c;
        const float v = rnn_cell<BWD>(part, tid, u, p, m, j);
        p.out[m * p.hs + j] = v;
        if (!BWD && t == p.T - 1 && p.last) p.last[(long)r * kRH + j] = v;
    }
}

// ------------------------------------------------------------------ host side
struct RnnLayout {
    long Y[8];
    long saved_total;
    long gx, fwd_total;
    long whhT, wihT, dP, mid[2], part, tmp, bwd_total;
    long ipf, ipb;        // D != 256: in_proj.hip's scratch behind the forward's / the backward's (the totals include it)
};

// D: the input width of layer 0 (cpc_rnn_*_in, one head); at 256 the layout is the one cpc_rnn_layout has always reported
static bool rnn_layout(int T, int R, int G, int nl, RnnLayout& g, int D = kRH) {
    if (T <= 0 || R <= 0 || G <= 0 || G > 64 || nl <= 0 || nl > 8) return false;
    if (D < 1 || D > kInProjMaxD || (D != kRH && G != 1)) return false;
    if (G > 1 && nl > 1) return false;                                    // stacked layers exist for one head only
    if ((long)T * R > (1L << 21) || (long)T * R * G > (1L << 21)) return false;     // int GEMM rows and offsets
    const long M = (long)T * R, mh = align64l(M * kRH), mg = align64l(M * G * kRH);
    long o = 0;
    for (int l = 0; l < nl; ++l) {
        g.Y[l] = -1;
        if (l < nl - 1) { g.Y[l] = o; o += mh; }
    }
    g.saved_total = o > 0 ? o : 64;                                       // (one layer saves nothing but y itself)
    g.gx = 0;
    g.fwd_total = mg;
    o = 0;
    g.whhT = o; o += (long)G * kRH * kRH;
    g.wihT = o; o += (long)G * kRH * kRH;
    g.dP = o; o += mg;
    g.mid[0] = o; o += nl > 1 ? mh : 0;
    g.mid[1] = o; o += nl > 1 ? mh : 0;
    const long pa = tn_gemm_part_floats((int)M, G * kRH, kRH), pb = (long)G * tn_gemm_part_floats((int)M, kRH, kRH);
    g.part = o; o += align64l(pa > pb ? pa : pb);
    g.tmp = o; o += align64l((long)kRowsSumGroups * G * kRH);
    g.bwd_total = o;
    g.ipf = g.fwd_total; g.ipb = g.bwd_total;
    if (D != kRH) {
        g.fwd_total += in_proj_w_floats(kRH, D);
        g.bwd_total += in_proj_scratch_floats(M, kRH, D);
    }
    return true;
}

// The T steps of one layer's recurrence (all G heads, 4 * ceil(R/16) workgroups each) in either direction
template <bool BWD>
static int rnn_recur(const RnnRec& p, int G, int per_step, hipStream_t st) {
    return recur_launch(rnn_persist_kernel<BWD>, rnn_step_kernel<BWD>, p, dim3(kRH / kRU, cdiv(p.R, 16)), G, p.T, BWD, per_step, p.out,
                        (size_t)p.T * p.R * p.hs, kRnnSpinLimit, st);
}

int rnn_error_flag_fetch(int clear, unsigned* out) { return device_flag_fetch(HIP_SYMBOL(g_rnn_poll_timeout), clear, out); }

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_rnn_layout(int T, int R, int G, int nl, long* sizes) {
    RnnLayout g;
    return layout_sizes(rnn_layout(T, R, G, nl, g), g, sizes);
}

extern "C" int cpc_rnn_layout_in(int T, int R, int nl, int D, long* sizes) {
    RnnLayout g;
    return layout_sizes(rnn_layout(T, R, 1, nl, g, D), g, sizes);
}

// D: x is (.,.,D) and weight_ih_l0 (H,D), one head, either layout (the projection works row by row); D == 256 is cpc_rnn_forward itself
static int rnn_forward_impl(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y,
                            float* hN, int T, int R, int G, int nl, int D, int flags, void* stream) {
    RnnLayout g;
    CPC_RETURN_IF(!rnn_layout(T, R, G, nl, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~(CPC_RNN_PER_STEP | CPC_RNN_TIME_MAJOR), CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !ptrs_ok(params, 4 * nl) || !saved || !scratch || !y, CPC_ERR_ARG);
    CPC_RETURN_IF(G > 1 && (h0 || hN), CPC_ERR_ARG);                     // carried and final state exist for one head only
    hipStream_t st = (hipStream_t)stream;
    const int M = T * R;
    const bool tm = flags & CPC_RNN_TIME_MAJOR;
    float* gx = scratch + g.gx;
    const float* in = x;
    for (int l = 0; l < nl; ++l) {
        float* out = l == nl - 1 ? y : saved + g.Y[l];
        int rc = layer_input_projection(l, D, in, params[4 * l], params[4 * l + 2], scratch + g.ipf, gx, M, G * kRH, st);
        if (rc) return rc;
        RnnRec p;
        p.w = params[4 * l + 1]; p.add = gx; p.bias = params[4 * l + 3];
        p.first = h0 ? h0 + (long)l * R * kRH : nullptr; p.yv = nullptr;
        p.out = out; p.last = hN ? hN + (long)l * R * kRH : nullptr;
        p.T = T; p.R = R; p.tsr = tm ? R : 1; p.rsr = tm ? 1 : T; p.g0 = 0; p.hs = (long)G * kRH;
        rc = rnn_recur<false>(p, G, flags & CPC_RNN_PER_STEP, st);
        if (rc) return rc;
        in = out;
    }
    return 0;
}

extern "C" int cpc_rnn_forward(const float* x, const float* h0, const float* const* params, float* saved, float* scratch, float* y,
                               float* hN, int T, int R, int G, int nl, int flags, void* stream) {
    return rnn_forward_impl(x, h0, params, saved, scratch, y, hN, T, R, G, nl, kRH, flags, stream);
}

extern "C" int cpc_rnn_forward_in(const float* x, const float* h0, const float* const* params, float* saved, float* scratch,
                                  float* y, float* hN, int T, int R, int nl, int D, int flags, void* stream) {
    return rnn_forward_impl(x, h0, params, saved, scratch, y, hN, T, R, 1, nl, D, flags, stream);
}

static int rnn_backward_impl(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                             const float* dy, float* scratch, float* dx, float* const* grads, int T, int R, int G, int nl, int D,
                             int flags, void* stream) {
    RnnLayout g;
    CPC_RETURN_IF(!rnn_layout(T, R, G, nl, g, D), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~(CPC_RNN_PER_STEP | CPC_RNN_TIME_MAJOR), CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !ptrs_ok(params, 4 * nl) || !saved || !y || !dy || !scratch || !dx ||
                  !ptrs_ok(const_cast<const float* const*>(grads), 4 * nl), CPC_ERR_ARG);
    CPC_RETURN_IF(G > 1 && h0, CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const bool tm = flags & CPC_RNN_TIME_MAJOR;
    float* dP = scratch + g.dP;
    const float* dYl = dy;
    for (int l = nl - 1; l >= 0; --l) {
        const float* out = l == nl - 1 ? y : saved + g.Y[l];
        GradTail t;
        t.N = kRH; t.G = G; t.T = T; t.R = R; t.D = l == 0 ? D : kRH; t.time_major = tm;
        t.dGi = t.dGh = dP; t.in = l == 0 ? x : saved + g.Y[l - 1]; t.out = out;
        t.h0 = h0 ? h0 + (long)l * R * kRH : nullptr;
        t.w = params + 4 * l; t.dw = grads + 4 * l; t.dx = l == 0 ? dx : scratch + g.mid[l & 1];
        t.whhT = scratch + g.whhT; t.wihT = scratch + g.wihT; t.part = scratch + g.part; t.tmp = scratch + g.tmp;
        t.ip_scratch = scratch + g.ipb;
        int rc = tail_transposes(t, st);
        if (rc) return rc;
        RnnRec p;
        p.w = t.whhT; p.add = dYl; p.bias = nullptr; p.first = nullptr; p.yv = out; p.out = dP; p.last = nullptr;
        p.T = T; p.R = R; p.tsr = tm ? R : 1; p.rsr = tm ? 1 : T; p.g0 = 0; p.hs = (long)G * kRH;
        rc = rnn_recur<true>(p, G, flags & CPC_RNN_PER_STEP, st);
        if (rc) return rc;
        rc = tail_gradients(t, st);
        if (rc) return rc;
        dYl = t.dx;
    }
    return 0;
}

extern "C" int cpc_rnn_backward(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                                const float* dy, float* scratch, float* dx, float* const* grads, int T, int R, int G, int nl,
                                int flags, void* stream) {
    return rnn_backward_impl(x, h0, params, saved, y, dy, scratch, dx, grads, T, R, G, nl, kRH, flags, stream);
}

extern "C" int cpc_rnn_backward_in(const float* x, const float* h0, const float* const* params, const float* saved, const float* y,
                                   const float* dy, float* scratch, float* dx, float* const* grads, int T, int R, int nl, int D,
                                   int flags, void* stream) {
    return rnn_backward_impl(x, h0, params, saved, y, dy, scratch, dx, grads, T, R, 1, nl, D, flags, stream);
}
