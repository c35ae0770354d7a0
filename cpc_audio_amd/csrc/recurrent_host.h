// Host-side code the recurrent cells share (gru.hip, lstm.hip, rnn.hip): what stands around a recurrence kernel is the same for
// every cell -- the input projection of a layer in front of it, the gradient GEMMs and reductions over all rows behind the
// backward one, and the choice between one persistent launch and one launch per step.  No device code here: the kernels and the
// structs they take stay with their cell.  H = kC = 256 is the hidden size of all three; the LSTM and the GRU at another hidden
// width (lstm.hip: cpc_lstm_*_h, gru.hip: cpc_gru_*_h) pass their padded width instead, from padded_cell.h, which holds what
// those two share -- device helpers included -- and drives this header's functions for them.
#pragma once
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"

namespace cpc {

static inline bool ptrs_ok(const float* const* v, int n) {
    if (!v) return false;
    for (int k = 0; k < n; ++k)
        if (!v[k]) return false;
    return true;
}

// Body of a cpc_*_layout entry: a shape the layout function refused is CPC_ERR_SHAPE whatever `sizes` is.
// sizes[0] = saved floats, [1] = forward scratch floats, [2] = backward scratch floats
template <class Layout>
static int layout_sizes(bool shape_ok, const Layout& g, long* sizes) {
    CPC_RETURN_IF(!shape_ok, CPC_ERR_SHAPE);
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    sizes[0] = g.saved_total; sizes[1] = g.fwd_total; sizes[2] = g.bwd_total;
    return 0;
}

// How many whole heads (wgs_per_head workgroups of `block` threads each) of a persistent kernel can be resident at once?
// 0: not even one.  Resident workgroups are counted as CUs * max(1, min(occupancy query - 1, 4)): the query is advisory and can
// over-report by one block, and more than 4 blocks of 256 threads per CU are not counted on.
template <class K>
static int heads_per_launch(K kernel, int block, long wgs_per_head) {
    int dev = 0, cus = 0, occ = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, block, 0) != hipSuccess) return 0;
    const int per_cu = occ - 1 > 4 ? 4 : (occ - 1 < 1 ? 1 : occ - 1);
    const long fit = (long)cus * per_cu / wgs_per_head;
    return fit > 64 ? 64 : (int)fit;
}

// The T steps of one layer's recurrence for all G heads, in either direction: as many whole heads per launch of `persist`
// (Rec, spin limit) as can be resident together, the launches one after another, over `handover` (the array the steps hand
// their values over in, `floats` long) pre-filled with the not-ready pattern (persist.h); where not even one head fits, or
// per_step is set, one launch of `step` (Rec, t) per step for all heads.  head_grid: the workgroups of one head (x, y), 256
// threads each; the heads ride in blockIdx.z and a launch starts at head Rec::g0.  *persistent (if given): which of the two ran.
template <class Rec, class KP, class KS>
static int recur_launch(KP persist, KS step, Rec p, dim3 head_grid, int G, int T, bool backward, int per_step, float* handover,
                        size_t floats, int spin_limit, hipStream_t st, bool* persistent = nullptr) {
    const int fit = per_step ? 0 : heads_per_launch(persist, 256, (long)head_grid.x * head_grid.y);
    if (persistent) *persistent = fit >= 1;
    if (fit >= 1) {
        if (hipMemsetAsync(handover, 0xFF, floats * sizeof(float), st) != hipSuccess) return CPC_ERR_ARG;
        for (p.g0 = 0; p.g0 < G; p.g0 += fit)
            hipLaunchKernelGGL(persist, dim3(head_grid.x, head_grid.y, G - p.g0 < fit ? G - p.g0 : fit), dim3(256), 0, st, p,
                               spin_limit);
    } else {
        p.g0 = 0;
        for (int q = 0; q < T; ++q)
            hipLaunchKernelGGL(step, dim3(head_grid.x, head_grid.y, G), dim3(256), 0, st, p, backward ? T - 1 - q : q);
    }
    CPC_LAUNCH_CHECK();
    return 0;
}

// Rows of a (.,.,hs) array over T steps of R sequences, as the B operand of a gradient GEMM whose row m is (sequence, step) in
// the array's own order: batch-first (sequence r, step t at row r * T + t) or time-major (row t * R + r).
//   prev_step_rows: row m reads step t - 1 of its sequence -- h_{t-1} -- and a zero row at t = 0
//   first_step_rows: the R rows at t = 0
// (a RowMap tells real elements from zeros per 256 columns -- element k at position t * tmul + tadd + (k >> 8) -- so a row of
// H > 256 columns counts q = ceil(H / 256) positions per step: the whole row of step -1 then lies below position 0)
static inline RowMap prev_step_rows(const float* a, int T, int R, long hs, bool time_major, int H = kC) {
    const int q = H > kC ? cdiv(H, kC) : 1;
    RowMap m;
    m.base = a; m.rstride = (int)hs; m.tmul = q; m.M = T * R;
    if (time_major) { m.R = T * R; m.bstride = 0; m.off = -(int)(R * hs); m.tadd = -q * R; m.Lin = q * T * R; }
    else { m.R = T; m.bstride = (long)T * hs; m.off = -(int)hs; m.tadd = -q; m.Lin = q * T; }
    return m;
}
static inline RowMap first_step_rows(const float* a, int T, int R, long hs, bool time_major) {
    RowMap m;
    m.base = a; m.R = 1; m.bstride = (time_major ? 1 : (long)T) * hs; m.rstride = 0; m.off = 0;
    m.tmul = 0; m.tadd = 0; m.Lin = 0x7fffffff; m.M = R;
    return m;
}

// Forward input projection of layer l over all M rows: out (M, N) = in . W_ih^T + b_ih, N the gate rows of all heads.  `in` is
// (M, H), but for layer 0 at an input width D != H, whose product runs in in_proj.hip (ip_scratch: in_proj_w_floats).
static inline int layer_input_projection(int l, int D, const float* in, const float* wih, const float* bih, float* ip_scratch,
                                         float* out, int M, int N, hipStream_t st, int H = kC) {
    return l == 0 && D != H ? in_proj_forward(in, D, wih, bih, ip_scratch, out, M, N, D, st)
                            : nt_gemm(plain_rows(in, M, H), wih, H, bih, out, N, N, H, st);
}

// What stands around the backward recurrence of one layer: the weight transposes in front of it (tail_transposes) and,
// behind it, every gradient that is a product or a sum over all T * R rows (tail_gradients).
struct GradTail {
    int N, G;                  // gate rows of a head (3H, 4H or H) and heads, side by side in the columns: rows of G * N floats
    int T, R, D;               // steps, sequences, width of this layer's input (H, but for a layer 0 that is narrower or wider)
    bool time_major;           // row order of dGi, dGh, in and out (prev_step_rows)
    const float* dGi, *dGh;    // pre-activation gradients of the input / the recurrent product (LSTM, RNN: one array for both)
    const float* in, *out;     // this layer's input (T*R, D) and output (T*R, G * H)
    const float* h0;           // (R, H) of this layer or NULL (one head)
    const float* const* w;     // W_ih, W_hh, b_ih, b_hh of this layer (the heads' one behind the other); only the first two are read
    float* const* dw;          // ... and their gradients, overwritten
    float* dx;                 // (T*R, D)
    float* whhT, *wihT;        // scratch: G * N * H floats each
    float* part, *tmp;         // scratch: the TN GEMMs' split partials, the bias reductions' partial sums
    float* ip_scratch;         // D != H: in_proj_scratch_floats
    int H = kC;                // hidden width (a multiple of 128: the TN GEMM's tile)
};

// per head (N,H) -> (H,N); the stacked (G N,H) -> (H,G N), but for a narrow layer 0 (in_proj.hip reads W_ih as it lies)
static inline int tail_transposes(const GradTail& t, hipStream_t st) {
    const int rc = transpose(t.w[1], t.whhT, t.N, t.H, st, t.G, (long)t.N * t.H, (long)t.N * t.H);
    if (rc || t.D != t.H) return rc;
    return transpose(t.w[0], t.wihT, t.G * t.N, t.H, st);
}

// stacked dW_ih = dGi^T . in, dW_hh = dGh^T . h_{t-1} head by head in one launch (+ dGh[t = 0]^T . h0), db_ih = sum dGi,
// db_hh = sum dGh, dx = dGi . W_ih summed over the heads (as NT against W_ih^T)
static inline int tail_gradients(const GradTail& t, hipStream_t st) {
    const int M = t.T * t.R, GN = t.G * t.N, H = t.H;
    const bool narrow = t.D != H;
    const RowMap gim = plain_rows(t.dGi, M, GN), ghm = plain_rows(t.dGh, M, GN);
    int rc = narrow ? in_proj_backward(t.in, t.D, t.w[0], t.dGi, t.ip_scratch, nullptr, t.dw[0], M, GN, t.D, st)
                    : tn_gemm(gim, GN, plain_rows(t.in, M, H), H, t.part, t.dw[0], 0, st);
    if (rc) return rc;
    GemmGroup grp;
    grp.G = t.G; grp.a = t.N; grp.b = H; grp.c = (long)t.N * H;
    rc = tn_gemm(ghm, t.N, prev_step_rows(t.out, t.T, t.R, (long)t.G * H, t.time_major, H), H, t.part, t.dw[1], 0, st, GemmBounds(),
                 grp);
    if (rc) return rc;
    if (t.h0) {
        rc = tn_gemm(first_step_rows(t.dGh, t.T, t.R, GN, t.time_major), t.N, plain_rows(t.h0, t.R, H), H, t.part, t.dw[1], 1, st);
        if (rc) return rc;
    }
    rc = rows_sum(t.dGi, M, GN, t.tmp, t.dw[2], st);
    if (rc) return rc;
    rc = rows_sum(t.dGh, M, GN, t.tmp, t.dw[3], st);
    if (rc) return rc;
    return narrow ? in_proj_backward(t.in, t.D, t.w[0], t.dGi, t.ip_scratch, t.dx, nullptr, M, GN, t.D, st)
                  : nt_gemm(gim, t.wihT, GN, nullptr, t.dx, H, H, GN, st);
}

}  // namespace cpc
