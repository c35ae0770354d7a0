// What the recurrent cells at any hidden width share (gru.hip: cpc_gru_*_h, lstm.hip: cpc_lstm_*_h): the recurrence at the padded
// width Hp = 128 * ceil(H / 128) on zero-padded copies of the parameters.  Everything here is independent of the cell but for
// its number of gates NG (3 or 4) and of carried states: the device helpers of the kernels -- index prologue, W_hh loads, the
// gate products, the backward's piecewise contraction -- and, on the host, the scratch layout, the width dispatch and the two
// drivers around the recurrence.  The kernels, their records and their gate math stay with their cell; a cell describes
// itself to the drivers in a small struct (GruHCell, LstmHCell).  Why a padded unit stays exactly zero is the cell's own
// argument and stands in its file; the drivers pad every carried state with WRITTEN zeros (pad_copy) because the GRU's needs it.
#pragma once
#include "cpc_common.h"
#include "cpc_internal.h"
#include "gemm_tile.h"
#include "persist.h"
#include "recurrent_host.h"

namespace cpc {

// ------------------------------------------------------------------ device side
// grid = (Hp/16, ceil(B/16)), 256 threads.  Lane (i, kq) of wave w feeds the MFMAs with batch row b0 + i (arow: clamped into
// the batch, ok: inside it); thread tid does the gate math of (b, j), live: inside the batch.  Wave w walks the w-th quarter
// of the contraction: the lane's first k is koff = (K / 4) w + 4 kq.
// In three steps, each where the kernels have always had it -- the indices first, feed_row behind the weight loads, gate_thread
// where the gate math starts: the compiler's schedule and register count follow the order of the source.
struct PadTile {
    int tid, lane, w, i, kq, j0, b0, arow, b, j;
    bool ok, live;
    __device__ __forceinline__ PadTile() {
        tid = threadIdx.x; lane = tid & 63; w = tid >> 6;
        i = lane & 15; kq = lane >> 4;
        j0 = blockIdx.x * 16; b0 = blockIdx.y * 16;
    }
    __device__ __forceinline__ void feed_row(int B) {
        ok = (b0 + i) < B;
        arow = ok ? b0 + i : b0;
    }
    __device__ __forceinline__ void gate_thread(int B) {
        b = b0 + (tid >> 4); j = j0 + (tid & 15);
        live = b < B;
    }
};

// Lane (i, kq) of wave w holds W_hh[gate * Hp + j0 + i][koff + 16 ii .. + 4], koff = 16 KF w + 4 kq
template <int NG, int KF>
__device__ __forceinline__ void pad_load_whh(float4 (&bw)[NG][KF], const float* __restrict__ whh, int j0, int i, int koff) {
    constexpr int HP = 64 * KF;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int ii = 0; ii < KF; ++ii)
            bw[g][ii] = *reinterpret_cast<const float4*>(whh + (long)(g * HP + j0 + i) * HP + koff + 16 * ii);
}

template <int NG, int KF>
__device__ __forceinline__ void pad_fwd_mfma(float (&part)[4][NG][256], const float4 (&a)[KF], const float4 (&bw)[NG][KF], int w,
                                             int i, int kq) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ii = 0; ii < KF; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[ii], jj), f4c(bw[g][ii], jj), acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) part[w][g][(kq * 4 + r) * 16 + i] = acc[r];
    }
}

// h_{t-1} of batch row b: h0 (B,Hp) or zeros at t == 0, else y (B,S,Hp)
template <int KF>
__device__ __forceinline__ void pad_load_h(float4 (&a)[KF], const float* h0, const float* y, int S, int b, bool ok, int koff, int t) {
    constexpr int HP = 64 * KF;
    const float* src = t == 0 ? (h0 ? h0 + (long)b * HP : nullptr) : y + ((long)b * S + t - 1) * HP;
#pragma unroll
    for (int ii = 0; ii < KF; ++ii)
        a[ii] = ok && src ? *reinterpret_cast<const float4*>(src + koff + 16 * ii) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- backward: K = NG Hp, a wave's quarter is NG Hp / 4 = 16 * (NG KF) wide.  NF fragments per lane, fetched and multiplied CH
// at a time: at most 16 live beside the NF of W_hh^T.  The pieces are each cell's as it was tuned (GRU: 6, 12, 9, 12; LSTM: 8, 16,
// 8, 16 for KF = 2, 4, 6, 8), not one rule of NF: 24 fragments are two pieces of 12 in the GRU and three of 8 in the LSTM.
template <int NG, int KF> struct PadBwd {
    static_assert(NG == 3 || NG == 4, "gates of a GRU or an LSTM");
    static constexpr int HP = 64 * KF, GP = NG * HP, NF = NG * KF;
    static constexpr int CH = NG == 3 ? (NF <= 16 ? NF : NF / 2) : (NF % 16 == 0 ? 16 : 8), NCH = NF / CH;
    static_assert(CH * NCH == NF && CH <= 16, "equal pieces of at most 16 fragments");
};

template <int NG, int KF>
__device__ __forceinline__ void pad_load_whhT(float4 (&bw)[NG * KF], const float* __restrict__ whhT, int j0, int i, int koff) {
#pragma unroll
    for (int ii = 0; ii < NG * KF; ++ii)
        bw[ii] = *reinterpret_cast<const float4*>(whhT + (long)(j0 + i) * (64 * NG * KF) + koff + 16 * ii);
}

// one piece of the contraction: fragments c0 .. c0 + CH of this lane
template <int NF, int CH>
__device__ __forceinline__ void pad_bwd_piece(f32x4& acc, const float4 (&a)[CH], const float4 (&bw)[NF], int c0) {
#pragma unroll
    for (int ii = 0; ii < CH; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(a[ii], jj), f4c(bw[c0 + ii], jj), acc, 0, 0, 0);
}
// (The loop over the NCH pieces -- poll or load one, multiply it, then the next, then part[w] = acc -- stands in each backward
// kernel, not here.  Behind a function of its own the compiler moves the MFMAs of a piece below the poll of the next one, and two
// pieces are live at once: lstmh_persist_bwd_kernel<8> then takes 256 + 28 registers for 214 + 4 and halves its occupancy.)

// ------------------------------------------------------------------ host side
static inline int padded_width(int H) { return 128 * cdiv(H, 128); }

// Offsets (floats) into saved, the forward scratch and the backward scratch.  The slots every cell has are named; the cell's
// own are numbered in the order it lists them: saved[l][k] per layer (the last of them the layer's padded output, Y[l]), the
// carried states (h0, then c0) and own[k], the backward's hand-over arrays.
struct PaddedLayout {
    int Hp;
    long saved[8][5], Y[8];                                   // saved: every layer keeps its padded output
    long saved_total;
    long gx, wih, whh, bih, bhh, st0[2], stN[2], ipf, fwd_total;
    long whhT, wihT, wihp, whhp, own[3], mid[2], bst[2], gwih, gwhh, gbih, gbhh, part, tmp, ipb, bwd_total;
};

// NG gates, ns carried states.  saved / own: one letter per slot -- 'g': (B,S,NG Hp), 'h': (B,S,Hp), 's': (B,Hp).
// The limits: the GEMM row maps (gemm_tile.h) count B * S rows in 21 bits, and a row offset into a (B,S,NG Hp) array is 32-bit.
static inline bool padded_layout(int NG, int ns, const char* saved, const char* own, int B, int S, int nl, int D, int H,
                                 PaddedLayout& g) {
    if (B <= 0 || S <= 0 || nl <= 0 || nl > 8 || D < 1 || D > kInProjMaxD || H < 1 || H > 512) return false;
    const int Hp = padded_width(H), Gp = NG * Hp;
    const long M = (long)B * S;
    if (M > (1L << 21) || M * Gp > (1L << 31)) return false;
    g.Hp = Hp;
    const long mh = align64l(M * Hp), mg = align64l(M * Gp), wi = (long)Gp * (D > Hp ? D : Hp), wh = (long)Gp * Hp;
    const long st = align64l((long)nl * B * Hp), bh = align64l((long)B * Hp);
    auto slot = [&](char c) { return c == 'g' ? mg : c == 'h' ? mh : bh; };
    long o = 0;
    for (int l = 0; l < nl; ++l)
        for (int k = 0; saved[k]; ++k) {
            g.saved[l][k] = g.Y[l] = o; o += slot(saved[k]);
        }
    g.saved_total = o;
    o = 0;
    g.gx = o; o += mg;
    g.wih = o; o += align64l(wi);
    g.whh = o; o += wh;
    g.bih = o; o += Gp;
    g.bhh = o; o += Gp;
    for (int k = 0; k < ns; ++k) { g.st0[k] = o; o += st; }
    for (int k = 0; k < ns; ++k) { g.stN[k] = o; o += st; }
    g.ipf = o; o += in_proj_w_floats(Gp, D);
    g.fwd_total = o;
    o = 0;
    g.whhT = o; o += wh;
    g.wihT = o; o += wh;
    g.wihp = o; o += align64l(wi);
    g.whhp = o; o += wh;
    for (int k = 0; own[k]; ++k) { g.own[k] = o; o += slot(own[k]); }
    g.mid[0] = o; o += mh;
    g.mid[1] = o; o += mh;
    for (int k = 0; k < ns; ++k) { g.bst[k] = o; o += bh; }
    g.gwih = o; o += align64l(wi);
    g.gwhh = o; o += wh;
    g.gbih = o; o += Gp;
    g.gbhh = o; o += Gp;
    g.part = o; o += align64l(tn_gemm_part_floats((int)M, Gp, Hp));
    g.tmp = o; o += align64l((long)kRowsSumGroups * Gp);
    g.ipb = o; o += in_proj_scratch_floats(M, Gp, D);
    g.bwd_total = o;
    return true;
}

template <class Cell>
static bool padded_layout(int B, int S, int nl, int D, int H, PaddedLayout& g) {
    return padded_layout(Cell::NG, Cell::NS, Cell::kSaved, Cell::kOwn, B, S, nl, D, H, g);
}

// One layer's recurrence at Hp = 64 KF (recur_launch): `polled` is (B,S,w Hp).  *paths: bit 0 a persistent launch ran, bit 1 the
// per-step ones (the residency fallback of recur_launch, or the cell's PER_STEP flag).
template <class Rec, class KP, class KS>
static int padded_recur_kf(KP persist, KS step, const Rec& p, int KF, bool backward, float* polled, int w, int spin_limit,
                           int per_step, int* paths, hipStream_t st) {
    bool persistent = false;
    const int rc = recur_launch(persist, step, p, dim3(4 * KF, cdiv(p.B, 16)), 1, p.S, backward, per_step, polled,
                                (size_t)p.B * p.S * 64 * w * KF, spin_limit, st, &persistent);
    *paths |= persistent ? 1 : 2;
    return rc;
}
// the instantiation of the padded width Hp in {128, 256, 384, 512}: Cell::recur<KF> names the cell's kernels
template <class Cell, class Rec>
static int padded_recur(const Rec& p, int Hp, int per_step, hipStream_t st) {
    switch (Hp) {
        case 128: return Cell::template recur<2>(p, per_step, st);
        case 256: return Cell::template recur<4>(p, per_step, st);
        case 384: return Cell::template recur<6>(p, per_step, st);
        case 512: return Cell::template recur<8>(p, per_step, st);
    }
    return CPC_ERR_SHAPE;
}

#define PAD_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// nn.GRU / nn.LSTM (D, H, nl, batch_first) forward.  st0: the Cell::NS carried states (nl,B,H), all or none; stN: the final ones.
template <class Cell>
static int padded_forward(const float* x, const float* const* st0, const float* const* params, float* saved, float* scratch,
                          float* y, float* const* stN, int B, int S, int nl, int D, int H, int flags, void* stream) {
    constexpr int NG = Cell::NG, NS = Cell::NS;
    PaddedLayout g;
    CPC_RETURN_IF(!padded_layout<Cell>(B, S, nl, D, H, g), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~Cell::kPerStep, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !ptrs_ok(params, 4 * nl) || !saved || !scratch || !y || !ptrs_ok(stN, NS), CPC_ERR_ARG);
    for (int k = 1; k < NS; ++k) CPC_RETURN_IF((st0[0] == nullptr) != (st0[k] == nullptr), CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const int Hp = g.Hp, Gp = NG * Hp, M = B * S;
    if (st0[0])
        for (int k = 0; k < NS; ++k) PAD_TRY(pad_copy(st0[k], scratch + g.st0[k], 1, (long)nl * B, H, (long)nl * B, Hp, st));
    const float* in = x;
    for (int l = 0; l < nl; ++l) {
        const int Dl = l == 0 ? D : H, Dlp = l == 0 ? D : Hp;          // true and internal width of this layer's input
        PAD_TRY(pad_copy(params[4 * l], scratch + g.wih, NG, H, Dl, Hp, Dlp, st));
        PAD_TRY(pad_copy(params[4 * l + 1], scratch + g.whh, NG, H, H, Hp, Hp, st));
        PAD_TRY(pad_copy(params[4 * l + 2], scratch + g.bih, NG, 1, H, 1, Hp, st));
        PAD_TRY(pad_copy(params[4 * l + 3], scratch + g.bhh, NG, 1, H, 1, Hp, st));
        PAD_TRY(layer_input_projection(l, D, in, scratch + g.wih, scratch + g.bih, scratch + g.ipf, scratch + g.gx, M, Gp, st, Hp));
        const float* s0[NS];
        float* sN[NS];
        for (int k = 0; k < NS; ++k) {
            s0[k] = st0[0] ? scratch + g.st0[k] + (long)l * B * Hp : nullptr;
            sN[k] = scratch + g.stN[k] + (long)l * B * Hp;
        }
        typename Cell::Fwd p;
        p.gx = scratch + g.gx; p.whh = scratch + g.whh; p.bhh = scratch + g.bhh;
        p.y = saved + g.Y[l];
        p.B = B; p.S = S; p.g0 = 0;
        Cell::fill(p, saved, g.saved[l], s0, sN);
        PAD_TRY(padded_recur<Cell>(p, Hp, flags & Cell::kPerStep, st));
        in = p.y;
    }
    PAD_TRY(pad_copy(in, y, 1, M, Hp, M, H, st));
    for (int k = 0; k < NS; ++k) PAD_TRY(pad_copy(scratch + g.stN[k], stN[k], 1, (long)nl * B, Hp, (long)nl * B, H, st));
    return 0;
}

template <class Cell>
static int padded_backward(const float* x, const float* const* st0, const float* const* params, const float* saved,
                           const float* y, const float* dy, float* scratch, float* dx, float* const* grads, int B, int S, int nl,
                           int D, int H, int flags, void* stream) {
    constexpr int NG = Cell::NG, NS = Cell::NS;
    PaddedLayout g;
    CPC_RETURN_IF(!padded_layout<Cell>(B, S, nl, D, H, g), CPC_ERR_SHAPE);
    CPC_RETURN_IF(flags & ~Cell::kPerStep, CPC_ERR_ARG);
    CPC_RETURN_IF(!x || !ptrs_ok(params, 4 * nl) || !saved || !y || !dy || !scratch || !dx ||
                  !ptrs_ok(const_cast<const float* const*>(grads), 4 * nl), CPC_ERR_ARG);
    for (int k = 1; k < NS; ++k) CPC_RETURN_IF((st0[0] == nullptr) != (st0[k] == nullptr), CPC_ERR_ARG);
    hipStream_t st = (hipStream_t)stream;
    const int Hp = g.Hp, Gp = NG * Hp, M = B * S;
    // dy at the padded width in the mid[] slot the top layer does not write (the layer below it may: dy is spent by then)
    float* dyp = scratch + g.mid[nl & 1];
    PAD_TRY(pad_copy(dy, dyp, 1, M, H, M, Hp, st));
    const float* dYl = dyp;
    for (int l = nl - 1; l >= 0; --l) {
        const int Dl = l == 0 ? D : H, Dlp = l == 0 ? D : Hp;
        PAD_TRY(pad_copy(params[4 * l], scratch + g.wihp, NG, H, Dl, Hp, Dlp, st));
        PAD_TRY(pad_copy(params[4 * l + 1], scratch + g.whhp, NG, H, H, Hp, Hp, st));
        const float* s0[NS];
        for (int k = 0; k < NS; ++k) {
            s0[k] = st0[0] ? scratch + g.bst[k] : nullptr;
            if (st0[0]) PAD_TRY(pad_copy(st0[k] + (long)l * B * H, scratch + g.bst[k], 1, B, H, B, Hp, st));
        }
        const float* wp[4] = {scratch + g.wihp, scratch + g.whhp, nullptr, nullptr};      // (the tail reads no bias)
        float* gp[4] = {scratch + g.gwih, scratch + g.gwhh, scratch + g.gbih, scratch + g.gbhh};
        GradTail t;
        t.H = Hp; t.N = Gp; t.G = 1; t.T = S; t.R = B; t.D = Dlp; t.time_major = false;
        t.dGi = scratch + g.own[0]; t.dGh = scratch + g.own[Cell::kDGh];
        t.in = l == 0 ? x : saved + g.Y[l - 1]; t.out = saved + g.Y[l];
        t.h0 = s0[0];
        t.w = wp; t.dw = gp; t.dx = l == 0 ? dx : scratch + g.mid[l & 1];
        t.whhT = scratch + g.whhT; t.wihT = scratch + g.wihT; t.part = scratch + g.part; t.tmp = scratch + g.tmp;
        t.ip_scratch = scratch + g.ipb;
        PAD_TRY(tail_transposes(t, st));
        typename Cell::Bwd p;
        p.whhT = t.whhT; p.dY = dYl;
        p.B = B; p.S = S; p.g0 = 0;
        Cell::fill(p, saved, g.saved[l], s0, scratch, g.own);
        PAD_TRY(padded_recur<Cell>(p, Hp, flags & Cell::kPerStep, st));
        PAD_TRY(tail_gradients(t, st));
        PAD_TRY(pad_copy(gp[0], grads[4 * l], NG, Hp, Dlp, H, Dl, st));
        PAD_TRY(pad_copy(gp[1], grads[4 * l + 1], NG, Hp, Hp, H, H, st));
        PAD_TRY(pad_copy(gp[2], grads[4 * l + 2], NG, 1, Hp, 1, H, st));
        PAD_TRY(pad_copy(gp[3], grads[4 * l + 3], NG, 1, Hp, 1, H, st));
        dYl = t.dx;
    }
    return 0;
}

}  // namespace cpc
