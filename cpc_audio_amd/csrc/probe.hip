// The frozen linear-separability step (cpc/eval/linear_separability.py:21-47 with feature_maker.optimize == False) as ONE C
// call: the linear classifier of SpeakerCriterion / PhoneCriterion on R rows of 256 frozen features, its mean cross-entropy and
// accuracy, the gradients of W and b, and torch.optim.Adam's update of both -- two or three launches instead of the eight of
// cpc_classifier_forward / _backward plus the optimiser's (the chain is latency-bound: DESIGN.md section 4.12).
//
//   probe_tile_kernel    one workgroup per (row slab, class step of 64 classes).  A tile of 32 rows of x and the step's 64 rows
//                        of W stay in LDS.  First walk: logits -> max / argmax / sum-exp per row (-> lse, loss, hit); second
//                        walk: the same logits again -> dlogits = (softmax - onehot) / R on the fly -> the slab's partial dW
//                        (C x 256) and db.  Logits and dlogits never leave the chip.  Products are exact-f32 FMA chains; the
//                        slab's loss and hit sums are float64, rows in order.
//                        C <= 64 (the phone probe): one step, both walks in ONE launch (<kFused>).  More classes (the speaker
//                        probe: B rows, 251 classes -- one workgroup per slab would leave the chip to one or two of them): the
//                        first walk (<kStats>) leaves every row's statistics per step in the workspace (16 bytes per row and
//                        step), the second (<kGrad>) merges them in step order and goes on as above.
//   probe_update_kernel  adds the slabs' partials in slab order and applies adam_one (adam_common.h) to the element it has just
//                        summed; its last workgroup adds the slabs' loss / hit sums and writes loss, acc and the running sums.
//   probe_sums_kernel / probe_sums_split_kernel    (cpc_probe_eval: first walk only) loss, acc and the running sums alone.
// cpc_probe_train_step: two launches for C <= 64, three beyond; cpc_probe_eval: two.  No float atomics, fixed orders everywhere:
// the same bits on every run.
//   probe_wide_kernel    the same tile at D features per row, 1 <= D <= 512 (cpc_probe_train_step_d / cpc_probe_eval_d /
//                        cpc_probe_layout_d): four LDS pitches, the k loop and the dW mapping follow D, 32 classes per step above
//                        256 features; see the comment in front of it.  The update and sums kernels serve both.
#include "adam_common.h"
#include "cpc_common.h"
#include "cpc_internal.h"
#include "probe_tile.h"

namespace cpc {

// (the tile itself -- kPrRows x kPrCls, its loaders, probe_logits, probe_row_stats, probe_merge -- is probe_tile.h's)
constexpr int kPrMaxSlabs = 256;
constexpr long kPrPartFloats = 1L << 22;   // the slabs' dW partials (Z x C x D) stay <= 2^22 floats (16 MiB): 2^14 / C slabs at D = 256
constexpr int kPrMaxDim = 512;             // widest feature row of the _d entry points
constexpr int kPrClsWide = 32;             // ... whose class step above 256 features is 32 classes (see probe_wide_kernel)
enum { kFused = 0, kStats = 1, kGrad = 2 };

// set (bit 0) by a tile that met a label outside [0, C): CPC_DEVERR_LABEL_RANGE, together with supervised.hip's word
static __device__ unsigned g_probe_label_range = 0;

struct ProbeLayout {
    long lse, part, dbp, sums, stat, total;      // offsets in floats (sums: 2 Z doubles; stat: G x R x 4 when G > 1)
    int Z, kchunk, G, D, cls;                    // D features per row; cls classes per step (64; 32 above 256 features)
};

static int probe_layout(int R, int C, int D, ProbeLayout* o) {
    CPC_RETURN_IF(D < 1 || D > kPrMaxDim, CPC_ERR_SHAPE);
    CPC_RETURN_IF(R < 1 || C < 2 || C > kPrMaxClasses, CPC_ERR_SHAPE);
    CPC_RETURN_IF((long)R * C >= (1L << 31), CPC_ERR_SHAPE);
    const int tiles = (R + kPrRows - 1) / kPrRows;
    const int zmax = (int)min((long)kPrMaxSlabs, max(1L, kPrPartFloats / ((long)C * D)));
    const int per = (tiles + zmax - 1) / zmax;
    o->kchunk = per * kPrRows;
    o->Z = (R + o->kchunk - 1) / o->kchunk;
    o->lse = 0;
    o->part = align64l(R);
    o->dbp = o->part + align64l((long)o->Z * C * D);
    o->sums = o->dbp + align64l((long)o->Z * C);
    o->D = D;
    o->cls = D > kC ? kPrClsWide : kPrCls;
    o->G = (C + o->cls - 1) / o->cls;                    // class steps: a workgroup per (slab, step)
    o->stat = o->sums + align64l(4L * o->Z);
    o->total = o->stat + (o->G > 1 ? align64l(4L * o->G * R) : 0);
    return 0;
}

struct ProbeArgs {
    const float* x; long ldx;
    const long long* labels;
    const float* W; const float* b;
    float* lse; float* part; float* dbp; double* sums; float4* stat;
    int R, C, kchunk;
    int D, D4, xvec, wvec;                       // (the _d kernels) features per row, rounded up to 4; may x / W be read 16 bytes at a time?
};

// a row's log-sum-exp, argmax and label logit from the statistics its class steps left in stat[step * R + row]
struct ProbeRow { float lse, ly; int ix; };
__device__ __forceinline__ ProbeRow probe_row(const float4* __restrict__ stat, int nsteps, int R, int row, int yc, int cls) {
    float M = 0.f, S = 1.f, ly = 0.f;
    int ix = 0;
    for (int s = 0; s < nsteps; ++s) {
        const float4 st = stat[(long)s * R + row];
        probe_merge(M, S, ix, st.x, st.y, __builtin_bit_cast(int, st.w), s == 0);
        if (yc / cls == s) ly = st.z;
    }
    return ProbeRow{M + logf(S), ly, ix};
}

// One workgroup per (row slab blockIdx.x, class step blockIdx.y: classes [64 y, 64 y + 64)).
//   kFused  (C <= 64, one step) both walks: statistics, then gradients
//   kStats  the first walk; one step: the rows' results are final (cpc_probe_eval), else this step's statistics go to p.stat
//   kGrad   (several steps) the second walk, from the rows' statistics merged over p.stat
template <int MODE>
__global__ __launch_bounds__(256) void probe_tile_kernel(ProbeArgs p) {
    __shared__ float xs[kPrRows][kPrLd];
    __shared__ float ws[kPrCls][kPrLd];
    __shared__ float lt[kPrRows][kPrCls + 1];            // the tile's logits (first walk), dlogits (second walk)
    __shared__ float bs[kPrCls];
    __shared__ float row_lse[kPrRows], row_loss[kPrRows], row_hit[kPrRows];
    __shared__ int row_y[kPrRows];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int z = blockIdx.x, step = blockIdx.y, nsteps = gridDim.y;
    const int s0 = z * p.kchunk, s1 = min(p.R, s0 + p.kchunk);
    const int ntiles = (s1 - s0 + kPrRows - 1) / kPrRows;
    const int c0 = step * kPrCls, nc = min(kPrCls, p.C - c0);
    const bool sums_here = MODE == kGrad ? step == 0 : nsteps == 1;      // does this workgroup own the slab's loss / hit sums?
    float acc[2][4];
    double loss_sum = 0., hit_sum = 0.;                  // thread 0: the slab's sums, rows in order
    probe_load_w(ws, bs, p, c0);                         // (the first barrier below is in front of its readers)

    // ---- first walk: per-row statistics.  Thread (sr, sq) scans classes sq, sq + 8, .. of row sr of the tile's logits.
    const int sr = tid >> 3, sq = tid & 7;
    for (int t = 0; MODE != kGrad && t < ntiles; ++t) {
        const int r0 = s0 + t * kPrRows;
        const bool live = r0 + sr < s1;
        const long long y = live ? p.labels[r0 + sr] : 0;
        const bool bad = y < 0 || y >= p.C;
        const int yc = bad ? (y < 0 ? 0 : p.C - 1) : (int)y;
        if (bad && sq == 0 && step == 0) atomicOr(&g_probe_label_range, 1u);
        __syncthreads();                                 // the readers of xs / lt of the tile before are done
        if (ntiles > 1 || t == 0) probe_load_x(xs, p, r0);
        __syncthreads();
        probe_logits(xs, ws, bs, tx, ty, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) lt[ty + 16 * i][tx + 16 * j] = acc[i][j];
        __syncthreads();
        float mx, e;
        int mi;
        probe_row_stats(lt, sr, sq, nc, mx, mi, e);
        const float ly = (yc >= c0 && yc < c0 + nc) ? lt[sr][yc - c0] : 0.f;
        if (nsteps > 1) {                                // this step's statistics of the row: merged by the second walk / the sums kernel
            if (sq == 0 && live) p.stat[(long)step * p.R + r0 + sr] = make_float4(mx, e, ly, __builtin_bit_cast(float, c0 + mi));
            continue;
        }
        if (sq == 0) {
            const float lse = mx + logf(e);
            row_lse[sr] = lse;
            row_y[sr] = yc;
            row_loss[sr] = bad ? __builtin_nanf("") : lse - ly;
            row_hit[sr] = (!bad && c0 + mi == yc) ? 1.f : 0.f;
            if (MODE == kFused && ntiles > 1 && live) p.lse[r0 + sr] = lse;
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < kPrRows && r0 + r < s1; ++r) {
                loss_sum += (double)row_loss[r];
                hit_sum += (double)row_hit[r];
            }
    }

    // ---- second walk: dlogits on the fly -> the slab's dW / db partials of this step's classes.  Thread (tk, tc): columns
    // 4 tk .. 4 tk + 3 of the 16 classes tc * 16 .. of the step.
    if (MODE != kStats) {
        const int tk = tid & 63, tc = tid >> 6;
        const float g = 1.f / (float)p.R;
        float dw[16][4];
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) dw[q][e] = 0.f;
        float dbs = 0.f;
        for (int t = 0; t < ntiles; ++t) {
            const int r0 = s0 + t * kPrRows;
            __syncthreads();
            if (ntiles > 1 || MODE == kGrad) probe_load_x(xs, p, r0);        // (kFused, one tile: xs still holds it)
            if (MODE == kGrad) {
                if (tid < kPrRows) {                     // the row's statistics: those of its steps, merged in step order
                    const bool live = r0 + tid < s1;
                    const long long y = live ? p.labels[r0 + tid] : 0;
                    const bool bad = y < 0 || y >= p.C;
                    const int yc = bad ? (y < 0 ? 0 : p.C - 1) : (int)y;
                    const ProbeRow rw = live ? probe_row(p.stat, nsteps, p.R, r0 + tid, yc, kPrCls) : ProbeRow{0.f, 0.f, 0};
                    row_lse[tid] = rw.lse;
                    row_y[tid] = yc;
                    row_loss[tid] = bad ? __builtin_nanf("") : rw.lse - rw.ly;
                    row_hit[tid] = (!bad && rw.ix == yc) ? 1.f : 0.f;
                }
            } else if (ntiles > 1 && tid < kPrRows) {    // (one tile: row_lse / row_y still hold it)
                const bool live = r0 + tid < s1;
                const long long y = live ? p.labels[r0 + tid] : 0;
                row_lse[tid] = live ? p.lse[r0 + tid] : 0.f;
                row_y[tid] = y < 0 ? 0 : (y >= p.C ? p.C - 1 : (int)y);
            }
            __syncthreads();
            if (MODE == kGrad && sums_here && tid == 0)
                for (int r = 0; r < kPrRows && r0 + r < s1; ++r) {
                    loss_sum += (double)row_loss[r];
                    hit_sum += (double)row_hit[r];
                }
            probe_logits(xs, ws, bs, tx, ty, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = ty + 16 * i;
                const float lse = row_lse[r];
                const int yc = row_y[r] - c0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int cc = tx + 16 * j;
                    const bool on = r0 + r < s1 && cc < nc;
                    lt[r][cc] = on ? g * (expf(acc[i][j] - lse) - (cc == yc ? 1.f : 0.f)) : 0.f;
                }
            }
            __syncthreads();
            for (int r = 0; r < kPrRows; ++r) {
                const float4 xv = *reinterpret_cast<const float4*>(&xs[r][4 * tk]);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float d = lt[r][tc * 16 + q];
                    dw[q][0] = fmaf(d, xv.x, dw[q][0]);
                    dw[q][1] = fmaf(d, xv.y, dw[q][1]);
                    dw[q][2] = fmaf(d, xv.z, dw[q][2]);
                    dw[q][3] = fmaf(d, xv.w, dw[q][3]);
                }
            }
            if (tid < kPrCls)
                for (int r = 0; r < kPrRows; ++r) dbs += lt[r][tid];
        }
        float* part = p.part + (long)z * p.C * kC;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int cls = c0 + tc * 16 + q;
            if (cls < p.C)
                *reinterpret_cast<float4*>(part + (long)cls * kC + 4 * tk) = make_float4(dw[q][0], dw[q][1], dw[q][2], dw[q][3]);
        }
        if (tid < nc) p.dbp[(long)z * p.C + c0 + tid] = dbs;
    }
    if (sums_here && tid == 0) {
        p.sums[2 * z] = loss_sum;
        p.sums[2 * z + 1] = hit_sum;
    }
}

// ------------------------------------------------------------------ any feature width: D features per row, 1 <= D <= 512
// The same two walks at a row pitch chosen by D (cpc_probe_*_d).  LD is the LDS pitch of an x or W row: the instantiation's widest
// row, a multiple of 4, plus the 4 floats of kPrLd; the rows themselves hold D4 = D rounded up to 4 columns, zeros behind column D,
// so that the k loop -- D4 / 4 trips, not LD / 4 -- still reads 16 bytes at a time and fmaf(0, 0, s) == s leaves every chain what
// it is over k = 0 .. D - 1.  CLS classes per step: 64, and 32 above 256 features, where 32 + 64 rows of 516 floats would not fit
// the 160 KB of a workgroup.  Halving the class step keeps the step's W resident over all the slab's tiles and each walk one pass
// over x; walking the features in two blocks of 256 would instead reload W for every tile and x twice per tile in the second walk
// (the dlogits of a tile exist only behind its last block).
//   LD   CLS   D          second walk: thread (tk, tc) owns columns 4 tk .. 4 tk + 3 of kQc classes
//   20   64    1 .. 16    tk 0..3,   tc 0..63, 1 class
//   68   64    17 .. 64   tk 0..15,  tc 0..15, 4 classes
//   260  64    65 .. 256  tk 0..63,  tc 0..3,  16 classes
//   516  32    257 .. 512 tk 0..127, tc 0..1,  16 classes
// Threads whose columns lie behind D4 neither accumulate nor store; the partials are (Z, C, D) dense.
template <int LD, int CLS>
struct PwCfg {
    static constexpr int kNv = (LD - 4) / 4;             // 16-byte column groups of the widest row
    static constexpr int kQc = CLS * kNv / 256;          // classes per thread in the second walk
    static constexpr int kJ = CLS / 16;                  // logits per thread and row in probe_wide_logits
    static_assert(kNv <= 128 && (kNv & (kNv - 1)) == 0 && kQc >= 1 && kJ >= 1, "probe_wide_kernel: tile mapping");
};

// rows [r0, r0 + 32) of x -> columns [0, D4) of xs (rows past R, columns past D: zeros); 8 threads per row
template <int LD>
__device__ __forceinline__ void probe_wide_load_x(float (*xs)[LD], const ProbeArgs& p, int r0) {
    const int r = threadIdx.x >> 3, q = threadIdx.x & 7;
    const bool live = r0 + r < p.R;
    const long row = live ? (long)(r0 + r) * p.ldx : 0;
    if (p.xvec) {
        for (int k = 4 * q; k < p.D4; k += 32) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) v = *reinterpret_cast<const float4*>(p.x + row + k);
            *reinterpret_cast<float4*>(&xs[r][k]) = v;
        }
    } else {
        for (int k = q; k < p.D4; k += 8) xs[r][k] = (live && k < p.D) ? p.x[row + k] : 0.f;
    }
}

// classes [c0, c0 + CLS) of W and b -> ws, bs (classes past C, columns past D: zeros); 256 / CLS threads per class
template <int LD, int CLS>
__device__ __forceinline__ void probe_wide_load_w(float (*ws)[LD], float* bs, const ProbeArgs& p, int c0) {
    constexpr int kT = 256 / CLS;
    const int tid = threadIdx.x, c = tid / kT, q = tid % kT;
    const bool live = c0 + c < p.C;
    const long row = live ? (long)(c0 + c) * p.D : 0;
    if (p.wvec) {
        for (int k = 4 * q; k < p.D4; k += 4 * kT) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) v = *reinterpret_cast<const float4*>(p.W + row + k);
            *reinterpret_cast<float4*>(&ws[c][k]) = v;
        }
    } else {
        for (int k = q; k < p.D4; k += kT) ws[c][k] = (live && k < p.D) ? p.W[row + k] : 0.f;
    }
    if (tid < CLS) bs[tid] = c0 + tid < p.C ? p.b[c0 + tid] : 0.f;
}

// acc[i][j] = <x row ty + 16 i, W class tx + 16 j> + b: probe_logits' chain, k = 0 .. D4 - 1 in order for every element, in every walk
template <int LD, int CLS>
__device__ __forceinline__ void probe_wide_logits(const float (*xs)[LD], const float (*ws)[LD], const float* bs, int tx, int ty,
                                                  int D4, float (&acc)[2][PwCfg<LD, CLS>::kJ]) {
    constexpr int kJ = PwCfg<LD, CLS>::kJ;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < kJ; ++j) acc[i][j] = 0.f;
    for (int k = 0; k < D4; k += 4) {
        float4 a[2], w[kJ];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const float4*>(&xs[ty + 16 * i][k]);
#pragma unroll
        for (int j = 0; j < kJ; ++j) w[j] = *reinterpret_cast<const float4*>(&ws[tx + 16 * j][k]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < kJ; ++j) {
                float s = acc[i][j];
                s = fmaf(a[i].x, w[j].x, s);
                s = fmaf(a[i].y, w[j].y, s);
                s = fmaf(a[i].z, w[j].z, s);
                s = fmaf(a[i].w, w[j].w, s);
                acc[i][j] = s;
            }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < kJ; ++j) acc[i][j] += bs[tx + 16 * j];
}

// probe_tile_kernel at D features: one workgroup per (row slab blockIdx.x, class step blockIdx.y: classes [CLS y, CLS y + CLS)),
// the same modes, the same orders; at D = 256 (LD 260, CLS 64) every sum is formed as probe_tile_kernel forms it.
template <int MODE, int LD, int CLS>
__global__ __launch_bounds__(256) void probe_wide_kernel(ProbeArgs p) {
    using Cfg = PwCfg<LD, CLS>;
    __shared__ __attribute__((aligned(16))) float xs[kPrRows][LD];
    __shared__ __attribute__((aligned(16))) float ws[CLS][LD];
    __shared__ float lt[kPrRows][CLS + 1];               // the tile's logits (first walk), dlogits (second walk)
    __shared__ float bs[CLS];
    __shared__ float row_lse[kPrRows], row_loss[kPrRows], row_hit[kPrRows];
    __shared__ int row_y[kPrRows];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int z = blockIdx.x, step = blockIdx.y, nsteps = gridDim.y;
    const int s0 = z * p.kchunk, s1 = min(p.R, s0 + p.kchunk);
    const int ntiles = (s1 - s0 + kPrRows - 1) / kPrRows;
    const int c0 = step * CLS, nc = min(CLS, p.C - c0);
    const bool sums_here = MODE == kGrad ? step == 0 : nsteps == 1;
    float acc[2][Cfg::kJ];
    double loss_sum = 0., hit_sum = 0.;                  // thread 0: the slab's sums, rows in order
    probe_wide_load_w<LD, CLS>(ws, bs, p, c0);           // (the first barrier below is in front of its readers)

    // ---- first walk: per-row statistics.  Thread (sr, sq) scans classes sq, sq + 8, .. of row sr of the tile's logits.
    const int sr = tid >> 3, sq = tid & 7;
    for (int t = 0; MODE != kGrad && t < ntiles; ++t) {
        const int r0 = s0 + t * kPrRows;
        const bool live = r0 + sr < s1;
        const long long y = live ? p.labels[r0 + sr] : 0;
        const bool bad = y < 0 || y >= p.C;
        const int yc = bad ? (y < 0 ? 0 : p.C - 1) : (int)y;
        if (bad && sq == 0 && step == 0) atomicOr(&g_probe_label_range, 1u);
        __syncthreads();                                 // the readers of xs / lt of the tile before are done
        if (ntiles > 1 || t == 0) probe_wide_load_x(xs, p, r0);
        __syncthreads();
        probe_wide_logits<LD, CLS>(xs, ws, bs, tx, ty, p.D4, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < Cfg::kJ; ++j) lt[ty + 16 * i][tx + 16 * j] = acc[i][j];
        __syncthreads();
        float mx, e;
        int mi;
        probe_row_stats(lt, sr, sq, nc, mx, mi, e);
        const float ly = (yc >= c0 && yc < c0 + nc) ? lt[sr][yc - c0] : 0.f;
        if (nsteps > 1) {                                // this step's statistics of the row: merged by the second walk / the sums kernel
            if (sq == 0 && live) p.stat[(long)step * p.R + r0 + sr] = make_float4(mx, e, ly, __builtin_bit_cast(float, c0 + mi));
            continue;
        }
        if (sq == 0) {
            const float lse = mx + logf(e);
            row_lse[sr] = lse;
            row_y[sr] = yc;
            row_loss[sr] = bad ? __builtin_nanf("") : lse - ly;
            row_hit[sr] = (!bad && c0 + mi == yc) ? 1.f : 0.f;
            if (MODE == kFused && ntiles > 1 && live) p.lse[r0 + sr] = lse;
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < kPrRows && r0 + r < s1; ++r) {
                loss_sum += (double)row_loss[r];
                hit_sum += (double)row_hit[r];
            }
    }

    // ---- second walk: dlogits on the fly -> the slab's dW / db partials of this step's classes (the mapping: the table above)
    if (MODE != kStats) {
        const int tk = tid % Cfg::kNv, tc = tid / Cfg::kNv;
        const bool cols = 4 * tk < p.D4;                 // does this thread own columns of the row at all?
        const float g = 1.f / (float)p.R;
        float dw[Cfg::kQc][4];
#pragma unroll
        for (int q = 0; q < Cfg::kQc; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) dw[q][e] = 0.f;
        float dbs = 0.f;
        for (int t = 0; t < ntiles; ++t) {
            const int r0 = s0 + t * kPrRows;
            __syncthreads();
            if (ntiles > 1 || MODE == kGrad) probe_wide_load_x(xs, p, r0);   // (kFused, one tile: xs still holds it)
            if (MODE == kGrad) {
                if (tid < kPrRows) {                     // the row's statistics: those of its steps, merged in step order
                    const bool live = r0 + tid < s1;
                    const long long y = live ? p.labels[r0 + tid] : 0;
                    const bool bad = y < 0 || y >= p.C;
                    const int yc = bad ? (y < 0 ? 0 : p.C - 1) : (int)y;
                    const ProbeRow rw = live ? probe_row(p.stat, nsteps, p.R, r0 + tid, yc, CLS) : ProbeRow{0.f, 0.f, 0};
                    row_lse[tid] = rw.lse;
                    row_y[tid] = yc;
                    row_loss[tid] = bad ? __builtin_nanf("") : rw.lse - rw.ly;
                    row_hit[tid] = (!bad && rw.ix == yc) ? 1.f : 0.f;
                }
            } else if (ntiles > 1 && tid < kPrRows) {    // (one tile: row_lse / row_y still hold it)
                const bool live = r0 + tid < s1;
                const long long y = live ? p.labels[r0 + tid] : 0;
                row_lse[tid] = live ? p.lse[r0 + tid] : 0.f;
                row_y[tid] = y < 0 ? 0 : (y >= p.C ? p.C - 1 : (int)y);
            }
            __syncthreads();
            if (MODE == kGrad && sums_here && tid == 0)
                for (int r = 0; r < kPrRows && r0 + r < s1; ++r) {
                    loss_sum += (double)row_loss[r];
                    hit_sum += (double)row_hit[r];
                }
            probe_wide_logits<LD, CLS>(xs, ws, bs, tx, ty, p.D4, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = ty + 16 * i;
                const float lse = row_lse[r];
                const int yc = row_y[r] - c0;
#pragma unroll
                for (int j = 0; j < Cfg::kJ; ++j) {
                    const int cc = tx + 16 * j;
                    const bool on = r0 + r < s1 && cc < nc;
                    lt[r][cc] = on ? g * (expf(acc[i][j] - lse) - (cc == yc ? 1.f : 0.f)) : 0.f;
                }
            }
            __syncthreads();
            if (cols)
                for (int r = 0; r < kPrRows; ++r) {
                    const float4 xv = *reinterpret_cast<const float4*>(&xs[r][4 * tk]);
#pragma unroll
                    for (int q = 0; q < Cfg::kQc; ++q) {
                        const float d = lt[r][tc * Cfg::kQc + q];
                        dw[q][0] = fmaf(d, xv.x, dw[q][0]);
                        dw[q][1] = fmaf(d, xv.y, dw[q][1]);
                        dw[q][2] = fmaf(d, xv.z, dw[q][2]);
                        dw[q][3] = fmaf(d, xv.w, dw[q][3]);
                    }
                }
            if (tid < CLS)
                for (int r = 0; r < kPrRows; ++r) dbs += lt[r][tid];
        }
        float* part = p.part + (long)z * p.C * p.D;
        if (cols) {
#pragma unroll
            for (int q = 0; q < Cfg::kQc; ++q) {
                const int cls = c0 + tc * Cfg::kQc + q;
                if (cls >= p.C) continue;
                float* dst = part + (long)cls * p.D + 4 * tk;
                if ((p.D & 3) == 0) {                    // (the partials' rows then start 16-byte aligned)
                    *reinterpret_cast<float4*>(dst) = make_float4(dw[q][0], dw[q][1], dw[q][2], dw[q][3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * tk + e < p.D) dst[e] = dw[q][e];
                }
            }
        }
        if (tid < nc) p.dbp[(long)z * p.C + c0 + tid] = dbs;
    }
    if (sums_here && tid == 0) {
        p.sums[2 * z] = loss_sum;
        p.sums[2 * z + 1] = hit_sum;
    }
}

// loss = (sum of the slabs' loss sums) / R, acc likewise, slabs in order (float64); accum[0] += loss, accum[1] += acc
__device__ __forceinline__ void probe_finish(const double* __restrict__ sums, int Z, int R, float* __restrict__ loss,
                                             double* __restrict__ acc, double* __restrict__ accum) {
    double a = 0., h = 0.;
    for (int z = 0; z < Z; ++z) {
        a += sums[2 * z];
        h += sums[2 * z + 1];
    }
    const float l = (float)(a / (double)R);
    const double ac = h / (double)R;
    loss[0] = l;
    acc[0] = ac;
    if (accum) {
        accum[0] += (double)l;
        accum[1] += ac;
    }
}

__global__ __launch_bounds__(64) void probe_sums_kernel(const double* __restrict__ sums, int Z, int R, float* __restrict__ loss,
                                                        double* __restrict__ acc, double* __restrict__ accum) {
    if (threadIdx.x == 0) probe_finish(sums, Z, R, loss, acc, accum);
}

// cpc_probe_eval behind split first walks: every row's steps merged (step order), loss and hit summed per thread over its rows
// (row order) and then over the threads by a fixed tree, in float64
__global__ __launch_bounds__(256) void probe_sums_split_kernel(const float4* __restrict__ stat, const long long* __restrict__ labels,
                                                              int G, int R, int C, int cls, float* __restrict__ loss,
                                                              double* __restrict__ acc, double* __restrict__ accum) {
    __shared__ double sv[256], sh[256];
    const int tid = threadIdx.x;
    double a = 0., h = 0.;
    for (int r = tid; r < R; r += 256) {
        const long long y = labels[r];
        const bool bad = y < 0 || y >= C;
        const int yc = bad ? (y < 0 ? 0 : C - 1) : (int)y;
        const ProbeRow rw = probe_row(stat, G, R, r, yc, cls);
        a += bad ? (double)__builtin_nanf("") : (double)(rw.lse - rw.ly);
        h += (!bad && rw.ix == yc) ? 1. : 0.;
    }
    sv[tid] = a;
    sh[tid] = h;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) { sv[tid] += sv[tid + s]; sh[tid] += sh[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const float l = (float)(sv[0] / (double)R);
        const double ac = sh[0] / (double)R;
        loss[0] = l;
        acc[0] = ac;
        if (accum) {
            accum[0] += (double)l;
            accum[1] += ac;
        }
    }
}

struct ProbeUpdate {
    const float* part; const float* dbp; const double* sums;
    float* W; float* b; float* mW; float* vW; float* mb; float* vb;
    float* dW_out; float* db_out;
    float* loss; double* acc; double* accum;
    int R, C, D, Z;
};

__global__ __launch_bounds__(128) void probe_update_kernel(ProbeUpdate u, AdamCoef coef) {
    if (blockIdx.x == gridDim.x - 1) {                   // the extra workgroup: loss and accuracy
        if (threadIdx.x == 0) probe_finish(u.sums, u.Z, u.R, u.loss, u.acc, u.accum);
        return;
    }
    const long i = (long)blockIdx.x * 128 + threadIdx.x;
    const long nw = (long)u.C * u.D;
    if (i < nw) {
        float s = 0.f;
        for (int z = 0; z < u.Z; ++z) s += u.part[(long)z * nw + i];
        if (u.dW_out) u.dW_out[i] = s;
        float pv = u.W[i], m = u.mW[i], v = u.vW[i];
        adam_one(pv, s, m, v, coef);
        u.W[i] = pv; u.mW[i] = m; u.vW[i] = v;
    } else if (i < nw + u.C) {
        const long c = i - nw;
        float s = 0.f;
        for (int z = 0; z < u.Z; ++z) s += u.dbp[(long)z * u.C + c];
        if (u.db_out) u.db_out[c] = s;
        float pv = u.b[c], m = u.mb[c], v = u.vb[c];
        adam_one(pv, s, m, v, coef);
        u.b[c] = pv; u.mb[c] = m; u.vb[c] = v;
    }
}

int probe_error_flag_fetch(int clear, unsigned* out) { return device_flag_fetch(HIP_SYMBOL(g_probe_label_range), clear, out); }

static ProbeArgs probe_args(const float* x, long ldx, const long long* labels, const float* W, const float* b, float* ws,
                            const ProbeLayout& ly, int R, int C) {
    ProbeArgs p;
    p.x = x; p.ldx = ldx; p.labels = labels; p.W = W; p.b = b;
    p.lse = ws + ly.lse; p.part = ws + ly.part; p.dbp = ws + ly.dbp;
    p.sums = reinterpret_cast<double*>(ws + ly.sums);
    p.stat = reinterpret_cast<float4*>(ws + ly.stat);
    p.R = R; p.C = C; p.kchunk = ly.kchunk;
    p.D = ly.D; p.D4 = (ly.D + 3) & ~3;
    // 16-byte loads only where every one of them is aligned and stays inside the row it reads: with D % 4 != 0 the last one of a
    // row would run up to three floats past it -- past the caller's buffer in the last row
    p.wvec = ((uintptr_t)W & 15) == 0 && (ly.D & 3) == 0;
    p.xvec = ((uintptr_t)x & 15) == 0 && (ldx & 3) == 0 && (ly.D & 3) == 0;
    return p;
}

// the tile kernel of one mode: probe_tile_kernel (the 256 entry points), or probe_wide_kernel at the pitch the width asks for
template <int MODE>
static int probe_launch_tile(const ProbeArgs& p, const ProbeLayout& ly, bool wide, hipStream_t st) {
    const dim3 grid(ly.Z, MODE == kFused ? 1 : ly.G);
    if (!wide) hipLaunchKernelGGL(probe_tile_kernel<MODE>, grid, dim3(256), 0, st, p);
    else if (ly.D <= 16) hipLaunchKernelGGL((probe_wide_kernel<MODE, 20, kPrCls>), grid, dim3(256), 0, st, p);
    else if (ly.D <= 64) hipLaunchKernelGGL((probe_wide_kernel<MODE, 68, kPrCls>), grid, dim3(256), 0, st, p);
    else if (ly.D <= kC) hipLaunchKernelGGL((probe_wide_kernel<MODE, kC + 4, kPrCls>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((probe_wide_kernel<MODE, kPrMaxDim + 4, kPrClsWide>), grid, dim3(256), 0, st, p);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int probe_train_step(const float* x, long ldx, const long long* labels, int R, int C, int D, bool wide, float* W, float* b,
                            float* exp_avg_W, float* exp_avg_sq_W, float* exp_avg_b, float* exp_avg_sq_b, double lr, double beta1,
                            double beta2, double eps, double bias_correction1, double bias_correction2_sqrt, float* workspace,
                            float* loss, double* acc, double* accum, float* dW_out, float* db_out, hipStream_t st) {
    ProbeLayout ly;
    const int rc = probe_layout(R, C, D, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || ldx < D || !labels || !W || !b || !exp_avg_W || !exp_avg_sq_W || !exp_avg_b || !exp_avg_sq_b, CPC_ERR_ARG);
    CPC_RETURN_IF(!workspace || ((uintptr_t)workspace & 15) || !loss || !acc, CPC_ERR_ARG);
    CPC_RETURN_IF(!(bias_correction1 > 0.) || !(bias_correction2_sqrt > 0.), CPC_ERR_ARG);
    const ProbeArgs p = probe_args(x, ldx, labels, W, b, workspace, ly, R, C);
    int r2 = 0;
    if (ly.G == 1) {
        r2 = probe_launch_tile<kFused>(p, ly, wide, st);
    } else {
        r2 = probe_launch_tile<kStats>(p, ly, wide, st);
        if (!r2) r2 = probe_launch_tile<kGrad>(p, ly, wide, st);
    }
    if (r2) return r2;
    ProbeUpdate u;
    u.part = p.part; u.dbp = p.dbp; u.sums = p.sums;
    u.W = W; u.b = b; u.mW = exp_avg_W; u.vW = exp_avg_sq_W; u.mb = exp_avg_b; u.vb = exp_avg_sq_b;
    u.dW_out = dW_out; u.db_out = db_out;
    u.loss = loss; u.acc = acc; u.accum = accum;
    u.R = R; u.C = C; u.D = D; u.Z = ly.Z;
    const AdamCoef coef = adam_coef_from(lr, beta1, beta2, eps, bias_correction1, bias_correction2_sqrt);
    const long n = (long)C * D + C;
    hipLaunchKernelGGL(probe_update_kernel, dim3((unsigned)((n + 127) / 128) + 1), dim3(128), 0, st, u, coef);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int probe_eval(const float* x, long ldx, const long long* labels, int R, int C, int D, bool wide, const float* W,
                      const float* b, float* workspace, float* loss, double* acc, double* accum, hipStream_t st) {
    ProbeLayout ly;
    const int rc = probe_layout(R, C, D, &ly);
    if (rc) return rc;
    CPC_RETURN_IF(!x || ldx < D || !labels || !W || !b, CPC_ERR_ARG);
    CPC_RETURN_IF(!workspace || ((uintptr_t)workspace & 15) || !loss || !acc, CPC_ERR_ARG);
    const ProbeArgs p = probe_args(x, ldx, labels, W, b, workspace, ly, R, C);
    const int r2 = probe_launch_tile<kStats>(p, ly, wide, st);
    if (r2) return r2;
    if (ly.G == 1) hipLaunchKernelGGL(probe_sums_kernel, dim3(1), dim3(64), 0, st, p.sums, ly.Z, R, loss, acc, accum);
    else hipLaunchKernelGGL(probe_sums_split_kernel, dim3(1), dim3(256), 0, st, p.stat, labels, ly.G, R, C, ly.cls, loss, acc, accum);
    CPC_LAUNCH_CHECK();
    return 0;
}

static int probe_layout_sizes(int R, int C, int D, long* sizes) {
    CPC_RETURN_IF(!sizes, CPC_ERR_ARG);
    ProbeLayout ly;
    const int rc = probe_layout(R, C, D, &ly);
    if (rc) return rc;
    sizes[0] = ly.total;
    sizes[1] = ly.Z;
    sizes[2] = ly.kchunk;
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_probe_layout(int R, int C, long* sizes) { return probe_layout_sizes(R, C, kC, sizes); }

extern "C" int cpc_probe_layout_d(int R, int C, int D, long* sizes) { return probe_layout_sizes(R, C, D, sizes); }

extern "C" int cpc_probe_train_step(const float* x, long ldx, const long long* labels, int R, int C, float* W, float* b,
                                    float* exp_avg_W, float* exp_avg_sq_W, float* exp_avg_b, float* exp_avg_sq_b, double lr,
                                    double beta1, double beta2, double eps, double bias_correction1,
                                    double bias_correction2_sqrt, float* workspace, float* loss, double* acc, double* accum,
                                    float* dW_out, float* db_out, void* stream) {
    return probe_train_step(x, ldx, labels, R, C, kC, false, W, b, exp_avg_W, exp_avg_sq_W, exp_avg_b, exp_avg_sq_b, lr, beta1, beta2,
                            eps, bias_correction1, bias_correction2_sqrt, workspace, loss, acc, accum, dW_out, db_out,
                            (hipStream_t)stream);
}

extern "C" int cpc_probe_train_step_d(const float* x, long ldx, const long long* labels, int R, int C, int D, float* W, float* b,
                                      float* exp_avg_W, float* exp_avg_sq_W, float* exp_avg_b, float* exp_avg_sq_b, double lr,
                                      double beta1, double beta2, double eps, double bias_correction1,
                                      double bias_correction2_sqrt, float* workspace, float* loss, double* acc, double* accum,
                                      float* dW_out, float* db_out, void* stream) {
    return probe_train_step(x, ldx, labels, R, C, D, true, W, b, exp_avg_W, exp_avg_sq_W, exp_avg_b, exp_avg_sq_b, lr, beta1, beta2,
                            eps, bias_correction1, bias_correction2_sqrt, workspace, loss, acc, accum, dW_out, db_out,
                            (hipStream_t)stream);
}

extern "C" int cpc_probe_eval(const float* x, long ldx, const long long* labels, int R, int C, const float* W, const float* b,
                              float* workspace, float* loss, double* acc, double* accum, void* stream) {
    return probe_eval(x, ldx, labels, R, C, kC, false, W, b, workspace, loss, acc, accum, (hipStream_t)stream);
}

extern "C" int cpc_probe_eval_d(const float* x, long ldx, const long long* labels, int R, int C, int D, const float* W,
                                const float* b, float* workspace, float* loss, double* acc, double* accum, void* stream) {
    return probe_eval(x, ldx, labels, R, C, D, true, W, b, workspace, loss, acc, accum, (hipStream_t)stream);
}
