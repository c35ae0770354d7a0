// The front of the PER phone classifier (cpc/eval/common_voices_eval.py, CTCphone_criterion.getPrediction): --seqNorm, the
// per-utterance normalisation of every channel over the utterance's valid frames, with the per-(utterance, channel) scale of
// --dropout (nn.Dropout2d on (B, 256, S): a whole channel of an utterance is kept times 2 or dropped) folded into it.
//
// x (B, S, 256) channels-last, len[b] = n valid frames (int64, read on the device; NULL: n = S), per (b, c):
//   m = mean_{t<n} x[b,t,c]     v = sum_{t<n} (x[b,t,c] - m)^2 / (n - 1)     r = 1 / sqrt(v + 1e-8)
//   y[b,t,c] = (x[b,t,c] - m) r scale[b,c]      for EVERY t < S: the reference normalises the padding with the valid frames'
//                                               statistics, and the head's windows that straddle n read it
// The variance is two-pass (mean first): E[x^2] - m^2 loses 1e-4 .. 1e-3 on features with a channel offset of 30.
// Backward, with g = dy scale, xh = (x - m) r, G1 = sum_{t<S} g, G2 = sum_{t<S} g xh (the padding's y depends on m and r too):
//   dx[b,t,c] = r (g - [t < n] (G1 / n + xh G2 / (n - 1)))
// normalise = 0: y = x scale, dx = dy scale (the dropout alone, behind the LSTM).
//
// One launch each way.  A workgroup of 8 waves owns one utterance and one slab of 64 channels (256 bytes of every frame):
// frame t belongs to time lane q = t & 31, a time lane adds its frames in increasing t, the 32 lane sums of a channel meet in
// LDS and are added in a fixed order (four runs of 8 in lane order, then (p0 + p1) + (p2 + p3)).  So a sum's order depends on
// S and n only -- never on B, the grid or which load path ran -- and an utterance gives the same bits alone and inside a
// batch.  16-byte path: lane = (time lane & 3, channel quad), a wave instruction reads four whole 256-byte rows; where a
// pointer is not 16-byte aligned, the scalar path: lane = channel, four time lanes per wave in four accumulators.  The
// arithmetic is written component by component (no packed fp32, see build.py).  No float atomics.
// n > S or n < 0 sets CPC_DEVERR_LENGTH_RANGE and is clamped; n < 2 (0 included) is no error: r, and with it every y and dx of
// that utterance, is NaN, as torch.var gives, and the other utterances keep their bits.
//
// Any feature width (cpc_seqnorm_*_d, 1 <= D <= 512): the same kernels with the width as their template argument DC -- 256 for
// the entry points above, 0 for "read the argument".  Rows, stats and scale are dense at pitch D, an utterance has ceil(D / 64)
// slabs, and the last slab's threads whose channel is >= D neither load nor store (they add zeros into LDS columns nobody
// reads).  The 16-byte path also needs D % 4 == 0: otherwise a row's start is misaligned and a quad can straddle its end.
// A channel's arithmetic still depends on S and n only, so channel c of an utterance has the same bits at every D.
#include "cpc_common.h"
#include "cpc_internal.h"

namespace cpc {

constexpr int kSnSlab = 64;                          // channels of a workgroup
constexpr int kSnMaxD = 512;                         // widest row of the _d entry points
constexpr int kSnThreads = 512, kSnWaves = kSnThreads / 64;
constexpr int kSnTile = 4 * kSnWaves;                // time lanes = frames of one step of the workgroup
constexpr int kSnRuns = 4, kSnRunLen = kSnTile / kSnRuns;
constexpr float kSnEps = 1e-8f;

static __device__ unsigned g_sn_error = 0;           // != 0: CPC_DEVERR_LENGTH_RANGE

struct SnLds {
    float part[kSnTile][kSnSlab];
    float run[kSnRuns][kSnSlab];
};

// A thread's four elements e of one step: VEC: channels cl + e of time lane q; scalar: channel cl of time lanes q + e.
// D = DC, or the argument where DC is 0: the row pitch; b, c0: the workgroup's utterance and first channel; live: the thread's
// channels exist (VEC: D % 4 == 0, so a quad is whole or absent).
template <bool VEC, int DC>
struct SnLane {
    int q, cl, D, b, c0;
    bool live;
    __device__ SnLane(int Dr) {
        const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
        q = VEC ? 4 * w + (lane >> 4) : 4 * w;
        cl = VEC ? 4 * (lane & 15) : lane;
        D = DC ? DC : Dr;
        const int slabs = (D + kSnSlab - 1) / kSnSlab;
        b = blockIdx.x / slabs;
        c0 = (blockIdx.x % slabs) * kSnSlab;
        live = DC ? true : c0 + cl < D;
    }
    __device__ __forceinline__ int chan(int e) const { return VEC ? cl + e : cl; }
    __device__ __forceinline__ int frame(int e) const { return VEC ? q : q + e; }
};

// frames t0 + .. of the slab's rows at p (row stride D); FULL: every frame of the step is below lim
template <bool VEC, bool FULL, int DC>
__device__ __forceinline__ void sn_load(const float* __restrict__ p, const SnLane<VEC, DC>& ln, int t0, int lim, float (&v)[4]) {
    if (VEC) {
        const int t = t0 + ln.q;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if ((FULL || t < lim) && ln.live) a = *reinterpret_cast<const f32x4*>(p + (long)t * ln.D + ln.cl);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = t0 + ln.q + e;
            v[e] = ((FULL || t < lim) && ln.live) ? p[(long)t * ln.D + ln.cl] : 0.f;
        }
    }
}

template <bool VEC, bool FULL, int DC>
__device__ __forceinline__ void sn_store(float* __restrict__ p, const SnLane<VEC, DC>& ln, int t0, int lim, const float (&v)[4]) {
    if (VEC) {
        const int t = t0 + ln.q;
        const f32x4 a = {v[0], v[1], v[2], v[3]};
        if ((FULL || t < lim) && ln.live) *reinterpret_cast<f32x4*>(p + (long)t * ln.D + ln.cl) = a;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = t0 + ln.q + e;
            if ((FULL || t < lim) && ln.live) p[(long)t * ln.D + ln.cl] = v[e];
        }
    }
}

// the 32 time-lane sums of every channel of the slab -> the channel's total, in every thread that owns the channel
template <bool VEC, int DC>
__device__ __forceinline__ void sn_reduce(SnLds& s, const SnLane<VEC, DC>& ln, const float (&acc)[4], float (&tot)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s.part[ln.frame(e)][ln.chan(e)] = acc[e];
    __syncthreads();
    if (threadIdx.x < kSnRuns * kSnSlab) {
        const int c = threadIdx.x & (kSnSlab - 1), g = threadIdx.x >> 6;
        float a = s.part[g * kSnRunLen][c];
#pragma unroll
        for (int i = 1; i < kSnRunLen; ++i) a += s.part[g * kSnRunLen + i][c];
        s.run[g][c] = a;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = ln.chan(e);
        tot[e] = (s.run[0][c] + s.run[1][c]) + (s.run[2][c] + s.run[3][c]);
    }
}

// n of utterance b, clamped into [0, S]
__device__ __forceinline__ int sn_length(const long long* __restrict__ len, int b, int S) {
    if (!len) return S;
    const long long l = len[b];
    const int n = l < 0 ? 0 : (l > S ? S : (int)l);
    if (l != n && threadIdx.x == 0) atomicOr(&g_sn_error, 1u);
    return n;
}

// BODY for every step of the frames below lim, each time lane in increasing t: whole steps unmasked (FULL), then the ragged one.
// The loop vectoriser is kept off the step loop: on the scalar path it turns the four frames of a lane into v_pk_*_f32.
#define SN_FOR_STEPS(lim, ...)                                              \
    {                                                                       \
        const int full__ = (lim) / kSnTile * kSnTile;                       \
        _Pragma("clang loop vectorize(disable)") _Pragma("unroll 4")        \
        for (int t0 = 0; t0 < full__; t0 += kSnTile) {                      \
            constexpr bool FULL = true;                                     \
            __VA_ARGS__                                                     \
        }                                                                   \
        if (full__ < (lim)) {                                               \
            constexpr bool FULL = false;                                    \
            const int t0 = full__;                                          \
            __VA_ARGS__                                                     \
        }                                                                   \
    }
#define SN_EACH _Pragma("unroll") for (int e = 0; e < 4; ++e)

template <bool VEC, int DC>
__global__ __launch_bounds__(kSnThreads) void sn_forward_kernel(const float* __restrict__ x, const long long* __restrict__ len,
                                                                const float* __restrict__ scale, float* __restrict__ y,
                                                                float* __restrict__ stats, int S, int normalise, int Dr) {
    __shared__ SnLds s;
    const SnLane<VEC, DC> ln(Dr);
    const int b = ln.b, c0 = ln.c0, D = ln.D;
    const float* xs = x + (long)b * S * D + c0;
    float* ys = y + (long)b * S * D + c0;
    float m[4] = {0.f, 0.f, 0.f, 0.f}, r[4] = {1.f, 1.f, 1.f, 1.f}, sc[4];
    if (normalise) {
        const int n = sn_length(len, b, S);
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, tot[4], v[4];
        SN_FOR_STEPS(n, {
            sn_load<VEC, FULL, DC>(xs, ln, t0, n, v);
            SN_EACH acc[e] += v[e];
        })
        sn_reduce<VEC, DC>(s, ln, acc, tot);
#pragma unroll
        for (int e = 0; e < 4; ++e) { m[e] = tot[e] / (float)n; acc[e] = 0.f; }
        SN_FOR_STEPS(n, {
            sn_load<VEC, FULL, DC>(xs, ln, t0, n, v);
            SN_EACH {
                const float d = (FULL || t0 + ln.frame(e) < n) ? v[e] - m[e] : 0.f;
                acc[e] += d * d;
            }
        })
        sn_reduce<VEC, DC>(s, ln, acc, tot);
#pragma unroll
        for (int e = 0; e < 4; ++e)               // n = 1 is 0 / 0 by itself; n = 0 would be 0 / -1: NaN as torch.var's, not 1e4
            r[e] = n < 2 ? __builtin_nanf("") : 1.0f / sqrtf(tot[e] / (float)(n - 1) + kSnEps);
        if (stats && threadIdx.x < (VEC ? 16 : 64) && ln.live) {  // these threads hold every channel of the slab between them
#pragma unroll
            for (int e = 0; e < (VEC ? 4 : 1); ++e) {
                stats[((long)b * 2 + 0) * D + c0 + ln.chan(e)] = m[e];
                stats[((long)b * 2 + 1) * D + c0 + ln.chan(e)] = r[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sc[e] = (scale && ln.live) ? scale[(long)b * D + c0 + ln.chan(e)] : 1.f;
    float v[4];
    SN_FOR_STEPS(S, {
        sn_load<VEC, FULL, DC>(xs, ln, t0, S, v);
        SN_EACH v[e] = ((v[e] - m[e]) * r[e]) * sc[e];
        sn_store<VEC, FULL, DC>(ys, ln, t0, S, v);
    })
}

template <bool VEC, int DC>
__global__ __launch_bounds__(kSnThreads) void sn_backward_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const long long* __restrict__ len,
                                                                 const float* __restrict__ scale, const float* __restrict__ stats,
                                                                 float* __restrict__ dx, int S, int normalise, int Dr) {
    __shared__ SnLds s;
    const SnLane<VEC, DC> ln(Dr);
    const int b = ln.b, c0 = ln.c0, D = ln.D;
    const long off = (long)b * S * D + c0;
    const float* gs = dy + off;
    float* ds = dx + off;
    float sc[4], g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sc[e] = (scale && ln.live) ? scale[(long)b * D + c0 + ln.chan(e)] : 1.f;
    if (!normalise) {
        SN_FOR_STEPS(S, {
            sn_load<VEC, FULL, DC>(gs, ln, t0, S, g);
            SN_EACH g[e] *= sc[e];
            sn_store<VEC, FULL, DC>(ds, ln, t0, S, g);
        })
        return;
    }
    const float* xs = x + off;
    const int n = sn_length(len, b, S);
    float m[4], r[4], a1[4] = {0.f, 0.f, 0.f, 0.f}, a2[4] = {0.f, 0.f, 0.f, 0.f}, k1[4], k2[4], v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m[e] = ln.live ? stats[((long)b * 2 + 0) * D + c0 + ln.chan(e)] : 0.f;
        r[e] = ln.live ? stats[((long)b * 2 + 1) * D + c0 + ln.chan(e)] : 0.f;
    }
    SN_FOR_STEPS(S, {
        sn_load<VEC, FULL, DC>(gs, ln, t0, S, g);
        sn_load<VEC, FULL, DC>(xs, ln, t0, S, v);
        SN_EACH {
            const bool on = FULL || t0 + ln.frame(e) < S;
            const float ge = g[e] * sc[e], xh = on ? (v[e] - m[e]) * r[e] : 0.f;
            a1[e] += ge;
            a2[e] += ge * xh;
        }
    })
    sn_reduce<VEC, DC>(s, ln, a1, k1);
    sn_reduce<VEC, DC>(s, ln, a2, k2);
#pragma unroll
    for (int e = 0; e < 4; ++e) { k1[e] = k1[e] / (float)n; k2[e] = k2[e] / (float)(n - 1); }
    SN_FOR_STEPS(S, {
        sn_load<VEC, FULL, DC>(gs, ln, t0, S, g);
        sn_load<VEC, FULL, DC>(xs, ln, t0, S, v);
        SN_EACH {
            const float ge = g[e] * sc[e], xh = (v[e] - m[e]) * r[e];
            const float corr = t0 + ln.frame(e) < n ? k1[e] + xh * k2[e] : 0.f;
            g[e] = r[e] * (ge - corr);
        }
        sn_store<VEC, FULL, DC>(ds, ln, t0, S, g);
    })
}

static int sn_shape(int B, int S, int D) {
    CPC_RETURN_IF(D < 1 || D > kSnMaxD, CPC_ERR_SHAPE);
    CPC_RETURN_IF(B < 1 || S < 1 || (long)B * S * D >= (1L << 31), CPC_ERR_SHAPE);
    return 0;
}

static bool sn_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int seqnorm_error_flag_fetch(int clear, unsigned* out) { return device_flag_fetch(HIP_SYMBOL(g_sn_error), clear, out); }

// fixed: the 256 instantiations (the cpc_seqnorm_* entry points); otherwise the ones that read D
#define SN_LAUNCH(kernel, vec, ...)                                                                              \
    if (fixed) {                                                                                                 \
        if (vec) hipLaunchKernelGGL((kernel<true, kC>), grid, block, 0, st, __VA_ARGS__);                        \
        else hipLaunchKernelGGL((kernel<false, kC>), grid, block, 0, st, __VA_ARGS__);                           \
    } else {                                                                                                     \
        if (vec) hipLaunchKernelGGL((kernel<true, 0>), grid, block, 0, st, __VA_ARGS__);                         \
        else hipLaunchKernelGGL((kernel<false, 0>), grid, block, 0, st, __VA_ARGS__);                            \
    }

static int sn_forward(const float* x, const long long* lengths, const float* scale, float* y, float* stats, int B, int S, int D,
                      int normalise, bool fixed, void* stream) {
    const int rc = sn_shape(B, S, D);
    if (rc) return rc;
    CPC_RETURN_IF(!x || !y || x == y || normalise < 0 || normalise > 1, CPC_ERR_ARG);
    const dim3 grid((unsigned)B * ((D + kSnSlab - 1) / kSnSlab)), block(kSnThreads);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && sn_aligned16(x) && sn_aligned16(y);
    SN_LAUNCH(sn_forward_kernel, vec, x, lengths, scale, y, stats, S, normalise, D)
    CPC_LAUNCH_CHECK();
    return 0;
}

static int sn_backward(const float* x, const float* dy, const long long* lengths, const float* scale, const float* stats,
                       float* dx, int B, int S, int D, int normalise, bool fixed, void* stream) {
    const int rc = sn_shape(B, S, D);
    if (rc) return rc;
    CPC_RETURN_IF(!dy || !dx || dy == dx || normalise < 0 || normalise > 1 || (normalise && (!x || !stats || x == dx)),
                  CPC_ERR_ARG);
    const dim3 grid((unsigned)B * ((D + kSnSlab - 1) / kSnSlab)), block(kSnThreads);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && sn_aligned16(dy) && sn_aligned16(dx) && (!normalise || sn_aligned16(x));
    SN_LAUNCH(sn_backward_kernel, vec, x, dy, lengths, scale, stats, dx, S, normalise, D)
    CPC_LAUNCH_CHECK();
    return 0;
}

}  // namespace cpc

using namespace cpc;

extern "C" int cpc_seqnorm_forward(const float* x, const long long* lengths, const float* scale, float* y, float* stats, int B,
                                   int S, int normalise, void* stream) {
    return sn_forward(x, lengths, scale, y, stats, B, S, kC, normalise, true, stream);
}

extern "C" int cpc_seqnorm_forward_d(const float* x, const long long* lengths, const float* scale, float* y, float* stats, int B,
                                     int S, int D, int normalise, void* stream) {
    return sn_forward(x, lengths, scale, y, stats, B, S, D, normalise, false, stream);
}

extern "C" int cpc_seqnorm_backward(const float* x, const float* dy, const long long* lengths, const float* scale,
                                    const float* stats, float* dx, int B, int S, int normalise, void* stream) {
    return sn_backward(x, dy, lengths, scale, stats, dx, B, S, kC, normalise, true, stream);
}

extern "C" int cpc_seqnorm_backward_d(const float* x, const float* dy, const long long* lengths, const float* scale,
                                      const float* stats, float* dx, int B, int S, int D, int normalise, void* stream) {
    return sn_backward(x, dy, lengths, scale, stats, dx, B, S, D, normalise, false, stream);
}
