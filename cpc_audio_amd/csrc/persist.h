// Fill-pattern hand-over of the persistent recurrences (gru.hip, lstm.hip, rnn.hip).
//
// A persistent launch runs all S steps of a recurrence; a workgroup takes the values other workgroups produced in the
// previous step straight from the arrays they are written to.  The host fills those arrays with 0xFFFFFFFF (a NaN payload
// no arithmetic result carries), producers store with agent-scope atomics (write-through) and consumers poll the
// fragments they need with agent-scope atomic loads until no lane sees the fill pattern.  Each 4-byte value validates
// itself, so there is no flag, counter or fence on the chain.  Polling is bounded: a wave that gives up sets its
// kernel's device error bit and lets the fill pattern -- a NaN -- through, and the launch still terminates.
#pragma once
#include "cpc_common.h"

namespace cpc {

constexpr unsigned kNotReady = 0xFFFFFFFFu;

__device__ __forceinline__ float4 load4_coherent(const float* p) {
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float4(__uint_as_float((unsigned)lo), __uint_as_float((unsigned)(lo >> 32)),
                       __uint_as_float((unsigned)hi), __uint_as_float((unsigned)(hi >> 32)));
}
// the same 16 bytes by PLAIN loads (wavefront-scope atomics: global_load without sc bits -- served by this XCD's L2, which the
// workgroups of a tile on the XCD then share; what it returns may be stale, so only a FIRST look may use it: poll_frags)
__device__ __forceinline__ float4 load4_plain(const float* p) {
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return make_float4(__uint_as_float((unsigned)lo), __uint_as_float((unsigned)(lo >> 32)),
                       __uint_as_float((unsigned)hi), __uint_as_float((unsigned)(hi >> 32)));
}
__device__ __forceinline__ bool ready4(float4 v) {
    return __float_as_uint(v.x) != kNotReady && __float_as_uint(v.y) != kNotReady &&
           __float_as_uint(v.z) != kNotReady && __float_as_uint(v.w) != kNotReady;
}
__device__ __forceinline__ void store_coherent(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Fetch NII float4 fragments (STRIDE floats apart) of this lane's row, re-reading until every lane of the wave
// has complete data.  Lanes whose row is outside the batch contribute zeros (their loads still go out: `row` must
// point into the buffer for them too).  A wave that runs out of budget ORs 1 into *timeout_flag.
// Pacing.  Every look is a device-scope load that travels to L2 and back whatever it finds, and sixteen workgroups per XCD
// looking flat out slow one another's hand-over down (measured at B = 64: forward 0.41 -> 0.28 ms, backward 0.77 -> 0.67 ms
// once the looks that cannot succeed are left out).  The data cannot be there before the producers' gate math is done, so a
// wave first sleeps `delay` x 64 clocks.  The right delay depends on the kernel, the batch and on what else runs on the
// chip, so each wave steers its own (PollPace): a look that had to be repeated came too early (delay += 2; 4 until round 6), four first-time
// hits in a row may have come late (delay -= 1); the steady state is about one repeated look in twenty steps.
// fixed >= 0 pins the delay instead (cpc_set_gru_poll_pacing).
struct PollPace {
    int delay, streak, fixed, up, clean;
    // fixed_ >= 0: pinned delay; -1: self-steering with the default steps (up 2, one down per 4 clean steps -- round 6: (2, 4)
    // against the (4, 4) of rounds 2-5 is worth 4 us forward and 9 us backward at B = 64, tools/ab_gru_pace.py); <= -2: self-steering
    // with up = (-fixed_) >> 4, clean = (-fixed_) & 15 (cpc_set_gru_poll_pacing: A/B of the steering constants)
    __device__ explicit PollPace(int fixed_) : delay(fixed_ > 0 ? fixed_ : 0), streak(0), fixed(fixed_), up(2), clean(4) {
        if (fixed_ <= -2) { up = (-fixed_) >> 4; clean = (-fixed_) & 15; if (clean < 1) clean = 1; }
    }
    __device__ __forceinline__ void update(int repeats) {     // wave-uniform
        if (fixed >= 0) return;
        if (repeats == 0) {
            if (++streak >= clean) { streak = 0; delay = delay > 0 ? delay - 1 : 0; }
        } else {
            streak = 0;
            delay = delay + up < 96 ? delay + up : 96;
        }
    }
};

// plain_first: the first look with plain loads (load4_plain) -- a hand-over address is read once per launch by a wave, the
// buffers were filled by a previous launch and written since by write-through stores only, so a line this XCD's L2 does not hold
// yet comes from memory as it is now, and the other workgroups of the tile on this XCD hit it there instead of crossing the
// fabric each; a line fetched too early stays stale in that L2, which the repeated looks (always device scope) get around.
template <int NII, int STRIDE>
__device__ __forceinline__ void poll_frags(const float* __restrict__ row, bool ok, float4 (&a)[NII], int& budget,
                                           PollPace& pace, unsigned* timeout_flag, bool plain_first = false) {
    for (int q = 0; q < pace.delay; ++q) __builtin_amdgcn_s_sleep(1);
    // Unconditional loads (a predicated load costs a branch and a full vmcnt(0) each): rows past the batch
    // are inside the buffer, never written, and masked out below.
    if (plain_first) {                                            // wave-uniform
#pragma unroll
        for (int ii = 0; ii < NII; ++ii) a[ii] = load4_plain(row + STRIDE * ii);
    } else {
#pragma unroll
        for (int ii = 0; ii < NII; ++ii) a[ii] = load4_coherent(row + STRIDE * ii);
    }
    int repeats = 0;
    for (;;) {
        bool rdy = true;
#pragma unroll
        for (int ii = 0; ii < NII; ++ii) rdy = rdy && ready4(a[ii]);
        if (__all(rdy || !ok) || budget <= 0) break;
        --budget;
        ++repeats;
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int ii = 0; ii < NII; ++ii)                          // re-read only what was incomplete
            if (ok && !ready4(a[ii])) a[ii] = load4_coherent(row + STRIDE * ii);
    }
    pace.update(repeats);
    if (budget <= 0) atomicOr(timeout_flag, 1u);
    if (!ok) {
#pragma unroll
        for (int ii = 0; ii < NII; ++ii) a[ii] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Workgroup numberings of a persistent two-layer launch over G batch tiles of 32 workgroups each (2 layer slots x 16 unit
// tiles; gru.hip: PersistIds), shared by the kernels and by the host code that sizes the grid and checks residency.
//   kPackNone   grid 32 G, the ids of one tile G apart (tiles interleaved over the XCDs)
//   kPackTile   workgroup b goes to XCD b % 8 (the dispatcher's round-robin on an idle device): tile (slot / 32) * 8 + xcd
//               takes 32 consecutive slots of its XCD, grid 256 ceil(G / 8)
//   kPackGroup  the same per (tile, layer slot) GROUP of 16 workgroups: group g = 2 tile + slot takes 16 consecutive slots of
//               XCD g % 8, grid 128 ceil(2 G / 8); beyond 8 groups an XCD hosts group g, g + 8, ... one after the other
// Ids whose tile is >= G are surplus and exit at once.
constexpr int kPackNone = 0, kPackTile = 1, kPackGroup = 2;
struct PersistSlot { int tile, rest; };              // rest = layer slot * 16 + unit tile
__host__ __device__ inline PersistSlot persist_slot(int bid, int G, int pack) {
    PersistSlot s;
    const int xcd = bid & 7, slot = bid >> 3;
    if (pack == kPackGroup) {
        const int group = (slot >> 4) * 8 + xcd;
        s.tile = group >> 1;
        s.rest = (group & 1) * 16 + (slot & 15);
    } else if (pack == kPackTile) {
        s.tile = (slot >> 5) * 8 + xcd;
        s.rest = slot & 31;
    } else {
        s.tile = bid % G;
        s.rest = bid / G;
    }
    return s;
}
__host__ __device__ inline int persist_grid_size(int G, int pack) {
    return pack == kPackGroup ? 128 * ((2 * G + 7) / 8) : pack == kPackTile ? 256 * ((G + 7) / 8) : 32 * G;
}
// can a device of `cus` CUs (8 XCDs of cus / 8) with `occ` workgroups per CU keep every working workgroup of the packed
// numbering resident, each on the XCD the numbering assumes?
__host__ __device__ inline bool persist_pack_fits(int G, int pack, int cus, int occ) {
    if (pack == kPackNone) return 32L * G <= (long)cus * occ;
    if (cus <= 0 || cus % 8 != 0) return false;
    return (long)(persist_grid_size(G, pack) / 8) <= (long)(cus / 8) * occ;
}

}  // namespace cpc
