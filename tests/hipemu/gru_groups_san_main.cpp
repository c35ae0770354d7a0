// The host-side layout and numbering code of the persistent GRU backward (csrc/persist.h: persist_slot / persist_grid_size /
// persist_pack_fits; csrc/gru.hip: PersistIds, persist_chunk, persist_grid, gru_layout, cpc_gru_coef_floats) in a stand-alone
// program for AddressSanitizer + UndefinedBehaviorSanitizer (TEST TOOL ONLY): built by tests/test_emu_gru_layer_groups_sanitized.py
// with -fsanitize=address,undefined and linked with the sanitized emulator objects of the kernels
// (tests/hipemu/build_emu.build(sanitize=True)) into one executable that carries the sanitizer runtime itself -- it is run as it
// is, nothing is preloaded.
//
// Every tensor -- the workspaces and the `coef` buffer included -- is a heap block of exactly its size, so the sanitizer's red
// zone starts at the first byte behind it.  For B = 16, 40 and 144 at S = 12: first the numbering itself (every working
// (tile, layer slot, unit tile) exactly once, each group's ids on one id % 8, the grid the host launches), then the two-layer
// forward and the backward through cpc_gru_backward_coef + cpc_gru_backward_with_coef with the (tile, layer) group numbering on
// (groups each on one XCD, HIPEMU_XCDS=8): finite results, no polling time-out; at B = 16 and 40 also with the groups straddling
// (HIPEMU_XCDS=3) and with the numbering off: same bits (B = 144 against off: tests/test_emu_gru_layer_groups.py).
// Run with HIPEMU_THREADS=384 (see that file).  Exit status 0 and "gru_groups_san: ok" on success; a sanitizer report aborts.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../cpc_audio_amd/csrc/persist.h"
#include "cpc_hip.h"

// the emulator switches between its own fiber stacks: no fake stacks
extern "C" const char* __asan_default_options() { return "detect_stack_use_after_return=0:abort_on_error=1"; }
extern "C" const char* __ubsan_default_options() { return "print_stacktrace=1:halt_on_error=1"; }

namespace {

constexpr int H = 256, S = 12;
int g_failed = 0;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::printf("gru_groups_san: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                                 \
        }                                                                               \
    } while (0)

struct Buf {                                        // n floats in a heap block of exactly that size
    float* p;
    size_t n;
    explicit Buf(size_t n_, float fill = 7.0f) : n(n_) {
        p = static_cast<float*>(std::malloc(n ? n * sizeof(float) : 1));
        if (!p) std::abort();
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { std::free(p); }
    bool same_bits(const Buf& o) const { return n == o.n && std::memcmp(p, o.p, n * sizeof(float)) == 0; }
};

void fill_uniform(Buf& b, float a, std::mt19937& gen) {
    std::uniform_real_distribution<float> ud(-a, a);
    for (size_t i = 0; i < b.n; ++i) b.p[i] = ud(gen);
}

// every (tile, rest) of G tiles x 32 exactly once among the ids of the grid, nothing else valid; packed: a tile's / a group's ids
// all on one id % 8
void check_numbering(int G) {
    for (int pack : {cpc::kPackNone, cpc::kPackTile, cpc::kPackGroup}) {
        const int grid = cpc::persist_grid_size(G, pack);
        std::vector<int> seen((size_t)G * 32, 0), xcd((size_t)G * 2, -1);
        for (int b = 0; b < grid; ++b) {
            const cpc::PersistSlot s = cpc::persist_slot(b, G, pack);
            CHECK(s.tile >= 0 && s.rest >= 0 && s.rest < 32);
            if (s.tile >= G) continue;                            // surplus id
            ++seen[(size_t)s.tile * 32 + s.rest];
            if (pack == cpc::kPackNone) continue;
            const int unit = pack == cpc::kPackGroup ? s.tile * 2 + (s.rest >> 4) : s.tile * 2;
            if (xcd[unit] < 0) xcd[unit] = b & 7;
            CHECK(xcd[unit] == (b & 7));
            if (pack == cpc::kPackGroup) CHECK((b & 7) == unit % 8);
        }
        for (int v : seen) CHECK(v == 1);
        // residency: exactly where every XCD has room for the slots the numbering assumes there
        const int per_xcd = grid / 8;
        if (pack != cpc::kPackNone) {
            CHECK(cpc::persist_pack_fits(G, pack, 8 * per_xcd, 1));
            CHECK(!cpc::persist_pack_fits(G, pack, 8 * per_xcd - 8, 1));
            CHECK(!cpc::persist_pack_fits(G, pack, 8 * per_xcd + 1, 1));          // not 8 equal XCDs
            CHECK(cpc::persist_pack_fits(G, pack, 8 * ((per_xcd + 1) / 2), 2));
        } else {
            CHECK(cpc::persist_pack_fits(G, pack, 32 * G, 1) && !cpc::persist_pack_fits(G, pack, 32 * G - 1, 1));
        }
    }
}

void run_shape(int B, bool compare) {
    std::mt19937 gen(1000u + (unsigned)B);
    const int nl = 2, G3 = 3 * H;
    check_numbering((B + 15) / 16);
    Buf wih0((size_t)G3 * H), whh0((size_t)G3 * H), bih0(G3), bhh0(G3), wih1((size_t)G3 * H), whh1((size_t)G3 * H), bih1(G3), bhh1(G3);
    Buf* prm[8] = {&wih0, &whh0, &bih0, &bhh0, &wih1, &whh1, &bih1, &bhh1};
    const float* params[8];
    for (int i = 0; i < 8; ++i) { fill_uniform(*prm[i], 0.0625f, gen); params[i] = prm[i]->p; }
    Buf x((size_t)B * S * H), dy((size_t)B * S * H);
    fill_uniform(x, 1.0f, gen);
    fill_uniform(dy, 1.0f, gen);
    long sizes[3] = {0, 0, 0};
    CHECK(cpc_gru_layout(B, S, nl, sizes) == 0);
    Buf saved((size_t)sizes[0]), fscr((size_t)sizes[1]), y((size_t)B * S * H), hN((size_t)nl * B * H);
    CHECK(cpc_gru_forward(x.p, nullptr, params, saved.p, fscr.p, y.p, hN.p, B, S, nl, nullptr) == 0);
    const long ncoef = cpc_gru_coef_floats(B, S, nl);
    CHECK(ncoef > 0);

    struct Out {
        Buf dx;
        std::vector<Buf*> g;
        explicit Out(int B_) : dx((size_t)B_ * S * H) {
            for (int i = 0; i < 8; ++i) g.push_back(new Buf(i % 4 < 2 ? (size_t)3 * H * H : (size_t)3 * H));
        }
        ~Out() { for (Buf* b : g) delete b; }
    };
    auto backward = [&](int local, const char* xcds, Out& o) {
        setenv("HIPEMU_XCDS", xcds, 1);
        CHECK(cpc_set_gru_xcd_local(local) == 0);
        Buf coef((size_t)ncoef), bscr((size_t)sizes[2]);
        float* grads[8];
        for (int i = 0; i < 8; ++i) grads[i] = o.g[i]->p;
        CHECK(cpc_gru_backward_coef(nullptr, params, saved.p, y.p, coef.p, 0, B, S, nl, nullptr) == 0);
        CHECK(cpc_gru_backward_with_coef(x.p, nullptr, params, saved.p, y.p, dy.p, coef.p, bscr.p, o.dx.p, grads, B, S, nl, nullptr) == 0);
        CHECK(cpc_set_gru_xcd_local(1) == 0);
        CHECK(cpc_device_error_flags(1) == 0);
    };
    auto same = [&](const Out& a, const Out& b) {
        bool ok = a.dx.same_bits(b.dx);
        for (int i = 0; i < 8; ++i) ok = ok && a.g[i]->same_bits(*b.g[i]);
        return ok;
    };
    Out on(B);
    backward(3, "8", on);
    for (size_t i = 0; i < on.dx.n; ++i)
        if (!(on.dx.p[i] == on.dx.p[i])) { CHECK(!"NaN in dx"); break; }
    if (compare) {
        Out off(B), st(B);
        backward(1, "8", off);
        backward(3, "3", st);
        CHECK(same(off, on));
        CHECK(same(off, st));
    }
    std::printf("gru_groups_san: B = %d done\n", B);
}

}  // namespace

int main() {
    run_shape(16, true);
    run_shape(40, true);
    run_shape(144, false);
    if (g_failed) {
        std::printf("gru_groups_san: %d check(s) FAILED\n", g_failed);
        return 1;
    }
    std::printf("gru_groups_san: ok\n");
    return 0;
}
