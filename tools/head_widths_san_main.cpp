// The six feature-width entry points (cpc_phone_head_layout_d / _forward_d / _backward_d, cpc_seqnorm_forward_d / _backward_d,
// cpc_posterior_forward_d) in a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer (TEST TOOL ONLY): built by
// tools/build_head_widths_san.py with -fsanitize=address,undefined and linked with the sanitized emulator objects of the
// kernels into one executable that carries the sanitizer runtime itself -- it is run as it is, nothing is preloaded.
//
// Canaries in the tests see writes; this sees reads.  Every tensor is a heap block of exactly its size, so the sanitizer's red
// zone starts at the first byte behind it, and at D = 13 and D = 257 a row neither starts nor ends on a 16-byte boundary (D = 260
// adds the 16-byte path whose last slab and last 16-column group are partial): a
// 16-byte access that straddles a row's end at the end of a tensor, or a masked-out channel that is read all the same, is a
// report.  Each call also runs with its tensors 4 bytes past a 16-byte boundary.  Values are checked loosely against float64
// in this file (the tests hold them to their bounds).  Exit status 0 and "head_widths_san: ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "cpc_hip.h"

// the emulator switches between its own fiber stacks: no fake stacks
extern "C" const char* __asan_default_options() { return "detect_stack_use_after_return=0:abort_on_error=1"; }
extern "C" const char* __ubsan_default_options() { return "print_stacktrace=1:halt_on_error=1"; }

namespace {

int g_failed = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("head_widths_san: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                              \
        }                                                                            \
    } while (0)

// n elements in a heap block of exactly that size (plus the 4 bytes in front that misalign it)
template <class T>
struct Buf {
    char* base;
    T* p;
    size_t n;
    Buf(size_t n_, bool misalign, T fill) : n(n_) {
        base = static_cast<char*>(std::malloc(n * sizeof(T) + (misalign ? 4 : 0)));
        if (!base || (reinterpret_cast<uintptr_t>(base) & 15u)) std::abort();
        p = reinterpret_cast<T*>(base + (misalign ? 4 : 0));
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    Buf(const std::vector<T>& v, bool misalign) : Buf(v.size(), misalign, T(0)) { std::memcpy(p, v.data(), n * sizeof(T)); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { std::free(base); }
};
using FBuf = Buf<float>;

std::vector<float> randn(size_t n, std::mt19937& gen, float scale = 1.f) {
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> v(n);
    for (float& x : v) x = scale * nd(gen);
    return v;
}

bool finite(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

void run_head(int D, int B, int S, int C, bool misalign) {
    std::mt19937 gen(100 + D + S);
    long sizes[5];
    CHECK(cpc_phone_head_layout_d(B, S, C, 0, D, sizes) == CPC_OK);
    const int T = (int)sizes[0];
    const std::vector<float> hx = randn((size_t)B * S * D, gen), hW = randn((size_t)C * D * 8, gen, 1.f / std::sqrt(8.f * D)),
                             hb = randn(C, gen, 0.1f), hdl = randn((size_t)B * T * C, gen);
    const FBuf x(hx, misalign), W(hW, misalign), b(hb, misalign), dl(hdl, misalign);
    FBuf wr(sizes[1], misalign, 7.f), scratch(sizes[2], misalign, NAN), logits(sizes[3], misalign, 7.f);
    CHECK(sizes[3] == (long)B * T * C && sizes[1] == (long)C * 8 * D);
    CHECK(cpc_phone_head_forward_d(x.p, W.p, b.p, wr.p, scratch.p, logits.p, B, S, C, D, nullptr) == CPC_OK);
    double worst = 0;                                  // logits against float64
    for (int bi = 0; bi < B; ++bi)
        for (int t = 0; t < T; ++t)
            for (int o = 0; o < C; ++o) {
                double s = hb[o];
                for (int j = 0; j < 8; ++j)
                    for (int c = 0; c < D; ++c) s += (double)hx[((size_t)bi * S + 4 * t + j) * D + c] * hW[((size_t)o * D + c) * 8 + j];
                worst = std::fmax(worst, std::fabs(s - logits.p[((size_t)bi * T + t) * C + o]));
            }
    CHECK(worst < 1e-4);
    FBuf dW((size_t)C * D * 8, misalign, 7.f), db(C, misalign, 7.f), dX((size_t)B * S * D, misalign, 7.f);
    CHECK(cpc_phone_head_backward_d(x.p, wr.p, dl.p, scratch.p, dW.p, db.p, dX.p, B, S, C, D, nullptr) == CPC_OK);
    CHECK(finite(dW.p, dW.n) && finite(db.p, db.n) && finite(dX.p, dX.n));
    CHECK(cpc_phone_head_backward_d(x.p, wr.p, dl.p, scratch.p, dW.p, db.p, nullptr, B, S, C, D, nullptr) == CPC_OK);
    std::printf("  head D=%d B=%d S=%d C=%d %s: logits within %.3g\n", D, B, S, C, misalign ? "offset" : "aligned", worst);
}

void run_seqnorm(int D, int B, int S, std::vector<long long> len, bool misalign) {
    std::mt19937 gen(200 + D + S);
    const size_t N = (size_t)B * S * D;
    const std::vector<float> hx = randn(N, gen), hdy = randn(N, gen);
    std::vector<float> hs((size_t)B * D);
    for (float& s : hs) s = (gen() & 1u) ? 2.0f : 0.0f;
    const FBuf x(hx, misalign), dy(hdy, misalign), scale(hs, misalign);
    const Buf<long long> lens(len, false);
    FBuf y(N, misalign, 7.f), stats((size_t)B * 2 * D, misalign, 7.f), dx(N, misalign, 7.f);
    CHECK(cpc_seqnorm_forward_d(x.p, lens.p, scale.p, y.p, stats.p, B, S, D, 1, nullptr) == CPC_OK);
    CHECK(cpc_seqnorm_backward_d(x.p, dy.p, lens.p, scale.p, stats.p, dx.p, B, S, D, 1, nullptr) == CPC_OK);
    CHECK(finite(y.p, N) && finite(dx.p, N) && finite(stats.p, stats.n));
    double worst = 0;                                  // the mean against float64
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < D; ++c) {
            double m = 0;
            for (int t = 0; t < len[b]; ++t) m += hx[((size_t)b * S + t) * D + c];
            worst = std::fmax(worst, std::fabs(m / (double)len[b] - stats.p[((size_t)b * 2) * D + c]));
        }
    CHECK(worst < 1e-5);
    CHECK(cpc_seqnorm_forward_d(x.p, nullptr, nullptr, y.p, nullptr, B, S, D, 1, nullptr) == CPC_OK);
    CHECK(cpc_seqnorm_forward_d(x.p, nullptr, scale.p, y.p, nullptr, B, S, D, 0, nullptr) == CPC_OK);
    CHECK(cpc_seqnorm_backward_d(nullptr, dy.p, nullptr, scale.p, nullptr, dx.p, B, S, D, 0, nullptr) == CPC_OK);
    CHECK(cpc_device_error_flags(1) == 0);
    std::printf("  seqnorm D=%d B=%d S=%d %s: means within %.3g\n", D, B, S, misalign ? "offset" : "aligned", worst);
}

void run_posterior(int D, int R, int C, bool misalign) {
    std::mt19937 gen(300 + D + R + C);
    const std::vector<float> hx = randn((size_t)R * D, gen), hW = randn((size_t)C * D, gen, 1.f / std::sqrt((float)D)),
                             hb = randn(C, gen, 0.05f);
    const FBuf x(hx, misalign), W(hW, misalign), b(hb, misalign);
    FBuf prob((size_t)R * C, misalign, 7.f);
    Buf<long long> hot((size_t)R * C, false, 7);
    Buf<int> am(R, misalign, -7);
    CHECK(cpc_posterior_forward_d(x.p, D, W.p, b.p, R, C, D, 0, prob.p, am.p, nullptr) == CPC_OK);
    CHECK(cpc_posterior_forward_d(x.p, D, W.p, b.p, R, C, D, 1, hot.p, nullptr, nullptr) == CPC_OK);
    double worst = 0;
    for (int r = 0; r < R; ++r) {
        double s = 0;
        long ones = 0;
        for (int c = 0; c < C; ++c) { s += prob.p[(size_t)r * C + c]; ones += hot.p[(size_t)r * C + c]; }
        worst = std::fmax(worst, std::fabs(s - 1.0));
        CHECK(ones == 1 && am.p[r] >= 0 && am.p[r] < C && hot.p[(size_t)r * C + am.p[r]] == 1);
    }
    CHECK(worst < 1e-5);
    std::printf("  posterior D=%d R=%d C=%d %s: row sums within %.3g of 1\n", D, R, C, misalign ? "offset" : "aligned", worst);
}

}  // namespace

int main() {
    for (const int D : {13, 257, 260})
        for (const bool misalign : {false, true}) {
            run_head(D, 2, 11, 7, misalign);           // an uncovered tail
            run_head(D, 1, 77, 65, misalign);          // a second class tile
            run_seqnorm(D, 1, 2, {2}, misalign);
            run_seqnorm(D, 3, 33, {33, 20, 2}, misalign);
            run_seqnorm(D, 2, 70, {70, 37}, misalign);
            run_posterior(D, 1, 2, misalign);
            run_posterior(D, 33, 42, misalign);
            run_posterior(D, 70, 65, misalign);
            run_posterior(D, 5, 385, misalign);        // past the logits a tile keeps: the second walk
        }
    if (g_failed) {
        std::printf("head_widths_san: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("head_widths_san: ok\n");
    return 0;
}
