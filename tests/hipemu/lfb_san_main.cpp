// The learned-filter-bank entry points (csrc/lfb.hip) in a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer (TEST TOOL ONLY): built by tests/test_emu_lfb_sanitized.py with -fsanitize=address,undefined and
// linked with the sanitized emulator objects of the kernels (tests/hipemu/build_emu.build(sanitize=True)) into one executable
// that carries the sanitizer runtime itself -- it is run as it is, nothing is preloaded.
//
// Every tensor -- the workspace included -- is a heap block of exactly its size, so the sanitizer's red zone starts at the first
// byte behind it.  Covered: the argument checks, cpc_lfb_energy_forward / _backward at D = 32 for (N, L) = (2, 400) (one conv
// position), (3, 419) (three frames) and (2, 1040) (two groups of hops, a ragged last tile), both lognorm calls at F = 2 and
// F = 12 with the norm on and off.  Values are checked as well, against float64 loops in this file (forward 1e-5, gradients 1e-4
// norm-relative).  Exit status 0 and "lfb_san: ok" on success; a sanitizer report aborts.
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

constexpr int TAPS = 400, HOP = 160, PAD = 350;
int g_failed = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("lfb_san: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

// n floats in a heap block of exactly that size
struct Buf {
    float* p;
    size_t n;
    explicit Buf(size_t n_, float fill = 7.0f) : n(n_) {
        p = static_cast<float*>(std::malloc(n ? n * sizeof(float) : 1));
        if (!p) std::abort();
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    explicit Buf(const std::vector<float>& v) : Buf(v.size()) { std::memcpy(p, v.data(), n * sizeof(float)); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { std::free(p); }
    bool same_bits(const Buf& o) const { return n == o.n && std::memcmp(p, o.p, n * sizeof(float)) == 0; }
    bool is(const std::vector<float>& v) const { return n == v.size() && std::memcmp(p, v.data(), n * sizeof(float)) == 0; }
};

double rel_err(const float* a, const std::vector<double>& b) {
    double num = 0, den = 0;
    for (size_t i = 0; i < b.size(); ++i) { num += (a[i] - b[i]) * (a[i] - b[i]); den += b[i] * b[i]; }
    return std::sqrt(num) / (std::sqrt(den) + 1e-30);
}

std::vector<float> randn(size_t n, float scale, std::mt19937& gen) {
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> v(n);
    for (float& x : v) x = scale * nd(gen);
    return v;
}

void run_energy(int N, int L, int D, unsigned seed) {
    std::mt19937 gen(seed);
    const int T = L - 399, F = (L - 99) / HOP + 1, C = 2 * D;
    long sizes[3] = {-1, -1, -1};
    CHECK(cpc_lfb_layout(N, L, D, sizes) == CPC_OK && sizes[0] == F && sizes[1] >= 0 && sizes[2] > 0);
    const std::vector<float> x = randn((size_t)N * L, 0.1f, gen), W = randn((size_t)C * TAPS, 0.05f, gen), b = randn(C, 0.05f, gen),
                             gs = randn((size_t)N * F * D, 1.0f, gen);
    std::vector<float> han(TAPS);
    for (int j = 0; j < TAPS; ++j) han[j] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * j / TAPS));
    // float64: y, s, then ge, gy, dW, db
    std::vector<double> y((size_t)N * C * T), s((size_t)N * F * D, 0.0), dW((size_t)C * TAPS, 0.0), db(C, 0.0);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c)
            for (int t = 0; t < T; ++t) {
                double a = b[c];
                for (int j = 0; j < TAPS; ++j) a += (double)W[(size_t)c * TAPS + j] * x[(size_t)n * L + t + j];
                y[((size_t)n * C + c) * T + t] = a;
            }
    for (int n = 0; n < N; ++n)
        for (int d = 0; d < D; ++d)
            for (int t = 0; t < T; ++t) {
                const double re = y[((size_t)n * C + 2 * d) * T + t], im = y[((size_t)n * C + 2 * d + 1) * T + t];
                double ge = 0;
                for (int f = 0; f < F; ++f) {
                    const int j = t - HOP * f + PAD;
                    if (j < 0 || j >= TAPS) continue;
                    s[((size_t)n * F + f) * D + d] += han[j] * (re * re + im * im);
                    ge += (double)han[j] * gs[((size_t)n * F + f) * D + d];
                }
                for (int p = 0; p < 2; ++p) {
                    const double gy = 2 * (p ? im : re) * ge;
                    db[2 * d + p] += gy;
                    for (int j = 0; j < TAPS; ++j) dW[(size_t)(2 * d + p) * TAPS + j] += gy * x[(size_t)n * L + t + j];
                }
            }
    const Buf bx(x), bW(W), bb(b), bh(han), bg(gs);
    Buf out(s.size()), out2(s.size()), ws1((size_t)sizes[1] / 4), ws2((size_t)sizes[2] / 4), gW(dW.size()), gb(db.size()),
        gW2(dW.size()), gb2(db.size());
    CHECK(cpc_lfb_energy_forward(bx.p, bW.p, bb.p, bh.p, out.p, ws1.n ? ws1.p : nullptr, N, L, D, nullptr) == CPC_OK);
    CHECK(cpc_lfb_energy_forward(bx.p, bW.p, bb.p, bh.p, out2.p, ws1.n ? ws1.p : nullptr, N, L, D, nullptr) == CPC_OK);
    CHECK(cpc_lfb_energy_backward(bx.p, bW.p, bb.p, bh.p, bg.p, gW.p, gb.p, ws2.p, N, L, D, nullptr) == CPC_OK);
    CHECK(cpc_lfb_energy_backward(bx.p, bW.p, bb.p, bh.p, bg.p, gW2.p, gb2.p, ws2.p, N, L, D, nullptr) == CPC_OK);
    const double es = rel_err(out.p, s), ew = rel_err(gW.p, dW), eb = rel_err(gb.p, db);
    std::printf("  energy N=%d L=%d D=%d: s %.3g dW %.3g db %.3g\n", N, L, D, es, ew, eb);
    CHECK(es < 1e-5 && ew < 1e-4 && eb < 1e-4);
    CHECK(out.same_bits(out2) && gW.same_bits(gW2) && gb.same_bits(gb2));
    CHECK(bx.is(x) && bW.is(W) && bb.is(b) && bh.is(han) && bg.is(gs));                // the inputs are not written
    CHECK(cpc_device_error_flags(1) == 0);
}

void run_lognorm(int N, int F, int D, int normalise, unsigned seed) {
    std::mt19937 gen(seed);
    const size_t n = (size_t)N * F * D;
    std::vector<float> s = randn(n, 3.0f, gen), dy = randn(n, 1.0f, gen);
    for (float& v : s) v = v * v;
    std::vector<double> y(n), ds(n);
    for (int b = 0; b < N; ++b)
        for (int d = 0; d < D; ++d) {
            auto at = [&](int f) { return ((size_t)b * F + f) * D + d; };
            double m = 0, v = 0, g1 = 0, g2 = 0, r = 1;
            if (normalise) {
                for (int f = 0; f < F; ++f) m += std::log1p((double)s[at(f)]);
                m /= F;
                for (int f = 0; f < F; ++f) v += (std::log1p((double)s[at(f)]) - m) * (std::log1p((double)s[at(f)]) - m);
                r = 1.0 / std::sqrt(v / F + 1e-5);
            }
            for (int f = 0; f < F; ++f) {
                y[at(f)] = (std::log1p((double)s[at(f)]) - m) * r;
                g1 += dy[at(f)];
                g2 += dy[at(f)] * y[at(f)];
            }
            for (int f = 0; f < F; ++f) {
                const double g = normalise ? r * (dy[at(f)] - g1 / F - y[at(f)] * g2 / F) : dy[at(f)];
                ds[at(f)] = g / (1.0 + s[at(f)]);
            }
        }
    const Buf bs(s), bdy(dy);
    Buf by(n), by2(n), st((size_t)N * 2 * D), bds(n);
    CHECK(cpc_lfb_lognorm_forward(bs.p, by.p, st.p, N, F, D, normalise, nullptr) == CPC_OK);
    CHECK(cpc_lfb_lognorm_forward(bs.p, by2.p, nullptr, N, F, D, normalise, nullptr) == CPC_OK);     // no statistics asked for
    CHECK(cpc_lfb_lognorm_backward(bs.p, normalise ? st.p : nullptr, bdy.p, bds.p, N, F, D, normalise, nullptr) == CPC_OK);
    const double ey = rel_err(by.p, y), ed = rel_err(bds.p, ds);
    std::printf("  lognorm N=%d F=%d D=%d normalise=%d: y %.3g ds %.3g\n", N, F, D, normalise, ey, ed);
    CHECK(ey < 1e-5 && ed < 1e-4);
    CHECK(by.same_bits(by2) && bs.is(s) && bdy.is(dy));
}

void run_argument_checks() {
    Buf b(64);
    long sizes[3] = {-1, -1, -1};
    float* p = b.p;
    const int bad[4][3] = {{1, 400, 48}, {1, 400, 544}, {1, 399, 32}, {0, 400, 32}};
    for (const auto& c : bad) {
        CHECK(cpc_lfb_layout(c[0], c[1], c[2], sizes) == CPC_ERR_SHAPE);
        CHECK(cpc_lfb_energy_forward(p, p, p, p, p, nullptr, c[0], c[1], c[2], nullptr) == CPC_ERR_SHAPE);
        CHECK(cpc_lfb_energy_backward(p, p, p, p, p, p, p, p, c[0], c[1], c[2], nullptr) == CPC_ERR_SHAPE);
    }
    CHECK(cpc_lfb_layout(1 << 20, 64000, 32, sizes) == CPC_ERR_SHAPE);                       // N F D >= 2^31
    CHECK(cpc_lfb_layout(1 << 12, (1 << 19) + 399, 32, sizes) == CPC_ERR_SHAPE);             // N (L - 399) = 2^31
    CHECK(sizes[0] == -1 && sizes[1] == -1 && sizes[2] == -1);
    CHECK(cpc_lfb_layout(1, 400, 32, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lfb_energy_forward(nullptr, p, p, p, p, nullptr, 1, 400, 32, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lfb_energy_backward(p, p, p, p, p, p, p, nullptr, 1, 400, 32, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lfb_lognorm_forward(p, p, nullptr, 1, 2, 32, 1, nullptr) == CPC_ERR_ARG);      // in place
    CHECK(cpc_lfb_lognorm_forward(p, p + 1, nullptr, 1, 1, 32, 1, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_lfb_lognorm_forward(p, p + 1, nullptr, 1, 2, 32, 2, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lfb_lognorm_backward(p, nullptr, p + 1, p + 2, 1, 2, 32, 1, nullptr) == CPC_ERR_ARG);  // the norm needs statistics
    for (size_t i = 0; i < b.n; ++i) CHECK(b.p[i] == 7.0f);                                  // nothing ran
}

}  // namespace

int main() {
    run_argument_checks();
    run_energy(2, 400, 32, 11);
    run_energy(3, 419, 32, 12);
    run_energy(2, 1040, 32, 13);
    for (const int normalise : {1, 0}) {
        run_lognorm(3, 2, 32, normalise, 21);
        run_lognorm(2, 12, 32, normalise, 22);
    }
    if (g_failed) {
        std::printf("lfb_san: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("lfb_san: ok\n");
    return 0;
}
