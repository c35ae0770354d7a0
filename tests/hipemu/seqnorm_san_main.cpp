// cpc_seqnorm_forward / cpc_seqnorm_backward (csrc/seqnorm.hip) in a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer (TEST TOOL ONLY): built by tests/test_emu_seqnorm_sanitized.py with -fsanitize=address,undefined
// and linked with the sanitized emulator objects of the kernels (tests/hipemu/build_emu.build(sanitize=True)) into one
// executable that carries the sanitizer runtime itself -- it is run as it is, nothing is preloaded.
//
// Every tensor is a heap block of exactly its size, so the sanitizer's red zone starts at the first byte behind it; a tensor of
// the scalar path sits 4 bytes past a 16-byte boundary, where a 16-byte access would be a misaligned-access report.  Covered:
// the argument checks, the 16-byte path and the scalar path, S = 2 and 3 (one ragged tile), S = 45 (a whole tile of 32 frames
// and a ragged one) and S = 130 (four whole tiles and a ragged one), lengths given / NULL / out of range (clamped and flagged),
// scale given / NULL, statistics asked for or not, and the scale-only calls.  Values are checked as well, against float64 in
// this file: the forward against the two-pass statistics (1e-5 norm-relative), the backward against the closed form of
// include/cpc_hip.h (1e-4) -- tests/test_emu_seqnorm.py holds that form against autograd.  Exit status 0 and "seqnorm_san: ok"
// on success; a sanitizer report aborts.
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

constexpr int H = 256;
int g_failed = 0;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("seqnorm_san: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

// n floats in a heap block of exactly that size (plus the 4 bytes in front that misalign it)
struct Buf {
    float* base;
    float* p;
    size_t n;
    Buf(size_t n_, bool misalign, float fill = 7.0f) : n(n_) {
        base = static_cast<float*>(std::malloc((n + (misalign ? 1 : 0)) * sizeof(float)));
        if (!base || (reinterpret_cast<uintptr_t>(base) & 15u)) std::abort();
        p = base + (misalign ? 1 : 0);
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    Buf(const std::vector<float>& v, bool misalign) : Buf(v.size(), misalign) { std::memcpy(p, v.data(), n * sizeof(float)); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { std::free(base); }
    bool same_bits(const Buf& o) const { return n == o.n && std::memcmp(p, o.p, n * sizeof(float)) == 0; }
    bool all(float v) const {
        for (size_t i = 0; i < n; ++i)
            if (p[i] != v) return false;
        return true;
    }
};

struct Case {
    int B, S;
    std::vector<long long> len;
    std::vector<float> x, dy, scale;
};

Case make_case(int B, int S, std::vector<long long> len, float offset, unsigned seed) {
    Case c{B, S, std::move(len), {}, {}, {}};
    std::mt19937 gen(seed);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> off(H);
    for (float& o : off) o = offset * (1.0f + 0.1f * nd(gen));
    c.x.resize((size_t)B * S * H);
    c.dy.resize(c.x.size());
    for (size_t i = 0; i < c.x.size(); ++i) { c.x[i] = nd(gen) + off[i % H]; c.dy[i] = nd(gen); }
    c.scale.resize((size_t)B * H);
    for (float& s : c.scale) s = (gen() & 1u) ? 2.0f : 0.0f;            // the dropout's factor
    for (int b = 0; b < B; ++b) { c.scale[(size_t)b * H] = 0.0f; c.scale[(size_t)b * H + 1] = 2.0f; }
    return c;
}

struct Ref { std::vector<double> y, m, r, dx; };

// float64: two-pass statistics over the n valid frames, y and dx over all S
Ref reference(const Case& c, const long long* len, const float* scale) {
    Ref o;
    const size_t N = (size_t)c.B * c.S * H;
    o.y.resize(N); o.dx.resize(N); o.m.resize((size_t)c.B * H); o.r.resize((size_t)c.B * H);
    for (int b = 0; b < c.B; ++b) {
        const int n = len ? (int)len[b] : c.S;
        for (int ch = 0; ch < H; ++ch) {
            auto at = [&](int t) { return ((size_t)b * c.S + t) * H + ch; };
            double m = 0, v = 0, g1 = 0, g2 = 0;
            for (int t = 0; t < n; ++t) m += c.x[at(t)];
            m /= n;
            for (int t = 0; t < n; ++t) v += (c.x[at(t)] - m) * (c.x[at(t)] - m);
            const double r = 1.0 / std::sqrt(v / (n - 1) + 1e-8), sc = scale ? scale[(size_t)b * H + ch] : 1.0;
            o.m[(size_t)b * H + ch] = m;
            o.r[(size_t)b * H + ch] = r;
            for (int t = 0; t < c.S; ++t) {
                const double xh = (c.x[at(t)] - m) * r, g = c.dy[at(t)] * sc;
                o.y[at(t)] = xh * sc;
                g1 += g;
                g2 += g * xh;
            }
            for (int t = 0; t < c.S; ++t) {
                const double xh = (c.x[at(t)] - m) * r, g = c.dy[at(t)] * sc;
                o.dx[at(t)] = r * (g - (t < n ? g1 / n + xh * g2 / (n - 1) : 0.0));
            }
        }
    }
    return o;
}

double rel_err(const float* a, const std::vector<double>& b) {
    double num = 0, den = 0;
    for (size_t i = 0; i < b.size(); ++i) { num += (a[i] - b[i]) * (a[i] - b[i]); den += b[i] * b[i]; }
    return std::sqrt(num) / (std::sqrt(den) + 1e-30);
}

// stats (B, 2, 256) against m and r
void check_stats(const Case& c, const Buf& st, const Ref& ref) {
    std::vector<float> m((size_t)c.B * H), r((size_t)c.B * H);
    for (int b = 0; b < c.B; ++b)
        for (int ch = 0; ch < H; ++ch) {
            m[(size_t)b * H + ch] = st.p[((size_t)b * 2 + 0) * H + ch];
            r[(size_t)b * H + ch] = st.p[((size_t)b * 2 + 1) * H + ch];
        }
    CHECK(rel_err(r.data(), ref.r) < 1e-5);
    double num = 0, den = 0;                      // m is 0 +- rounding without an offset: measured against the spread of x, 1
    for (size_t i = 0; i < m.size(); ++i) { num += (m[i] - ref.m[i]) * (m[i] - ref.m[i]); den += ref.m[i] * ref.m[i] + 1.0; }
    CHECK(std::sqrt(num / den) < 1e-5);
}

// forward and, where every length is >= 3, backward of one case on one load path; lengths NULL: every frame is valid
void run_case(const Case& c, bool misalign, bool with_len, bool with_scale, bool backward) {
    const size_t N = (size_t)c.B * c.S * H;
    const long long* len = with_len ? c.len.data() : nullptr;
    const Buf x(c.x, misalign), dy(c.dy, misalign);
    const Buf scale(c.scale, false);
    const float* sc = with_scale ? scale.p : nullptr;
    const Ref ref = reference(c, len, sc);
    Buf y(N, misalign), y2(N, misalign), st((size_t)c.B * 2 * H, false);
    CHECK(cpc_seqnorm_forward(x.p, len, sc, y.p, st.p, c.B, c.S, 1, nullptr) == CPC_OK);
    const double ferr = rel_err(y.p, ref.y);
    std::printf("  B=%d S=%d %s len=%d scale=%d: forward %.3g", c.B, c.S, misalign ? "scalar" : "vec16", (int)with_len,
                (int)with_scale, ferr);
    CHECK(ferr < 1e-5);
    check_stats(c, st, ref);
    CHECK(std::memcmp(x.p, c.x.data(), N * sizeof(float)) == 0);       // the input is not written
    CHECK(cpc_seqnorm_forward(x.p, len, sc, y2.p, nullptr, c.B, c.S, 1, nullptr) == CPC_OK);      // no statistics asked for
    CHECK(y.same_bits(y2));
    if (backward) {
        Buf dx(N, misalign);
        CHECK(cpc_seqnorm_backward(x.p, dy.p, len, sc, st.p, dx.p, c.B, c.S, 1, nullptr) == CPC_OK);
        const double berr = rel_err(dx.p, ref.dx);
        std::printf(" backward %.3g", berr);
        CHECK(berr < 1e-4);
        if (misalign) {                             // the two load paths give the same bits
            const Buf xa(c.x, false), dya(c.dy, false);
            Buf ya(N, false), sta((size_t)c.B * 2 * H, false), dxa(N, false);
            CHECK(cpc_seqnorm_forward(xa.p, len, sc, ya.p, sta.p, c.B, c.S, 1, nullptr) == CPC_OK);
            CHECK(cpc_seqnorm_backward(xa.p, dya.p, len, sc, sta.p, dxa.p, c.B, c.S, 1, nullptr) == CPC_OK);
            CHECK(ya.same_bits(y) && sta.same_bits(st) && dxa.same_bits(dx));
        }
    }
    std::printf("\n");
    CHECK(cpc_device_error_flags(1) == 0);
}

// normalise off: y = x * scale and dx = dy * scale to the bit; lengths, statistics and the backward's x are not read
void run_scale_only(const Case& c, bool misalign) {
    const size_t N = (size_t)c.B * c.S * H;
    const Buf x(c.x, misalign), dy(c.dy, misalign), scale(c.scale, false);
    Buf y(N, misalign), dx(N, misalign), y1(N, misalign);
    CHECK(cpc_seqnorm_forward(x.p, nullptr, scale.p, y.p, nullptr, c.B, c.S, 0, nullptr) == CPC_OK);
    CHECK(cpc_seqnorm_backward(nullptr, dy.p, nullptr, scale.p, nullptr, dx.p, c.B, c.S, 0, nullptr) == CPC_OK);
    CHECK(cpc_seqnorm_forward(x.p, nullptr, nullptr, y1.p, nullptr, c.B, c.S, 0, nullptr) == CPC_OK);
    bool ok = true;
    for (size_t i = 0; i < N; ++i) {
        const float s = c.scale[i / ((size_t)c.S * H) * H + i % H];
        ok = ok && y.p[i] == c.x[i] * s && dx.p[i] == c.dy[i] * s && y1.p[i] == c.x[i];
    }
    CHECK(ok);
}

// a length outside [0, S]: flagged, clamped for addressing, and the result of the clamped length
void run_length_range(const Case& c, long long bad, bool misalign) {
    const size_t N = (size_t)c.B * c.S * H;
    const Buf x(c.x, misalign), dy(c.dy, misalign), scale(c.scale, false);
    std::vector<long long> clamped = c.len, given = c.len;
    clamped[0] = bad > 0 ? c.S : 0;
    given[0] = bad;
    Buf want(N, misalign), want_st((size_t)c.B * 2 * H, false), y(N, misalign), st((size_t)c.B * 2 * H, false);
    Buf want_dx(N, misalign), dx(N, misalign);
    cpc_device_error_flags(1);
    CHECK(cpc_seqnorm_forward(x.p, clamped.data(), scale.p, want.p, want_st.p, c.B, c.S, 1, nullptr) == CPC_OK);
    CHECK(cpc_seqnorm_backward(x.p, dy.p, clamped.data(), scale.p, want_st.p, want_dx.p, c.B, c.S, 1, nullptr) == CPC_OK);
    CHECK(cpc_device_error_flags(1) == 0);
    CHECK(cpc_seqnorm_forward(x.p, given.data(), scale.p, y.p, st.p, c.B, c.S, 1, nullptr) == CPC_OK);
    CHECK(cpc_device_error_flags(1) == CPC_DEVERR_LENGTH_RANGE);
    CHECK(cpc_seqnorm_backward(x.p, dy.p, given.data(), scale.p, st.p, dx.p, c.B, c.S, 1, nullptr) == CPC_OK);
    CHECK(cpc_device_error_flags(1) == CPC_DEVERR_LENGTH_RANGE);
    CHECK(cpc_device_error_flags(1) == 0);
    const size_t row = (size_t)c.S * H;            // n = 0 is NaN, which compares by its bits here too
    if (bad > 0) CHECK(y.same_bits(want) && st.same_bits(want_st) && dx.same_bits(want_dx));
    CHECK(std::memcmp(y.p + row, want.p + row, (N - row) * sizeof(float)) == 0);
    CHECK(std::memcmp(dx.p + row, want_dx.p + row, (N - row) * sizeof(float)) == 0);
    if (bad < 0) CHECK(std::isnan(y.p[0]) && std::isnan(y.p[row - 1]) && std::isnan(dx.p[0]) && std::isnan(st.p[H]));
}

void run_argument_checks() {
    Buf buf(2 * H, false), out(2 * H, false);
    const long long one = 1;
    float *b = buf.p, *o = out.p;
    CHECK(cpc_seqnorm_forward(b, &one, nullptr, o, nullptr, 0, 1, 1, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_seqnorm_forward(b, &one, nullptr, o, nullptr, 1, 0, 1, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_seqnorm_forward(b, &one, nullptr, o, nullptr, 1 << 15, 1 << 8, 1, nullptr) == CPC_ERR_SHAPE);    // B S 256 = 2^31
    CHECK(cpc_seqnorm_forward(nullptr, &one, nullptr, o, nullptr, 1, 1, 1, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_seqnorm_forward(b, &one, nullptr, nullptr, nullptr, 1, 1, 1, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_seqnorm_forward(b, &one, nullptr, b, nullptr, 1, 1, 1, nullptr) == CPC_ERR_ARG);                 // in place
    CHECK(cpc_seqnorm_forward(b, &one, nullptr, o, nullptr, 1, 1, 2, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_seqnorm_backward(b, b, &one, nullptr, b, o, 0, 1, 1, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_seqnorm_backward(b, b, &one, nullptr, b, o, 1 << 15, 1 << 8, 1, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_seqnorm_backward(b, nullptr, &one, nullptr, b, o, 1, 1, 1, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_seqnorm_backward(b, b, &one, nullptr, b, nullptr, 1, 1, 1, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_seqnorm_backward(nullptr, b, &one, nullptr, b, o, 1, 1, 1, nullptr) == CPC_ERR_ARG);             // normalise needs x
    CHECK(cpc_seqnorm_backward(b, b, &one, nullptr, nullptr, o, 1, 1, 1, nullptr) == CPC_ERR_ARG);             // and the statistics
    CHECK(cpc_seqnorm_backward(b, b, &one, nullptr, b, o, 1, 1, -1, nullptr) == CPC_ERR_ARG);
    CHECK(buf.all(7.0f) && out.all(7.0f));                                                                     // nothing ran
}

}  // namespace

int main() {
    run_argument_checks();
    const Case one = make_case(1, 2, {2}, 0.f, 3), three = make_case(1, 3, {3}, 0.f, 4);
    const Case fwd45 = make_case(3, 45, {45, 38, 2}, 0.f, 48), bwd45 = make_case(3, 45, {45, 38, 3}, 30.f, 49);
    const Case tiles = make_case(2, 130, {130, 67}, 30.f, 132);
    for (const bool misalign : {false, true}) {
        run_case(one, misalign, true, false, false);
        run_case(three, misalign, true, true, true);
        run_case(fwd45, misalign, true, true, false);             // a length of 2: forward only
        run_case(bwd45, misalign, true, true, true);
        run_case(bwd45, misalign, false, false, true);            // lengths NULL
        run_case(tiles, misalign, true, false, true);
        run_case(tiles, misalign, true, true, true);
        run_scale_only(bwd45, misalign);
        run_length_range(bwd45, 46, misalign);
        run_length_range(bwd45, -1, misalign);
    }
    if (g_failed) {
        std::printf("seqnorm_san: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("seqnorm_san: ok\n");
    return 0;
}
