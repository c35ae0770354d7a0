// The grouped LSTM (csrc/lstm.hip: cpc_lstm_group_*) and Elman RNN (csrc/rnn.hip: cpc_rnn_*) entry points in a stand-alone program
// for AddressSanitizer + UndefinedBehaviorSanitizer (TEST TOOL ONLY): built by tests/test_emu_recurrent_sanitized.py with
// -fsanitize=address,undefined and linked with the sanitized emulator objects of the kernels
// (tests/hipemu/build_emu.build(sanitize=True)) into one executable that carries the sanitizer runtime itself -- it is run as it
// is, nothing is preloaded.
//
// Every tensor -- the workspaces included -- is a heap block of exactly its size, so the sanitizer's red zone starts at the first
// byte behind it.  Covered: the argument checks; the LSTM group at (B, S, G) = (5, 7, 3) and (2, 6, 3); the RNN time-major at
// (T, R, G) = (2, 6, 3) and (5, 7, 3), and batch-first with two layers and a carried state at (R, T) = (5, 7); each on the
// persistent and on the per-step path (same bits).  Values are checked against float64 loops in this file (outputs 1e-5
// absolute, gradients 1e-5 norm-relative).  Exit status 0 and "rnn_san: ok" on success; a sanitizer report aborts.
#include <cmath>
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
            std::printf("rnn_san: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
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
double max_err(const float* a, const std::vector<double>& b) {
    double m = 0;
    for (size_t i = 0; i < b.size(); ++i) m = std::fmax(m, std::fabs(a[i] - b[i]));
    return m;
}

std::vector<float> randn(size_t n, float scale, std::mt19937& gen) {
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> v(n);
    for (float& x : v) x = scale * nd(gen);
    return v;
}
std::vector<float> uniform(size_t n, std::mt19937& gen) {      // nn.LSTM / nn.RNN: U(-1/16, 1/16) at hidden size 256
    std::uniform_real_distribution<float> ud(-0.0625f, 0.0625f);
    std::vector<float> v(n);
    for (float& x : v) x = ud(gen);
    return v;
}
double sigm(double v) { return 1.0 / (1.0 + std::exp(-v)); }

// ---- G LSTM heads on x (B,S,H): y (B,S,G*H), dx (B,S,H), the stacked gradients; float64
struct LstmRef {
    std::vector<double> y, dx, dwi, dwh, dbi;
};
LstmRef lstm_ref(int B, int S, int G, const std::vector<float>& x, const std::vector<float>& wi, const std::vector<float>& wh,
                 const std::vector<float>& bi, const std::vector<float>& bh, const std::vector<float>& dy) {
    const int N = 4 * H;
    LstmRef r;
    r.y.assign((size_t)B * S * G * H, 0.0); r.dx.assign((size_t)B * S * H, 0.0);
    r.dwi.assign((size_t)G * N * H, 0.0); r.dwh.assign((size_t)G * N * H, 0.0); r.dbi.assign((size_t)G * N, 0.0);
    std::vector<double> gate((size_t)S * N), c((size_t)S * H), h((size_t)S * H), dpre(N), dh(H), dc(H), dhn(H);
    for (int g = 0; g < G; ++g)
        for (int b = 0; b < B; ++b) {
            const float* Wi = &wi[(size_t)g * N * H], *Wh = &wh[(size_t)g * N * H];
            for (int t = 0; t < S; ++t) {
                const float* xt = &x[((size_t)b * S + t) * H];
                for (int n = 0; n < N; ++n) {
                    double a = (double)bi[(size_t)g * N + n] + bh[(size_t)g * N + n];
                    for (int k = 0; k < H; ++k) a += (double)Wi[(size_t)n * H + k] * xt[k];
                    if (t > 0)
                        for (int k = 0; k < H; ++k) a += (double)Wh[(size_t)n * H + k] * h[(size_t)(t - 1) * H + k];
                    gate[(size_t)t * N + n] = n / H == 2 ? std::tanh(a) : sigm(a);
                }
                for (int j = 0; j < H; ++j) {
                    const double* q = &gate[(size_t)t * N];
                    c[(size_t)t * H + j] = q[H + j] * (t > 0 ? c[(size_t)(t - 1) * H + j] : 0.0) + q[j] * q[2 * H + j];
                    h[(size_t)t * H + j] = q[3 * H + j] * std::tanh(c[(size_t)t * H + j]);
                    r.y[((size_t)b * S + t) * G * H + (size_t)g * H + j] = h[(size_t)t * H + j];
                }
            }
            std::fill(dhn.begin(), dhn.end(), 0.0);
            std::fill(dc.begin(), dc.end(), 0.0);
            for (int t = S - 1; t >= 0; --t) {
                const double* q = &gate[(size_t)t * N];
                for (int j = 0; j < H; ++j) {
                    dh[j] = dhn[j] + dy[((size_t)b * S + t) * G * H + (size_t)g * H + j];
                    const double tc = std::tanh(c[(size_t)t * H + j]);
                    const double d = dh[j] * q[3 * H + j] * (1 - tc * tc) + dc[j];
                    const double cp = t > 0 ? c[(size_t)(t - 1) * H + j] : 0.0;
                    dpre[j] = d * q[2 * H + j] * q[j] * (1 - q[j]);
                    dpre[H + j] = d * cp * q[H + j] * (1 - q[H + j]);
                    dpre[2 * H + j] = d * q[j] * (1 - q[2 * H + j] * q[2 * H + j]);
                    dpre[3 * H + j] = dh[j] * tc * q[3 * H + j] * (1 - q[3 * H + j]);
                    dc[j] = d * q[H + j];
                }
                std::fill(dhn.begin(), dhn.end(), 0.0);
                const float* xt = &x[((size_t)b * S + t) * H];
                for (int n = 0; n < N; ++n) {
                    r.dbi[(size_t)g * N + n] += dpre[n];
                    for (int k = 0; k < H; ++k) {
                        r.dwi[((size_t)g * N + n) * H + k] += dpre[n] * xt[k];
                        r.dx[((size_t)b * S + t) * H + k] += dpre[n] * Wi[(size_t)n * H + k];
                        dhn[k] += dpre[n] * Wh[(size_t)n * H + k];
                        if (t > 0) r.dwh[((size_t)g * N + n) * H + k] += dpre[n] * h[(size_t)(t - 1) * H + k];
                    }
                }
            }
        }
    return r;
}

void run_lstm_group(int B, int S, int G, unsigned seed) {
    std::mt19937 gen(seed);
    const int N = 4 * H;
    const size_t M = (size_t)B * S;
    const std::vector<float> x = randn(M * H, 1.f, gen), wi = uniform((size_t)G * N * H, gen), wh = uniform((size_t)G * N * H, gen),
                             bi = uniform((size_t)G * N, gen), bh = uniform((size_t)G * N, gen), dy = randn(M * G * H, 1.f, gen);
    const LstmRef ref = lstm_ref(B, S, G, x, wi, wh, bi, bh, dy);
    long sizes[3] = {-1, -1, -1};
    CHECK(cpc_lstm_group_layout(B, S, G, sizes) == CPC_OK && sizes[0] > 0 && sizes[1] > 0 && sizes[2] > 0);
    const Buf bx(x), bwi(wi), bwh(wh), bbi(bi), bbh(bh), bdy(dy);
    Buf* first[6] = {nullptr};
    for (int pass = 0; pass < 2; ++pass) {
        const int flags = pass ? CPC_LSTM_PER_STEP : 0;
        Buf saved((size_t)sizes[0]), fscr((size_t)sizes[1]), bscr((size_t)sizes[2]);
        Buf* o[6] = {new Buf(M * G * H), new Buf(M * H), new Buf(wi.size()), new Buf(wh.size()), new Buf(bi.size()),
                     new Buf(bh.size())};
        CHECK(cpc_lstm_group_forward(bx.p, bwi.p, bwh.p, bbi.p, bbh.p, saved.p, fscr.p, o[0]->p, B, S, G, flags, nullptr) == CPC_OK);
        CHECK(cpc_lstm_group_backward(bx.p, bwi.p, bwh.p, saved.p, o[0]->p, bdy.p, bscr.p, o[1]->p, o[2]->p, o[3]->p, o[4]->p,
                                      o[5]->p, B, S, G, flags, nullptr) == CPC_OK);
        const double ey = max_err(o[0]->p, ref.y), ex = rel_err(o[1]->p, ref.dx), ei = rel_err(o[2]->p, ref.dwi),
                     eh = rel_err(o[3]->p, ref.dwh), eb = rel_err(o[4]->p, ref.dbi), eb2 = rel_err(o[5]->p, ref.dbi);
        std::printf("  lstm group B=%d S=%d G=%d flags=%d: y %.3g dx %.3g dW_ih %.3g dW_hh %.3g db %.3g\n", B, S, G, flags, ey, ex, ei,
                    eh, eb);
        CHECK(ey < 1e-5 && ex < 1e-5 && ei < 1e-5 && eh < 1e-5 && eb < 1e-5 && eb2 < 1e-5);
        for (int k = 0; k < 6; ++k) {
            if (pass == 0) first[k] = o[k];
            else { CHECK(o[k]->same_bits(*first[k])); delete o[k]; delete first[k]; }
        }
    }
    CHECK(bx.is(x) && bwi.is(wi) && bwh.is(wh) && bbi.is(bi) && bbh.is(bh) && bdy.is(dy));      // the inputs are not written
    CHECK(cpc_device_error_flags(1) == 0);
}

// ---- Elman RNN, float64: rows m(t, r) = time-major ? t * R + r : r * T + t; G heads (one layer) or nl layers (one head)
struct RnnRef {
    std::vector<double> y, hN, dx;
    std::vector<std::vector<double>> grads;      // per layer: dW_ih, dW_hh, db
};
RnnRef rnn_ref(int T, int R, int G, int nl, bool tm, const std::vector<float>& x, const std::vector<std::vector<float>>& prm,
               const std::vector<float>* h0, const std::vector<float>& dy) {
    auto row = [&](int t, int r) { return (size_t)(tm ? (size_t)t * R + r : (size_t)r * T + t); };
    const size_t M = (size_t)T * R;
    RnnRef out;
    out.hN.assign((size_t)nl * R * H, 0.0);
    std::vector<std::vector<double>> act(nl + 1);       // act[0] = x, act[l + 1] = layer l's output (M, G*H)
    act[0].assign(x.begin(), x.end());
    for (int l = 0; l < nl; ++l) {
        const std::vector<float>&wi = prm[4 * l], &wh = prm[4 * l + 1], &bi = prm[4 * l + 2], &bh = prm[4 * l + 3];
        act[l + 1].assign(M * G * H, 0.0);
        for (int g = 0; g < G; ++g)
            for (int t = 0; t < T; ++t)
                for (int r = 0; r < R; ++r)
                    for (int j = 0; j < H; ++j) {
                        const size_t n = (size_t)g * H + j;
                        double a = (double)bi[n] + bh[n];
                        for (int k = 0; k < H; ++k) a += (double)wi[n * H + k] * act[l][row(t, r) * H + k];
                        for (int k = 0; k < H; ++k) {
                            const double hp = t > 0 ? act[l + 1][row(t - 1, r) * G * H + (size_t)g * H + k]
                                                    : (h0 ? (double)(*h0)[((size_t)l * R + r) * H + k] : 0.0);
                            a += (double)wh[n * H + k] * hp;
                        }
                        const double v = std::tanh(a);
                        act[l + 1][row(t, r) * G * H + n] = v;
                        if (t == T - 1 && G == 1) out.hN[((size_t)l * R + r) * H + j] = v;
                    }
    }
    out.y = act[nl];
    out.grads.resize(3 * nl);
    std::vector<double> dout(dy.begin(), dy.end());
    for (int l = nl - 1; l >= 0; --l) {
        const std::vector<float>&wi = prm[4 * l], &wh = prm[4 * l + 1];
        std::vector<double>&dwi = out.grads[3 * l], &dwh = out.grads[3 * l + 1], &db = out.grads[3 * l + 2];
        dwi.assign((size_t)G * H * H, 0.0); dwh.assign((size_t)G * H * H, 0.0); db.assign((size_t)G * H, 0.0);
        std::vector<double> din(M * H, 0.0), dp(H), carry((size_t)R * H);
        for (int g = 0; g < G; ++g) {
            std::fill(carry.begin(), carry.end(), 0.0);
            for (int t = T - 1; t >= 0; --t)
                for (int r = 0; r < R; ++r) {
                    for (int j = 0; j < H; ++j) {
                        const double yv = act[l + 1][row(t, r) * G * H + (size_t)g * H + j];
                        dp[j] = (dout[row(t, r) * G * H + (size_t)g * H + j] + carry[(size_t)r * H + j]) * (1 - yv * yv);
                    }
                    for (int k = 0; k < H; ++k) carry[(size_t)r * H + k] = 0.0;
                    for (int j = 0; j < H; ++j) {
                        const size_t n = (size_t)g * H + j;
                        db[n] += dp[j];
                        for (int k = 0; k < H; ++k) {
                            dwi[n * H + k] += dp[j] * act[l][row(t, r) * H + k];
                            din[row(t, r) * H + k] += dp[j] * wi[n * H + k];
                            carry[(size_t)r * H + k] += dp[j] * wh[n * H + k];
                            const double hp = t > 0 ? act[l + 1][row(t - 1, r) * G * H + (size_t)g * H + k]
                                                    : (h0 ? (double)(*h0)[((size_t)l * R + r) * H + k] : 0.0);
                            dwh[n * H + k] += dp[j] * hp;
                        }
                    }
                }
        }
        dout = din;
    }
    out.dx = dout;
    return out;
}

void run_rnn(int T, int R, int G, int nl, bool tm, bool with_h0, unsigned seed) {
    std::mt19937 gen(seed);
    const size_t M = (size_t)T * R;
    const std::vector<float> x = randn(M * H, 1.f, gen), dy = randn(M * G * H, 1.f, gen), h0 = randn((size_t)nl * R * H, 0.5f, gen);
    std::vector<std::vector<float>> prm;
    for (int l = 0; l < nl; ++l) {
        prm.push_back(uniform((size_t)G * H * H, gen)); prm.push_back(uniform((size_t)G * H * H, gen));
        prm.push_back(uniform((size_t)G * H, gen)); prm.push_back(uniform((size_t)G * H, gen));
    }
    const RnnRef ref = rnn_ref(T, R, G, nl, tm, x, prm, with_h0 ? &h0 : nullptr, dy);
    long sizes[3] = {-1, -1, -1};
    CHECK(cpc_rnn_layout(T, R, G, nl, sizes) == CPC_OK && sizes[0] > 0 && sizes[1] > 0 && sizes[2] > 0);
    const Buf bx(x), bdy(dy), bh0(h0);
    std::vector<Buf*> bp;
    std::vector<const float*> pp;
    for (const auto& v : prm) { bp.push_back(new Buf(v)); pp.push_back(bp.back()->p); }
    std::vector<Buf*> first;
    for (int pass = 0; pass < 2; ++pass) {
        const int flags = (pass ? CPC_RNN_PER_STEP : 0) | (tm ? CPC_RNN_TIME_MAJOR : 0);
        Buf saved((size_t)sizes[0]), fscr((size_t)sizes[1]), bscr((size_t)sizes[2]);
        std::vector<Buf*> o = {new Buf(M * G * H), new Buf((size_t)nl * R * H), new Buf(M * H)};
        std::vector<float*> gp;
        for (const auto& v : prm) { o.push_back(new Buf(v.size())); gp.push_back(o.back()->p); }
        CHECK(cpc_rnn_forward(bx.p, with_h0 ? bh0.p : nullptr, pp.data(), saved.p, fscr.p, o[0]->p, G == 1 ? o[1]->p : nullptr, T, R, G,
                              nl, flags, nullptr) == CPC_OK);
        CHECK(cpc_rnn_backward(bx.p, with_h0 ? bh0.p : nullptr, pp.data(), saved.p, o[0]->p, bdy.p, bscr.p, o[2]->p, gp.data(), T, R, G,
                               nl, flags, nullptr) == CPC_OK);
        double ey = max_err(o[0]->p, ref.y), eh = G == 1 ? max_err(o[1]->p, ref.hN) : 0.0, ex = rel_err(o[2]->p, ref.dx), eg = 0;
        for (int l = 0; l < nl; ++l) {
            eg = std::fmax(eg, rel_err(o[3 + 4 * l]->p, ref.grads[3 * l]));
            eg = std::fmax(eg, rel_err(o[4 + 4 * l]->p, ref.grads[3 * l + 1]));
            eg = std::fmax(eg, rel_err(o[5 + 4 * l]->p, ref.grads[3 * l + 2]));
            eg = std::fmax(eg, rel_err(o[6 + 4 * l]->p, ref.grads[3 * l + 2]));
        }
        std::printf("  rnn T=%d R=%d G=%d nl=%d time_major=%d h0=%d flags=%d: y %.3g hN %.3g dx %.3g grads %.3g\n", T, R, G, nl, (int)tm,
                    (int)with_h0, flags, ey, eh, ex, eg);
        CHECK(ey < 1e-5 && eh < 1e-5 && ex < 1e-5 && eg < 1e-5);
        for (size_t k = 0; k < o.size(); ++k) {
            if (pass == 0) first.push_back(o[k]);
            else { CHECK(o[k]->same_bits(*first[k])); delete o[k]; delete first[k]; }
        }
    }
    CHECK(bx.is(x) && bdy.is(dy) && bh0.is(h0));
    for (size_t k = 0; k < bp.size(); ++k) { CHECK(bp[k]->is(prm[k])); delete bp[k]; }
    CHECK(cpc_device_error_flags(1) == 0);
}

void run_argument_checks() {
    Buf b(64);
    long sizes[3] = {-1, -1, -1};
    float* p = b.p;
    const float* pp[8] = {p, p, p, p, p, p, p, p};
    float* gp[8] = {p, p, p, p, p, p, p, p};
    CHECK(cpc_lstm_group_layout(2, 6, 65, sizes) == CPC_ERR_SHAPE && cpc_lstm_group_layout(0, 6, 3, sizes) == CPC_ERR_SHAPE);
    CHECK(cpc_rnn_layout(2, 6, 65, 1, sizes) == CPC_ERR_SHAPE && cpc_rnn_layout(2, 6, 2, 2, sizes) == CPC_ERR_SHAPE);
    CHECK(sizes[0] == -1 && sizes[1] == -1 && sizes[2] == -1);
    CHECK(cpc_lstm_group_layout(2, 6, 3, nullptr) == CPC_ERR_ARG && cpc_rnn_layout(2, 6, 3, 1, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lstm_group_forward(p, p, p, p, p, p, p, p, 2, 6, 0, 0, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_lstm_group_forward(p, p, p, p, p, p, p, nullptr, 2, 6, 3, 0, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lstm_group_forward(p, p, p, p, p, p, p, p, 2, 6, 3, 2, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_lstm_group_backward(p, p, p, p, p, p, p, p, p, p, p, nullptr, 2, 6, 3, 0, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_rnn_forward(p, nullptr, pp, p, p, p, nullptr, 2, 6, 2, 2, 0, nullptr) == CPC_ERR_SHAPE);
    CHECK(cpc_rnn_forward(p, p, pp, p, p, p, nullptr, 2, 6, 2, 1, 0, nullptr) == CPC_ERR_ARG);          // h0 with two heads
    CHECK(cpc_rnn_forward(p, nullptr, pp, p, p, p, nullptr, 2, 6, 1, 1, 4, nullptr) == CPC_ERR_ARG);
    CHECK(cpc_rnn_backward(p, nullptr, pp, p, p, p, p, nullptr, gp, 2, 6, 1, 1, 0, nullptr) == CPC_ERR_ARG);
    for (size_t i = 0; i < b.n; ++i) CHECK(b.p[i] == 7.0f);                                              // nothing ran
}

}  // namespace

int main() {
    run_argument_checks();
    run_lstm_group(5, 7, 3, 11);
    run_lstm_group(2, 6, 3, 14);
    run_rnn(2, 6, 3, 1, true, false, 12);
    run_rnn(5, 7, 3, 1, true, false, 15);
    run_rnn(7, 5, 1, 2, false, true, 13);
    if (g_failed) {
        std::printf("rnn_san: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("rnn_san: ok\n");
    return 0;
}
