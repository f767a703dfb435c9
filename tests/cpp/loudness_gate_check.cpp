// The loudness bus's host arithmetic (openpbso_amd/csrc/loudness_gate.h) as a program of its own, built with the host compiler
// under AddressSanitizer + UBSan (make loudness_gate_check):
//   loudness_gate_check                 the validation, the grid of sub-blocks against brute force, the gating against a second,
//                                       per-block formulation; exit 0 when all hold
//   loudness_gate_check design rate     the ten coefficients [2][5] as hex bit patterns
//   loudness_gate_check taps rate       O, then the O * 12 taps of the true peak's phase table as hex bit patterns
// tests/test_loudness_abi.py compares what it prints with tests/loudness_model.py bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "loudness_gate.h"
#include "resample_clock.h"

using namespace pbso;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// a second formulation of the report: the loudness of every gating block first, in arrays, then the gates as set operations
static pbso_loudness_summary second(const std::vector<pbso_loudness_block> &b, int C, const double *G, int hs) {
    const long long n = (long long)b.size() / C;
    pbso_loudness_summary r;
    r.integrated = r.momentary = r.short_term = r.max_momentary = r.max_short_term = r.relative_threshold = -HUGE_VAL;
    r.true_peak = r.sample_peak = 0.0;
    r.n_blocks = n;
    r.n_gated = 0;
    for (const pbso_loudness_block &x : b) {
        r.true_peak = std::fmax(r.true_peak, (double)x.true_peak);
        r.sample_peak = std::fmax(r.sample_peak, (double)x.sample_peak);
    }
    auto window = [&](long long i, int W) {
        std::vector<double> ms((size_t)C);
        for (int c = 0; c < C; ++c) {
            double e = 0.0;
            bool first = true;
            for (long long k = i - W + 1; k <= i; ++k) {
                e = first ? b[(size_t)k * C + c].energy : e + b[(size_t)k * C + c].energy;
                first = false;
            }
            ms[(size_t)c] = e / ((double)W * (double)hs);
        }
        double w = 0.0;
        for (int c = 0; c < C; ++c) w = w + (G ? G[c] : 1.0) * ms[(size_t)c];
        return w;
    };
    std::vector<double> w, l;
    for (long long i = 3; i < n; ++i) {
        w.push_back(window(i, 4));
        l.push_back(w.back() > 0.0 ? -0.691 + 10.0 * std::log10(w.back()) : -HUGE_VAL);
    }
    if (!l.empty()) r.momentary = l.back();
    for (double v : l) r.max_momentary = std::fmax(r.max_momentary, v);
    for (long long i = 29; i < n; ++i) {
        const double ws = window(i, 30), ls = ws > 0.0 ? -0.691 + 10.0 * std::log10(ws) : -HUGE_VAL;
        r.short_term = ls;
        r.max_short_term = std::fmax(r.max_short_term, ls);
    }
    std::vector<size_t> A;
    for (size_t i = 0; i < l.size(); ++i)
        if (l[i] > -70.0) A.push_back(i);
    if (A.empty()) return r;
    double sum = 0.0;
    for (size_t i : A) sum = sum + w[i];
    r.relative_threshold = -0.691 + 10.0 * std::log10(sum / (double)A.size()) - 10.0;
    std::vector<size_t> B;
    for (size_t i : A)
        if (l[i] > r.relative_threshold) B.push_back(i);
    r.n_gated = (int64_t)B.size();
    if (B.empty()) return r;
    sum = 0.0;
    for (size_t i : B) sum = sum + w[i];
    r.integrated = -0.691 + 10.0 * std::log10(sum / (double)B.size());
    return r;
}

static void check_report(const std::vector<pbso_loudness_block> &b, int C, const double *G, int hs) {
    pbso_loudness_summary got;
    std::memset(&got, 0, sizeof(got));
    CHECK(loudness_report(b.data(), (long long)b.size() / C, C, G, hs, &got));
    const pbso_loudness_summary want = second(b, C, G, hs);
    CHECK(same(got.integrated, want.integrated) && same(got.momentary, want.momentary) && same(got.short_term, want.short_term));
    CHECK(same(got.max_momentary, want.max_momentary) && same(got.max_short_term, want.max_short_term));
    CHECK(same(got.relative_threshold, want.relative_threshold) && same(got.true_peak, want.true_peak) && same(got.sample_peak, want.sample_peak));
    CHECK(got.n_blocks == want.n_blocks && got.n_gated == want.n_gated);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {                                // xorshift64*, in [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

int main(int argc, char **argv) {
    if (argc == 3 && std::strcmp(argv[1], "design") == 0) {
        const double rate = std::strtod(argv[2], nullptr);
        if (const char *why = loudness_design_refusal(rate)) {
            std::fprintf(stderr, "refused: %s\n", why);
            return 2;
        }
        double c[2][5];
        loudness_design(rate, c);
        for (int i = 0; i < 10; ++i) {
            uint64_t u;
            std::memcpy(&u, &c[i / 5][i % 5], 8);
            std::printf("%016" PRIx64 "\n", u);
        }
        return 0;
    }
    if (argc == 3 && std::strcmp(argv[1], "taps") == 0) {
        const int rate = std::atoi(argv[2]), O = loudness_oversampling(rate);
        std::vector<float> h;
        resample_design(O, 1, LOUDNESS_TAPS, LOUDNESS_BETA, LOUDNESS_CUTOFF, h);
        std::printf("%d\n", O);
        for (float v : h) {
            uint32_t u;
            std::memcpy(&u, &v, 4);
            std::printf("%08" PRIx32 "\n", u);
        }
        return 0;
    }

    // the validation
    CHECK(loudness_hop(44100) == 4410 && loudness_hop(48000) == 4800 && loudness_hop(22050) == 2205 && loudness_hop(2560) == 256);
    CHECK(loudness_hop(44101) == 0 && loudness_hop(2550) == 0 && loudness_hop(0) == 0 && loudness_hop(-10) == 0);
    CHECK(loudness_oversampling(44100) == 4 && loudness_oversampling(79990) == 4 && loudness_oversampling(80000) == 2 && loudness_oversampling(96000) == 2);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double ok_w[8] = {1, 1, 1, 1.41, 1.41, 0, 0, 2}, neg_w[2] = {1, -1e-300}, nan_w[2] = {nan, 1}, inf_w[1] = {inf};
    CHECK(!loudness_refusal(44100, 8, ok_w, 1) && !loudness_refusal(44100, 1, nullptr, 1 << 22));
    CHECK(loudness_refusal(44100, 0, nullptr, 1) && loudness_refusal(44100, 9, nullptr, 1) && loudness_refusal(44101, 1, nullptr, 1));
    CHECK(loudness_refusal(44100, 1, nullptr, 0) && loudness_refusal(44100, 1, nullptr, (1 << 22) + 1));
    CHECK(loudness_refusal(44100, 2, neg_w, 1) && loudness_refusal(44100, 2, nan_w, 1) && loudness_refusal(44100, 1, inf_w, 1));
    CHECK(loudness_design_refusal(3000.0) && loudness_design_refusal(nan) && loudness_design_refusal(inf) && !loudness_design_refusal(8000.0));

    // the grid against a per-sample labelling
    for (int hs : {256, 257, 2205, 4410})
        for (long long t : {0LL, 1LL, 255LL, 256LL, 2204LL, 2205LL, 4409LL, 4410LL, 4411LL, 8820LL, 251370LL - 513, 251370LL, (1LL << 40) + 77})
            for (long long n : {1LL, 27LL, 255LL, 256LL, 513LL, 2205LL, 4410LL, 9234LL, 20001LL}) {
                const LoudnessSpan s = loudness_span(t, n, hs);
                long long touched = 0, complete = 0, prev = -1;
                for (long long i = t; i < t + n; ++i) {
                    const long long j = i / hs;
                    if (j != prev) ++touched;
                    prev = j;
                    if ((i + 1) % hs == 0) ++complete;
                }
                CHECK(s.j0 == t / hs && s.k0 == (int)(t % hs) && s.n_touched == touched && s.n_complete == complete);
                CHECK(s.open_last == ((t + n) % hs != 0) && s.n_touched == (s.k0 + n - 1) / hs + 1 && s.n_complete == (s.k0 + n) / hs);
                CHECK(s.n_touched - s.n_complete == (s.open_last ? 1 : 0));
            }

    // the gating against the second formulation
    pbso_loudness_summary r;
    CHECK(!loudness_report(nullptr, 1, 1, nullptr, 4410, &r) && !loudness_report(nullptr, 0, 0, nullptr, 4410, &r));
    CHECK(!loudness_report(nullptr, 0, 1, nullptr, 0, &r) && !loudness_report(nullptr, 0, 1, nullptr, 4410, nullptr));
    CHECK(!loudness_report(nullptr, 0, 2, neg_w, 4410, &r));
    CHECK(loudness_report(nullptr, 0, 1, nullptr, 4410, &r) && r.n_blocks == 0 && r.n_gated == 0 && r.integrated == -HUGE_VAL && r.true_peak == 0.0);
    for (int C : {1, 2, 5, 8})
        for (int n : {0, 1, 3, 4, 5, 29, 30, 31, 100, 700}) {
            for (int kind = 0; kind < 5; ++kind) {
                std::vector<pbso_loudness_block> b((size_t)n * C);
                for (int i = 0; i < n; ++i)
                    for (int c = 0; c < C; ++c) {
                        // energies of 4410 samples: silence, one level, levels spread over 80 dB, a loud middle, all below the absolute gate
                        double level = kind == 0 ? 0.0 : kind == 1 ? 0.01 : kind == 2 ? std::pow(10.0, -8.0 * uniform()) : kind == 3 ? (i > n / 3 && i < 2 * n / 3 ? 0.1 : 1e-5) : 1e-9;
                        if (kind >= 2) level *= 0.5 + uniform();
                        pbso_loudness_block &x = b[(size_t)i * C + c];
                        x.energy = level * 4410.0;
                        x.true_peak = (float)(std::sqrt(level) * (1.0 + 0.2 * uniform()));
                        x.sample_peak = (float)std::sqrt(level);
                    }
                check_report(b, C, nullptr, 4410);
                check_report(b, C, ok_w, 4410);
            }
        }
    // known figures: a constant mean square of 1 is -0.691 LUFS whatever the gates; a silent log has no loudness
    {
        std::vector<pbso_loudness_block> b(40);
        for (pbso_loudness_block &x : b) x = {4800.0, 1.5f, 1.f};
        CHECK(loudness_report(b.data(), 40, 1, nullptr, 4800, &r));
        CHECK(std::fabs(r.integrated + 0.691) < 1e-12 && std::fabs(r.momentary + 0.691) < 1e-12 && std::fabs(r.short_term + 0.691) < 1e-12);
        CHECK(std::fabs(r.relative_threshold + 10.691) < 1e-12 && r.n_gated == 37 && r.true_peak == 1.5 && r.sample_peak == 1.0);
        for (pbso_loudness_block &x : b) x = {0.0, 0.f, 0.f};
        CHECK(loudness_report(b.data(), 40, 1, nullptr, 4800, &r));
        CHECK(r.integrated == -HUGE_VAL && r.momentary == -HUGE_VAL && r.relative_threshold == -HUGE_VAL && r.n_gated == 0 && r.n_blocks == 40);
    }

    if (failures) {
        std::fprintf(stderr, "loudness_gate_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("loudness_gate_check: ok\n");
    return 0;
}
