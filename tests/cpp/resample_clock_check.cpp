// Pins openpbso_amd/csrc/resample_clock.h -- the reduction of the rates, the output range of a call with the advance of p0, and the
// prototype design -- against the rules of include/openpbso_amd.h "resampler bus", by brute force where the code under test has
// a closed form.  Host compiler only, AddressSanitizer + UBSan (make -C openpbso_amd/csrc resample_clock_check);
// tests/test_resample_clock.py builds and runs it.  Prints "resample clock check ok" and returns 0, or says what failed and
// returns 1.  With the arguments `design RATE_IN RATE_OUT T BETA CUTOFF` it prints L, M, T and the phase table [L][T], one tap per
// line as the hex of its f32 bits, for tests/test_resample_abi.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "resample_clock.h"

using namespace pbso;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// "Output m reads at i = floor(m M / L)": the outputs with t <= i < t + n, by walking m (m_from is any m whose i is below t)
static void brute_range(long long t, long long n, int L, int M, long long &lo, long long &cnt) {
    long long m = t * L / M;                             // floor: i(m) <= t; step back while i(m) >= t, forward while i(m) < t
    while (m > 0 && m * M / L >= t) --m;
    while (m * M / L < t) ++m;
    lo = m;
    cnt = 0;
    while (m * M / L < t + n) {
        ++m;
        ++cnt;
    }
}

static void ratio_case(int rate_out_units, int rate_in_units) {
    int L = 0, M = 0;
    CHECK(resample_reduce(rate_in_units, rate_out_units, L, M));
    CHECK(L == rate_out_units && M == rate_in_units);    // (given in lowest terms)
    CHECK(resample_reduce(rate_in_units * 300, rate_out_units * 300, L, M) && L == rate_out_units && M == rate_in_units);
    for (long long t = 0; t < 3LL * M; ++t) {
        for (long long n = 1; n <= 2LL * M + 3; ++n) {
            ResampleClock c;
            c.start_at(t, L, M);
            long long lo, cnt;
            brute_range(t, n, L, M, lo, cnt);
            CHECK(c.m == lo);
            CHECK(c.p0 == lo * M - t * L && c.p0 >= 0 && c.p0 < M);
            CHECK(c.n_out(n, L, M) == cnt);
            CHECK(cnt <= resample_max_out(n, L, M));
            CHECK(resample_first_output(t + n, L, M) - resample_first_output(t, L, M) == cnt);
            // every output of the call reads inside it, with the phase of the definition
            if (cnt > 0) {
                const long long first = c.p0, last = c.p0 + (cnt - 1) * M;
                CHECK(first / L == lo * M / L - t && first % L == lo * M % L);
                CHECK(last / L < n && last / L == (lo + cnt - 1) * M / L - t && last % L == (lo + cnt - 1) * M % L);
            }
            ResampleClock d = c;
            d.advance(n, L, M);
            CHECK(d.t == t + n && d.m == lo + cnt && d.p0 == d.m * M - d.t * L && d.p0 >= 0 && d.p0 < M);
        }
    }
    // from 0 in steps of 513: the clock that counts equals the clock that is started at t
    ResampleClock c;
    for (int s = 0; s < 50; ++s) {
        ResampleClock at;
        at.start_at(c.t, L, M);
        CHECK(at.m == c.m && at.p0 == c.p0);
        c.advance(513, L, M);
    }
}

// consecutive calls tile the output axis far from 0, where t L no longer fits in 53 bits of a double and m M is near 2^48
static void tiling_far_out(int L, int M) {
    const long long t0 = 1LL << 40;
    ResampleClock c;
    c.start_at(t0, L, M);
    typedef unsigned __int128 u128;
    CHECK((u128)c.m * M >= (u128)t0 * L && (u128)(c.m - 1) * M < (u128)t0 * L);      // m = ceil(t L / M)
    CHECK(c.p0 >= 0 && c.p0 < M && (u128)c.p0 == (u128)c.m * M - (u128)t0 * L);
    const long long lengths[] = {1, 1, 3, 513, 2, 27, 7 * 513, 1, 860 * 513, 5};
    long long next_m = c.m;
    for (int round = 0; round < 40; ++round) {
        const long long n = lengths[round % 10];
        const long long k = c.n_out(n, L, M);
        CHECK(c.m == next_m);                            // begins where the last call ended
        // the first output reads at or behind t, the one before it in front of t; the last inside, the next one behind the call
        CHECK((u128)c.m * M / L >= (u128)c.t && (c.m == 0 || (u128)(c.m - 1) * M / L < (u128)c.t));
        CHECK(k == 0 || (u128)(c.m + k - 1) * M / L < (u128)(c.t + n));
        CHECK((u128)(c.m + k) * M / L >= (u128)(c.t + n));
        CHECK(k <= resample_max_out(n, L, M));
        next_m = c.m + k;
        c.advance(n, L, M);
        CHECK(c.m == resample_first_output(c.t, L, M));
        CHECK((u128)c.p0 == (u128)c.m * M - (u128)c.t * L);
    }
}

static void limits() {
    int L, M;
    CHECK(resample_reduce(44100, 48000, L, M) && L == 160 && M == 147);
    CHECK(resample_reduce(48000, 44100, L, M) && L == 147 && M == 160);
    CHECK(resample_reduce(44100, 96000, L, M) && L == 320 && M == 147);
    CHECK(resample_reduce(44100, 22050, L, M) && L == 1 && M == 2);
    CHECK(resample_reduce(44100, 44100, L, M) && L == 1 && M == 1);
    CHECK(resample_reduce(4095, 4096, L, M) && L == 4096 && M == 4095);
    CHECK(!resample_reduce(4096, 4097, L, M));           // L = 4097
    CHECK(!resample_reduce(44100, 44101, L, M));
    CHECK(!resample_reduce(0, 48000, L, M) && !resample_reduce(44100, 0, L, M) && !resample_reduce(-1, 1, L, M));
    CHECK(resample_refusal(44100, 48000, 32, 9.0, 0.9) == nullptr);
    CHECK(resample_refusal(44100, 48000, 0, 9.0, 0.9) && resample_refusal(44100, 48000, 257, 9.0, 0.9));
    CHECK(resample_refusal(4095, 4096, 64, 9.0, 0.9) == nullptr && resample_refusal(4095, 4096, 65, 9.0, 0.9));
    CHECK(resample_refusal(44100, 48000, 32, -0.1, 0.9) && resample_refusal(44100, 48000, 32, 20.5, 0.9) && resample_refusal(44100, 48000, 32, NAN, 0.9));
    CHECK(resample_refusal(44100, 48000, 32, 9.0, 0.0) && resample_refusal(44100, 48000, 32, 9.0, 1.01) && resample_refusal(44100, 48000, 32, 9.0, INFINITY));
    CHECK(resample_refusal(44100, 44101, 32, 9.0, 0.9));
    // 160 / 147 at n = 513: 559, then 558
    ResampleClock c;
    CHECK(c.n_out(513, 160, 147) == 559);
    c.advance(513, 160, 147);
    CHECK(c.n_out(513, 160, 147) == 558);
    CHECK(resample_max_out(513, 160, 147) == 559);
}

static void design_rules() {
    CHECK(resample_i0(0.0) == 1.0);
    CHECK(std::fabs(resample_i0(1.0) - 1.2660658777520084) < 1e-15);
    CHECK(std::fabs(resample_i0(9.0) / 1093.5883545113745 - 1.0) < 1e-14);
    std::vector<float> h;
    resample_design(1, 1, 1, 9.0, 0.9, h);               // N = 1: the window is 1, g[0] = L 2 fc = cutoff
    CHECK(h.size() == 1 && h[0] == 0.9f);
    resample_design(160, 147, 32, 9.0, 0.9, h);
    CHECK(h.size() == 160u * 32u);
    const int N = 160 * 32;
    for (int j = 0; j < N / 2; ++j) {                    // linear phase: g[j] = g[N - 1 - j], through the table's layout
        const int a = j, b = N - 1 - j;
        CHECK(h[(size_t)(a % 160) * 32 + a / 160] == h[(size_t)(b % 160) * 32 + b / 160]);
    }
    double dc_min = 1e9, dc_max = -1e9;                  // every phase passes DC at gain ~ 1
    for (int phi = 0; phi < 160; ++phi) {
        double s = 0.0;
        for (int k = 0; k < 32; ++k) s += h[(size_t)phi * 32 + k];
        dc_min = s < dc_min ? s : dc_min;
        dc_max = s > dc_max ? s : dc_max;
    }
    CHECK(dc_min > 0.999 && dc_max < 1.001);
}

int main(int argc, char **argv) {
    if (argc == 7 && !std::strcmp(argv[1], "design")) {
        const int rate_in = std::atoi(argv[2]), rate_out = std::atoi(argv[3]), T = std::atoi(argv[4]);
        const double beta = std::atof(argv[5]), cutoff = std::atof(argv[6]);
        if (const char *why = resample_refusal(rate_in, rate_out, T, beta, cutoff)) {
            std::printf("refused: %s\n", why);
            return 2;
        }
        int L, M;
        resample_reduce(rate_in, rate_out, L, M);
        std::vector<float> h;
        resample_design(L, M, T, beta, cutoff, h);
        std::printf("%d %d %d\n", L, M, T);
        for (float v : h) {
            uint32_t b;
            std::memcpy(&b, &v, 4);
            std::printf("%08x\n", b);
        }
        return 0;
    }
    limits();
    const int ratios[][2] = {{160, 147}, {147, 160}, {320, 147}, {1, 2}, {2, 1}, {3, 2}, {1, 1}};
    for (const auto &r : ratios) {
        ratio_case(r[0], r[1]);
        tiling_far_out(r[0], r[1]);
    }
    tiling_far_out(4096, 4095);
    tiling_far_out(1, 4096);
    design_rules();
    if (failures) {
        std::printf("resample clock check: %d failures\n", failures);
        return 1;
    }
    std::printf("resample clock check ok\n");
    return 0;
}
