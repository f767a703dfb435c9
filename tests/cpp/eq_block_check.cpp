// The EQ bus's host arithmetic (openpbso_amd/csrc/eq_block.h) as a program of its own, built with the host compiler under
// AddressSanitizer + UBSan (make eq_block_check):
//   eq_block_check                               the validation, the identity's tables, the block offsets; exit 0 when all hold
//   eq_block_check tables b0 b1 b2 a1 a2         P, then the 5 P table words h r s p q as hex bit patterns
//   eq_block_check design kind rate f0 q gain    the five coefficients as hex bit patterns (kind 0 .. 4)
// tests/test_eq_abi.py compares what it prints with tests/eq_model.py bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "eq_block.h"

using namespace pbso;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static void print_bits(const double *v, int n) {
    for (int i = 0; i < n; ++i) {
        uint64_t u;
        std::memcpy(&u, v + i, 8);
        std::printf("%016" PRIx64 "\n", u);
    }
}

int main(int argc, char **argv) {
    if (argc == 7 && std::strcmp(argv[1], "tables") == 0) {
        double c[5];
        for (int k = 0; k < 5; ++k) c[k] = std::strtod(argv[2 + k], nullptr);
        if (eq_refusal(c, 1)) {
            std::fprintf(stderr, "refused: %s\n", eq_refusal(c, 1));
            return 2;
        }
        std::vector<double> tab((size_t)EQ_TABLES * EQ_BLOCK);
        eq_tables(c, tab.data());
        std::printf("%d\n", EQ_BLOCK);
        print_bits(tab.data(), (int)tab.size());
        return 0;
    }
    if (argc == 7 && std::strcmp(argv[1], "design") == 0) {
        const int kind = std::atoi(argv[2]);
        const double rate = std::strtod(argv[3], nullptr), f0 = std::strtod(argv[4], nullptr), q = std::strtod(argv[5], nullptr),
                     gain = std::strtod(argv[6], nullptr);
        if (const char *why = eq_design_refusal(kind, rate, f0, q, gain)) {
            std::fprintf(stderr, "refused: %s\n", why);
            return 2;
        }
        double c[5];
        eq_design(kind, rate, f0, q, gain, c);
        print_bits(c, 5);
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: eq_block_check [tables b0 b1 b2 a1 a2 | design kind rate f0 q gain]\n");
        return 2;
    }
    // the validation: finite, and inside the stability triangle
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double good[10] = {1, 0, 0, 0, 0, 0.5, 0.1, 0.2, -1.9, 0.95};
    CHECK(eq_refusal(good, 2) == nullptr);
    for (int k = 0; k < 10; ++k) {
        double bad[10];
        std::memcpy(bad, good, sizeof(bad));
        bad[k] = nan;
        CHECK(eq_refusal(bad, 2) != nullptr);
        bad[k] = k & 1 ? inf : -inf;
        CHECK(eq_refusal(bad, 2) != nullptr);
    }
    const double edge[][2] = {{0, 1}, {0, -1}, {2, 1}, {-2, 1}, {1.5, 0.5}, {-1.5, 0.5}, {0.1, -0.9}, {0, 1.0000001}};
    for (const auto &e : edge) {
        const double c[5] = {1, 0, 0, e[0], e[1]};
        CHECK(eq_refusal(c, 1) != nullptr);
    }
    const double inside[][2] = {{1.4999, 0.5}, {-1.4999, 0.5}, {0, 0.999999}, {0, -0.999999}, {-1.99, 0.9901}, {0.05, -0.9}};
    for (const auto &e : inside) {
        const double c[5] = {1, 0, 0, e[0], e[1]};
        CHECK(eq_refusal(c, 1) == nullptr);
    }
    // the identity: h is the unit impulse, the four other tables are zero
    {
        double c[5];
        std::vector<double> tab((size_t)EQ_TABLES * EQ_BLOCK);
        eq_identity(c);
        eq_tables(c, tab.data());
        for (int i = 0; i < EQ_TABLES * EQ_BLOCK; ++i) CHECK(tab[i] == (i == 0 ? 1.0 : 0.0));
    }
    // the tables of a real section: p and q carry the homogeneous recurrence, r and s the feed-forward taps into it
    {
        double c[5];
        eq_design(PBSO_EQ_HIGHPASS, 44100.0, 30.0, 0.707, 0.0, c);
        CHECK(eq_refusal(c, 1) == nullptr);
        std::vector<double> tab((size_t)EQ_TABLES * EQ_BLOCK);
        eq_tables(c, tab.data());
        const double *h = tab.data(), *r = h + EQ_BLOCK, *s = r + EQ_BLOCK, *p = s + EQ_BLOCK, *q = p + EQ_BLOCK;
        CHECK(h[0] == c[0] && r[0] == c[1] && s[0] == c[2] && p[0] == -c[3] && q[0] == -c[4]);
        CHECK(s[1] == -c[3] * c[2] && q[1] == -c[3] * q[0]);
        for (int i = 0; i < EQ_TABLES * EQ_BLOCK; ++i) CHECK(std::isfinite(tab[i]));
    }
    // every kind, across the band: a stable section
    for (int kind = PBSO_EQ_LOWPASS; kind <= PBSO_EQ_HIGHSHELF; ++kind)
        for (double f0 : {5.0, 30.0, 1000.0, 18000.0, 22049.0})
            for (double gain : {-24.0, 0.0, 12.0}) {
                double c[5];
                CHECK(eq_design_refusal(kind, 44100.0, f0, 0.7, gain) == nullptr);
                eq_design(kind, 44100.0, f0, 0.7, gain, c);
                CHECK(eq_refusal(c, 1) == nullptr);
            }
    CHECK(eq_design_refusal(5, 44100, 100, 1, 0) && eq_design_refusal(-1, 44100, 100, 1, 0) && eq_design_refusal(0, 0, 100, 1, 0) &&
          eq_design_refusal(0, 44100, 22050, 1, 0) && eq_design_refusal(0, 44100, 0, 1, 0) && eq_design_refusal(0, 44100, 100, 0, 0) &&
          eq_design_refusal(0, 44100, nan, 1, 0) && eq_design_refusal(2, 44100, 100, 1, inf) && eq_design_refusal(2, 44100, 100, 1, 121));
    // where a sample lies in its block, far from 0
    CHECK(eq_block_offset(0, 0) == 0 && eq_block_offset(EQ_BLOCK, 0) == 0 && eq_block_offset(513, 0) == 513 % EQ_BLOCK);
    CHECK(eq_block_offset(513 + 700, 513) == 700 % EQ_BLOCK);
    const long long far = (1LL << 62) + 12345;
    CHECK(eq_block_offset(far + 3 * (long long)EQ_BLOCK + 7, far) == 7);
    if (failures) return 1;
    std::printf("eq_block_check: ok (P = %d)\n", EQ_BLOCK);
    return 0;
}
