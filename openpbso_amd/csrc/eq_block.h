// The host arithmetic of the EQ bus (include/openpbso_amd.h "EQ bus"; eq.cpp, kernels_eq.hip): the validation of a set, the five
// tables of a section's block form, where a step lies on a cascade's block grid, and the Audio-EQ-Cookbook designs.  Integers and
// doubles only and no HIP call, as resample_clock.h: tests/cpp/eq_block_check.cpp pins it on the host compiler alone.  Compile
// with -ffp-contract=off: the tables come from the recurrence in its literal order of operations.
#pragma once

#include <cmath>

#include "openpbso_amd.h"

namespace pbso {

constexpr int EQ_BLOCK = PBSO_EQ_BLOCK;                  // P: part of the definition
constexpr int EQ_HIST = EQ_BLOCK + 2;                    // samples of every signal the device keeps
constexpr int EQ_MAX_SECTIONS = 8;
constexpr int EQ_TABLES = 5;                             // h, r, s, p, q

// why a set of n coefficient words [..][5] = b0 b1 b2 a1 a2 is refused, or nullptr
inline const char *eq_refusal(const double *sos, long long n_sections) {
    for (long long i = 0; i < n_sections; ++i) {
        const double *c = sos + 5 * i;
        for (int k = 0; k < 5; ++k)
            if (!std::isfinite(c[k])) return "every coefficient must be finite";
        const double a1 = c[3], a2 = c[4];
        if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2)) return "every section must be stable (|a2| < 1 and |a1| < 1 + a2)";
    }
    return nullptr;
}

// one step of the recurrence, in this order: (((b0 v + b1 x1) + b2 x2) - a1 y1) - a2 y2
inline double eq_step(const double c[5], double v, double x1, double x2, double y1, double y2) {
    return c[0] * v + c[1] * x1 + c[2] * x2 - c[3] * y1 - c[4] * y2;
}

// P outputs of the recurrence from the state (x1, x2, y1, y2) = (x(-1), x(-2), y(-1), y(-2)) with the input v0 at sample 0 and 0 behind it
inline void eq_response(const double c[5], double v0, double x1, double x2, double y1, double y2, double *out) {
    double v = v0;
    for (int k = 0; k < EQ_BLOCK; ++k) {
        const double o = eq_step(c, v, x1, x2, y1, y2);
        x2 = x1;
        x1 = v;
        y2 = y1;
        y1 = o;
        out[k] = o;
        v = 0.0;
    }
}

// tab [5][P] of one section: h (unit impulse from zero state), then the zero-input responses r, s, p, q to unit x(T0-1), x(T0-2),
// y(T0-1), y(T0-2)
inline void eq_tables(const double c[5], double *tab) {
    eq_response(c, 1.0, 0.0, 0.0, 0.0, 0.0, tab);
    eq_response(c, 0.0, 1.0, 0.0, 0.0, 0.0, tab + EQ_BLOCK);
    eq_response(c, 0.0, 0.0, 1.0, 0.0, 0.0, tab + 2 * EQ_BLOCK);
    eq_response(c, 0.0, 0.0, 0.0, 1.0, 0.0, tab + 3 * EQ_BLOCK);
    eq_response(c, 0.0, 0.0, 0.0, 0.0, 1.0, tab + 4 * EQ_BLOCK);
}

// the identity section: b0 = 1, the rest 0
inline void eq_identity(double c[5]) {
    c[0] = 1.0;
    c[1] = c[2] = c[3] = c[4] = 0.0;
}

// where sample t lies in the block of a cascade in force since t_set (t >= t_set): k with t = T0 + k, 0 <= k < P
inline int eq_block_offset(long long t, long long t_set) { return (int)((t - t_set) % EQ_BLOCK); }

// why a design is refused, or nullptr
inline const char *eq_design_refusal(int kind, double rate, double f0, double q, double gain_db) {
    if (kind < PBSO_EQ_LOWPASS || kind > PBSO_EQ_HIGHSHELF) return "kind must be one of the five PBSO_EQ_* forms";
    if (!(std::isfinite(rate) && rate > 0.0)) return "rate must be positive";
    if (!(std::isfinite(f0) && f0 > 0.0 && f0 < 0.5 * rate)) return "0 < f0 < rate / 2";
    if (!(std::isfinite(q) && q > 0.0)) return "Q must be positive";
    if (!(std::isfinite(gain_db) && std::fabs(gain_db) <= 120.0)) return "|gain dB| <= 120";
    return nullptr;
}

// the cookbook's five forms, every line as the public header spells it; out = b0 b1 b2 a1 a2, divided by a0
inline void eq_design(int kind, double rate, double f0, double q, double gain_db, double out[5]) {
    const double pi = 3.14159265358979323846;
    const double w0 = 2.0 * pi * f0 / rate, cs = std::cos(w0), sn = std::sin(w0), alpha = sn / (2.0 * q);
    const double A = std::pow(10.0, gain_db / 40.0), g = 2.0 * std::sqrt(A) * alpha;
    double b0, b1, b2, a0, a1, a2;
    switch (kind) {
    case PBSO_EQ_LOWPASS:
        b1 = 1.0 - cs; b0 = b1 / 2.0; b2 = b0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        break;
    case PBSO_EQ_HIGHPASS:
        b1 = -(1.0 + cs); b0 = (1.0 + cs) / 2.0; b2 = b0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        break;
    case PBSO_EQ_PEAK:
        b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
        break;
    case PBSO_EQ_LOWSHELF:
        b0 = A * ((A + 1.0) - (A - 1.0) * cs + g); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs); b2 = A * ((A + 1.0) - (A - 1.0) * cs - g);
        a0 = (A + 1.0) + (A - 1.0) * cs + g; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs); a2 = (A + 1.0) + (A - 1.0) * cs - g;
        break;
    default:                                             // PBSO_EQ_HIGHSHELF
        b0 = A * ((A + 1.0) + (A - 1.0) * cs + g); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs); b2 = A * ((A + 1.0) + (A - 1.0) * cs - g);
        a0 = (A + 1.0) - (A - 1.0) * cs + g; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs); a2 = (A + 1.0) - (A - 1.0) * cs - g;
        break;
    }
    out[0] = b0 / a0;
    out[1] = b1 / a0;
    out[2] = b2 / a0;
    out[3] = a1 / a0;
    out[4] = a2 / a0;
}

}  // namespace pbso
