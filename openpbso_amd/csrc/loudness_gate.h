// The host arithmetic of the loudness bus (include/openpbso_amd.h "Loudness bus"; loudness.cpp, kernels_loudness.hip): the
// K-weighting design, the validation of an enable, where a step lies on the grid of 100 ms sub-blocks, and the gating of
// ITU-R BS.1770-4 / EBU Tech 3341 over a log of sub-block records.  Integers and doubles only and no HIP call, as eq_block.h:
// tests/cpp/loudness_gate_check.cpp pins it on the host compiler alone.  Compile with -ffp-contract=off: the design and the sums
// are computed in their literal order of operations.
#pragma once

#include <cmath>
#include <cstdint>

#include "openpbso_amd.h"

namespace pbso {

constexpr int LOUDNESS_LANES = 64;                       // accumulators of a sub-block's energy, per channel
constexpr int LOUDNESS_TAPS = 12;                        // T: taps per phase of the true-peak interpolator
constexpr int LOUDNESS_TAIL = LOUDNESS_TAPS - 1;         // input samples the device keeps per channel
constexpr int LOUDNESS_MIN_HOP = 256;                    // a workgroup of the peak kernel touches at most two sub-blocks
constexpr int LOUDNESS_MAX_BLOCKS = 1 << 22;
constexpr double LOUDNESS_BETA = 8.0, LOUDNESS_CUTOFF = 1.0;

// Hs = rate / 10, or 0 when the rate has no hop (not a multiple of 10, or Hs < 256)
inline int loudness_hop(int rate) {
    if (rate < 10 || rate % 10 != 0) return 0;
    const int hs = rate / 10;
    return hs >= LOUDNESS_MIN_HOP ? hs : 0;
}

// the oversampling factor of the true peak
inline int loudness_oversampling(int rate) { return rate < 80000 ? 4 : 2; }

// the two sections of the K-weighting, every line as the public header spells it; out [2][5] = b0 b1 b2 a1 a2
inline void loudness_design(double rate, double out[2][5]) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out[0][0] = (Vh + Vb * K / Q + K * K) / a0;
        out[0][1] = 2.0 * (K * K - Vh) / a0;
        out[0][2] = (Vh - Vb * K / Q + K * K) / a0;
        out[0][3] = 2.0 * (K * K - 1.0) / a0;
        out[0][4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / rate);
        const double a0 = 1.0 + K / Q + K * K;
        out[1][0] = 1.0;
        out[1][1] = -2.0;
        out[1][2] = 1.0;
        out[1][3] = 2.0 * (K * K - 1.0) / a0;
        out[1][4] = (1.0 - K / Q + K * K) / a0;
    }
}

// why pbso_loudness_design refuses a rate, or nullptr (the shelf's corner must lie below Nyquist)
inline const char *loudness_design_refusal(double rate) {
    if (!(std::isfinite(rate) && rate > 2.0 * 1681.974450955533)) return "rate must be finite and above 3364 Hz";
    return nullptr;
}

// why an enable is refused, or nullptr; weight may be null (all 1)
inline const char *loudness_refusal(int rate, int n_channels, const double *weight, long long max_blocks) {
    if (n_channels < 1 || n_channels > 8) return "n_channels must be 1 .. 8";
    if (!loudness_hop(rate)) return "the sample rate must be a multiple of 10 with rate / 10 >= 256";
    if (max_blocks < 1 || max_blocks > LOUDNESS_MAX_BLOCKS) return "max_blocks must be 1 .. 1 << 22";
    if (weight)
        for (int c = 0; c < n_channels; ++c)
            if (!(std::isfinite(weight[c]) && weight[c] >= 0.0)) return "every channel weight must be finite and >= 0";
    return nullptr;
}

// Where the step [t, t + n), n >= 1, lies on the grid of sub-blocks j = [j Hs, (j + 1) Hs)
struct LoudnessSpan {
    long long j0 = 0;                                    // the first sub-block the step touches
    int k0 = 0;                                          // t - j0 Hs: where the step's first sample lies in it (> 0: it is open, a carry is loaded)
    long long n_touched = 0;                             // sub-blocks with a sample in the step
    long long n_complete = 0;                            // of them, those whose last sample is in the step: records j0 .. j0 + n_complete - 1
    bool open_last = false;                              // the last touched one ends behind the step: a carry is stored
};
inline LoudnessSpan loudness_span(long long t, long long n, int hs) {
    LoudnessSpan s;
    s.j0 = t / hs;
    s.k0 = (int)(t - s.j0 * hs);
    s.n_touched = (t + n - 1) / hs - s.j0 + 1;
    s.n_complete = (t + n) / hs - s.j0;
    s.open_last = (t + n) % hs != 0;
    return s;
}

// l = -0.691 + 10 log10(w), -infinity for w = 0
inline double loudness_lufs(double w) { return w > 0.0 ? -0.691 + 10.0 * std::log10(w) : -HUGE_VAL; }

// the weighted mean square of the W sub-blocks that end with sub-block i (i >= W - 1): per channel the energies summed left to
// right in ascending order and divided by W Hs, the channels in ascending c
inline double loudness_window(const pbso_loudness_block *blocks, int C, const double *weight, int hs, long long i, int W) {
    double w = 0.0;
    for (int c = 0; c < C; ++c) {
        double e = blocks[(size_t)(i - W + 1) * C + c].energy;
        for (int k = W - 2; k >= 0; --k) e = e + blocks[(size_t)(i - k) * C + c].energy;
        const double ms = e / ((double)W * (double)hs);
        w = w + (weight ? weight[c] : 1.0) * ms;
    }
    return w;
}

constexpr int LOUDNESS_GATE_BLOCKS = 4, LOUDNESS_SHORT_BLOCKS = 30;

// the report over blocks [n_blocks][C]; false when an argument is out of range (then out is untouched)
inline bool loudness_report(const pbso_loudness_block *blocks, long long n_blocks, int C, const double *weight, int hs, pbso_loudness_summary *out) {
    if (!out || n_blocks < 0 || (n_blocks > 0 && !blocks) || hs < 1 || C < 1 || C > 8) return false;
    if (weight)
        for (int c = 0; c < C; ++c)
            if (!(std::isfinite(weight[c]) && weight[c] >= 0.0)) return false;
    pbso_loudness_summary r;
    r.integrated = r.momentary = r.short_term = r.max_momentary = r.max_short_term = r.relative_threshold = -HUGE_VAL;
    r.true_peak = r.sample_peak = 0.0;
    r.n_blocks = n_blocks;
    r.n_gated = 0;
    for (long long i = 0; i < n_blocks * C; ++i) {
        if ((double)blocks[i].true_peak > r.true_peak) r.true_peak = (double)blocks[i].true_peak;
        if ((double)blocks[i].sample_peak > r.sample_peak) r.sample_peak = (double)blocks[i].sample_peak;
    }
    // the absolute gate and the mean behind it
    double sum_a = 0.0;
    long long n_a = 0;
    for (long long i = LOUDNESS_GATE_BLOCKS - 1; i < n_blocks; ++i) {
        const double w = loudness_window(blocks, C, weight, hs, i, LOUDNESS_GATE_BLOCKS), l = loudness_lufs(w);
        r.momentary = l;
        if (l > r.max_momentary) r.max_momentary = l;
        if (l > -70.0) {
            sum_a = sum_a + w;
            ++n_a;
        }
    }
    for (long long i = LOUDNESS_SHORT_BLOCKS - 1; i < n_blocks; ++i) {
        const double l = loudness_lufs(loudness_window(blocks, C, weight, hs, i, LOUDNESS_SHORT_BLOCKS));
        r.short_term = l;
        if (l > r.max_short_term) r.max_short_term = l;
    }
    if (n_a > 0) {
        r.relative_threshold = loudness_lufs(sum_a / (double)n_a) - 10.0;
        double sum_g = 0.0;
        for (long long i = LOUDNESS_GATE_BLOCKS - 1; i < n_blocks; ++i) {
            const double w = loudness_window(blocks, C, weight, hs, i, LOUDNESS_GATE_BLOCKS), l = loudness_lufs(w);
            if (l > -70.0 && l > r.relative_threshold) {
                sum_g = sum_g + w;
                ++r.n_gated;
            }
        }
        if (r.n_gated > 0) r.integrated = loudness_lufs(sum_g / (double)r.n_gated);
    }
    *out = r;
    return true;
}

}  // namespace pbso
