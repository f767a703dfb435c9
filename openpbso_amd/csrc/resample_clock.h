// The host arithmetic of the resampler bus (include/openpbso_amd.h "resampler bus"; resample.cpp, kernels_resample.hip): the
// reduction of the two rates to L / M with its limits, the output range of a call and the advance of the one number the host keeps
// between calls (p0), and the design of the prototype.  Integers and doubles only and no HIP call, as bus_clock.h:
// tests/cpp/resample_clock_check.cpp pins all of it on the host compiler alone.
#pragma once

#include <cmath>
#include <vector>

namespace pbso {

constexpr int RESAMPLE_MAX_FACTOR = 4096;                // L and M
constexpr int RESAMPLE_MAX_TAPS = 256;                   // T, per output sample
constexpr int RESAMPLE_MAX_TABLE = 1 << 18;              // L T

// L = rate_out / gcd, M = rate_in / gcd; false when a rate is not positive or a factor is over the limit
inline bool resample_reduce(int rate_in, int rate_out, int &L, int &M) {
    if (rate_in < 1 || rate_out < 1) return false;
    int a = rate_in, b = rate_out;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    L = rate_out / a;
    M = rate_in / a;
    return L <= RESAMPLE_MAX_FACTOR && M <= RESAMPLE_MAX_FACTOR;
}

// ceil(n L / M): the most outputs a call of n input samples can have (n L < 2^63 for every n L the engine can be given)
inline long long resample_max_out(long long n, int L, int M) { return (n * L + M - 1) / M; }

// ceil(t L / M) for any t >= 0, exact: the first output that reads at or behind input sample t (the check program's yardstick and
// the start of a clock that does not begin at 0; the engine's own clock never multiplies an absolute index)
inline long long resample_first_output(long long t, int L, int M) {
    const unsigned __int128 x = (unsigned __int128)(unsigned long long)t * (unsigned)L;
    return (long long)((x + (unsigned)(M - 1)) / (unsigned)M);
}

// Output m reads at input i = floor(m M / L) with phase (m M) mod L.  Between calls: t input samples taken, m outputs made, and
// p0 = m M - t L, in [0, M): the position of the next output, in units of 1 / L input samples, relative to the next input sample.
struct ResampleClock {
    long long t = 0, m = 0, p0 = 0;
    // the outputs of a call that takes n input samples: those at positions p0 + j M < n L
    long long n_out(long long n, int L, int M) const {
        const long long span = n * L - p0;
        return span > 0 ? (span + M - 1) / M : 0;
    }
    void advance(long long n, int L, int M) {
        const long long k = n_out(n, L, M);
        p0 += k * M - n * L;
        t += n;
        m += k;
    }
    // as if t input samples had been taken already
    void start_at(long long t0, int L, int M) {
        t = t0;
        m = resample_first_output(t0, L, M);
        p0 = (long long)((unsigned __int128)(unsigned long long)m * (unsigned)M - (unsigned __int128)(unsigned long long)t0 * (unsigned)L);
    }
    void reset() { t = m = p0 = 0; }
};

// I0(x) = sum over k of ((x / 2)^k / k!)^2, in ascending k until a term is below 1e-17 of the sum
inline double resample_i0(double x) {
    double q = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        q *= (0.5 * x) / (double)k;
        const double term = q * q;
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// the prototype g[j], j < N = L T, in fp64: a sinc at fc = cutoff * 0.5 / max(L, M) under a Kaiser window, gain L
inline double resample_prototype(int j, int L, int M, int T, double beta, double cutoff) {
    const long long N = (long long)L * T;
    const double c = 0.5 * (double)(N - 1), x = (double)j - c;
    const double fc = cutoff * 0.5 / (double)(L > M ? L : M);
    const double a = 2.0 * fc * x;
    const double sinc = a == 0.0 ? 1.0 : std::sin(M_PI * a) / (M_PI * a);
    double win = 1.0;
    if (N > 1) {
        const double r = 2.0 * x / (double)(N - 1);
        const double s = 1.0 - r * r;
        win = resample_i0(beta * std::sqrt(s > 0.0 ? s : 0.0)) / resample_i0(beta);
    }
    return (double)L * 2.0 * fc * sinc * win;
}

// the phase table h[phi][k] = (float)g[k L + phi], [L][T]: every tap rounded to f32 once
inline void resample_design(int L, int M, int T, double beta, double cutoff, std::vector<float> &h) {
    h.resize((size_t)L * T);
    for (int phi = 0; phi < L; ++phi)
        for (int k = 0; k < T; ++k) h[(size_t)phi * T + k] = (float)resample_prototype(k * L + phi, L, M, T, beta, cutoff);
}

// the parameters pbso_resample_enable takes besides the channel count; nullptr when they are in range, else what is wrong
inline const char *resample_refusal(int rate_in, int rate_out, int taps, double beta, double cutoff) {
    int L = 0, M = 0;
    if (rate_in < 1 || rate_out < 1) return "the rates must be positive";
    if (!resample_reduce(rate_in, rate_out, L, M)) return "L = rate_out / gcd and M = rate_in / gcd must be <= 4096";
    if (taps < 1 || taps > RESAMPLE_MAX_TAPS) return "taps must be 1 .. 256";
    if ((long long)L * taps > RESAMPLE_MAX_TABLE) return "L * taps must be <= 1 << 18";
    if (!(std::isfinite(cutoff) && cutoff > 0.0 && cutoff <= 1.0)) return "cutoff must be finite, 0 < cutoff <= 1";
    if (!(std::isfinite(beta) && beta >= 0.0 && beta <= 20.0)) return "beta must be finite, 0 <= beta <= 20";
    return nullptr;
}

}  // namespace pbso
