// The loudness bus (pbso_loudness; include/openpbso_amd.h "Loudness bus"): the gated energies of the K-weighted signal and the true
// peak of the input, per channel and per sub-block of Hs = rate / 10 samples, appended to a log of pbso_loudness_block on the device.
// The K-weighting itself is the EQ bus's block form (launch_eq_cascade with S = 2, kernels_eq.hip), whose fp64 rows these kernels
// read.  A step [t, t + n) touches the sub-blocks j0 .. j0 + n_touched - 1; its first sample lies k0 samples into sub-block j0.
//
//   energy    one wave64 per (sub-block touched, channel).  Lane l walks the samples k = l, l + 64, ... of the sub-block that lie in
//             the step, in ascending k, acc = fma(z, z, acc): a wave reads 64 consecutive doubles per turn.  A first sub-block that
//             was open before the step starts from the carry, a last one that stays open stores it; a sub-block that ends in the
//             step does the tree (s = 32 .. 1, acc_l + acc_{l+s}) and writes its record: the energy, and the peaks' start values
//             (the carried maxima, or 0).  The carry is double-buffered, since one wave may read it while another writes.
//   peak      one thread per input sample; the 256 + 11 samples a workgroup reads staged in LDS (the 11 before the step from the
//             tail the device keeps); O chains of 12 fmaf per thread; maxima per workgroup and per sub-block (with Hs >= 256 a
//             workgroup touches at most two), merged into the record or the carry by an unsigned atomicMax on the bits of the
//             non-negative floats.  Runs behind the energy kernel, which wrote the start values.
//
// Built with -ffp-contract=off and without any fast-math or denormal flag.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "loudness_gate.h"

namespace pbso {

namespace {
constexpr int LANES = LOUDNESS_LANES, T = LOUDNESS_TAPS, TAIL = LOUDNESS_TAIL;
constexpr int PEAK_TPB = 256;
static_assert(LANES == 64, "one accumulator per lane of a wave64");
static_assert(PEAK_TPB <= LOUDNESS_MIN_HOP, "a workgroup of the peak kernel touches at most two sub-blocks");
}  // namespace

// z rows of z_stride doubles, the step's sample i at z[c * z_stride + z_off + i].  carry / carry_next [C][64]; peaks / peaks_next
// [C][2] the running maxima (true peak, sample peak) as bits; log + the first record of sub-block j0, records C apart.
__global__ __launch_bounds__(64) void loudness_energy_kernel(const double *__restrict__ z, long long z_stride, long long z_off, long long n, int hs,
                                                             int k0, const double *__restrict__ carry, double *__restrict__ carry_next,
                                                             const unsigned *__restrict__ peaks, unsigned *__restrict__ peaks_next,
                                                             pbso_loudness_block *__restrict__ log, int C) {
    const long long b = blockIdx.x;
    const int c = blockIdx.y, lane = threadIdx.x;
    const long long origin = b * hs - k0;                // the sub-block's first sample, as an index into the step; < 0 only for an open first
    const bool carried = b == 0 && k0 > 0;
    const long long lo = origin < 0 ? 0 : origin, hi = origin + hs < n ? origin + hs : n;
    const bool complete = origin + hs <= n;
    double acc = carried ? carry[c * LANES + lane] : 0.0;
    // the first k >= lo - origin with k mod 64 == lane
    long long k = lo - origin;
    k += ((long long)lane - k % LANES + LANES) % LANES;
    const long long base = c * z_stride + z_off + origin;                      // (>= 0 wherever it is read: origin + k >= 0)
    for (; origin + k < hi; k += LANES) {
        const double v = z[base + k];
        acc = fma(v, v, acc);
    }
    if (!complete) {
        carry_next[c * LANES + lane] = acc;
        if (lane < 2) peaks_next[c * 2 + lane] = carried ? peaks[c * 2 + lane] : 0u;
        return;
    }
    for (int s = LANES / 2; s >= 1; s >>= 1) {
        const double other = __shfl_down(acc, s, LANES);
        acc = acc + other;                               // (lanes >= s hold values nobody reads)
    }
    if (lane == 0) {
        pbso_loudness_block *r = log + b * C + c;
        r->energy = acc;
        r->true_peak = __uint_as_float(carried ? peaks[c * 2] : 0u);
        r->sample_peak = __uint_as_float(carried ? peaks[c * 2 + 1] : 0u);
    }
}

// in [C][n]; tail / tail_next [C][11] the input samples before / behind the step; h [O][12]
template <int O>
__global__ __launch_bounds__(PEAK_TPB) void loudness_peak_kernel(const float *__restrict__ in, long long n, int hs, int k0,
                                                                 const float *__restrict__ tail, float *__restrict__ tail_next,
                                                                 const float *__restrict__ h, unsigned *__restrict__ peaks_next,
                                                                 pbso_loudness_block *__restrict__ log, int C) {
    __shared__ float win[PEAK_TPB + TAIL];
    __shared__ unsigned red[PEAK_TPB / 64][4];
    const int c = blockIdx.y, tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * PEAK_TPB, i = i0 + tid;
    const float *__restrict__ u = in + c * n;
    for (int l = tid; l < PEAK_TPB + TAIL; l += PEAK_TPB) {
        const long long s = i0 - TAIL + l;
        win[l] = s < 0 ? tail[c * TAIL + (int)(s + TAIL)] : s < n ? u[s] : 0.f;
    }
    // the samples before the next step: the step's last 11, or what stays of the old ones in front of a shorter step
    if (blockIdx.x == 0 && tid < TAIL) {
        const long long s = n - TAIL + tid;
        tail_next[c * TAIL + tid] = s < 0 ? tail[c * TAIL + (int)(s + TAIL)] : u[s];
    }
    __syncthreads();
    float tp = 0.f, sp = 0.f;
    if (i < n) {
        const float *w = win + tid + TAIL;
        sp = fabsf(w[0]);
#pragma unroll
        for (int phi = 0; phi < O; ++phi) {
            float acc = 0.f;
#pragma unroll
            for (int k = T - 1; k >= 0; --k) acc = fmaf(h[phi * T + k], w[-k], acc);
            tp = fmaxf(tp, fabsf(acc));
        }
    }
    // the workgroup's samples lie in sub-block b_lo (relative to j0) and perhaps the one behind it
    const long long b_lo = (k0 + i0) / hs;
    const long long split = (b_lo + 1) * hs - k0;        // the first sample of the sub-block behind b_lo
    const bool low = i < split;
    unsigned v[4] = {low ? __float_as_uint(tp) : 0u, low ? __float_as_uint(sp) : 0u, low ? 0u : __float_as_uint(tp), low ? 0u : __float_as_uint(sp)};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned o = (unsigned)__shfl_down((int)v[q], s, 64);
            v[q] = v[q] > o ? v[q] : o;
        }
        if ((tid & 63) == 0) red[tid >> 6][q] = v[q];
    }
    __syncthreads();
    if (tid < 4) {
        unsigned m = red[0][tid];
        for (int wv = 1; wv < PEAK_TPB / 64; ++wv) m = m > red[wv][tid] ? m : red[wv][tid];
        const long long b = b_lo + (tid >> 1);
        const long long last = i0 + PEAK_TPB < n ? i0 + PEAK_TPB : n;          // one behind the workgroup's last sample
        if (tid < 2 || last > split) {
            const bool complete = (b + 1) * hs - k0 <= n;
            pbso_loudness_block *r = log + b * C + c;
            unsigned *dst = complete ? (unsigned *)((tid & 1) ? &r->sample_peak : &r->true_peak) : peaks_next + c * 2 + (tid & 1);
            atomicMax(dst, m);
        }
    }
}

int launch_loudness_energy(const double *z, long long z_stride, long long z_off, int C, long long n, int hs, int k0, long long n_touched,
                           const double *carry, double *carry_next, const unsigned *peaks, unsigned *peaks_next, void *log_j0, hipStream_t stream) {
    if (!z || !carry || !carry_next || !peaks || !peaks_next || !log_j0 || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0 || hs < LOUDNESS_MIN_HOP ||
        k0 < 0 || k0 >= hs || z_off < 0 || z_stride < z_off + n || n_touched != (k0 + n - 1) / hs + 1 || n_touched > 0x7fffffffll)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(loudness_energy_kernel, dim3((unsigned)n_touched, C), dim3(64), 0, stream, z, z_stride, z_off, n, hs, k0, carry, carry_next, peaks,
                       peaks_next, (pbso_loudness_block *)log_j0, C);
    return (int)hipGetLastError();
}

int launch_loudness_peak(const float *in, int C, long long n, int hs, int k0, int O, const float *tail, float *tail_next, const float *h,
                         unsigned *peaks_next, void *log_j0, hipStream_t stream) {
    if (!in || !tail || !tail_next || !h || !peaks_next || !log_j0 || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0 || hs < LOUDNESS_MIN_HOP || k0 < 0 ||
        k0 >= hs || (O != 2 && O != 4) || (n + PEAK_TPB - 1) / PEAK_TPB > 0x7fffffffll)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + PEAK_TPB - 1) / PEAK_TPB), C);
    pbso_loudness_block *log = (pbso_loudness_block *)log_j0;
    if (O == 4) hipLaunchKernelGGL(loudness_peak_kernel<4>, grid, dim3(PEAK_TPB), 0, stream, in, n, hs, k0, tail, tail_next, h, peaks_next, log, C);
    else hipLaunchKernelGGL(loudness_peak_kernel<2>, grid, dim3(PEAK_TPB), 0, stream, in, n, hs, k0, tail, tail_next, h, peaks_next, log, C);
    return (int)hipGetLastError();
}

}  // namespace pbso
