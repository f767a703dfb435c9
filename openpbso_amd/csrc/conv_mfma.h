// What the kernels of the scene filter mix and the scene reverb (kernels_fir.hip, kernels_reverb.hip) share, and the history
// kernel the scene mixer (kernels_mix.hip) has in common with the filter mix.  Both run one f32 fmaf chain per output sample on
// v_mfma_f32_16x16x4_f32 (kernels_fir.hip has the formulation) from a window of samples in padded LDS, and both end in the same
// second stage.
//
// The first stages stay instruction for instruction what was measured, and that decides how their bodies -- staging the window
// and the tap rows, the walk over window positions, the write-out of the accumulators -- can be shared.  A piece moved into a
// forced-inline function on its own, or a whole body called from thin __global__ wrappers, changes the instruction stream (the
// compiler optimises an inline function before it inlines it, and the schedule that comes out differs); so does a kernel whose
// argument layout moves.  ONE kernel template whose variant parts are `if constexpr` regions, each variant with the kernel
// arguments it was measured with, does not: that is how the variants of scene_fir_stage1 (kernels_fir.hip) share their body.
// scene_reverb_stage1 has another loop structure (one window, the taps in pieces): what it has in common with them are pieces
// of a body, so it spells them out itself.  What is here compiles to the same instructions as when every file spelled it out.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace pbso {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// f(std::integral_constant<int, C>{}) for a channel count the caller has checked (1 .. 8 = SCENE_MAX_CHANNELS): the switch from
// a launch's C to the kernels built per channel count
template <class F>
void for_channel_count(int C, F &&f) {
    switch (C) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

// window position i of a strip in LDS: one pad word per 16, so that the 16 blocks a B operand reads at one m lie in 16 banks
__device__ __forceinline__ int win_at(int i) { return i + (i >> 4); }

// Stage 2, one thread per (sample, channel = blockIdx.y): the partial rows [2][C][n_rows][n] added in row order from 0.f; inside a
// fade (the step's first n_fade samples) the same sum of the set faded out and out = Yfrom + w (Yto - Yfrom), w = (float)((double)
// (t - t_set + 1) / (double)R), three rounded operations; then add + out when add is given (add may be out: every thread reads
// its own sample before it writes it; a literal null folds the branch away).  n_rows = 0: silence.
__device__ __forceinline__ void conv_stage2(const float *parts, int C, int n_rows, long long n, long long n_fade, long long t0,
                                            long long t_set, int R, const float *add, float *out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = blockIdx.y;
    const float *p = parts + (long long)c * n_rows * n + i;
    float y = 0.f;
    for (int g = 0; g < n_rows; ++g) y = y + p[(long long)g * n];
    if (i < n_fade) {
        const float *q = p + (long long)C * n_rows * n;
        float yfrom = 0.f;
        for (int g = 0; g < n_rows; ++g) yfrom = yfrom + q[(long long)g * n];
        const float w = (float)((double)(t0 + i - t_set + 1) / (double)R);
        const float d = y - yfrom;
        const float wd = w * d;
        y = yfrom + wd;
    }
    if (add) y = add[(long long)c * n + i] + y;
    out[(long long)c * n + i] = y;
}

// hist_next[o] = the last H samples of hist[o] ++ rows[o]: the kernel behind a mix of the step's rows, o striding over
// blockIdx.y.  One definition; a file that launches it gives it the name its profiles know it by.  (A macro and not a function
// for the reason above: the kernel is the same instructions under either name.)
#define PBSO_DEFINE_HISTORY_KERNEL(name)                                                                                              \
    __global__ __launch_bounds__(256) void name(const float *__restrict__ rows, int n_obj, long long n, const float *__restrict__ hist, \
                                                float *__restrict__ hist_next, int H) {                                                 \
        const long long k = (long long)blockIdx.x * 256 + threadIdx.x;                                                                  \
        if (k >= H) return;                                                                                                             \
        const long long j = n + k; /* index into hist ++ rows */                                                                        \
        for (long long o = blockIdx.y; o < n_obj; o += gridDim.y)                                                                       \
            hist_next[o * H + k] = j < H ? hist[o * H + j] : rows[o * n + (j - H)];                                                     \
    }

}  // namespace pbso
