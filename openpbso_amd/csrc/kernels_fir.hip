// The scene filter mix (pbso_scene_fir): C output channels, a K-tap FIR per (channel, object) behind an integer onset per object.
//
//   y_c(t) = sum_o sum_{k < K} h_co[k] * x_o(t - D_o - k)
//
// as ONE f32 fmaf chain per (channel, group of 32 objects, output sample): objects ascending, taps K-1 down to 0, i.e. upward
// through the object's window of samples; then the groups' partial rows in group order (pbso_mix_objects' two stages).  The chain
// runs on v_mfma_f32_16x16x4_f32, which is bit for bit a k-ordered fmaf chain on its accumulator: for a tile of 256 output samples
// s = 16 a + b,
//
//   Y[b][a] += T[b][m] * XW[m][a],   XW[m][a] = x(16 a + m - (K - 1) - D),   T[b][m] = h[b + K - 1 - m] (0 outside 0 .. K-1)
//
// over the window positions m = 0 .. K + 14 in ascending order, four per instruction (padded with zero taps to a multiple of 8).  The products with a zero tap add nothing
// (fmaf(0, x, acc) == acc for finite x), so every output sample sees exactly the chain above wherever it sits in its tile.  One
// accumulator per (channel, tile) carries the chain through the taps and the group's objects: nothing is split and summed later.
// Built with -ffp-contract=off (the blend of a fade is three separately rounded operations) and without any fast-math or
// denormal flag: subnormal samples come through as fmaf gives them.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int FIR_GROUP = 32;                            // = MIX_GROUP of kernels_exact.hip (mix_objects_groups)
constexpr int FIR_WAVE_TILES = 2;                        // tiles of 256 samples per wave: two independent accumulators per channel
constexpr int FIR_WAVE_SAMPLES = 256 * FIR_WAVE_TILES;
constexpr int FIR_STAGE_BATCH = 8;                       // global loads a thread issues before it waits, when staging a window
}  // namespace

// P[c][o][LP] = the taps reversed behind 15 zeros and zero-padded: P[15 + j] = h_co[K - 1 - j], so that T[b][m] = P[15 + m - b]
__global__ __launch_bounds__(256) void fir_prepare_kernel(const float *__restrict__ taps, long long n_co, int K, int LP, float *__restrict__ P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_co * LP) return;
    const long long co = i / LP;
    const int j = (int)(i - co * LP) - 15;
    P[i] = j >= 0 && j < K ? taps[co * K + (K - 1 - j)] : 0.f;
}

// One workgroup per (strip of blockDim.x / 64 * 512 samples, group of 32 objects, filter set).  Per object the workgroup stages the
// object's window -- the strip's samples and the K - 1 before them, shifted by the onset, the history in front of the step's
// row -- and its C padded tap rows in LDS once for all channels; every wave then walks the window positions four at a time, one
// A operand per channel (the taps) and one B operand per tile (the window), 2 C MFMAs per step.
//   LDS: win [win_at(W)] | taps [C][LP],  W = strip + Mp window positions
// (The lane decomposition, the batched staging, the two-round walk and the write-out below are the same text in
//  scene_reverb_stage1 of kernels_reverb.hip -- conv_mfma.h says why they are not shared: an edit here wants the same edit there.)
template <int C>
__global__ __launch_bounds__(256) void scene_fir_stage1(const float *__restrict__ rows, int n_obj, long long n, const float *__restrict__ hist,
                                                        int H, const float *__restrict__ P0, const float *__restrict__ P1,
                                                        const int *__restrict__ onset0, const int *__restrict__ onset1, int K, int Mp,
                                                        int LP, float *__restrict__ parts, int groups, long long n_second) {
    extern __shared__ float lds[];
    const int strip = (int)(blockDim.x / 64) * FIR_WAVE_SAMPLES, W = strip + Mp;
    const long long s0 = (long long)blockIdx.x * strip;
    const int grp = blockIdx.y, set = blockIdx.z;
    if (set == 1 && s0 >= n_second) return;              // (the set faded out is needed for the fade's samples only)
    const float *__restrict__ P = set ? P1 : P0;
    const int *__restrict__ onset = set ? onset1 : onset0;
    float *win = lds, *tp = lds + win_at(W) + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int la = lane & 15, lr = lane >> 4;
    const int o0 = grp * FIR_GROUP, o1 = o0 + FIR_GROUP < n_obj ? o0 + FIR_GROUP : n_obj;
    f32x4 acc[C][FIR_WAVE_TILES];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int w = 0; w < FIR_WAVE_TILES; ++w) acc[c][w] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B: lane (k = lr, col a = la) reads window position 16 a + m, m = 4 q + lr;  A: lane (row b = la, k = lr) reads P[15 + m - b]
    int wb[FIR_WAVE_TILES];
#pragma unroll
    for (int w = 0; w < FIR_WAVE_TILES; ++w) wb[w] = (wave * FIR_WAVE_TILES + w) * 256 + 16 * la + lr;
    const int ab = 15 + lr - la;
    const bool wave_live = s0 + (long long)wave * FIR_WAVE_SAMPLES < n;
    for (int o = o0; o < o1; ++o) {
        const float *__restrict__ row = rows + (long long)o * n, *__restrict__ hrow = hist + (long long)o * H;
        const long long shift = s0 - (K - 1) - onset[o];
        __syncthreads();                                 // (the previous object's operands are read)
        // (FIR_STAGE_BATCH loads in flight per thread before the first LDS write: a one-wave workgroup stages ten rounds per object)
        for (int i0 = threadIdx.x; i0 < W; i0 += FIR_STAGE_BATCH * blockDim.x) {
            float v[FIR_STAGE_BATCH];
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                const long long j = shift + i;           // the step's local sample; -H <= j by 0 <= onset <= max_onset
                v[u] = 0.f;
                if (i < W) {
                    if (j >= 0) { if (j < n) v[u] = row[j]; }
                    else if (j >= -(long long)H) v[u] = hrow[H + j];
                }
            }
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                if (i < W) win[win_at(i)] = v[u];
            }
        }
        for (int i0 = threadIdx.x; i0 < C * LP; i0 += FIR_STAGE_BATCH * blockDim.x) {
            float v[FIR_STAGE_BATCH];
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x, c = i / LP;
                v[u] = i < C * LP ? P[((long long)c * n_obj + o) * LP + (i - c * LP)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                if (i < C * LP) tp[i] = v[u];
            }
        }
        __syncthreads();
        if (!wave_live) continue;
        // two rounds of four window positions per pass (Mp is a multiple of 8): the operands of both are read before the first MFMA
        for (int m = 0; m < Mp; m += 8) {
            float b[2][FIR_WAVE_TILES], a[2][C];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int w = 0; w < FIR_WAVE_TILES; ++w) b[r][w] = win[win_at(wb[w] + m + 4 * r)];
#pragma unroll
                for (int c = 0; c < C; ++c) a[r][c] = tp[c * LP + ab + m + 4 * r];
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int w = 0; w < FIR_WAVE_TILES; ++w)
                        acc[c][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][c], b[r][w], acc[c][w], 0, 0, 0);
        }
    }
    // D: lane (col a = la, rows b = 4 lr + g) holds samples 16 a + 4 lr + g of its tile
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float *__restrict__ prow = parts + (((long long)set * C + c) * groups + grp) * n;
#pragma unroll
        for (int w = 0; w < FIR_WAVE_TILES; ++w) {
            const long long s = s0 + (wave * FIR_WAVE_TILES + w) * 256 + 16 * la + 4 * lr;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (s + g < n) prow[s + g] = acc[c][w][g];
        }
    }
}

// the groups' partial rows in group order per channel, blended inside a fade (conv_mfma.h; nothing is added: the null folds away)
__global__ __launch_bounds__(256) void scene_fir_stage2(const float *__restrict__ parts, int C, int n_groups, long long n, long long n_fade,
                                                        long long t0, long long t_set, int R, float *__restrict__ out) {
    conv_stage2(parts, C, n_groups, n, n_fade, t0, t_set, R, nullptr, out);
}

PBSO_DEFINE_HISTORY_KERNEL(fir_history_kernel)

int scene_fir_padded_taps(int K) { return (K + 15 + 7) / 8 * 8 + 16; }

int launch_scene_fir_prepare(const float *taps, long long n_co, int K, float *P, hipStream_t stream) {
    if (n_co <= 0 || K < 1 || K > SCENE_FIR_MAX_TAPS) return (int)hipErrorInvalidValue;
    const long long total = n_co * scene_fir_padded_taps(K);
    hipLaunchKernelGGL(fir_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, taps, n_co, K, scene_fir_padded_taps(K), P);
    return (int)hipGetLastError();
}

template <int C>
static void launch_fir_stage1(dim3 grid, int waves, size_t lds, hipStream_t stream, const float *rows, int n_obj, long long n, const float *hist,
                              int H, const float *P0, const float *P1, const int *on0, const int *on1, int K, int Mp, int LP, float *parts,
                              int groups, long long n_second) {
    hipLaunchKernelGGL(scene_fir_stage1<C>, grid, dim3(64 * waves), lds, stream, rows, n_obj, n, hist, H, P0, P1, on0, on1, K, Mp, LP, parts, groups,
                       n_second);
}

int launch_scene_fir(const float *rows, int n_obj, long long n, const float *hist, float *hist_next, int H, const float *P_to,
                     const float *P_from, const int *onset_to, const int *onset_from, int C, int K, long long n_fade, long long t0,
                     long long t_set, int R, float *parts, float *out, hipStream_t stream) {
    if (n_obj <= 0 || n <= 0 || C < 1 || C > SCENE_MAX_CHANNELS || K < 1 || K > SCENE_FIR_MAX_TAPS || H < 0 || n_fade < 0 || n_fade > n ||
        (n_fade > 0 && (!P_from || !onset_from || R < 2)))
        return (int)hipErrorInvalidValue;
    const int groups = (n_obj + FIR_GROUP - 1) / FIR_GROUP;
    const int LP = scene_fir_padded_taps(K), Mp = LP - 16;
    if (!P_to) {                                         // no filters set yet: silence, and the history moves on
        if (hipMemsetAsync(out, 0, (size_t)C * n * sizeof(float), stream) != hipSuccess) return (int)hipGetLastError();
        if (H > 0)
            hipLaunchKernelGGL(fir_history_kernel, dim3((unsigned)((H + 255) / 256), n_obj < 65535 ? n_obj : 65535), dim3(256), 0, stream, rows, n_obj,
                               n, hist, hist_next, H);
        return (int)hipGetLastError();
    }
    if (!onset_to) return (int)hipErrorInvalidValue;
    // four waves per workgroup once that still gives every CU two workgroups; one wave (strips of 512 samples) for short steps
    int waves = 4;
    if (((n + 4 * FIR_WAVE_SAMPLES - 1) / (4 * FIR_WAVE_SAMPLES)) * groups * (n_fade ? 2 : 1) < 512) waves = 1;
    const int strip = waves * FIR_WAVE_SAMPLES, W = strip + Mp;
    const long long strips = (n + strip - 1) / strip;
    if (strips > 0x7fffffffll) return (int)hipErrorInvalidValue;
    const size_t lds = (size_t)(W + (W >> 4) + 1 + C * LP) * sizeof(float);
    const dim3 grid((unsigned)strips, (unsigned)groups, n_fade ? 2 : 1);
#define PBSO_FIR_CASE(c) \
    case c: launch_fir_stage1<c>(grid, waves, lds, stream, rows, n_obj, n, hist, H, P_to, P_from, onset_to, onset_from, K, Mp, LP, parts, groups, n_fade); break;
    switch (C) {
        PBSO_FIR_CASE(1) PBSO_FIR_CASE(2) PBSO_FIR_CASE(3) PBSO_FIR_CASE(4) PBSO_FIR_CASE(5) PBSO_FIR_CASE(6) PBSO_FIR_CASE(7)
    default: launch_fir_stage1<8>(grid, waves, lds, stream, rows, n_obj, n, hist, H, P_to, P_from, onset_to, onset_from, K, Mp, LP, parts, groups, n_fade); break;
    }
#undef PBSO_FIR_CASE
    hipLaunchKernelGGL(scene_fir_stage2, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, stream, parts, C, groups, n, n_fade, t0, t_set, R, out);
    if (H > 0)
        hipLaunchKernelGGL(fir_history_kernel, dim3((unsigned)((H + 255) / 256), n_obj < 65535 ? n_obj : 65535), dim3(256), 0, stream, rows, n_obj, n,
                           hist, hist_next, H);
    return (int)hipGetLastError();
}

}  // namespace pbso
