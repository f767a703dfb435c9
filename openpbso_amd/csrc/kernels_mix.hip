// The scene mixer (pbso_scene_mix): C output channels, each (channel, object) pair with a ramped gain and a fractional delay.
//
//   out_c(t) = sum_o g_co(t) * x_o(t - d_co(t)),   t = t0 + i the absolute sample, summed in object order
//
// in the two stages of fixed order of pbso_mix_objects (kernels_exact.hip): groups of MIX_GROUP consecutive objects side by side,
// then the groups' partial rows in group order.  Every per-sample quantity is a function of the absolute sample t alone (the
// ramps are evaluated per sample from (from, to, t_set, slope), the read position is split into an integer offset and a fraction in
// fp64), so the result does not depend on how the caller cuts its samples into steps.  Meant to be bound by the HBM reads of the
// step's rows (DESIGN.md section 4 has the byte count and what was measured).  Built with -ffp-contract=off: the fast path
// (parameters constant over a wave's samples) and the per-sample path must round alike.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "delay_read.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int SCENE_GROUP = 32;                          // = MIX_GROUP of kernels_exact.hip (mix_objects_groups)

// (delay_split and interp: delay_read.h)
// x_o at the step's local sample j: the step's row for j >= 0, the history before it for -H <= j < 0.  Every read of the mix
// lies there (0 <= d <= max_delay = H - 1, and x(i0 + 1) is read only with a fraction, i0 + 1 <= t); the clamp keeps an address
// in the buffers whatever the arguments.
__device__ __forceinline__ float fetch(const float *__restrict__ row, const float *__restrict__ hrow, long long n, int H, long long j) {
    j = j < -(long long)H ? -(long long)H : (j >= n ? n - 1 : j);
    return j >= 0 ? row[j] : hrow[H + j];
}
}  // namespace

// One wave per (64 samples, group of 32 objects), one sample per lane: every load of the wave reads 64 consecutive floats of one
// row.  The objects go in batches of NB: while every parameter of the batch is at its target over the wave's samples (the
// steady state between set calls), the reads of all NB objects and C channels are issued before the first add -- NB x C x 2
// loads in flight per lane -- and the adds follow in object order.  Channel c of an object reads the row shifted by its delay:
// what the wave of those samples reads for channel c' is read again by the wave (d_c - d_c') / 64 tiles away.  The tiles of one
// group are laid out in contiguous runs per XCD (the workgroup index is swizzled below), so that such re-reads can be served by
// that XCD's L2 rather than HBM -- an expectation, see DESIGN.md section 4 for what was measured.
// Anything else (a ramp in the wave's samples, a ragged last batch) takes the per-sample path, which computes the same values.
//
// SCHED (a step with scheduled sets inside it, pbso_scene_mix_schedule): params holds K + 1 blocks of parameters, block k in force
// from t_set[k - 1] on (block 0: what the step began with), so at sample t the block in force is the number of sets with
// t_set <= t.  The wave finds the blocks of its first and of its last sample in the sorted times -- its tile is the same for
// every lane, so the search is uniform -- and where they are one block it runs on that block as above: the steady path and its
// batches as they are.  Otherwise every lane counts on to the block of its own sample (a tile may hold any number of sets) and
// every batch takes the per-sample path from there.
template <int C, bool SCHED>
__global__ __launch_bounds__(64) void scene_mix_stage1(const float *__restrict__ rows, int n_obj, long long n, const float *__restrict__ hist,
                                                       int H, const SceneParam *__restrict__ params, int R, long long t0,
                                                       float *__restrict__ parts, unsigned tiles, unsigned groups,
                                                       const long long *__restrict__ t_set, int K) {
    constexpr int NB = C >= 5 ? 1 : (C >= 3 ? 2 : 8 / C);
    // workgroups are dealt to the 8 XCDs in turn: renumber them so that XCD x runs a contiguous run of (tile, group) pairs
    const unsigned total = tiles * groups, L = blockIdx.x, q = total / 8, r = total % 8, x = L % 8, k8 = L / 8;
    const unsigned id = x < r ? x * (q + 1) + k8 : r * (q + 1) + (x - r) * q + k8;
    const unsigned tile = id % tiles, grp = id / tiles;
    const long long s = (long long)tile * 64 + threadIdx.x, ta = t0 + (long long)tile * 64;
    const int o0 = grp * SCENE_GROUP, o1 = o0 + SCENE_GROUP < n_obj ? o0 + SCENE_GROUP : n_obj;
    bool one_block = true;
    const SceneParam *mine = params;                     // the block in force at the lane's own sample
    if (SCHED) {
        const long long block = (long long)C * n_obj * 2;
        const long long tb = ta + 63 < t0 + n - 1 ? ta + 63 : t0 + n - 1;    // the tile's last sample inside the step
        int lo = 0, hi = K;                              // seg_a: the sets with t_set <= ta
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (t_set[mid] <= ta) lo = mid + 1;
            else hi = mid;
        }
        const int seg_a = lo;
        hi = K;                                          // seg_b: the sets with t_set <= tb (>= seg_a)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (t_set[mid] <= tb) lo = mid + 1;
            else hi = mid;
        }
        const int seg_b = lo;
        one_block = seg_a == seg_b;
        int seg = seg_a;                                 // (lanes past the step's end stop at seg_b: they store nothing)
        for (int k = seg_a; k < seg_b; ++k) seg += t_set[k] <= t0 + s ? 1 : 0;
        mine = params + (long long)seg * block;
        params += (long long)seg_a * block;
    }
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (int ob = o0; ob < o1; ob += NB) {
        bool steady = ob + NB <= o1 && one_block;
        if (R != 0 && steady) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const SceneParam *q = params + ((long long)c * n_obj + ob + j) * 2;
                    steady = steady && ta - q[0].t_set + 1 >= R && ta - q[1].t_set + 1 >= R;
                }
        }
        if (steady) {
            // what ramp_value returns over the whole wave, split once per (object, channel)
            float g[NB][C], f[NB][C], x0[NB][C], x1[NB][C];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float *row = rows + (long long)(ob + j) * n, *hrow = hist + (long long)(ob + j) * H;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const SceneParam *q = params + ((long long)c * n_obj + ob + j) * 2;
                    long long off;
                    g[j][c] = (float)q[0].to;
                    delay_split(q[1].to, &off, &f[j][c]);
                    x0[j][c] = fetch(row, hrow, n, H, s - off);
                    x1[j][c] = fetch(row, hrow, n, H, s - off + 1);       // (unused when the fraction is 0)
                }
            }
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += g[j][c] * interp(x0[j][c], x1[j][c], f[j][c]);
        } else {
            const int oe = ob + NB < o1 ? ob + NB : o1;
            for (int o = ob; o < oe; ++o) {
                const float *row = rows + (long long)o * n, *hrow = hist + (long long)o * H;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const SceneParam *q = (SCHED ? mine : params) + ((long long)c * n_obj + o) * 2;
                    const float g = (float)ramp_value(q[0], t0 + s, R);
                    long long off;
                    float f;
                    delay_split(ramp_value(q[1], t0 + s, R), &off, &f);
                    const float x0 = fetch(row, hrow, n, H, s - off), x1 = f == 0.f ? x0 : fetch(row, hrow, n, H, s - off + 1);
                    acc[c] += g * interp(x0, x1, f);
                }
            }
        }
    }
    if (s >= n) return;
#pragma unroll
    for (int c = 0; c < C; ++c) parts[((long long)c * groups + grp) * n + s] = acc[c];
}

// A schedule's sets, one after the other, for one parameter per thread (i = (channel * n_obj + object) * 2 + kind, the index into
// params): block 0 of the records is the parameter as it stands, block k + 1 what set k leaves (ramp_next of scene_ramp.h, the
// body of pbso_scene_mix_set itself), and the last block goes back to params: what the next step starts from.
__global__ __launch_bounds__(64) void scene_schedule_expand_kernel(SceneParam *__restrict__ params, SceneParam *__restrict__ records,
                                                                   const long long *__restrict__ t_set, const int *__restrict__ has_delay,
                                                                   const float *__restrict__ targets, int K, long long cn, int R, int any_set) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= 2 * cn) return;
    const int kind = (int)(i & 1);
    const float *v = targets + (long long)kind * cn + (i >> 1);
    SceneParam q = params[i];
    records[i] = q;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const bool changed = kind == 0 || has_delay[k] != 0;
        const double to = changed ? (double)v[(long long)k * 2 * cn] : 0.0;
        q = ramp_next(q, to, changed, t_set[k], R, any_set != 0 || k > 0);
        records[(long long)(k + 1) * 2 * cn + i] = q;
    }
    params[i] = q;
}

// the groups' partial rows in group order, per channel (mix_objects_stage2 with a channel axis: blockIdx.y)
__global__ __launch_bounds__(256) void scene_mix_stage2(const float *__restrict__ parts, int n_groups, long long n, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *p = parts + (long long)blockIdx.y * n_groups * n + i;
    float acc = 0.f;
    for (int g = 0; g < n_groups; ++g) acc += p[(long long)g * n];
    out[(long long)blockIdx.y * n + i] = acc;
}

PBSO_DEFINE_HISTORY_KERNEL(scene_history_kernel)

template <int C>
static void launch_stage1(long long n, int groups, hipStream_t stream, const float *rows, int n_obj, const float *hist, int H,
                          const SceneParam *params, int R, long long t0, float *parts) {
    const unsigned tiles = (unsigned)((n + 63) / 64);
    // (no set inside the step: the build without the schedule, whose two trailing arguments are not read)
    hipLaunchKernelGGL((scene_mix_stage1<C, false>), dim3(tiles * (unsigned)groups), dim3(64), 0, stream, rows, n_obj, n, hist, H, params, R, t0,
                       parts, tiles, (unsigned)groups, (const long long *)nullptr, 0);
}

int launch_scene_mix(const float *rows, int n_obj, long long n, const float *hist, float *hist_next, int H, const SceneParam *params,
                     int C, int ramp, long long t0, float *parts, float *out, hipStream_t stream) {
    if (n_obj <= 0 || n <= 0 || C < 1 || C > SCENE_MAX_CHANNELS || H < 1) return (int)hipErrorInvalidValue;
    const int groups = (n_obj + SCENE_GROUP - 1) / SCENE_GROUP;
    if ((unsigned long long)((n + 63) / 64) * groups > 0xffffffffull) return (int)hipErrorInvalidValue;
    switch (C) {
    case 1: launch_stage1<1>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    case 2: launch_stage1<2>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    case 3: launch_stage1<3>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    case 4: launch_stage1<4>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    case 5: launch_stage1<5>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    case 6: launch_stage1<6>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    case 7: launch_stage1<7>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    default: launch_stage1<8>(n, groups, stream, rows, n_obj, hist, H, params, ramp, t0, parts); break;
    }
    hipLaunchKernelGGL(scene_mix_stage2, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, stream, parts, groups, n, out);
    hipLaunchKernelGGL(scene_history_kernel, dim3((unsigned)((H + 255) / 256), n_obj < 65535 ? n_obj : 65535), dim3(256), 0, stream,
                       rows, n_obj, n, hist, hist_next, H);
    return (int)hipGetLastError();
}

template <int C>
static void launch_stage1_schedule(long long n, int groups, hipStream_t stream, const float *rows, int n_obj, const float *hist, int H,
                                   const SceneParam *records, const long long *t_set, int K, int R, long long t0, float *parts) {
    const unsigned tiles = (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL((scene_mix_stage1<C, true>), dim3(tiles * (unsigned)groups), dim3(64), 0, stream, rows, n_obj, n, hist, H, records, R, t0,
                       parts, tiles, (unsigned)groups, t_set, K);
}

int launch_scene_mix_schedule(const float *rows, int n_obj, long long n, const float *hist, float *hist_next, int H, SceneParam *params,
                              int C, int ramp, long long t0, float *parts, float *out, hipStream_t stream, SceneParam *records,
                              const long long *t_set, const int *has_delay, const float *targets, int K, int any_set) {
    if (n_obj <= 0 || n <= 0 || C < 1 || C > SCENE_MAX_CHANNELS || H < 1 || K < 1 || K > SCENE_MAX_SETS_PER_STEP)
        return (int)hipErrorInvalidValue;
    const int groups = (n_obj + SCENE_GROUP - 1) / SCENE_GROUP;
    if ((unsigned long long)((n + 63) / 64) * groups > 0xffffffffull) return (int)hipErrorInvalidValue;
    const long long cn = (long long)C * n_obj;
    hipLaunchKernelGGL(scene_schedule_expand_kernel, dim3((unsigned)((2 * cn + 63) / 64)), dim3(64), 0, stream, params, records, t_set,
                       has_delay, targets, K, cn, ramp, any_set);
    switch (C) {
    case 1: launch_stage1_schedule<1>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    case 2: launch_stage1_schedule<2>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    case 3: launch_stage1_schedule<3>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    case 4: launch_stage1_schedule<4>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    case 5: launch_stage1_schedule<5>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    case 6: launch_stage1_schedule<6>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    case 7: launch_stage1_schedule<7>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    default: launch_stage1_schedule<8>(n, groups, stream, rows, n_obj, hist, H, records, t_set, K, ramp, t0, parts); break;
    }
    hipLaunchKernelGGL(scene_mix_stage2, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, stream, parts, groups, n, out);
    hipLaunchKernelGGL(scene_history_kernel, dim3((unsigned)((H + 255) / 256), n_obj < 65535 ? n_obj : 65535), dim3(256), 0, stream,
                       rows, n_obj, n, hist, hist_next, H);
    return (int)hipGetLastError();
}

}  // namespace pbso
