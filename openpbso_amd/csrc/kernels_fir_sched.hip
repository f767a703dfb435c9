// The scene filter mix with scheduled sets inside a step (pbso_scene_fir_schedule, pbso_scene_fir_delay_schedule;
// include/openpbso_amd.h "scene filter mix", SCHEDULE): filter sets and delay records change at any sample of one launch.
//
// The step is cut at every filter change point into segments and those into work strips (fir_schedule.h); all filter sets the
// step needs lie in one pool of padded reversed taps, [S + 2] sets of [C][n_obj][LP] with onsets [S + 2][n_obj]: 0 and 1 are the
// set in force and the set faded out when the step begins, 2 + k is the step's scheduled set k.  scene_fir_sched_stage1<C, DELAY>
// is scene_fir_stage1<C> / scene_fir_delay_stage1<C> (kernels_fir.hip, kernels_fir_delay.hip: untouched, a step without a
// scheduled set is launched there as before) with the strip, its end and its filter set taken from the table.  The chain per
// output sample is theirs: objects ascending, taps K - 1 down to 0 on v_mfma_f32_16x16x4_f32, groups of 32.  A window reaches
// back across a segment boundary in the same row: the input does not depend on the filter sets.
// With DELAY the delay records are K_d + 1 blocks of [n_obj], block b in force from t_d[b - 1] on: at tau the block is the number
// of delay sets with t_d <= tau.  fir_delay_expand_kernel chains them with ramp_next (scene_ramp.h), one thread per object.
// Built with -ffp-contract=off, as its siblings.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "fir_schedule.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int FIR_GROUP = 32;                            // the four constants of kernels_fir.hip
constexpr int FIR_WAVE_TILES = 2;
constexpr int FIR_WAVE_SAMPLES = 256 * FIR_WAVE_TILES;
constexpr int FIR_STAGE_BATCH = 8;

// the scene mix's read (kernels_fir_delay.hip has the same three functions; that file is left as it is)
__device__ __forceinline__ void delay_split(double d, long long *off, float *f) {
    const double fl = floor(d), fr = d - fl;             // (exact)
    *off = (long long)fl + (fr != 0.0 ? 1 : 0);
    *f = fr != 0.0 ? (float)(1.0 - fr) : 0.f;
}
__device__ __forceinline__ const float *x_at(const float *__restrict__ row, const float *__restrict__ xrow, long long n, int Hx, long long j) {
    j = j < -(long long)Hx ? -(long long)Hx : (j >= n ? n - 1 : j);
    return j >= 0 ? row + j : xrow + (Hx + j);
}
__device__ __forceinline__ float interp(float x0, float x1, float f) { return f == 0.f ? x0 : x0 + f * (x1 - x0); }

// how many of the ascending times t[0 .. K) are <= tau, given that t[0 .. lo) are and t[hi .. K) are not
__device__ __forceinline__ int count_le(const long long *__restrict__ t, int lo, int hi, long long tau) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= tau) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
}  // namespace

// The delay records of a step: block 0 is the record as it stands, block k + 1 what delay set k leaves (ramp_next, the body of
// pbso_scene_fir_set_delay itself), and the last block goes back to params: what the next step starts from.
__global__ __launch_bounds__(64) void fir_delay_expand_kernel(SceneParam *__restrict__ params, SceneParam *__restrict__ records,
                                                              const long long *__restrict__ t_d, const float *__restrict__ targets, int Kd,
                                                              int n_obj, int Rd, int any_set) {
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= n_obj) return;
    SceneParam q = params[o];
    records[o] = q;
#pragma unroll 4
    for (int k = 0; k < Kd; ++k) {
        q = ramp_next(q, (double)targets[(long long)k * n_obj + o], true, t_d[k], Rd, any_set != 0 || k > 0);
        records[(long long)(k + 1) * n_obj + o] = q;
    }
    params[o] = q;
}

// One workgroup per (work strip, group of 32 objects, to / from).  hist is the history of x, or with DELAY that of z (hist_x then
// holds x's).  rec / t_d / Kd / Rd: the delay blocks (DELAY only).  pool / onpool: the step's filter sets.
template <int C, bool DELAY>
__global__ __launch_bounds__(256) void scene_fir_sched_stage1(const float *__restrict__ rows, int n_obj, long long n,
                                                              const float *__restrict__ hist, int H, const float *__restrict__ hist_x,
                                                              int Hx, const SceneParam *__restrict__ rec, const long long *__restrict__ t_d,
                                                              int Kd, int Rd, long long t0, const FirStrip *__restrict__ strips,
                                                              const float *__restrict__ pool, const int *__restrict__ onpool, int K, int Mp,
                                                              int LP, float *__restrict__ parts, int groups) {
    extern __shared__ float lds[];
    const int strip = (int)(blockDim.x / 64) * FIR_WAVE_SAMPLES, W = strip + Mp;
    const FirStrip e = strips[blockIdx.x];
    const long long s0 = e.s_begin, s_end = e.s_end;
    const int grp = blockIdx.y, set = blockIdx.z;
    const int idx = set ? e.set_from : e.set_to;
    if (idx < 0) return;                                 // (the set faded out is needed by the strips of a fade only)
    const float *__restrict__ P = pool + (long long)idx * C * n_obj * LP;
    const int *__restrict__ onset = onpool + (long long)idx * n_obj;
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
    const bool wave_live = s0 + (long long)wave * FIR_WAVE_SAMPLES < s_end;
    // the delay blocks of the first and last in-step sample any window of this workgroup can hold (its objects' onsets lie in
    // 0 .. H - (K - 1)): the search over all of the step's sets is done once, every object then searches between the two
    int wg_a = 0, wg_b = 0;
    if (DELAY) {
        const long long ja = s0 - H > 0 ? s0 - H : 0, jb = s0 - (K - 1) + W - 1 < n - 1 ? s0 - (K - 1) + W - 1 : n - 1;
        wg_a = count_le(t_d, 0, Kd, t0 + ja);
        wg_b = count_le(t_d, wg_a, Kd, t0 + jb);
        // (what only the staging reads lives in vector registers across the walk, which needs nearly every scalar one:
        //  kernels_fir_delay.hip says why an empty asm says so)
        asm volatile("" : "+v"(t_d), "+v"(rec), "+v"(wg_a), "+v"(wg_b), "+v"(hist_x), "+v"(Hx), "+v"(Rd), "+v"(t0));
    }
    long long s_last = s_end;                            // (the write-out's bound, not needed before it)
    asm volatile("" : "+v"(s_last));
    for (int o = o0; o < o1; ++o) {
        const float *row = rows + (long long)o * n, *hrow = hist + (long long)o * H;
        long long shift = s0 - (K - 1) - onset[o];
        __syncthreads();                                 // (the previous object's operands are read)
        if (DELAY) {
            const float *xrow = hist_x + (long long)o * Hx;
            // the blocks of this object's first and last window positions that lie in the step
            const long long ja = shift > 0 ? shift : 0, jb = shift + W - 1 < n - 1 ? shift + W - 1 : n - 1;
            const int ba = __builtin_amdgcn_readfirstlane(count_le(t_d, wg_a, wg_b, t0 + ja)),
                      bb = __builtin_amdgcn_readfirstlane(count_le(t_d, ba, wg_b, t0 + jb));
            if (ba == bb) {
                // one block: the steady / ramp logic of scene_fir_delay_stage1 on that block's record
                SceneParam q = rec[(long long)ba * n_obj + o];
                const bool steady = Rd == 0 || t0 + ja - q.t_set + 1 >= Rd || (q.slope == 0.0 && q.from == q.to);
                long long off_s = 0;
                float f_s = 0.f;
                if (steady) delay_split(q.to, &off_s, &f_s);
                // (what only the staging reads lives in vector registers across the walk: kernels_fir_delay.hip says why)
                asm volatile("" : "+v"(row), "+v"(hrow), "+v"(xrow), "+v"(shift), "+v"(q.from), "+v"(q.slope));
                for (int i0 = threadIdx.x; i0 < W; i0 += FIR_STAGE_BATCH * blockDim.x) {
                    float v[FIR_STAGE_BATCH], x1[FIR_STAGE_BATCH], f[FIR_STAGE_BATCH];
                    unsigned live = 0;
#pragma unroll
                    for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                        const int i = i0 + u * (int)blockDim.x;
                        const long long j = shift + i;   // the step's local sample tau - t0; -H <= j
                        long long off = off_s;
                        f[u] = f_s;
                        if (!steady) delay_split(ramp_value(q, t0 + j, Rd), &off, &f[u]);
                        const float *p0 = x_at(row, xrow, n, Hx, j - off), *p1 = x_at(row, xrow, n, Hx, j - off + 1);
                        if (j < 0) {
                            p0 = p1 = hrow + (j >= -(long long)H ? H + j : 0);
                            f[u] = 0.f;
                        }
                        v[u] = *p0;
                        x1[u] = *p1;                     // (unused when the fraction is 0)
                        live |= (i < W && j < n && j >= -(long long)H ? 1u : 0u) << u;
                    }
#pragma unroll
                    for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                        const int i = i0 + u * (int)blockDim.x;
                        if (i < W) win[win_at(i)] = (live >> u & 1u) ? interp(v[u], x1[u], f[u]) : 0.f;
                    }
                }
            } else {
                // several blocks in the window: every position finds its own block and takes the per-sample path
                asm volatile("" : "+v"(row), "+v"(hrow), "+v"(xrow), "+v"(shift));
                for (int i = threadIdx.x; i < W; i += blockDim.x) {
                    const long long j = shift + i;
                    float z = 0.f;
                    if (j < 0) {
                        if (j >= -(long long)H) z = hrow[H + j];
                    } else if (j < n) {
                        const int b = count_le(t_d, ba, bb, t0 + j);
                        const SceneParam q = rec[(long long)b * n_obj + o];
                        long long off;
                        float f;
                        delay_split(ramp_value(q, t0 + j, Rd), &off, &f);
                        z = interp(*x_at(row, xrow, n, Hx, j - off), *x_at(row, xrow, n, Hx, j - off + 1), f);
                    }
                    win[win_at(i)] = z;
                }
            }
        } else {
            for (int i0 = threadIdx.x; i0 < W; i0 += FIR_STAGE_BATCH * blockDim.x) {
                float v[FIR_STAGE_BATCH];
#pragma unroll
                for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                    const int i = i0 + u * (int)blockDim.x;
                    const long long j = shift + i;       // the step's local sample; -H <= j by 0 <= onset <= max_onset
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
    // D: lane (col a = la, rows b = 4 lr + g) holds samples 16 a + 4 lr + g of its tile; nothing is written past the strip's end
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float *__restrict__ prow = parts + (((long long)set * C + c) * groups + grp) * n;
#pragma unroll
        for (int w = 0; w < FIR_WAVE_TILES; ++w) {
            const long long s = s0 + (wave * FIR_WAVE_TILES + w) * 256 + 16 * la + 4 * lr;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (s + g < s_last) prow[s + g] = acc[c][w][g];
        }
    }
}

// Stage 2, one thread per (sample, channel = blockIdx.y): the sample's segment is the number of the step's filter sets with
// t_f <= t (0: what the step began with -- have_to0 / have_from0 / t_set0); the groups' partial rows in group order from 0.f, and
// inside that segment's fade the three separately rounded operations of conv_stage2 (conv_mfma.h) with the segment's t_set.
__global__ __launch_bounds__(256) void scene_fir_sched_stage2(const float *__restrict__ parts, int C, int n_groups, long long n,
                                                              long long t0, int R, const long long *__restrict__ t_f, int S, int have_to0,
                                                              int have_from0, long long t_set0, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = blockIdx.y;
    const long long t = t0 + i;
    const int seg = count_le(t_f, 0, S, t);
    const bool has_to = seg > 0 || have_to0 != 0;
    const bool has_from = seg == 0 ? have_to0 != 0 && have_from0 != 0 : (seg == 1 ? have_to0 != 0 : true);
    const long long t_set = seg > 0 ? t_f[seg - 1] : t_set0;
    float y = 0.f;
    if (has_to) {
        const float *p = parts + (long long)c * n_groups * n + i;
        for (int g = 0; g < n_groups; ++g) y = y + p[(long long)g * n];
        if (has_from && t - t_set + 1 < (long long)R) {
            const float *q = p + (long long)C * n_groups * n;
            float yfrom = 0.f;
            for (int g = 0; g < n_groups; ++g) yfrom = yfrom + q[(long long)g * n];
            const float w = (float)((double)(t - t_set + 1) / (double)R);
            const float d = y - yfrom;
            const float wd = w * d;
            y = yfrom + wd;
        }
    }
    out[(long long)c * n + i] = y;
}

// hist_z_next[o] = the last H samples of hist_z[o] ++ z_o(step), z computed again under the block in force at each sample (a pure
// function of hist_x ++ rows, the record and the absolute sample: the bits are those the windows staged)
__global__ __launch_bounds__(256) void fir_sched_z_history_kernel(const float *__restrict__ rows, int n_obj, long long n,
                                                                  const float *__restrict__ hist_z, float *__restrict__ hist_z_next, int H,
                                                                  const float *__restrict__ hist_x, int Hx, const SceneParam *__restrict__ rec,
                                                                  const long long *__restrict__ t_d, int Kd, int Rd, long long t0) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= H) return;
    const long long j = n + k - H;                       // the step's local sample; negative: still in hist_z
    const int b = j >= 0 ? count_le(t_d, 0, Kd, t0 + j) : 0;
    for (long long o = blockIdx.y; o < n_obj; o += gridDim.y) {
        float z;
        if (j < 0) z = hist_z[o * H + (n + k)];
        else {
            const float *__restrict__ row = rows + o * n, *__restrict__ xrow = hist_x + o * Hx;
            long long off;
            float f;
            delay_split(ramp_value(rec[(long long)b * n_obj + o], t0 + j, Rd), &off, &f);
            z = interp(*x_at(row, xrow, n, Hx, j - off), *x_at(row, xrow, n, Hx, j - off + 1), f);
        }
        hist_z_next[o * H + k] = z;
    }
}

PBSO_DEFINE_HISTORY_KERNEL(fir_sched_x_history_kernel)

int scene_fir_sched_strip(long long n, int n_obj) {
    const int groups = (n_obj + FIR_GROUP - 1) / FIR_GROUP;
    // the rule of launch_scene_fir without its factor for a fade (a step's strips differ in that): four waves per workgroup once
    // that still gives every CU two workgroups; one wave (strips of 512 samples) for short steps
    return ((n + 4 * FIR_WAVE_SAMPLES - 1) / (4 * FIR_WAVE_SAMPLES)) * groups < 512 ? FIR_WAVE_SAMPLES : 4 * FIR_WAVE_SAMPLES;
}

template <int C, bool DELAY>
static void launch_sched_stage1(dim3 grid, int waves, size_t lds, hipStream_t stream, const FirSchedStep &a, int Mp, int LP, int groups) {
    hipLaunchKernelGGL((scene_fir_sched_stage1<C, DELAY>), grid, dim3(64 * waves), lds, stream, a.rows, a.n_obj, a.n, a.hist, a.H, a.hist_x, a.Hx,
                       a.rec, a.t_d, a.Kd, a.Rd, a.t0, a.strips, a.pool, a.onpool, a.K, Mp, LP, a.parts, groups);
}
template <int C>
static void launch_sched_stage1_c(bool delay, dim3 grid, int waves, size_t lds, hipStream_t stream, const FirSchedStep &a, int Mp, int LP,
                                  int groups) {
    if (delay) launch_sched_stage1<C, true>(grid, waves, lds, stream, a, Mp, LP, groups);
    else launch_sched_stage1<C, false>(grid, waves, lds, stream, a, Mp, LP, groups);
}

int launch_scene_fir_sched(const FirSchedStep &a, hipStream_t stream) {
    const bool delay = a.params != nullptr;
    if (a.n_obj <= 0 || a.n <= 0 || a.C < 1 || a.C > SCENE_MAX_CHANNELS || a.K < 1 || a.K > SCENE_FIR_MAX_TAPS || a.H < 0 || a.S < 0 ||
        a.S > SCENE_FIR_MAX_SETS_PER_STEP || a.Kd < 0 || a.Kd > SCENE_MAX_SETS_PER_STEP || a.n_strips < 0 || (a.n_strips && !a.strips) ||
        (a.strip != FIR_WAVE_SAMPLES && a.strip != 4 * FIR_WAVE_SAMPLES) || (a.S && !a.t_f) || !a.pool || !a.onpool ||
        (delay && (a.Hx < 1 || a.Rd < 0 || !a.hist_x || !a.hist_x_next || !a.rec || (a.Kd && (!a.t_d || !a.targets)))) || (!delay && a.Kd))
        return (int)hipErrorInvalidValue;
    const int groups = (a.n_obj + FIR_GROUP - 1) / FIR_GROUP;
    const int LP = scene_fir_padded_taps(a.K), Mp = LP - 16;
    const unsigned gy = a.n_obj < 65535 ? a.n_obj : 65535;
    if (delay) {
        // block 0 of the records is the record in force (a step without a delay set in it runs on that block alone)
        hipLaunchKernelGGL(fir_delay_expand_kernel, dim3((unsigned)((a.n_obj + 63) / 64)), dim3(64), 0, stream, a.params, a.rec, a.t_d, a.targets,
                           a.Kd, a.n_obj, a.Rd, a.any_set);
    }
    if (a.n_strips) {
        const int waves = a.strip / FIR_WAVE_SAMPLES, W = a.strip + Mp;
        const size_t lds = (size_t)(W + (W >> 4) + 1 + a.C * LP) * sizeof(float);
        const dim3 grid((unsigned)a.n_strips, (unsigned)groups, a.any_from ? 2 : 1);
#define PBSO_FIR_SCHED_CASE(c) \
    case c: launch_sched_stage1_c<c>(delay, grid, waves, lds, stream, a, Mp, LP, groups); break;
        switch (a.C) {
            PBSO_FIR_SCHED_CASE(1) PBSO_FIR_SCHED_CASE(2) PBSO_FIR_SCHED_CASE(3) PBSO_FIR_SCHED_CASE(4) PBSO_FIR_SCHED_CASE(5)
            PBSO_FIR_SCHED_CASE(6) PBSO_FIR_SCHED_CASE(7)
        default: launch_sched_stage1_c<8>(delay, grid, waves, lds, stream, a, Mp, LP, groups); break;
        }
#undef PBSO_FIR_SCHED_CASE
    }
    hipLaunchKernelGGL(scene_fir_sched_stage2, dim3((unsigned)((a.n + 255) / 256), a.C), dim3(256), 0, stream, a.parts, a.C, groups, a.n, a.t0,
                       a.R, a.t_f, a.S, a.have_to0, a.have_from0, a.t_set0, a.out);
    if (delay) {
        if (a.H > 0)
            hipLaunchKernelGGL(fir_sched_z_history_kernel, dim3((unsigned)((a.H + 255) / 256), gy), dim3(256), 0, stream, a.rows, a.n_obj, a.n,
                               a.hist, a.hist_next, a.H, a.hist_x, a.Hx, a.rec, a.t_d, a.Kd, a.Rd, a.t0);
        hipLaunchKernelGGL(fir_sched_x_history_kernel, dim3((unsigned)((a.Hx + 255) / 256), gy), dim3(256), 0, stream, a.rows, a.n_obj, a.n,
                           a.hist_x, a.hist_x_next, a.Hx);
    } else if (a.H > 0) {
        hipLaunchKernelGGL(fir_sched_x_history_kernel, dim3((unsigned)((a.H + 255) / 256), gy), dim3(256), 0, stream, a.rows, a.n_obj, a.n, a.hist,
                           a.hist_next, a.H);
    }
    return (int)hipGetLastError();
}

}  // namespace pbso
