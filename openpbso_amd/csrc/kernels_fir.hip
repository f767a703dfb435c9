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
//
// Behind a ramped fractional delay per object (pbso_scene_fir_delay_enable; include/openpbso_amd.h "scene filter mix") x_o above
// is z_o(tau) = x_o read at tau - d_o(tau), the scene mix's read (delay_read.h).  A window position that lies in the step is z,
// computed on the way into LDS from the x history ++ the step's row (two loads, three rounded f32 operations); one before the
// step is read from the z history, where the step that contained it left it under the record in force then.  z rows are never
// written to memory.
//
// With scheduled sets inside a step (pbso_scene_fir_schedule, pbso_scene_fir_delay_schedule; SCHEDULE in the header) filter sets
// and delay records change at any sample of one launch.  The step is cut at every filter change point into segments and those into
// work strips (fir_schedule.h); all filter sets the step needs lie in one pool of padded reversed taps, [S + 2] sets of
// [C][n_obj][LP] with onsets [S + 2][n_obj]: 0 and 1 are the set in force and the set faded out when the step begins, 2 + k is the
// step's scheduled set k.  A window reaches back across a segment boundary in the same row: the input does not depend on the
// filter sets.  The delay records are K_d + 1 blocks of [n_obj], block b in force from t_d[b - 1] on: at tau the block is the
// number of delay sets with t_d <= tau.  fir_delay_expand_kernel chains them with ramp_next (scene_ramp.h), one thread per object.
//
// Built with -ffp-contract=off (the read and the blend of a fade are separately rounded operations, and the steady path -- the
// delay split once per object -- and the per-sample path must round alike) and without any fast-math or denormal flag: subnormal
// samples come through as fmaf gives them.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "delay_read.h"
#include "fir_schedule.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int FIR_GROUP = 32;                            // = MIX_GROUP of kernels_exact.hip (mix_objects_groups)
constexpr int FIR_WAVE_TILES = 2;                        // tiles of 256 samples per wave: two independent accumulators per channel
constexpr int FIR_WAVE_SAMPLES = 256 * FIR_WAVE_TILES;
constexpr int FIR_STAGE_BATCH = 8;                       // global loads a thread issues before it waits, when staging a window

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

// The kernel arguments of the first stage's four variants.  Flat is the list the kernel is declared on, argument by argument
// (scene_fir_stage1 takes it as a pack and rebuilds the struct): every variant has its own argument layout, and keeps it.
//   hist: the history of x, or with DELAY that of z (hist_x then holds x's);  rec, Rd, t0: the delay records, their ramp, the step's
//   first absolute sample;  t_d / Kd: the times of the record blocks;  strips / pool / onpool: the step's work strips and filter sets
template <class... A>
struct KernArgs {};

struct FirPlain {
    static constexpr bool DELAY = false, SCHED = false;
    using Flat = KernArgs<const float *__restrict__, int, long long, const float *__restrict__, int, const float *__restrict__,
                          const float *__restrict__, const int *__restrict__, const int *__restrict__, int, int, int, float *__restrict__, int,
                          long long>;
    const float *__restrict__ rows; int n_obj; long long n; const float *__restrict__ hist; int H;
    const float *__restrict__ P0, *__restrict__ P1; const int *__restrict__ onset0, *__restrict__ onset1;
    int K, Mp, LP; float *__restrict__ parts; int groups; long long n_second;
};
struct FirDelay {
    static constexpr bool DELAY = true, SCHED = false;
    using Flat = KernArgs<const float *__restrict__, int, long long, const float *__restrict__, int, const float *__restrict__, int,
                          const SceneParam *__restrict__, int, long long, const float *__restrict__, const float *__restrict__,
                          const int *__restrict__, const int *__restrict__, int, int, int, float *__restrict__, int, long long>;
    const float *__restrict__ rows; int n_obj; long long n; const float *__restrict__ hist; int H;
    const float *__restrict__ hist_x; int Hx; const SceneParam *__restrict__ rec; int Rd; long long t0;
    const float *__restrict__ P0, *__restrict__ P1; const int *__restrict__ onset0, *__restrict__ onset1;
    int K, Mp, LP; float *__restrict__ parts; int groups; long long n_second;
};
template <bool D>
struct FirSched {
    static constexpr bool DELAY = D, SCHED = true;
    using Flat = KernArgs<const float *__restrict__, int, long long, const float *__restrict__, int, const float *__restrict__, int,
                          const SceneParam *__restrict__, const long long *__restrict__, int, int, long long, const FirStrip *__restrict__,
                          const float *__restrict__, const int *__restrict__, int, int, int, float *__restrict__, int>;
    const float *__restrict__ rows; int n_obj; long long n; const float *__restrict__ hist; int H;
    const float *__restrict__ hist_x; int Hx; const SceneParam *__restrict__ rec; const long long *__restrict__ t_d; int Kd, Rd; long long t0;
    const FirStrip *__restrict__ strips; const float *__restrict__ pool; const int *__restrict__ onpool;
    int K, Mp, LP; float *__restrict__ parts; int groups;
};

// P[c][o][LP] = the taps reversed behind 15 zeros and zero-padded: P[15 + j] = h_co[K - 1 - j], so that T[b][m] = P[15 + m - b]
__global__ __launch_bounds__(256) void fir_prepare_kernel(const float *__restrict__ taps, long long n_co, int K, int LP, float *__restrict__ P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_co * LP) return;
    const long long co = i / LP;
    const int j = (int)(i - co * LP) - 15;
    P[i] = j >= 0 && j < K ? taps[co * K + (K - 1 - j)] : 0.f;
}

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

// One workgroup per (strip of at most blockDim.x / 64 * 512 samples, group of 32 objects, filter set: to / from).  Per object the
// workgroup stages the object's window -- the strip's samples and the K - 1 before them, shifted by the onset, the history in
// front of the step's row -- and its C padded tap rows in LDS once for all channels; every wave then walks the window positions
// four at a time, one A operand per channel (the taps) and one B operand per tile (the window), 2 C MFMAs per step.
//   LDS: win [win_at(W)] | taps [C][LP],  W = strip + Mp window positions
// The variants (Args, above) differ in where the strip and its filter set come from -- the launch's grid and two sets, or with
// SCHED the step's table -- and in what is staged into the window: x, or with DELAY z.  conv_mfma.h says why they are one template
// with `if constexpr` regions and nothing finer; scene_reverb_stage1 (kernels_reverb.hip) has the lane decomposition, the batched
// staging, the two-round walk and the write-out in a loop of its own.
template <int C, class Args, class... A>
__global__ __launch_bounds__(256) void scene_fir_stage1(A... flat) {
    constexpr bool DELAY = Args::DELAY, SCHED = Args::SCHED;
    Args p{flat...};
    extern __shared__ float lds[];
    const int strip = (int)(blockDim.x / 64) * FIR_WAVE_SAMPLES, W = strip + p.Mp;
    const int grp = blockIdx.y, set = blockIdx.z;
    // the strip [s0, s_end) and the filter set idx (to / from: 0 / 1): the launch's grid, or with SCHED an entry of the step's table
    // and an index into its pool
    long long s0 = (long long)blockIdx.x * strip, s_end = p.n;
    int idx = set;
    if constexpr (SCHED) {
        const FirStrip e = p.strips[blockIdx.x];
        s0 = e.s_begin, s_end = e.s_end;
        idx = set ? e.set_from : e.set_to;
        if (idx < 0) return;                             // (the set faded out is needed by the strips of a fade only)
    } else {
        if (set == 1 && s0 >= p.n_second) return;        // (the set faded out is needed for the fade's samples only)
    }
    const float *__restrict__ P;
    const int *__restrict__ onset;
    if constexpr (SCHED) P = p.pool + (long long)idx * C * p.n_obj * p.LP, onset = p.onpool + (long long)idx * p.n_obj;
    else P = idx ? p.P1 : p.P0, onset = idx ? p.onset1 : p.onset0;
    float *win = lds, *tp = lds + win_at(W) + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int la = lane & 15, lr = lane >> 4;
    const int o0 = grp * FIR_GROUP, o1 = o0 + FIR_GROUP < p.n_obj ? o0 + FIR_GROUP : p.n_obj;
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
    // (What only the staging reads goes to vector registers in the asm statements from here on.  Left to itself the compiler
    //  (AMD clang 22, ROCm 7.2) keeps every uniform value in a scalar register; the walk below already needs 96-98 of the 102, and
    //  these values were then spilled to spare vector lanes across it.  An empty asm with a "v" constraint is the only way to say
    //  "this uniform value lives in a VGPR"; tests/test_scene_fir_asm_guards.py (no SGPR spills) tells when a compiler no longer
    //  needs it, or needs more.)
    int wg_a = 0, wg_b = 0;
    if constexpr (SCHED && DELAY) {
        // the delay blocks of the first and last in-step sample any window of this workgroup can hold (its objects' onsets lie in
        // 0 .. H - (K - 1)): the search over all of the step's sets is done once, every object then searches between the two
        const long long ja = s0 - p.H > 0 ? s0 - p.H : 0, jb = s0 - (p.K - 1) + W - 1 < p.n - 1 ? s0 - (p.K - 1) + W - 1 : p.n - 1;
        wg_a = count_le(p.t_d, 0, p.Kd, p.t0 + ja);
        wg_b = count_le(p.t_d, wg_a, p.Kd, p.t0 + jb);
        asm volatile("" : "+v"(p.t_d), "+v"(p.rec), "+v"(wg_a), "+v"(wg_b), "+v"(p.hist_x), "+v"(p.Hx), "+v"(p.Rd), "+v"(p.t0));
    }
    long long s_last = s_end;                            // (the write-out's bound, not needed before it)
    if constexpr (SCHED) asm volatile("" : "+v"(s_last));
    for (int o = o0; o < o1; ++o) {
        const float *row = p.rows + (long long)o * p.n, *hrow = p.hist + (long long)o * p.H;
        long long shift = s0 - (p.K - 1) - onset[o];
        if constexpr (SCHED || !DELAY) __syncthreads();  // (the previous object's operands are read)
        if constexpr (DELAY) {
            const float *xrow = p.hist_x + (long long)o * p.Hx;
            // the blocks of this object's first and last window positions that lie in the step: one, block 0, without a schedule
            const long long ja = shift > 0 ? shift : 0;
            int ba = 0, bb = 0;
            if constexpr (SCHED) {
                const long long jb = shift + W - 1 < p.n - 1 ? shift + W - 1 : p.n - 1;
                ba = __builtin_amdgcn_readfirstlane(count_le(p.t_d, wg_a, wg_b, p.t0 + ja));
                bb = __builtin_amdgcn_readfirstlane(count_le(p.t_d, ba, wg_b, p.t0 + jb));
            }
            if (!SCHED || ba == bb) {
                // (without a schedule the index is spelled `o`: behind `0 * n_obj + o` scene_fir_stage1<1, FirDelay> comes out
                //  with other registers than the build that was measured)
                SceneParam q = p.rec[SCHED ? (long long)ba * p.n_obj + o : o];
                // steady: the object's ramp is over at the first sample of the window that lies in the step, hence at all of them, or
                // the record does not move at all (from == to and slope 0: a first set, the records a reset settled, the zeros before
                // any set) -- what ramp_value returns there is `to` (from + 0 * k == from), split once (a uniform decision: one
                // branch per object, none per position)
                const bool steady = p.Rd == 0 || p.t0 + ja - q.t_set + 1 >= p.Rd || (q.slope == 0.0 && q.from == q.to);
                long long off_s = 0;
                float f_s = 0.f;
                if (steady) delay_split(q.to, &off_s, &f_s);
                asm volatile("" : "+v"(row), "+v"(hrow), "+v"(xrow), "+v"(shift), "+v"(q.from), "+v"(q.slope));
                if constexpr (!SCHED) __syncthreads();   // (the previous object's operands are read; here: behind the record's load)
                // (FIR_STAGE_BATCH positions per thread, two loads each in flight before the first LDS write)
                for (int i0 = threadIdx.x; i0 < W; i0 += FIR_STAGE_BATCH * blockDim.x) {
                    float v[FIR_STAGE_BATCH], x1[FIR_STAGE_BATCH], f[FIR_STAGE_BATCH];
                    unsigned live = 0;                   // bit u: position u of the batch stages a value (kept in a register, not in masks)
#pragma unroll
                    for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                        const int i = i0 + u * (int)blockDim.x;
                        const long long j = shift + i;   // the step's local sample tau - t0; -H <= j by 0 <= onset <= max_onset
                        // every position loads from an address inside the buffers and selects afterwards (no branch per position):
                        // in the step the two samples of the read, before it the z history twice with a fraction of 0 (which
                        // stages the value itself), and 0 past the step's end and past the window's
                        long long off = off_s;
                        f[u] = f_s;
                        if (!steady) delay_split(ramp_value(q, p.t0 + j, p.Rd), &off, &f[u]);
                        const float *p0 = x_at(row, xrow, p.n, p.Hx, j - off), *p1 = x_at(row, xrow, p.n, p.Hx, j - off + 1);
                        if (j < 0) {
                            p0 = p1 = hrow + (j >= -(long long)p.H ? p.H + j : 0);
                            f[u] = 0.f;
                        }
                        v[u] = *p0;
                        x1[u] = *p1;                     // (unused when the fraction is 0)
                        live |= (i < W && j < p.n && j >= -(long long)p.H ? 1u : 0u) << u;
                    }
#pragma unroll
                    for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                        const int i = i0 + u * (int)blockDim.x;
                        if (i < W) win[win_at(i)] = (live >> u & 1u) ? interp(v[u], x1[u], f[u]) : 0.f;
                    }
                }
            } else if constexpr (SCHED) {
                // several blocks in the window: every position finds its own block and takes the per-sample path
                asm volatile("" : "+v"(row), "+v"(hrow), "+v"(xrow), "+v"(shift));
                for (int i = threadIdx.x; i < W; i += blockDim.x) {
                    const long long j = shift + i;
                    float z = 0.f;
                    if (j < 0) {
                        if (j >= -(long long)p.H) z = hrow[p.H + j];
                    } else if (j < p.n) {
                        const int b = count_le(p.t_d, ba, bb, p.t0 + j);
                        const SceneParam q = p.rec[(long long)b * p.n_obj + o];
                        long long off;
                        float f;
                        delay_split(ramp_value(q, p.t0 + j, p.Rd), &off, &f);
                        z = interp(*x_at(row, xrow, p.n, p.Hx, j - off), *x_at(row, xrow, p.n, p.Hx, j - off + 1), f);
                    }
                    win[win_at(i)] = z;
                }
            }
        } else {
            // (FIR_STAGE_BATCH loads in flight per thread before the first LDS write: a one-wave workgroup stages ten rounds per object)
            for (int i0 = threadIdx.x; i0 < W; i0 += FIR_STAGE_BATCH * blockDim.x) {
                float v[FIR_STAGE_BATCH];
#pragma unroll
                for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                    const int i = i0 + u * (int)blockDim.x;
                    const long long j = shift + i;       // the step's local sample; -H <= j by 0 <= onset <= max_onset
                    v[u] = 0.f;
                    if (i < W) {
                        if (j >= 0) { if (j < p.n) v[u] = row[j]; }
                        else if (j >= -(long long)p.H) v[u] = hrow[p.H + j];
                    }
                }
#pragma unroll
                for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                    const int i = i0 + u * (int)blockDim.x;
                    if (i < W) win[win_at(i)] = v[u];
                }
            }
        }
        for (int i0 = threadIdx.x; i0 < C * p.LP; i0 += FIR_STAGE_BATCH * blockDim.x) {
            float v[FIR_STAGE_BATCH];
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x, c = i / p.LP;
                v[u] = i < C * p.LP ? P[((long long)c * p.n_obj + o) * p.LP + (i - c * p.LP)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                if (i < C * p.LP) tp[i] = v[u];
            }
        }
        __syncthreads();
        if (!wave_live) continue;
        // two rounds of four window positions per pass (Mp is a multiple of 8): the operands of both are read before the first MFMA
        for (int m = 0; m < p.Mp; m += 8) {
            float b[2][FIR_WAVE_TILES], a[2][C];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int w = 0; w < FIR_WAVE_TILES; ++w) b[r][w] = win[win_at(wb[w] + m + 4 * r)];
#pragma unroll
                for (int c = 0; c < C; ++c) a[r][c] = tp[c * p.LP + ab + m + 4 * r];
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
        float *__restrict__ prow = p.parts + (((long long)set * C + c) * p.groups + grp) * p.n;
#pragma unroll
        for (int w = 0; w < FIR_WAVE_TILES; ++w) {
            const long long s = s0 + (wave * FIR_WAVE_TILES + w) * 256 + 16 * la + 4 * lr;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (s + g < s_last) prow[s + g] = acc[c][w][g];
        }
    }
}

// the groups' partial rows in group order per channel, blended inside a fade (conv_mfma.h; nothing is added: the null folds away)
__global__ __launch_bounds__(256) void scene_fir_stage2(const float *__restrict__ parts, int C, int n_groups, long long n, long long n_fade,
                                                        long long t0, long long t_set, int R, float *__restrict__ out) {
    conv_stage2(parts, C, n_groups, n, n_fade, t0, t_set, R, nullptr, out);
}

// Stage 2 of a step with scheduled sets, one thread per (sample, channel = blockIdx.y): the sample's segment is the number of the
// step's filter sets with t_f <= t (0: what the step began with -- have_to0 / have_from0 / t_set0); the groups' partial rows in
// group order from 0.f, and inside that segment's fade the three separately rounded operations of conv_stage2 (conv_mfma.h) with
// the segment's t_set.
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

// hist_z_next[o] = the last H samples of hist_z[o] ++ z_o(step), z computed again under the record in force at each sample (a pure
// function of hist_x ++ rows, the record and the absolute sample: the bits are those the windows staged), o striding over
// blockIdx.y.  Sched: nothing (one record per object, rec [n_obj]), or the arguments t_d, Kd of a step with a schedule (rec
// [Kd + 1][n_obj], the block searched once per thread) -- two kernels, each with no argument it does not read.
template <class... Sched>
__global__ __launch_bounds__(256) void fir_z_history_kernel(const float *__restrict__ rows, int n_obj, long long n,
                                                            const float *__restrict__ hist_z, float *__restrict__ hist_z_next, int H,
                                                            const float *__restrict__ hist_x, int Hx, const SceneParam *__restrict__ rec,
                                                            Sched... sched, int Rd, long long t0) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= H) return;
    const long long j = n + k - H;                       // the step's local sample; negative: still in hist_z
    int b = 0;
    if constexpr (sizeof...(Sched) != 0) {
        const struct { const long long *__restrict__ t_d; int Kd; } s{sched...};
        if (j >= 0) b = count_le(s.t_d, 0, s.Kd, t0 + j);
    }
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

PBSO_DEFINE_HISTORY_KERNEL(fir_history_kernel)

int scene_fir_padded_taps(int K) { return (K + 15 + 7) / 8 * 8 + 16; }

int launch_scene_fir_prepare(const float *taps, long long n_co, int K, float *P, hipStream_t stream) {
    if (n_co <= 0 || K < 1 || K > SCENE_FIR_MAX_TAPS) return (int)hipErrorInvalidValue;
    const long long total = n_co * scene_fir_padded_taps(K);
    hipLaunchKernelGGL(fir_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, taps, n_co, K, scene_fir_padded_taps(K), P);
    return (int)hipGetLastError();
}

namespace {
// The launch shape of the first stage, for every variant.  The strip of a step of n samples whose workgroups run `sets` filter
// sets (2 inside a fade): four waves per workgroup once that still gives every CU two workgroups; one wave (strips of 512 samples)
// for short steps.  scene_fir_sched_strip is this rule without the factor for a fade: the strips of a step with a schedule
// differ in that.
int fir_strip(long long n, int groups, int sets) {
    return ((n + 4 * FIR_WAVE_SAMPLES - 1) / (4 * FIR_WAVE_SAMPLES)) * groups * sets < 512 ? FIR_WAVE_SAMPLES : 4 * FIR_WAVE_SAMPLES;
}
int fir_groups(int n_obj) { return (n_obj + FIR_GROUP - 1) / FIR_GROUP; }

struct FirLaunch { dim3 grid, block; size_t lds; };
FirLaunch fir_launch(int strip, long long n_strips, int groups, int sets, int C, int Mp, int LP) {
    const int W = strip + Mp;
    return {dim3((unsigned)n_strips, (unsigned)groups, sets), dim3(64 * (strip / FIR_WAVE_SAMPLES)),
            (size_t)(W + (W >> 4) + 1 + C * LP) * sizeof(float)};
}

template <int C, class Args, class... A, class... V>
void launch_stage1(KernArgs<A...>, const FirLaunch &l, hipStream_t stream, V... v) {
    hipLaunchKernelGGL((scene_fir_stage1<C, Args, A...>), l.grid, l.block, l.lds, stream, (A)v...);
}

void launch_history(hipStream_t stream, const float *rows, int n_obj, long long n, const float *hist, float *hist_next, int H) {
    if (H > 0)
        hipLaunchKernelGGL(fir_history_kernel, dim3((unsigned)((H + 255) / 256), n_obj < 65535 ? n_obj : 65535), dim3(256), 0, stream, rows, n_obj, n,
                           hist, hist_next, H);
}

// A step without scheduled sets; delay: behind the delay stage (hist is then z's history).
int launch_fir_step(bool delay, const float *rows, int n_obj, long long n, const float *hist, float *hist_next, int H, const float *hist_x,
                    float *hist_x_next, int Hx, const SceneParam *params, int Rd, const float *P_to, const float *P_from, const int *onset_to,
                    const int *onset_from, int C, int K, long long n_fade, long long t0, long long t_set, int R, float *parts, float *out,
                    hipStream_t stream) {
    if (n_obj <= 0 || n <= 0 || C < 1 || C > SCENE_MAX_CHANNELS || K < 1 || K > SCENE_FIR_MAX_TAPS || H < 0 ||
        (delay && (Hx < 1 || Rd < 0 || !params || !hist_x || !hist_x_next)) || n_fade < 0 || n_fade > n ||
        (n_fade > 0 && (!P_from || !onset_from || R < 2)))
        return (int)hipErrorInvalidValue;
    const int groups = fir_groups(n_obj), sets = n_fade ? 2 : 1;
    const int LP = scene_fir_padded_taps(K), Mp = LP - 16;
    if (!P_to) {                                         // no filters set yet: silence, and the histories move on
        if (hipMemsetAsync(out, 0, (size_t)C * n * sizeof(float), stream) != hipSuccess) return (int)hipGetLastError();
    } else {
        if (!onset_to) return (int)hipErrorInvalidValue;
        const int strip = fir_strip(n, groups, sets);
        const long long strips = (n + strip - 1) / strip;
        if (strips > 0x7fffffffll) return (int)hipErrorInvalidValue;
        const FirLaunch l = fir_launch(strip, strips, groups, sets, C, Mp, LP);
        for_channel_count(C, [&](auto c) {
            if (delay)
                launch_stage1<decltype(c)::value, FirDelay>(FirDelay::Flat{}, l, stream, rows, n_obj, n, hist, H, hist_x, Hx, params, Rd, t0, P_to,
                                                            P_from, onset_to, onset_from, K, Mp, LP, parts, groups, n_fade);
            else
                launch_stage1<decltype(c)::value, FirPlain>(FirPlain::Flat{}, l, stream, rows, n_obj, n, hist, H, P_to, P_from, onset_to,
                                                            onset_from, K, Mp, LP, parts, groups, n_fade);
        });
        hipLaunchKernelGGL(scene_fir_stage2, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, stream, parts, C, groups, n, n_fade, t0, t_set, R, out);
    }
    if (!delay) {
        launch_history(stream, rows, n_obj, n, hist, hist_next, H);
    } else {
        if (H > 0)
            hipLaunchKernelGGL(fir_z_history_kernel<>, dim3((unsigned)((H + 255) / 256), n_obj < 65535 ? n_obj : 65535), dim3(256), 0, stream, rows,
                               n_obj, n, hist, hist_next, H, hist_x, Hx, params, Rd, t0);
        launch_history(stream, rows, n_obj, n, hist_x, hist_x_next, Hx);
    }
    return (int)hipGetLastError();
}
}  // namespace

int launch_scene_fir(const float *rows, int n_obj, long long n, const float *hist, float *hist_next, int H, const float *P_to,
                     const float *P_from, const int *onset_to, const int *onset_from, int C, int K, long long n_fade, long long t0,
                     long long t_set, int R, float *parts, float *out, hipStream_t stream) {
    return launch_fir_step(false, rows, n_obj, n, hist, hist_next, H, nullptr, nullptr, 0, nullptr, 0, P_to, P_from, onset_to, onset_from, C, K,
                           n_fade, t0, t_set, R, parts, out, stream);
}

int launch_scene_fir_delay(const float *rows, int n_obj, long long n, const float *hist_z, float *hist_z_next, int H, const float *hist_x,
                           float *hist_x_next, int Hx, const SceneParam *params, int Rd, const float *P_to, const float *P_from,
                           const int *onset_to, const int *onset_from, int C, int K, long long n_fade, long long t0, long long t_set, int R,
                           float *parts, float *out, hipStream_t stream) {
    return launch_fir_step(true, rows, n_obj, n, hist_z, hist_z_next, H, hist_x, hist_x_next, Hx, params, Rd, P_to, P_from, onset_to, onset_from,
                           C, K, n_fade, t0, t_set, R, parts, out, stream);
}

int scene_fir_sched_strip(long long n, int n_obj) { return fir_strip(n, fir_groups(n_obj), 1); }

int launch_scene_fir_sched(const FirSchedStep &a, hipStream_t stream) {
    const bool delay = a.params != nullptr;
    if (a.n_obj <= 0 || a.n <= 0 || a.C < 1 || a.C > SCENE_MAX_CHANNELS || a.K < 1 || a.K > SCENE_FIR_MAX_TAPS || a.H < 0 || a.S < 0 ||
        a.S > SCENE_FIR_MAX_SETS_PER_STEP || a.Kd < 0 || a.Kd > SCENE_MAX_SETS_PER_STEP || a.n_strips < 0 || (a.n_strips && !a.strips) ||
        (a.strip != FIR_WAVE_SAMPLES && a.strip != 4 * FIR_WAVE_SAMPLES) || (a.S && !a.t_f) || !a.pool || !a.onpool ||
        (delay && (a.Hx < 1 || a.Rd < 0 || !a.hist_x || !a.hist_x_next || !a.rec || (a.Kd && (!a.t_d || !a.targets)))) || (!delay && a.Kd))
        return (int)hipErrorInvalidValue;
    const int groups = fir_groups(a.n_obj);
    const int LP = scene_fir_padded_taps(a.K), Mp = LP - 16;
    if (delay) {
        // block 0 of the records is the record in force (a step without a delay set in it runs on that block alone)
        hipLaunchKernelGGL(fir_delay_expand_kernel, dim3((unsigned)((a.n_obj + 63) / 64)), dim3(64), 0, stream, a.params, a.rec, a.t_d, a.targets,
                           a.Kd, a.n_obj, a.Rd, a.any_set);
    }
    if (a.n_strips) {
        const FirLaunch l = fir_launch(a.strip, a.n_strips, groups, a.any_from ? 2 : 1, a.C, Mp, LP);
        const auto stage1 = [&](auto c, auto d) {
            using Args = FirSched<decltype(d)::value>;
            launch_stage1<decltype(c)::value, Args>(typename Args::Flat{}, l, stream, a.rows, a.n_obj, a.n, a.hist, a.H, a.hist_x, a.Hx, a.rec, a.t_d,
                                                    a.Kd, a.Rd, a.t0, a.strips, a.pool, a.onpool, a.K, Mp, LP, a.parts, groups);
        };
        for_channel_count(a.C, [&](auto c) {
            if (delay) stage1(c, std::true_type{});
            else stage1(c, std::false_type{});
        });
    }
    hipLaunchKernelGGL(scene_fir_sched_stage2, dim3((unsigned)((a.n + 255) / 256), a.C), dim3(256), 0, stream, a.parts, a.C, groups, a.n, a.t0,
                       a.R, a.t_f, a.S, a.have_to0, a.have_from0, a.t_set0, a.out);
    if (!delay) {
        launch_history(stream, a.rows, a.n_obj, a.n, a.hist, a.hist_next, a.H);
    } else {
        if (a.H > 0)
            hipLaunchKernelGGL((fir_z_history_kernel<const long long *__restrict__, int>), dim3((unsigned)((a.H + 255) / 256),
                               a.n_obj < 65535 ? a.n_obj : 65535), dim3(256), 0, stream, a.rows, a.n_obj, a.n, a.hist, a.hist_next, a.H, a.hist_x,
                               a.Hx, a.rec, a.t_d, a.Kd, a.Rd, a.t0);
        launch_history(stream, a.rows, a.n_obj, a.n, a.hist_x, a.hist_x_next, a.Hx);
    }
    return (int)hipGetLastError();
}

}  // namespace pbso
