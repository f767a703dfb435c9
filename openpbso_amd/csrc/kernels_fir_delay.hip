// The scene filter mix behind a ramped fractional delay per object (pbso_scene_fir_delay_enable; include/openpbso_amd.h "scene
// filter mix"):
//
//   y_c(t) = sum_o sum_{k < K} h_co[k] * z_o(t - D_o - k),   z_o(tau) = x_o read at tau - d_o(tau), the scene mix's read
//
// scene_fir_delay_stage1<C> is scene_fir_stage1<C> of kernels_fir.hip with ONE piece replaced: what is staged into the window.
// A window position that lies in the step is z, computed on the way into LDS from the x history ++ the step's row (two loads,
// three rounded f32 operations); one before the step is read from the z history, where the step that contained it left it
// under the record in force then.  z rows are never written to memory.  The walk over the window, the chain on
// v_mfma_f32_16x16x4_f32, the write-out, the second stage and the launch shape are the text of kernels_fir.hip (which says why
// the text is not shared: an edit there wants the same edit here).  The kernels of kernels_fir.hip are not touched: a mixer
// without the delay stage is launched as before.
// Built with -ffp-contract=off: the read and a fade's blend are separately rounded operations, and the steady path (the delay
// split once per object) and the per-sample path must round alike.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int FIR_GROUP = 32;                            // the four constants of kernels_fir.hip
constexpr int FIR_WAVE_TILES = 2;
constexpr int FIR_WAVE_SAMPLES = 256 * FIR_WAVE_TILES;
constexpr int FIR_STAGE_BATCH = 8;

// The scene mix's read (kernels_mix.hip has the same three functions; that file is left as it is).
// the read position t - d as i0 + f with i0 = t - off: a fraction of exactly 0 reads x(i0) itself
__device__ __forceinline__ void delay_split(double d, long long *off, float *f) {
    const double fl = floor(d), fr = d - fl;             // (exact)
    *off = (long long)fl + (fr != 0.0 ? 1 : 0);
    *f = fr != 0.0 ? (float)(1.0 - fr) : 0.f;
}
// where x_o at the step's local sample j lies: the step's row for j >= 0, the x history before it for -Hx <= j < 0.  Every read
// lies there (0 <= d <= max_delay = Hx - 1, and x(i0 + 1) is read at i0 + 1 <= t); the clamp keeps the address in the buffers
// whatever the arguments, so that a load can be issued before it is known whether its value is used.
__device__ __forceinline__ const float *x_at(const float *__restrict__ row, const float *__restrict__ xrow, long long n, int Hx, long long j) {
    j = j < -(long long)Hx ? -(long long)Hx : (j >= n ? n - 1 : j);
    return j >= 0 ? row + j : xrow + (Hx + j);
}
__device__ __forceinline__ float interp(float x0, float x1, float f) { return f == 0.f ? x0 : x0 + f * (x1 - x0); }
}  // namespace

// scene_fir_stage1<C> (kernels_fir.hip) with the window staged from hist_z | z(hist_x ++ rows) | 0.  params [n_obj]: the delay
// records; Rd: their ramp; t0: the step's first absolute sample.
template <int C>
__global__ __launch_bounds__(256) void scene_fir_delay_stage1(const float *__restrict__ rows, int n_obj, long long n,
                                                              const float *__restrict__ hist_z, int H, const float *__restrict__ hist_x,
                                                              int Hx, const SceneParam *__restrict__ params, int Rd, long long t0,
                                                              const float *__restrict__ P0, const float *__restrict__ P1,
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
        const float *row = rows + (long long)o * n, *hrow = hist_z + (long long)o * H, *xrow = hist_x + (long long)o * Hx;
        long long shift = s0 - (K - 1) - onset[o];
        SceneParam q = params[o];
        // steady: the object's ramp is over at the first sample of the window that lies in the step, hence at all of them, or
        // the record does not move at all (from == to and slope 0: a first set, the records a reset settled, the zeros before
        // any set) -- what ramp_value returns there is `to` (from + 0 * k == from), split once (a uniform decision: one
        // branch per object, none per position)
        const bool steady = Rd == 0 || t0 + (shift > 0 ? shift : 0) - q.t_set + 1 >= Rd || (q.slope == 0.0 && q.from == q.to);
        long long off_s = 0;
        float f_s = 0.f;
        if (steady) delay_split(q.to, &off_s, &f_s);
        // (what only the staging reads goes to vector registers from here on.  Left to itself the compiler (AMD clang 22, ROCm 7.2)
        //  keeps every uniform value in a scalar register; the walk below already needs 96-98 of the 102, and these values
        //  were then spilled to spare vector lanes across it.  An empty asm with a "v" constraint is the only way to say "this
        //  uniform value lives in a VGPR"; tests/test_scene_fir_delay_asm_guards.py (no SGPR spills) tells when a compiler no
        //  longer needs it, or needs more.)
        asm volatile("" : "+v"(row), "+v"(hrow), "+v"(xrow), "+v"(shift), "+v"(q.from), "+v"(q.slope));
        __syncthreads();                                 // (the previous object's operands are read)
        // (FIR_STAGE_BATCH positions per thread, two loads each in flight before the first LDS write)
        for (int i0 = threadIdx.x; i0 < W; i0 += FIR_STAGE_BATCH * blockDim.x) {
            float v[FIR_STAGE_BATCH], x1[FIR_STAGE_BATCH], f[FIR_STAGE_BATCH];
            unsigned live = 0;                           // bit u: position u of the batch stages a value (kept in a register, not in masks)
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                const long long j = shift + i;           // the step's local sample tau - t0; -H <= j by 0 <= onset <= max_onset
                // every position loads from an address inside the buffers and selects afterwards (no branch per position):
                // in the step the two samples of the read, before it the z history twice with a fraction of 0 (which stages the
                // value itself), and 0 past the step's end and past the window's
                long long off = off_s;
                f[u] = f_s;
                if (!steady) delay_split(ramp_value(q, t0 + j, Rd), &off, &f[u]);
                const float *p0 = x_at(row, xrow, n, Hx, j - off), *p1 = x_at(row, xrow, n, Hx, j - off + 1);
                if (j < 0) {
                    p0 = p1 = hrow + (j >= -(long long)H ? H + j : 0);
                    f[u] = 0.f;
                }
                v[u] = *p0;
                x1[u] = *p1;                             // (unused when the fraction is 0)
                live |= (i < W && j < n && j >= -(long long)H ? 1u : 0u) << u;
            }
#pragma unroll
            for (int u = 0; u < FIR_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                if (i < W) win[win_at(i)] = (live >> u & 1u) ? interp(v[u], x1[u], f[u]) : 0.f;
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

// the same second stage as the undelayed mix's (conv_mfma.h), under a name of this file
__global__ __launch_bounds__(256) void scene_fir_delay_stage2(const float *__restrict__ parts, int C, int n_groups, long long n,
                                                              long long n_fade, long long t0, long long t_set, int R, float *__restrict__ out) {
    conv_stage2(parts, C, n_groups, n, n_fade, t0, t_set, R, nullptr, out);
}

// hist_z_next[o] = the last H samples of hist_z[o] ++ z_o(step), z computed again (a pure function of hist_x ++ rows, the record
// and the absolute sample: the bits are those the windows staged), o striding over blockIdx.y
__global__ __launch_bounds__(256) void fir_delay_z_history_kernel(const float *__restrict__ rows, int n_obj, long long n,
                                                                  const float *__restrict__ hist_z, float *__restrict__ hist_z_next, int H,
                                                                  const float *__restrict__ hist_x, int Hx,
                                                                  const SceneParam *__restrict__ params, int Rd, long long t0) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= H) return;
    const long long j = n + k - H;                       // the step's local sample; negative: still in hist_z
    for (long long o = blockIdx.y; o < n_obj; o += gridDim.y) {
        float z;
        if (j < 0) z = hist_z[o * H + (n + k)];
        else {
            const float *__restrict__ row = rows + o * n, *__restrict__ xrow = hist_x + o * Hx;
            long long off;
            float f;
            delay_split(ramp_value(params[o], t0 + j, Rd), &off, &f);
            z = interp(*x_at(row, xrow, n, Hx, j - off), *x_at(row, xrow, n, Hx, j - off + 1), f);
        }
        hist_z_next[o * H + k] = z;
    }
}

PBSO_DEFINE_HISTORY_KERNEL(fir_delay_x_history_kernel)

template <int C>
static void launch_fir_delay_stage1(dim3 grid, int waves, size_t lds, hipStream_t stream, const float *rows, int n_obj, long long n,
                                    const float *hist_z, int H, const float *hist_x, int Hx, const SceneParam *params, int Rd, long long t0,
                                    const float *P0, const float *P1, const int *on0, const int *on1, int K, int Mp, int LP, float *parts,
                                    int groups, long long n_second) {
    hipLaunchKernelGGL(scene_fir_delay_stage1<C>, grid, dim3(64 * waves), lds, stream, rows, n_obj, n, hist_z, H, hist_x, Hx, params, Rd, t0,
                       P0, P1, on0, on1, K, Mp, LP, parts, groups, n_second);
}

int launch_scene_fir_delay(const float *rows, int n_obj, long long n, const float *hist_z, float *hist_z_next, int H, const float *hist_x,
                           float *hist_x_next, int Hx, const SceneParam *params, int Rd, const float *P_to, const float *P_from,
                           const int *onset_to, const int *onset_from, int C, int K, long long n_fade, long long t0, long long t_set, int R,
                           float *parts, float *out, hipStream_t stream) {
    if (n_obj <= 0 || n <= 0 || C < 1 || C > SCENE_MAX_CHANNELS || K < 1 || K > SCENE_FIR_MAX_TAPS || H < 0 || Hx < 1 || Rd < 0 || !params ||
        !hist_x || !hist_x_next || n_fade < 0 || n_fade > n || (n_fade > 0 && (!P_from || !onset_from || R < 2)))
        return (int)hipErrorInvalidValue;
    const int groups = (n_obj + FIR_GROUP - 1) / FIR_GROUP;
    const int LP = scene_fir_padded_taps(K), Mp = LP - 16;
    const unsigned gy = n_obj < 65535 ? n_obj : 65535;
    if (!P_to) {                                         // no filters set yet: silence, and both histories move on
        if (hipMemsetAsync(out, 0, (size_t)C * n * sizeof(float), stream) != hipSuccess) return (int)hipGetLastError();
    } else {
        if (!onset_to) return (int)hipErrorInvalidValue;
        // the launch shape of launch_scene_fir: four waves per workgroup once that still gives every CU two workgroups
        int waves = 4;
        if (((n + 4 * FIR_WAVE_SAMPLES - 1) / (4 * FIR_WAVE_SAMPLES)) * groups * (n_fade ? 2 : 1) < 512) waves = 1;
        const int strip = waves * FIR_WAVE_SAMPLES, W = strip + Mp;
        const long long strips = (n + strip - 1) / strip;
        if (strips > 0x7fffffffll) return (int)hipErrorInvalidValue;
        const size_t lds = (size_t)(W + (W >> 4) + 1 + C * LP) * sizeof(float);
        const dim3 grid((unsigned)strips, (unsigned)groups, n_fade ? 2 : 1);
#define PBSO_FIR_DELAY_CASE(c) \
    case c: launch_fir_delay_stage1<c>(grid, waves, lds, stream, rows, n_obj, n, hist_z, H, hist_x, Hx, params, Rd, t0, P_to, P_from, onset_to, \
                                       onset_from, K, Mp, LP, parts, groups, n_fade); break;
        switch (C) {
            PBSO_FIR_DELAY_CASE(1) PBSO_FIR_DELAY_CASE(2) PBSO_FIR_DELAY_CASE(3) PBSO_FIR_DELAY_CASE(4) PBSO_FIR_DELAY_CASE(5)
            PBSO_FIR_DELAY_CASE(6) PBSO_FIR_DELAY_CASE(7)
        default: launch_fir_delay_stage1<8>(grid, waves, lds, stream, rows, n_obj, n, hist_z, H, hist_x, Hx, params, Rd, t0, P_to, P_from, onset_to,
                                            onset_from, K, Mp, LP, parts, groups, n_fade); break;
        }
#undef PBSO_FIR_DELAY_CASE
        hipLaunchKernelGGL(scene_fir_delay_stage2, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, stream, parts, C, groups, n, n_fade, t0,
                           t_set, R, out);
    }
    if (H > 0)
        hipLaunchKernelGGL(fir_delay_z_history_kernel, dim3((unsigned)((H + 255) / 256), gy), dim3(256), 0, stream, rows, n_obj, n, hist_z,
                           hist_z_next, H, hist_x, Hx, params, Rd, t0);
    hipLaunchKernelGGL(fir_delay_x_history_kernel, dim3((unsigned)((Hx + 255) / 256), gy), dim3(256), 0, stream, rows, n_obj, n, hist_x,
                       hist_x_next, Hx);
    return (int)hipGetLastError();
}

}  // namespace pbso
