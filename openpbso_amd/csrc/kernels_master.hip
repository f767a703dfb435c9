// The master bus (pbso_master; include/openpbso_amd.h "master bus"): a ramped gain, a linked look-ahead peak limiter, meters per
// buffer and 16-bit PCM, on a bus [C][n].  The limiter has no recursion: with v = gain * in and r(t) = min(1, T / max_c |v_c(t)|),
//
//   a(t) = min of r over t - (L + H) .. t                 (a sliding minimum)
//   g(t) = fminf(ONE f32 fmaf chain over w[k] a(t - k), k = L - 1 down to 0,  r(t - L))
//   y_c(t) = clamp(v_c(t - L) * g(t), -T, T)
//
// so every sample is a function of the 2 L + H samples before it and the kernels below are plain maps over
// E = history ++ step (index e = HL + q for the step's local sample q, HL = 2 L + H):
//
//   prepare   V[c][e], Rb[e]            v and r of history ++ step; the caller's input is read here and nowhere else (in-place calls)
//   minimum   M[e] = min Rb[e - 2^k + 1 .. e], 2^k <= L + H + 1 < 2^(k+1), by doubling: the first 10 levels in LDS, the rest
//             one pass over E each; a(e) = min(M[e], M[e - (L + H + 1 - 2^k)]) is formed where it is staged.  min is exact.
//   gain      G[q]: the window and a strip of a plus L - 1 halo in LDS, NS independent chains per lane
//   apply     out, and one meter record per (buffer, channel): one workgroup each
//   history   the last HL samples of V
// Built with -ffp-contract=off and without any fast-math or denormal flag; the f32 division is the correctly rounded one.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "openpbso_amd.h"

namespace pbso {

namespace {
constexpr int MS_STRIP = 1024;                           // samples of M a workgroup of the LDS minimum writes
constexpr int MS_LEVELS = 10;                            // doubling levels it can do: a halo of 2^10 - 1 in front of the strip
constexpr int GN_WIDE_NS = 4;                            // chains per lane of the wide gain launch (256 lanes: strips of 1024)
}  // namespace

__global__ __launch_bounds__(256) void master_prepare_kernel(const float *__restrict__ in, int C, long long n, const float *__restrict__ hist,
                                                             int HL, SceneParam gain, int R, long long t0, float T,
                                                             float *__restrict__ V, float *__restrict__ Rb) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, N = HL + n;
    if (e >= N) return;
    float pk = 0.f;
    if (e < HL) {
        for (int c = 0; c < C; ++c) {
            const float v = hist[(long long)c * HL + e];
            V[c * N + e] = v;
            pk = fmaxf(pk, fabsf(v));
        }
    } else {
        const long long q = e - HL;
        const float p = (float)ramp_value(gain, t0 + q, R);
        for (int c = 0; c < C; ++c) {
            const float v = p * in[c * n + q];
            V[c * N + e] = v;
            pk = fmaxf(pk, fabsf(v));
        }
    }
    Rb[e] = pk > T ? T / pk : 1.f;
}

// M[e] = min Rb[e - 2^K + 1 .. e] (1.f in front of E), K <= MS_LEVELS: K rounds of m(i) = min(m(i), m(i - 2^j)) on a strip in LDS
__global__ __launch_bounds__(256) void master_min_lds_kernel(const float *__restrict__ Rb, long long N, int K, float *__restrict__ M) {
    __shared__ float s[2 * MS_STRIP];
    const int halo = (1 << K) - 1, tot = MS_STRIP + halo;
    const long long e0 = (long long)blockIdx.x * MS_STRIP;
    for (int i = threadIdx.x; i < tot; i += 256) {
        const long long e = e0 - halo + i;
        s[i] = e >= 0 && e < N ? Rb[e] : 1.f;
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        const int d = 1 << j;
        float x[2 * MS_STRIP / 256];
#pragma unroll
        for (int u = 0; u < 2 * MS_STRIP / 256; ++u) {
            const int i = threadIdx.x + 256 * u;
            x[u] = i < tot ? fminf(s[i], i >= d ? s[i - d] : 1.f) : 1.f;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2 * MS_STRIP / 256; ++u) {
            const int i = threadIdx.x + 256 * u;
            if (i < tot) s[i] = x[u];
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < MS_STRIP; i += 256)
        if (e0 + i < N) M[e0 + i] = s[halo + i];
}

// one more level over all of E: Mo[e] = min(Mi[e], Mi[e - d])
__global__ __launch_bounds__(256) void master_min_pass_kernel(const float *__restrict__ Mi, long long N, long long d, float *__restrict__ Mo) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    Mo[e] = fminf(Mi[e], e >= d ? Mi[e - d] : 1.f);
}

// One workgroup per strip of TPB NS samples.  LDS: w [L] | a [strip + L - 1], a(i) the sliding minimum at local sample
// q0 - (L - 1) + i.  Lane l carries the chains of samples q0 + l + u TPB: at one k the lanes of a wave read 64 consecutive words
// of a and one word of w.  (e - D >= 0: e >= HL - (L - 1) = L + H + 1 > D.)
template <int NS, int TPB>
__global__ __launch_bounds__(TPB) void master_gain_kernel(const float *__restrict__ M, const float *__restrict__ Rb, const float *__restrict__ win,
                                                          long long n, int HL, int L, int D, float *__restrict__ G) {
    extern __shared__ float lds[];
    constexpr int strip = NS * TPB;
    float *w = lds, *a = lds + L;
    const long long q0 = (long long)blockIdx.x * strip;
    for (int k = threadIdx.x; k < L; k += TPB) w[k] = win[k];
    for (int i = threadIdx.x; i < strip + L - 1; i += TPB) {
        const long long q = q0 - (L - 1) + i, e = HL + q;
        a[i] = q < n ? fminf(M[e], M[e - D]) : 1.f;
    }
    __syncthreads();
    float acc[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) acc[u] = 0.f;
    const float *al = a + (L - 1) + threadIdx.x;
    for (int k = L - 1; k >= 0; --k) {
        const float wk = w[k];
#pragma unroll
        for (int u = 0; u < NS; ++u) acc[u] = fmaf(wk, al[u * TPB - k], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const long long q = q0 + threadIdx.x + u * TPB;
        if (q < n) G[q] = fminf(acc[u], Rb[HL + q - L]);
    }
}

// One workgroup per (buffer b of B samples, channel c): y = clamp(v(t - L) g(t)) and the buffer's meter record.
__global__ __launch_bounds__(256) void master_apply_kernel(const float *__restrict__ V, const float *__restrict__ G, long long n, int HL, int L,
                                                           int B, float T, float *__restrict__ out, pbso_master_meter *__restrict__ meters) {
    __shared__ float s_in[4], s_out[4], s_g[4];
    __shared__ int s_n[4];
    __shared__ double s_sq[4];
    const int b = blockIdx.x, c = blockIdx.y, C = gridDim.y;
    const long long N = HL + n;
    const float *__restrict__ v = V + (long long)c * N + HL;
    float in_peak = 0.f, out_peak = 0.f, min_gain = 1.f;
    int n_lim = 0;
    double sq = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const long long q = (long long)b * B + i;
        const float g = G[q];
        const float y = fminf(fmaxf(v[q - L] * g, -T), T);
        out[(long long)c * n + q] = y;
        in_peak = fmaxf(in_peak, fabsf(v[q]));
        out_peak = fmaxf(out_peak, fabsf(y));
        min_gain = fminf(min_gain, g);
        n_lim += g < 1.f ? 1 : 0;
        sq += (double)y * (double)y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        in_peak = fmaxf(in_peak, __shfl_xor(in_peak, o, 64));
        out_peak = fmaxf(out_peak, __shfl_xor(out_peak, o, 64));
        min_gain = fminf(min_gain, __shfl_xor(min_gain, o, 64));
        n_lim += __shfl_xor(n_lim, o, 64);
        sq += __shfl_xor(sq, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_in[wave] = in_peak;
        s_out[wave] = out_peak;
        s_g[wave] = min_gain;
        s_n[wave] = n_lim;
        s_sq[wave] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pbso_master_meter m;
        m.in_peak = fmaxf(fmaxf(s_in[0], s_in[1]), fmaxf(s_in[2], s_in[3]));
        m.out_peak = fmaxf(fmaxf(s_out[0], s_out[1]), fmaxf(s_out[2], s_out[3]));
        m.min_gain = fminf(fminf(s_g[0], s_g[1]), fminf(s_g[2], s_g[3]));
        m.n_limited = s_n[0] + s_n[1] + s_n[2] + s_n[3];
        m.sumsq = (s_sq[0] + s_sq[1]) + (s_sq[2] + s_sq[3]);
        meters[(long long)b * C + c] = m;
    }
}

// hist_next[c] = the last HL samples of V[c]
__global__ __launch_bounds__(256) void master_history_kernel(const float *__restrict__ V, long long n, int HL, float *__restrict__ hist_next) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= HL) return;
    const long long c = blockIdx.y;
    hist_next[c * HL + k] = V[c * (HL + n) + n + k];
}

// pcm[s][c] = (int16_t)lrintf(y[c][s] * 32767.f): one rounded multiplication, then to the nearest integer, ties to even
__global__ __launch_bounds__(256) void master_pcm16_kernel(const float *__restrict__ y, int C, long long n, short *__restrict__ pcm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * C) return;
    const long long s = i / C;
    const int c = (int)(i - s * C);
    const float x = y[(long long)c * n + s] * 32767.f;
    pcm[i] = (short)__float2int_rn(x);
}

int launch_master(const float *in, int C, long long n, int B, const float *hist, float *hist_next, int L, int H, float T, SceneParam gain,
                  int R, long long t0, const float *win, float *V, float *Rb, float *M0, float *M1, float *G, float *out, void *meters,
                  hipStream_t stream) {
    if (!in || !out || !meters || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0 || B <= 0 || n % B != 0 || L < 1 || L > MASTER_MAX_LOOKAHEAD ||
        H < 0 || H > MASTER_MAX_HOLD || !(T > 0.f && T <= 1.f))
        return (int)hipErrorInvalidValue;
    const int HL = 2 * L + H, W = L + H + 1;
    const long long N = HL + n;
    if ((N + 255) / 256 > 0x7fffffffll || n / B > 0x7fffffffll) return (int)hipErrorInvalidValue;
    const unsigned gridN = (unsigned)((N + 255) / 256);
    hipLaunchKernelGGL(master_prepare_kernel, dim3(gridN), dim3(256), 0, stream, in, C, n, hist, HL, gain, R, t0, T, V, Rb);
    int k = 0;
    while ((2 << k) <= W) ++k;                           // 2^k <= W < 2^(k+1)
    const int K = k < MS_LEVELS ? k : MS_LEVELS;
    hipLaunchKernelGGL(master_min_lds_kernel, dim3((unsigned)((N + MS_STRIP - 1) / MS_STRIP)), dim3(256), 0, stream, Rb, N, K, M0);
    float *m = M0, *other = M1;
    for (int j = K; j < k; ++j) {
        hipLaunchKernelGGL(master_min_pass_kernel, dim3(gridN), dim3(256), 0, stream, m, N, 1ll << j, other);
        float *t = m;
        m = other;
        other = t;
    }
    const int D = W - (1 << k);
    // strips of 1024 with four chains per lane once that gives 16 workgroups; else one wave of one chain per 64 samples: a
    // one-buffer step has nothing but its 513 samples to spread over the chip
    if (n >= 16 * GN_WIDE_NS * 256) {
        const size_t lds = (size_t)(L + GN_WIDE_NS * 256 + L - 1) * sizeof(float);
        hipLaunchKernelGGL((master_gain_kernel<GN_WIDE_NS, 256>), dim3((unsigned)((n + GN_WIDE_NS * 256 - 1) / (GN_WIDE_NS * 256))), dim3(256), lds,
                           stream, m, Rb, win, n, HL, L, D, G);
    } else {
        const size_t lds = (size_t)(L + 64 + L - 1) * sizeof(float);
        hipLaunchKernelGGL((master_gain_kernel<1, 64>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, stream, m, Rb, win, n, HL, L, D, G);
    }
    hipLaunchKernelGGL(master_apply_kernel, dim3((unsigned)(n / B), C), dim3(256), 0, stream, V, G, n, HL, L, B, T, out,
                       (pbso_master_meter *)meters);
    hipLaunchKernelGGL(master_history_kernel, dim3((unsigned)((HL + 255) / 256), C), dim3(256), 0, stream, V, n, HL, hist_next);
    return (int)hipGetLastError();
}

int launch_master_pcm16(const float *y, int C, long long n, short *pcm, hipStream_t stream) {
    if (!y || !pcm || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(master_pcm16_kernel, dim3((unsigned)((n * C + 255) / 256)), dim3(256), 0, stream, y, C, n, pcm);
    return (int)hipGetLastError();
}

}  // namespace pbso
