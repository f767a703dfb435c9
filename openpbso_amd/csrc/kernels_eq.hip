// The EQ bus (pbso_eq; include/openpbso_amd.h "EQ bus"): S biquad sections in cascade per channel of a bus [C][n], in block form
// and in fp64.  A cascade's time axis is cut into blocks of P = PBSO_EQ_BLOCK samples from its t_set on; inside a block every
// output is one fp64 fma chain over the block's inputs (table h), the two inputs before the block (r, s) and the two outputs before
// the block (q, p), so that the only serial dependence is the last two outputs of a block on the last two of the block before.
//
// All signals of a call live in "extended" rows of EQ_HIST + n doubles: the EQ_HIST = P + 2 samples before the step (the history)
// in front of the step's n.  Index EQ_HIST + i is sample t + i; the step's first block has its origin at index EQ_HIST - k0, where
// k0 = (t - t_set) mod P, so a block begun in the step before is finished from the same origin.  Per section, three kernels:
//
//   forward   one thread per sample, workgroups aligned to the block grid (256 positions = 256 / P blocks): the inputs they read,
//             256 + 2 doubles, staged in LDS; the chain over h, then r, then s; the partial sums go to W.  Lanes of a wave read
//             consecutive doubles of LDS and one table word per step, which is the same for all of them.
//   chain     one wave per channel: the last two outputs of every block from the last two of the block before, two dependent fma
//             each.  The partial sums of 64 blocks at a time are fetched by the 64 lanes and walked from LDS by all of them alike;
//             lane g keeps block g's pair and stores it.
//   finish    one thread per sample again: q and p on the other P - 2 samples of every block.
//
// Every kernel that completes samples of a signal also writes those among them that belong to the next history.  The input kernel
// makes signal 0 = (double)in; the output kernel rounds signal S to f32 once and blends the two cascades of a cross-fade in three
// separately rounded f32 operations.  Built with -ffp-contract=off and without any fast-math or denormal flag.
#include <hip/hip_runtime.h>

#include "eq_block.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int P = EQ_BLOCK, H = EQ_HIST;
constexpr int EQ_TPB = 256;                              // positions of a workgroup: whole blocks
static_assert(EQ_TPB % P == 0 && P >= 2 && P <= 64, "a workgroup holds whole blocks, the chain kernel's wave one table row");
}  // namespace

// x [C][H + n] = hist ++ (double)in, in's rows in_stride apart; hist_next = its last H samples.  hist rows are hist_stride apart
// (signal 0 of every channel).
__global__ __launch_bounds__(256) void eq_input_kernel(const float *__restrict__ in, long long in_stride, long long n, const double *__restrict__ hist,
                                                       double *__restrict__ hist_next, long long hist_stride, double *__restrict__ x) {
    const int c = blockIdx.y;
    const long long N = H + n, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double v = i < H ? hist[c * hist_stride + i] : (double)in[c * in_stride + (i - H)];
    x[c * N + i] = v;
    if (i >= n) hist_next[c * hist_stride + (i - n)] = v;
}

__global__ __launch_bounds__(EQ_TPB) void eq_forward_kernel(const double *__restrict__ x, double *__restrict__ W, double *__restrict__ y,
                                                            const double *__restrict__ hist_y, long long hist_stride,
                                                            const double *__restrict__ tab, long long tab_stride, long long n, int k0) {
    __shared__ double win[EQ_TPB + 2];
    const int c = blockIdx.y;
    const long long N = H + n;
    const double *__restrict__ xc = x + c * N;
    const long long first = (long long)(H - k0) + (long long)blockIdx.x * EQ_TPB;      // of the workgroup's first position; >= 3
    for (int l = threadIdx.x; l < EQ_TPB + 2; l += EQ_TPB) {
        const long long i = first - 2 + l;
        win[l] = i < N ? xc[i] : 0.0;
    }
    // the output signal's history in front of its row, for the chain and the finish
    if (blockIdx.x == 0 && threadIdx.x < H) y[c * N + threadIdx.x] = hist_y[c * hist_stride + threadIdx.x];
    __syncthreads();
    const int k = threadIdx.x % P, base = 2 + (threadIdx.x / P) * P;
    const double *__restrict__ t = tab + c * tab_stride;
    double acc = 0.0;
    for (int j = P - 1; j >= 0; --j) {
        const int d = k - j;
        const double v = win[base + (d < 0 ? 0 : d)];
        const double a = fma(t[j], v, acc);
        acc = d < 0 ? acc : a;
    }
    acc = fma(t[P + k], win[base - 1], acc);
    acc = fma(t[2 * P + k], win[base - 2], acc);
    const long long i = first + threadIdx.x;
    if (i >= H && i < N) W[c * N + i] = acc;
}

__global__ __launch_bounds__(64) void eq_chain_kernel(const double *__restrict__ W, double *__restrict__ y, double *__restrict__ hist_next_y,
                                                      long long hist_stride, const double *__restrict__ tab, long long tab_stride, long long n,
                                                      int k0) {
    __shared__ double sa[64], sb[64];
    const int c = blockIdx.x, lane = threadIdx.x;
    const long long N = H + n;
    const double *__restrict__ Wc = W + c * N;
    double *yc = y + c * N, *hn = hist_next_y + c * hist_stride;
    const double *__restrict__ t = tab + c * tab_stride;
    const double pa = t[3 * P + P - 2], pb = t[3 * P + P - 1], qa = t[4 * P + P - 2], qb = t[4 * P + P - 1];
    auto store = [&](long long i, double v) {
        yc[i] = v;
        if (i >= n) hn[i - n] = v;
    };
    // a step shorter than the history: the old samples that stay in it
    for (long long i = n + lane; i < H; i += 64) hn[i - n] = yc[i];
    const long long o0 = H - k0;                         // the origin of the step's first block
    double y2 = yc[o0 - 2], y1 = yc[o0 - 1];
    {
        const long long ia = o0 + P - 2, ib = ia + 1;    // (ib >= H always: o0 >= 3)
        double a;
        if (ia < H) a = yc[ia];                          // made by the step before
        else if (ia < N) {
            a = fma(pa, y1, fma(qa, y2, Wc[ia]));
            if (lane == 0) store(ia, a);
        } else return;
        if (ib >= N) return;
        const double b = fma(pb, y1, fma(qb, y2, Wc[ib]));
        if (lane == 0) store(ib, b);
        y2 = a;
        y1 = b;
    }
    const long long G = (N - o0 - P) / P;                // whole blocks behind the first
    for (long long g0 = 0; g0 < G; g0 += 64) {
        const long long g = g0 + lane, o = o0 + (g + 1) * P;
        double wa = 0.0, wb = 0.0;
        if (g < G) {
            wa = Wc[o + P - 2];
            wb = Wc[o + P - 1];
        }
        __syncthreads();
        sa[lane] = wa;
        sb[lane] = wb;
        __syncthreads();
        const int cnt = (int)(G - g0 < 64 ? G - g0 : 64);
        double ra = 0.0, rb = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const double na = fma(pa, y1, fma(qa, y2, sa[i]));
            const double nb = fma(pb, y1, fma(qb, y2, sb[i]));
            y2 = na;
            y1 = nb;
            if (i == lane) {
                ra = na;
                rb = nb;
            }
        }
        if (g < G) {
            store(o + P - 2, ra);
            store(o + P - 1, rb);
        }
    }
    const long long ia = o0 + (G + 1) * P + P - 2;       // a last block that ends behind the step may still have its sample P - 2 in it
    if (ia < N && lane == 0) store(ia, fma(pa, y1, fma(qa, y2, Wc[ia])));
}

__global__ __launch_bounds__(EQ_TPB) void eq_finish_kernel(const double *__restrict__ W, double *y, double *__restrict__ hist_next_y,
                                                           long long hist_stride, const double *__restrict__ tab, long long tab_stride,
                                                           long long n, int k0) {
    const int c = blockIdx.y;
    const long long N = H + n;
    const long long i = (long long)(H - k0) + (long long)blockIdx.x * EQ_TPB + threadIdx.x;
    const int k = threadIdx.x % P;
    if (i < H || i >= N || k >= P - 2) return;           // (samples P - 2 and P - 1 are the chain's)
    double *yc = y + c * N;
    const double *__restrict__ t = tab + c * tab_stride;
    const long long o = i - k;
    const double v = fma(t[3 * P + k], yc[o - 1], fma(t[4 * P + k], yc[o - 2], W[c * N + i]));
    yc[i] = v;
    if (i >= n) hist_next_y[c * hist_stride + (i - n)] = v;
}

// out[c][i] = (float)to[c][H + i]; for i < n_fade: yf + w (yt - yf) with yf = (float)from[c][H + i], w = (float)((double)(d0 + i) / (double)R)
__global__ __launch_bounds__(256) void eq_output_kernel(const double *__restrict__ to, const double *__restrict__ from, long long n,
                                                        long long n_fade, long long d0, int R, float *__restrict__ out) {
    const int c = blockIdx.y;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = (float)to[c * (H + n) + H + i];
    if (i < n_fade) {
        const float yf = (float)from[c * (H + n_fade) + H + i];
        const float w = (float)((double)(d0 + i) / (double)R);
        const float d = v - yf;
        const float wd = w * d;
        v = yf + wd;
    }
    out[c * n + i] = v;
}

size_t eq_work_doubles(int C, long long n) { return (size_t)3 * C * (size_t)(H + n); }

int launch_eq_cascade(const float *in, long long in_stride, int C, int S, long long n, int k0, const double *hist, double *hist_next, const double *tab,
                      double *work, const double **result, hipStream_t stream) {
    if (!in || !hist || !hist_next || !tab || !work || !result || C < 1 || C > SCENE_MAX_CHANNELS || S < 1 || S > EQ_MAX_SECTIONS || n <= 0 || in_stride < n ||
        k0 < 0 || k0 >= P)
        return (int)hipErrorInvalidValue;
    const long long N = H + n, hist_stride = (long long)(S + 1) * H, tab_stride = (long long)S * EQ_TABLES * P;
    if ((N + 255) / 256 > 0x7fffffffll) return (int)hipErrorInvalidValue;
    double *ext[2] = {work, work + (size_t)C * N}, *W = work + (size_t)2 * C * N;
    hipLaunchKernelGGL(eq_input_kernel, dim3((unsigned)((N + 255) / 256), C), dim3(256), 0, stream, in, in_stride, n, hist, hist_next, hist_stride, ext[0]);
    const dim3 grid((unsigned)((k0 + n + EQ_TPB - 1) / EQ_TPB), C);
    for (int s = 0; s < S; ++s) {
        const double *x = ext[s & 1], *ts = tab + (size_t)s * EQ_TABLES * P;
        double *y = ext[(s + 1) & 1], *hn = hist_next + (size_t)(s + 1) * H;
        hipLaunchKernelGGL(eq_forward_kernel, grid, dim3(EQ_TPB), 0, stream, x, W, y, hist + (size_t)(s + 1) * H, hist_stride, ts, tab_stride, n, k0);
        hipLaunchKernelGGL(eq_chain_kernel, dim3(C), dim3(64), 0, stream, (const double *)W, y, hn, hist_stride, ts, tab_stride, n, k0);
        hipLaunchKernelGGL(eq_finish_kernel, grid, dim3(EQ_TPB), 0, stream, (const double *)W, y, hn, hist_stride, ts, tab_stride, n, k0);
    }
    *result = ext[S & 1];
    return (int)hipGetLastError();
}

int launch_eq_output(const double *to, const double *from, int C, long long n, long long n_fade, long long d0, int R, float *out,
                     hipStream_t stream) {
    if (!to || !out || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0 || n_fade < 0 || n_fade > n || (n_fade && (!from || R < 2 || d0 < 1)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(eq_output_kernel, dim3((unsigned)((n + 255) / 256), C), dim3(256), 0, stream, to, from, n, n_fade, d0, R, out);
    return (int)hipGetLastError();
}

}  // namespace pbso
