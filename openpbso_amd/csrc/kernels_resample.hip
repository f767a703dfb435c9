// The resampler bus (pbso_resample; include/openpbso_amd.h "resampler bus"): a rational polyphase sample-rate converter L / M on a
// bus [C][n].  Output j of a call has position p = p0 + j M in units of 1 / L input samples from the call's first input sample:
// it reads at local input sample r = p div L with the tap row of phase phi = p mod L,
//
//   acc = 0.f; for k = T - 1 down to 0: acc = fmaf(h[phi][k], E[r + T - 1 - k], acc)        E = history (T - 1 samples) ++ input
//
// so every output is a function of T samples of E and the kernels below are plain maps:
//
//   convert   one workgroup per 256 consecutive outputs of one channel (blockIdx.y): the samples of E they read, at most
//             255 M / L + 1 + T, staged in LDS; every thread runs its own chain over its own tap row (neighbouring threads have
//             different phases), T contiguous floats of the table read with 16-byte loads where T is a multiple of four.  A ratio
//             whose window does not fit in LDS (M / L large) reads E from memory instead.  The table is not staged: a workgroup
//             reads 256 T taps of it once each, which is no more than staging a table of L T >= 256 T words would cost, and at
//             most 1 MB of it stays in L2.
//             The call's meters (max |y| and the count of |y| > 1.f per channel) are reduced per workgroup and merged with integer
//             atomics: the maximum of non-negative floats is the maximum of their bit patterns, so both are exact in any order.
//   history   the last T - 1 samples of E
//   pcm16     interleaved 16-bit PCM of an output
// Built with -ffp-contract=off and without any fast-math or denormal flag: subnormals are kept.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "kernels.h"
#include "openpbso_amd.h"

namespace pbso {

namespace {
constexpr int RS_TPB = 256;                              // outputs of a workgroup
constexpr int RS_MAX_WINDOW = 12288;                     // floats of E a workgroup stages (48 KB); above that E is read from memory
}  // namespace

PBSO_DEFINE_HISTORY_KERNEL(resample_history_kernel)

template <bool STAGED>
__global__ __launch_bounds__(RS_TPB) void resample_kernel(const float *__restrict__ in, long long n, const float *__restrict__ hist,
                                                          const float *__restrict__ h, int L, int M, int T, long long p0, long long n_out,
                                                          float *__restrict__ out, long long out_stride,
                                                          pbso_resample_meter *__restrict__ meters) {
    extern __shared__ float win[];
    __shared__ float s_pk[RS_TPB / 64];
    __shared__ int s_ov[RS_TPB / 64];
    const int c = blockIdx.y, H = T - 1;
    const long long j0 = (long long)blockIdx.x * RS_TPB, j = j0 + threadIdx.x;
    const float *__restrict__ x = in + (long long)c * n;
    const float *__restrict__ hc = hist + (long long)c * H;
    const long long r0 = (p0 + j0 * M) / L;              // the workgroup's first local input sample (j0 < n_out: the grid has no empty group)
    if (STAGED) {
        const long long jl = j0 + RS_TPB - 1 < n_out ? j0 + RS_TPB - 1 : n_out - 1;
        const int cnt = (int)((p0 + jl * M) / L - r0) + T;               // E[r0 .. r_last + T - 1], r_last < n
        for (int i = threadIdx.x; i < cnt; i += RS_TPB) {
            const long long e = r0 + i;
            win[i] = e < H ? hc[e] : x[e - H];
        }
        __syncthreads();
    }
    float pk = 0.f;
    int over = 0;
    if (j < n_out) {
        const long long p = p0 + j * M, r = p / L;
        const int phi = (int)(p - r * L);
        const float *__restrict__ row = h + (long long)phi * T;
        const long long e0 = r + H;                      // tap k reads E[e0 - k]
        const float *__restrict__ w0 = win + (e0 - r0);
        auto sample = [&](int k) -> float {
            if (STAGED) return w0[-k];
            const long long e = e0 - k;
            return e < H ? hc[e] : x[e - H];
        };
        float acc = 0.f;
        if ((T & 3) == 0) {
            for (int k = T - 4; k >= 0; k -= 4) {
                const float4 w = *reinterpret_cast<const float4 *>(row + k);
                acc = fmaf(w.w, sample(k + 3), acc);
                acc = fmaf(w.z, sample(k + 2), acc);
                acc = fmaf(w.y, sample(k + 1), acc);
                acc = fmaf(w.x, sample(k), acc);
            }
        } else {
            for (int k = T - 1; k >= 0; --k) acc = fmaf(row[k], sample(k), acc);
        }
        out[(long long)c * out_stride + j] = acc;
        pk = fabsf(acc);
        over = pk > 1.f ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) {
        pk = fmaxf(pk, __shfl_xor(pk, o, 64));
        over += __shfl_xor(over, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_pk[threadIdx.x >> 6] = pk;
        s_ov[threadIdx.x >> 6] = over;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pk = fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3]));
        over = s_ov[0] + s_ov[1] + s_ov[2] + s_ov[3];
        // (a NaN output leaves the peak as it is: fmaxf drops it)
        atomicMax(reinterpret_cast<unsigned int *>(&meters[c].out_peak), __float_as_uint(pk));
        if (over) atomicAdd(&meters[c].n_over, over);
    }
}

// pcm[s][c] = (int16_t)lrintf(fminf(fmaxf(y, -1.f), 1.f) * 32767.f) of y [C][stride]: the clamp, one rounded multiplication, then
// to the nearest integer, ties to even
__global__ __launch_bounds__(256) void resample_pcm16_kernel(const float *__restrict__ y, int C, long long n, long long stride,
                                                             short *__restrict__ pcm) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * C) return;
    const long long s = i / C;
    const int c = (int)(i - s * C);
    const float x = fminf(fmaxf(y[(long long)c * stride + s], -1.f), 1.f) * 32767.f;
    pcm[i] = (short)__float2int_rn(x);
}

int launch_resample(const float *in, int C, long long n, const float *hist, float *hist_next, const float *h, int L, int M, int T,
                    long long p0, long long n_out, float *out, long long out_stride, void *meters, hipStream_t stream) {
    if (!in || !hist || !hist_next || !h || !out || !meters || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0 || L < 1 || M < 1 || T < 1 ||
        p0 < 0 || p0 >= M || n_out < 0 || out_stride < n_out)
        return (int)hipErrorInvalidValue;
    // every output must read inside the call: the last one at local input sample (p0 + (n_out - 1) M) div L < n
    if (n_out > 0 && (p0 + (n_out - 1) * M) / L >= n) return (int)hipErrorInvalidValue;
    if ((n_out + RS_TPB - 1) / RS_TPB > 0x7fffffffll) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(meters, 0, (size_t)C * sizeof(pbso_resample_meter), stream);
    if (e != hipSuccess) return (int)e;
    if (n_out > 0) {
        const dim3 grid((unsigned)((n_out + RS_TPB - 1) / RS_TPB), C);
        const long long window = (long long)(RS_TPB - 1) * M / L + 1 + T;
        if (window <= RS_MAX_WINDOW)
            hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(RS_TPB), (size_t)window * sizeof(float), stream, in, n, hist, h, L, M, T, p0,
                               n_out, out, out_stride, (pbso_resample_meter *)meters);
        else
            hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(RS_TPB), 0, stream, in, n, hist, h, L, M, T, p0, n_out, out, out_stride,
                               (pbso_resample_meter *)meters);
    }
    if (T > 1)
        hipLaunchKernelGGL(resample_history_kernel, dim3((unsigned)((T - 1 + 255) / 256), C), dim3(256), 0, stream, in, C, n, hist, hist_next,
                           T - 1);
    return (int)hipGetLastError();
}

int launch_resample_pcm16(const float *y, int C, long long n, long long stride, short *pcm, hipStream_t stream) {
    if (!y || !pcm || C < 1 || C > SCENE_MAX_CHANNELS || n <= 0 || stride < n) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(resample_pcm16_kernel, dim3((unsigned)((n * C + 255) / 256)), dim3(256), 0, stream, y, C, n, stride, pcm);
    return (int)hipGetLastError();
}

}  // namespace pbso
