// The scene reverb (pbso_scene_reverb): n_in bus signals convolved with K taps per (output channel, input), K up to 1 << 17, in
// the direct form.  The taps are cut into J = ceil(K / S) segments of S = SCENE_REVERB_SEGMENT; segment j of input i is a FIR of
// K_j <= S taps behind an onset of j S, so per (channel c, input i, segment j, sample t)
//
//   p_cij(t) = ONE f32 fmaf chain, taps min(K, (j + 1) S) - 1 down to j S, i.e. upward through the window of input samples
//
// and Y_c(t) = the p_cij added from 0.f, i ascending, j ascending (stage 2).  The chain runs on v_mfma_f32_16x16x4_f32, which is bit
// for bit a k-ordered fmaf chain on its accumulator (the formulation of kernels_fir.hip): for a tile of 256 samples s = 16 a + b,
//
//   Y[b][a] += T[b][m] * XW[m][a],   XW[m][a] = u(16 a + m - (K_j - 1) - j S),   T[b][m] = h_j[b + K_j - 1 - m] (0 outside 0 .. K_j-1)
//
// over the window positions m = 0 .. K_j + 14 ascending, four per instruction (zero taps up to a multiple of 8).  A product with a
// zero tap adds nothing (fmaf(0, x, acc) == acc for finite x).  Unlike the filter mix there is no loop over objects: a workgroup
// stages one window once and every staged sample is used K_j times, so a wave carries as many tiles as its registers allow.
// Built with -ffp-contract=off and without any fast-math or denormal flag.
#include <hip/hip_runtime.h>

#include "conv_mfma.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int S = SCENE_REVERB_SEGMENT;
constexpr int RV_PIECE = 512;                            // window positions whose taps are in LDS at a time (66 KB a segment at C = 8 otherwise)
constexpr int RV_TPW = RV_PIECE + 16;                    // floats of one channel's piece
constexpr int RV_STAGE_BATCH = 8;                        // global loads a thread issues before it waits, when staging

__host__ __device__ __forceinline__ int seg_taps(int K, int j) { return K - j * S < S ? K - j * S : S; }
__host__ __device__ __forceinline__ int seg_positions(int Kj) { return (Kj + 15 + 7) / 8 * 8; }
}  // namespace

// P[row = (c n_in + i) J + j][LP] = segment j's taps reversed behind 15 zeros and zero-padded: P[15 + m] = r_ci[j S + K_j - 1 - m]
__global__ __launch_bounds__(256) void reverb_prepare_kernel(const float *__restrict__ taps, long long n_ci, int K, int J, int LP,
                                                             float *__restrict__ P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ci * J * LP) return;
    const long long row = i / LP;
    const long long ci = row / J;
    const int j = (int)(row - ci * J), Kj = seg_taps(K, j);
    const int m = (int)(i - row * LP) - 15;
    P[i] = m >= 0 && m < Kj ? taps[ci * K + (long long)j * S + (Kj - 1 - m)] : 0.f;
}

// One workgroup per (strip of blockDim.x / 64 * T * 256 samples, (input i, segment j), filter set).  The workgroup stages the
// strip's window of input i -- its samples and the K_j - 1 before them, shifted by j S, the history in front of the step -- in
// LDS once; the C tap rows of the segment follow in pieces of RV_PIECE window positions.  Every wave walks the positions four at a
// time: one A operand per channel (the taps), one B operand per tile (the window), C T MFMAs on C T accumulators.
//   LDS: win [win_at(W) + 1] | taps [C][RV_TPW],  W = strip + Mp window positions
// (The lane decomposition, the batched staging, the two-round walk and the write-out below are those of scene_fir_stage1 of
//  kernels_fir.hip in another loop structure: conv_mfma.h says why pieces of a body are not shared.)
template <int C, int T>
__global__ __launch_bounds__(256) void scene_reverb_stage1(const float *__restrict__ in, int n_in, long long n, const float *__restrict__ hist,
                                                           int H, const float *__restrict__ P0, const float *__restrict__ P1, int K, int J,
                                                           int LP, float *__restrict__ parts, long long n_second) {
    extern __shared__ float lds[];
    const int waves = (int)(blockDim.x / 64), strip = waves * T * 256;
    const long long s0 = (long long)blockIdx.x * strip;
    const int ij = blockIdx.y, set = blockIdx.z;
    if (set == 1 && s0 >= n_second) return;              // (the set faded out is needed for the fade's samples only)
    const int i_in = ij / J, j = ij - i_in * J;
    const int Kj = seg_taps(K, j), Mp = seg_positions(Kj), W = strip + Mp;
    const float *__restrict__ P = set ? P1 : P0;
    float *win = lds, *tp = lds + win_at(strip + seg_positions(seg_taps(K, 0))) + 1;   // (the layout of the longest segment)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int la = lane & 15, lr = lane >> 4;
    f32x4 acc[C][T];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int w = 0; w < T; ++w) acc[c][w] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B: lane (k = lr, col a = la) reads window position 16 a + m, m = 4 q + lr;  A: lane (row b = la, k = lr) reads P[15 + m - b]
    int wb[T];
#pragma unroll
    for (int w = 0; w < T; ++w) wb[w] = (wave * T + w) * 256 + 16 * la + lr;
    const int ab = 15 + lr - la;
    const bool wave_live = s0 + (long long)wave * T * 256 < n;
    {
        const float *__restrict__ row = in + (long long)i_in * n, *__restrict__ hrow = hist + (long long)i_in * H;
        const long long shift = s0 - (Kj - 1) - (long long)j * S;
        for (int i0 = threadIdx.x; i0 < W; i0 += RV_STAGE_BATCH * blockDim.x) {
            float v[RV_STAGE_BATCH];
#pragma unroll
            for (int u = 0; u < RV_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                const long long q = shift + i;           // the step's local sample; -H <= q by K_j - 1 + j S <= K - 1 = H
                v[u] = 0.f;
                if (i < W) {
                    if (q >= 0) { if (q < n) v[u] = row[q]; }
                    else if (q >= -(long long)H) v[u] = hrow[H + q];
                }
            }
#pragma unroll
            for (int u = 0; u < RV_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                if (i < W) win[win_at(i)] = v[u];
            }
        }
    }
    for (int m0 = 0; m0 < Mp; m0 += RV_PIECE) {
        const int mp = Mp - m0 < RV_PIECE ? Mp - m0 : RV_PIECE;         // positions of this piece; its taps: P[m0 .. m0 + mp + 16) <= LP
        __syncthreads();                                 // (the previous piece's operands are read)
        for (int i0 = threadIdx.x; i0 < C * RV_TPW; i0 += RV_STAGE_BATCH * blockDim.x) {
            float v[RV_STAGE_BATCH];
#pragma unroll
            for (int u = 0; u < RV_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x, c = i / RV_TPW, k = i - c * RV_TPW;
                v[u] = i < C * RV_TPW && k < mp + 16 ? P[(((long long)c * n_in + i_in) * J + j) * LP + m0 + k] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < RV_STAGE_BATCH; ++u) {
                const int i = i0 + u * (int)blockDim.x;
                if (i < C * RV_TPW) tp[i] = v[u];
            }
        }
        __syncthreads();
        if (!wave_live) continue;
        // two rounds of four window positions per pass (mp is a multiple of 8): the operands of both are read before the first MFMA
        for (int m = 0; m < mp; m += 8) {
            float b[2][T], a[2][C];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int w = 0; w < T; ++w) b[r][w] = win[win_at(wb[w] + m0 + m + 4 * r)];
#pragma unroll
                for (int c = 0; c < C; ++c) a[r][c] = tp[c * RV_TPW + ab + m + 4 * r];
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int w = 0; w < T; ++w)
                        acc[c][w] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][c], b[r][w], acc[c][w], 0, 0, 0);
        }
    }
    // D: lane (col a = la, rows b = 4 lr + g) holds samples 16 a + 4 lr + g of its tile
    const int rows = n_in * J;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float *__restrict__ prow = parts + (((long long)set * C + c) * rows + ij) * n;
#pragma unroll
        for (int w = 0; w < T; ++w) {
            const long long s = s0 + (wave * T + w) * 256 + 16 * la + 4 * lr;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (s + g < n) prow[s + g] = acc[c][w][g];
        }
    }
}

// the partial rows in (i, j) order per channel, blended inside a fade, then add + that when add is given (conv_mfma.h)
__global__ __launch_bounds__(256) void scene_reverb_stage2(const float *__restrict__ parts, int C, int n_rows, long long n, long long n_fade,
                                                           long long t0, long long t_set, int R, const float *add, float *out) {
    conv_stage2(parts, C, n_rows, n, n_fade, t0, t_set, R, add, out);
}

// hist_next[i] = the last H samples of hist[i] ++ in[i]
__global__ __launch_bounds__(256) void reverb_history_kernel(const float *__restrict__ in, long long n, const float *__restrict__ hist,
                                                             float *__restrict__ hist_next, int H) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= H) return;
    const long long q = n + k, i = blockIdx.y;           // q: index into hist ++ in
    hist_next[i * H + k] = q < H ? hist[i * H + q] : in[i * n + (q - H)];
}

int scene_reverb_segments(int K) { return (K + S - 1) / S; }
int scene_reverb_padded_taps(int K) { return seg_positions(K < S ? K : S) + 16; }

int launch_scene_reverb_prepare(const float *taps, int n_out, int n_in, int K, float *P, hipStream_t stream) {
    if (n_out < 1 || n_out > SCENE_MAX_CHANNELS || n_in < 1 || n_in > SCENE_MAX_CHANNELS || K < 1 || K > SCENE_REVERB_MAX_TAPS)
        return (int)hipErrorInvalidValue;
    const int J = scene_reverb_segments(K), LP = scene_reverb_padded_taps(K);
    const long long total = (long long)n_out * n_in * J * LP;
    hipLaunchKernelGGL(reverb_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, taps, (long long)n_out * n_in, K, J, LP, P);
    return (int)hipGetLastError();
}

namespace {
// tiles of 256 samples per wave of the wide launch: about 16 accumulators, so that a pass of C + T LDS reads feeds C T MFMAs
constexpr int wide_tiles(int C) { return C <= 2 ? 8 : C <= 4 ? 4 : 2; }

template <int C, int T>
void launch_stage1(dim3 grid, int waves, hipStream_t stream, const float *in, int n_in, long long n, const float *hist, int H, const float *P0,
                   const float *P1, int K, int J, int LP, float *parts, long long n_second) {
    const int W = waves * T * 256 + LP - 16;
    const size_t lds = (size_t)(W + (W >> 4) + 1 + C * RV_TPW) * sizeof(float);
    hipLaunchKernelGGL((scene_reverb_stage1<C, T>), grid, dim3(64 * waves), lds, stream, in, n_in, n, hist, H, P0, P1, K, J, LP, parts, n_second);
}

template <int C>
int launch_stage1_c(hipStream_t stream, const float *in, int n_in, long long n, const float *hist, int H, const float *P0, const float *P1,
                    int K, long long n_fade, float *parts) {
    const int J = scene_reverb_segments(K), LP = scene_reverb_padded_taps(K), sets = n_fade ? 2 : 1;
    // four waves of wide_tiles(C) tiles each once that gives every CU two workgroups; else one wave of one tile: a one-buffer step
    // has nothing but its 3 tiles x n_in J segments to spread over the chip
    constexpr int TW = wide_tiles(C);
    const long long wide = (n + 4 * TW * 256 - 1) / (4 * TW * 256);
    if (wide * n_in * J * sets >= 512) {
        if (wide > 0x7fffffffll) return (int)hipErrorInvalidValue;
        launch_stage1<C, TW>(dim3((unsigned)wide, (unsigned)(n_in * J), sets), 4, stream, in, n_in, n, hist, H, P0, P1, K, J, LP, parts, n_fade);
    } else {
        launch_stage1<C, 1>(dim3((unsigned)((n + 255) / 256), (unsigned)(n_in * J), sets), 1, stream, in, n_in, n, hist, H, P0, P1, K, J, LP, parts, n_fade);
    }
    return (int)hipGetLastError();
}
}  // namespace

int launch_scene_reverb(const float *in, int n_in, long long n, const float *hist, float *hist_next, const float *P_to, const float *P_from,
                        int n_out, int K, long long n_fade, long long t0, long long t_set, int R, float *parts, const float *add, float *out,
                        hipStream_t stream) {
    if (!in || !out || n_in < 1 || n_in > SCENE_MAX_CHANNELS || n <= 0 || n_out < 1 || n_out > SCENE_MAX_CHANNELS || K < 1 ||
        K > SCENE_REVERB_MAX_TAPS || n_fade < 0 || n_fade > n || (n_fade > 0 && (!P_from || !P_to || R < 2)))
        return (int)hipErrorInvalidValue;
    const int H = K - 1, rows = n_in * scene_reverb_segments(K);
    if (P_to) {
        int rc = 0;
        for_channel_count(n_out, [&](auto c) {
            rc = launch_stage1_c<decltype(c)::value>(stream, in, n_in, n, hist, H, P_to, P_from, K, n_fade, parts);
        });
        if (rc != 0) return rc;
    }
    // (nothing set yet: no rows, silence -- or add alone -- and the history moves on)
    hipLaunchKernelGGL(scene_reverb_stage2, dim3((unsigned)((n + 255) / 256), n_out), dim3(256), 0, stream, parts, n_out, P_to ? rows : 0, n, n_fade, t0,
                       t_set, R, add, out);
    if (H > 0)
        hipLaunchKernelGGL(reverb_history_kernel, dim3((unsigned)((H + 255) / 256), n_in), dim3(256), 0, stream, in, n, hist, hist_next, H);
    return (int)hipGetLastError();
}

}  // namespace pbso
