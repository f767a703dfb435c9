// The scene filter mix's bank (pbso_scene_fir_bank_create; include/openpbso_amd.h "scene filter mix", BANK): F filters of [C][K]
// f32 taps that stay on the device, and filter sets given as J (index, weight) pairs per object.  The taps such a set stands for,
//
//   h_co[k]:  acc = 0.f;  for j = 0 .. J-1 ascending:  acc = fmaf(weight[o][j], bank[index[o][j]][c][k], acc)
//
// are built here, straight into the padded reversed rows the first stage reads (kernels_fir.hip, fir_prepare_kernel's layout:
// P[15 + j] = h_co[K - 1 - j] behind 15 zeros, zero-padded to LP), for all the bank sets of a step in one launch.  Nothing else of
// the filter mix knows how a set's taps came about.
//
// A file of its own: the chain is an f32 fused multiply-add by definition, and kernels_fir.hip is held to containing none
// (tests/test_scene_fir_asm_guards.py).  Built with -ffp-contract=off all the same, so the only fused operations are the fmaf
// written below, and without any fast-math or denormal flag: subnormal taps come out as fmaf gives them.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace pbso {

// One thread per four consecutive floats of one row P[slot][c][o][.], rows in memory order: grid (x: the n_obj * LP / 4 vectors of
// one channel of one set, y: channel, z: bank set).  hdr [n_sets][2] = (pool slot, J) of each set; index / weight
// [n_sets][n_obj][Jmax], the first J of a row used.  The indices were validated on the host: [0, F).
__global__ __launch_bounds__(256) void fir_bank_prepare_kernel(const float *__restrict__ bank, const int *__restrict__ hdr,
                                                               const int *__restrict__ index, const float *__restrict__ weight, int Jmax,
                                                               int n_obj, int C, int K, int LP, float *__restrict__ pool) {
    const unsigned LP4 = (unsigned)LP >> 2;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)n_obj * LP4) return;
    const unsigned o = e / LP4;
    const int c = blockIdx.y, s = blockIdx.z;
    const int slot = hdr[2 * s], J = hdr[2 * s + 1];
    const int k0 = K - 1 - ((int)(e - o * LP4) * 4 - 15);        // the tap of this thread's first float, k0 - i that of float i
    const long long so = ((long long)s * n_obj + o) * Jmax;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < J; ++j) {
        const float w = weight[so + j];
        const float *__restrict__ b = bank + ((long long)index[so + j] * C + c) * K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 - i;
            if (k >= 0 && k < K) acc[i] = fmaf(w, b[k], acc[i]);
        }
    }
    float4 *dst = reinterpret_cast<float4 *>(pool + (((long long)slot * C + c) * n_obj + o) * LP) + (e - o * LP4);
    *dst = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

int launch_scene_fir_bank_prepare(const float *bank, const int *hdr, const int *index, const float *weight, int n_sets, int Jmax,
                                  int n_obj, int C, int K, float *pool, hipStream_t stream) {
    if (n_sets <= 0 || n_sets > SCENE_FIR_MAX_SETS_PER_STEP || Jmax < 1 || Jmax > SCENE_FIR_BANK_MAX_J || n_obj <= 0 || C < 1 ||
        C > SCENE_MAX_CHANNELS || K < 1 || K > SCENE_FIR_MAX_TAPS)
        return (int)hipErrorInvalidValue;
    const long long vecs = (long long)n_obj * (scene_fir_padded_taps(K) / 4);
    if (vecs > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(fir_bank_prepare_kernel, dim3((unsigned)((vecs + 255) / 256), (unsigned)C, (unsigned)n_sets), dim3(256), 0, stream,
                       bank, hdr, index, weight, Jmax, n_obj, C, K, scene_fir_padded_taps(K), pool);
    return (int)hipGetLastError();
}

}  // namespace pbso
