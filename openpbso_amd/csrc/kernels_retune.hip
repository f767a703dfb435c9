// pbso_set_material: the coefficient tables of some objects rebuilt on the device from (c1, c2, c3) per mode (retune.cpp).
// Plain fp64 VALU and HBM streaming; the arithmetic is mode_tables.h, the same functions finalize runs on the host, and this
// file is compiled without FMA contraction like kernels_exact.hip: the tables come out bit for bit as finalize would build them.
#include "mode_tables.h"

namespace pbso {

constexpr int RETUNE_THREADS = 256;

// One lane per (named object, mode column), padding columns included.  grid: (ceil(m_pad / 256), named objects in y, folded).
// A lane's chain of up to frames 2x2 products is dependent: latency-bound, nothing to price against a roof.
__global__ __launch_bounds__(RETUNE_THREADS) void retune_tables_kernel(const RetuneTables t, const RetuneObj *__restrict__ objs, int n_objs,
                                                                      const double *__restrict__ coefs) {
    const int m = blockIdx.x * RETUNE_THREADS + threadIdx.x;
    if (m >= t.m_pad) return;
    for (int y = blockIdx.y; y < n_objs; y += gridDim.y) retune_lane(t, objs[y], coefs, m);
}

// g32 = (float)(c3[m] * shape[dof][m]) of the named objects that have shapes: consecutive lanes on consecutive modes, 8 B read
// and 4 B written per element (plus the L2-resident c3).  One element per lane and pass: a wave's loads and stores cover whole
// lines; four consecutive elements per lane (32-byte loads, 16-byte stores) measured slower, 1.72 ms against 1.31 at 1024 x 512 x 768.
// grid: (blocks over n_dof * m_pad, grid-stride; named objects in y, folded).
__global__ __launch_bounds__(RETUNE_THREADS) void retune_g32_kernel(const RetuneObj *__restrict__ objs, int n_objs, const double *__restrict__ coefs,
                                                                   const double *__restrict__ shapes, float *__restrict__ g32, int m_pad) {
    for (int y = blockIdx.y; y < n_objs; y += gridDim.y) {
        const RetuneObj o = objs[y];
        const long long n = (long long)o.n_dof * m_pad;
        for (long long e = (long long)blockIdx.x * RETUNE_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * RETUNE_THREADS)
            retune_g32_lane(o, coefs, shapes, g32, m_pad, e);
    }
}

int launch_retune_tables(const RetuneTables &t, const RetuneObj *objs, int n_objs, const double *coefs, hipStream_t stream) {
    if (n_objs <= 0) return 0;
    const dim3 grid((t.m_pad + RETUNE_THREADS - 1) / RETUNE_THREADS, n_objs < 65535 ? n_objs : 65535);
    hipLaunchKernelGGL(retune_tables_kernel, grid, dim3(RETUNE_THREADS), 0, stream, t, objs, n_objs, coefs);
    return (int)hipGetLastError();
}

// max_elems: the largest n_dof * m_pad among the named objects (0: none has shapes, nothing is launched)
int launch_retune_g32(const RetuneObj *objs, int n_objs, const double *coefs, const double *shapes, float *g32, int m_pad, long long max_elems,
                      hipStream_t stream) {
    if (n_objs <= 0 || max_elems <= 0) return 0;
    long long bx = (max_elems + RETUNE_THREADS - 1) / RETUNE_THREADS;
    if (bx > 4096) bx = 4096;
    const dim3 grid((unsigned)bx, n_objs < 65535 ? n_objs : 65535);
    hipLaunchKernelGGL(retune_g32_kernel, grid, dim3(RETUNE_THREADS), 0, stream, objs, n_objs, coefs, shapes, g32, m_pad);
    return (int)hipGetLastError();
}

}  // namespace pbso
