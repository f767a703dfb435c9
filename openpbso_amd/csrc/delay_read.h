// The scene mix's read of a row behind a fractional delay: the one copy for the scene mixer (kernels_mix.hip) and for the delay
// stage of the scene filter mix (kernels_fir.hip), which must round alike.
#pragma once
#include <hip/hip_runtime.h>

namespace pbso {

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

}  // namespace pbso
