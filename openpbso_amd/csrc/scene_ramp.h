// The ramp of one scene parameter (include/openpbso_amd.h "scene mix"; the master bus's gain is one too): the record and its
// evaluation, ONE definition for the hosts (bus_clock.h) and the kernels (kernels_mix.hip, kernels_master.hip), all built with
// -ffp-contract=off.  Nothing else is here, and no HIP call: kernels.h includes this and every kernel file with it.
#pragma once

#if defined(__HIPCC__)
#define PBSO_HOST_DEVICE __host__ __device__
#else
#define PBSO_HOST_DEVICE
#endif

namespace pbso {

// p(t) = to once t >= t_set + R - 1 (or R == 0), else from + slope (t - t_set + 1) with slope = (to - from) / R stored at the
// set call, in fp64 (t: absolute sample)
struct SceneParam { double from, to; long long t_set; double slope; };

PBSO_HOST_DEVICE inline double ramp_value(const SceneParam &p, long long t, int R) {
    const long long k = t - p.t_set + 1;
    if (R == 0 || k >= R) return p.to;
    return p.from + p.slope * (double)k;
}

}  // namespace pbso
