// The ramp of one scene parameter (include/openpbso_amd.h "scene mix"; the master bus's gain is one too): the record and its
// evaluation, and the record that a set leaves behind; ONE definition for the hosts (bus_clock.h) and the kernels
// (kernels_mix.hip, kernels_master.hip), all built with -ffp-contract=off.  Nothing else is here, and no HIP call: kernels.h
// includes this and every kernel file with it.
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

// The record in force from sample t on, after a set to v that takes effect at t, given the record `cur` in force until t - 1: a
// running ramp is left at the value it had one sample before (from_current false: the first set after enable / reset, which
// takes effect without a ramp).  A set that leaves this parameter alone (changed false: the delays of a set of gains only)
// copies the record forward.  One body for pbso_scene_mix_set on the host (ramp_set of bus_clock.h) and for the sets of a
// schedule, which scene_schedule_expand_kernel chains on the device; the division is the correctly rounded one on both sides.
PBSO_HOST_DEVICE inline SceneParam ramp_next(const SceneParam &cur, double v, bool changed, long long t, int R, bool from_current) {
    if (!changed) return cur;
    SceneParam q;
    q.from = from_current ? ramp_value(cur, t - 1, R) : v;
    q.to = v;
    q.t_set = t;
    q.slope = R ? (q.to - q.from) / (double)R : 0.0;
    return q;
}

}  // namespace pbso
