// The host arithmetic the scene buses share (include/openpbso_amd.h "scene mix", "scene filter mix", "scene reverb", "master
// bus"): the set and reset of a ramp (scene_ramp.h has the record and its evaluation, which the kernels share), the clock of the
// rule that every step is handled exactly once, and the clock of a cross-fade between two sets.  Integers and doubles only and no
// HIP call: the hosts keep their state in these structs (bus_state.h), and tests/cpp/bus_clock_check.cpp pins all of it on the
// host compiler alone.
#pragma once

#include <algorithm>
#include <string>

#include "scene_ramp.h"

namespace pbso {

// a set takes effect at sample t, the first of the next step; a running ramp is left at the value it had one sample before
// (from_current false: the first set after enable / reset, which takes effect without a ramp)
inline void ramp_set(SceneParam &q, double v, long long t, int R, bool from_current) {
    q = ramp_next(q, v, true, t, R, from_current);
}
// reset: the parameter stays at its target, its ramp finished
inline void ramp_settle(SceneParam &q) {
    q.from = q.to;
    q.t_set = 0;
    q.slope = 0.0;
}

// Every step exactly once: t is the absolute sample of the next handled step's first sample, next_step the count of steps the
// next call must find.
struct StepClock {
    long long t = 0, next_step = 0;
    void arm(long long tot_steps) { next_step = tot_steps + 1; }          // (enable, reset: armed for the next step)
    // 0: the step to handle; < 0: no new step since the last call (or since enable / reset); > 0: a step was skipped
    int order(long long tot_steps) const { return tot_steps < next_step ? -1 : tot_steps > next_step ? 1 : 0; }
    void advance(long long n, long long tot_steps) { t += n; arm(tot_steps); }
    void reset(long long tot_steps) { t = 0; arm(tot_steps); }
};

// what a bus calls itself in its messages: "scene_mix", "mixed", "the mixer", "audio", "mix", "n_channels"
struct BusWords { const char *name, *verb, *bus, *signal, *result, *channels; };

// the message of a call that StepClock::order turned down
inline std::string step_refusal(int order, const BusWords &w) {
    const std::string name(w.name), verb(w.verb);
    if (order < 0) return name + ": the last step is " + verb + " already (or was taken before " + w.bus + " was enabled / reset)";
    return name + ": a step was not " + verb + ", the history is no longer the " + w.signal + " before this step (pbso_" + name +
           "_reset starts over)";
}

// Two sets of filters, `to` in force since t_set and cross-faded from `from` over R samples when there was one.  The sets live
// in two slots on the device; to_idx is the slot of `to`.  A set call waits (pending) for the next handled step.
struct XFade {
    int R = 0, to_idx = 0;
    bool have_to = false, have_from = false, pending = false;
    long long t_set = 0;
    // the fade of the sets in force is still running at sample t (R < 2 never fades)
    bool fading(long long t) const { return have_from && t - t_set + 1 < (long long)R; }
    // how many of the n samples from t on are inside the fade
    long long n_fade(long long t, long long n) const { return fading(t) ? std::min(n, t_set + R - 1 - t) : 0; }
    // the absolute sample at which the fade ends; t itself when none is running (info[1])
    long long fade_end(long long t) const { return fading(t) ? t_set + R - 1 : t; }
    // the slot a pending set is written to: the one its predecessor's predecessor had
    int incoming() const { return have_to ? to_idx ^ 1 : to_idx; }
    // the pending set takes effect at t: the set in force becomes the one faded out (the first set after enable / reset has
    // no predecessor and takes effect without a fade)
    void swap_in(long long t) {
        to_idx = incoming();
        have_from = have_to;
        have_to = true;
        t_set = t;
        pending = false;
    }
    void reset() {
        have_to = have_from = pending = false;
        t_set = 0;
    }
};

}  // namespace pbso
