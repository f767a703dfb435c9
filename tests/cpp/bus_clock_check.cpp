// Pins openpbso_amd/csrc/bus_clock.h and scene_ramp.h -- the cross-fade clock, the ramp of one parameter and the step clock that the four scene
// buses share -- against the rules of include/openpbso_amd.h, written out here once more and by brute force where there is a
// closed form in the code under test.  Host compiler only, AddressSanitizer + UBSan (make -C openpbso_amd/csrc bus_clock_check);
// tests/test_bus_clock.py builds and runs it.  Prints "bus clock check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <string>

#include "bus_clock.h"

using namespace pbso;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// "w(t) = ... while t - t_set + 1 < R, 1 from then on (at once for R = 0)": sample t is inside a fade that began at t_set
static bool in_fade(long long t, long long t_set, int R) { return t - t_set + 1 < (long long)R; }

// One bus with fade length R, its steps n samples long: two sets, the fade of the second followed to its end, a reset.
static void fade_case(int R, long long n) {
    XFade f;
    StepClock c;
    f.R = R;
    c.arm(0);
    CHECK(!f.fading(c.t) && f.fade_end(c.t) == c.t && f.n_fade(c.t, n) == 0);    // nothing set: silence, no fade
    // the first set after enable: in force at once, whatever R
    f.pending = true;
    const int first = f.incoming();
    CHECK(first == f.to_idx);                            // (nothing to keep: into the slot in force)
    f.swap_in(c.t);
    CHECK(f.have_to && !f.have_from && !f.pending && f.to_idx == first && f.t_set == 0);
    CHECK(!f.fading(c.t) && f.n_fade(c.t, n) == 0 && f.fade_end(c.t) == c.t);
    c.advance(n, 1);
    // the second set fades from the first, over R samples from t_set = n on, into the other slot
    CHECK(!f.fading(c.t));                               // (a set call is accepted)
    f.pending = true;
    CHECK(f.incoming() == (first ^ 1));
    f.swap_in(c.t);
    const long long t_set = n;
    CHECK(f.have_to && f.have_from && f.to_idx == (first ^ 1) && f.t_set == t_set);
    bool met_end = false, met_after = false;
    for (long long step = 2; step < 2 + 8; ++step) {
        const long long t = c.t;
        const bool fading = in_fade(t, t_set, R);
        CHECK(f.fading(t) == fading);                    // (a set call now is refused exactly while this holds)
        if (R < 2) CHECK(!f.fading(t));
        long long inside = 0, end = t;                   // samples of this step inside the fade; the first sample past the fade
        for (long long i = 0; i < n; ++i) inside += in_fade(t + i, t_set, R) ? 1 : 0;
        while (in_fade(end, t_set, R)) ++end;
        CHECK(f.n_fade(t, n) == inside);
        CHECK(f.fade_end(t) == end);                     // info[1]: == t when no fade runs
        if (fading) CHECK(end == t_set + R - 1 && inside == (n < end - t ? n : end - t));
        if (fading && t + n == end) met_end = true;      // the step that ends exactly at the fade's last sample
        if (!fading && met_end && !met_after) { met_after = true; CHECK(inside == 0 && end == t); }
        c.advance(n, step);
    }
    if (R >= 2 && (R - 1) % n == 0) CHECK(met_end && met_after);
    // after the fade a set is accepted again and goes back to the first slot
    CHECK(!f.fading(c.t) && f.incoming() == first);
    f.pending = true;
    f.reset();
    c.reset(10);
    CHECK(!f.have_to && !f.have_from && !f.pending && f.t_set == 0 && c.t == 0);
    f.pending = true;
    f.swap_in(c.t);                                      // the first set after reset: no fade
    CHECK(f.have_to && !f.have_from && !f.fading(c.t) && f.n_fade(c.t, n) == 0);
}

// p(t) = from + slope * k in fp64, k = t - t_set + 1, slope = (to - from) / R rounded once; to for k >= R and for R == 0
static double p_of(double from, double to, long long t_set, int R, long long t) {
    const long long k = t - t_set + 1;
    if (R == 0 || k >= R) return to;
    const double slope = (to - from) / (double)R;
    return from + slope * (double)k;
}

static void ramp_cases() {
    const int R = 4;
    SceneParam q{0.0, 0.0, 0, 0.0};
    ramp_set(q, 1.0, 0, R, false);                       // the first set: no ramp
    CHECK(q.from == 1.0 && q.to == 1.0 && q.slope == 0.0 && ramp_value(q, 0, R) == 1.0 && ramp_value(q, 100, R) == 1.0);
    ramp_set(q, 3.0, 8, R, true);                        // from p(7) = 1 to 3 over samples 8 .. 11
    CHECK(q.from == 1.0 && q.to == 3.0 && q.t_set == 8 && q.slope == 0.5);
    CHECK(ramp_value(q, 8, R) == 1.5 && ramp_value(q, 9, R) == 2.0);
    CHECK(ramp_value(q, 8 + R - 2, R) == 2.5);           // k = R - 1: the last sample of the ramp
    CHECK(ramp_value(q, 8 + R - 1, R) == 3.0 && ramp_value(q, 8 + R, R) == 3.0);   // k = R: the target itself, and beyond
    ramp_set(q, -1.0, 10, R, true);                      // a second set in the middle: from the value one sample before, p(9) = 2
    CHECK(q.from == 2.0 && q.to == -1.0 && q.t_set == 10 && q.slope == -0.75);
    CHECK(ramp_value(q, 10, R) == 1.25 && ramp_value(q, 13, R) == -1.0);
    // values that are not exact in binary: the two rounded operations of the header, from this file's own p_of
    SceneParam g{0.0, 0.0, 0, 0.0};
    ramp_set(g, (double)0.1f, 0, 7, false);
    ramp_set(g, (double)0.7f, 3, 7, true);
    for (long long t = 2; t < 14; ++t) CHECK(ramp_value(g, t, 7) == (t < 3 ? (double)0.1f : p_of((double)0.1f, (double)0.7f, 3, 7, t)));
    // ... and a set in the middle of that ramp whose from + slope * R misses the target in the last bit: at k = R it is the
    // target itself, not the line's value there
    const double mid = p_of((double)0.1f, (double)0.7f, 3, 7, 5);
    ramp_set(g, -1.0, 6, 7, true);
    CHECK(g.from == mid && g.slope == (-1.0 - mid) / 7.0 && g.from + g.slope * 7.0 != -1.0);
    CHECK(ramp_value(g, 6 + 7 - 2, 7) == mid + g.slope * 6.0 && ramp_value(g, 6 + 7 - 1, 7) == -1.0);
    // R = 0: at once
    SceneParam z{0.0, 0.0, 0, 0.0};
    ramp_set(z, 2.0, 0, 0, false);
    ramp_set(z, 5.0, 6, 0, true);
    CHECK(z.from == 2.0 && z.to == 5.0 && z.slope == 0.0 && ramp_value(z, 5, 0) == 5.0 && ramp_value(z, 6, 0) == 5.0);
    // reset in the middle of a ramp: at the target, the ramp finished
    ramp_settle(q);
    CHECK(q.from == q.to && q.to == -1.0 && q.slope == 0.0 && q.t_set == 0 && ramp_value(q, 0, R) == -1.0);
}

static void clock_cases() {
    StepClock c;
    c.arm(5);                                            // enabled after step 5: armed for step 6
    CHECK(c.order(5) < 0);                               // a call with no new step
    CHECK(c.order(6) == 0);
    CHECK(c.order(7) > 0);                               // a call after a skipped step
    c.advance(1026, 6);
    CHECK(c.t == 1026 && c.order(6) < 0 && c.order(7) == 0 && c.order(8) > 0);
    c.reset(9);                                          // a call after reset: the step before it is not to be handled
    CHECK(c.t == 0 && c.order(9) < 0 && c.order(10) == 0 && c.order(11) > 0);
    // the two messages, in the words of every bus
    const BusWords mix = {"scene_mix", "mixed", "the mixer", "audio", "mix", "n_channels"};
    const BusWords reverb = {"scene_reverb", "processed", "the reverb", "input", "processed step", "n_out"};
    const BusWords master = {"master", "processed", "the master bus", "signal", "processed step", "n_channels"};
    CHECK(step_refusal(-1, mix) == "scene_mix: the last step is mixed already (or was taken before the mixer was enabled / reset)");
    CHECK(step_refusal(1, mix) ==
          "scene_mix: a step was not mixed, the history is no longer the audio before this step (pbso_scene_mix_reset starts over)");
    CHECK(step_refusal(-1, reverb) == "scene_reverb: the last step is processed already (or was taken before the reverb was enabled / reset)");
    CHECK(step_refusal(1, reverb) == "scene_reverb: a step was not processed, the history is no longer the input before this step "
                                     "(pbso_scene_reverb_reset starts over)");
    CHECK(step_refusal(-1, master) == "master: the last step is processed already (or was taken before the master bus was enabled / reset)");
    CHECK(step_refusal(1, master) ==
          "master: a step was not processed, the history is no longer the signal before this step (pbso_master_reset starts over)");
}

int main() {
    for (int R : {0, 1, 2, 5})
        for (long long n : {1, 2, 3, 4, 7}) fade_case(R, n);
    ramp_cases();
    clock_cases();
    if (failures) {
        std::printf("bus clock check: %d failed\n", failures);
        return 1;
    }
    std::printf("bus clock check ok\n");
    return 0;
}
