// Pins ramp_next of openpbso_amd/csrc/scene_ramp.h -- the record one set leaves behind, the body that pbso_scene_mix_set runs on the
// host and that scene_schedule_expand_kernel chains over a step's scheduled sets on the device -- against the chain of plain sets
// it stands for.  Random schedules are walked twice: parameter by parameter and set by set as a thread of the kernel walks them
// (ramp_next; block k + 1 of the records from block k), and set by set over all parameters as Engine::scene_mix_set does between
// two steps cut at the set's sample (ramp_set of bus_clock.h, and the header's rule written out once more).  Every field of every
// record is compared bitwise.  Some sets leave the delays unchanged, one schedule begins with the first set after a reset.
// Host compiler only, AddressSanitizer + UBSan (make -C openpbso_amd/csrc scene_schedule_check); tests/test_scene_schedule_check.py
// builds and runs it.  Prints "scene schedule check ok" and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

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

static bool same(const SceneParam &a, const SceneParam &b) {
    return std::memcmp(&a.from, &b.from, 8) == 0 && std::memcmp(&a.to, &b.to, 8) == 0 && a.t_set == b.t_set &&
           std::memcmp(&a.slope, &b.slope, 8) == 0;
}

// the header's rule for one set of one parameter, written out: "p_from = the value at t_set - 1 of the record in force at t_set - 1",
// "slope = (p_to - p_from) / R divided once", "the first set after enable / reset takes effect without a ramp"
static SceneParam by_the_rule(const SceneParam &cur, double v, long long t, int R, bool first) {
    SceneParam q;
    if (first) q.from = v;
    else {
        const long long k = (t - 1) - cur.t_set + 1;
        q.from = (R == 0 || k >= R) ? cur.to : cur.from + cur.slope * (double)k;
    }
    q.to = v;
    q.t_set = t;
    q.slope = R ? (q.to - q.from) / (double)R : 0.0;
    return q;
}

struct Set { long long t; bool has_delay; std::vector<float> gain, delay; };

// One schedule of K sets over cn (channel, object) pairs, from the state `p` [cn][2] (any_set: a set was made since enable / reset)
static void schedule_case(std::mt19937_64 &rng, int cn, int K, int R, long long t0, int max_gap, std::vector<SceneParam> p, bool any_set,
                          bool some_without_delay) {
    std::uniform_real_distribution<float> gain(-2.f, 2.f), delay(0.f, 1400.f);
    std::vector<Set> sets((size_t)K);
    long long t = t0;
    for (int k = 0; k < K; ++k) {
        t += k == 0 ? (long long)(rng() % 3) : 1 + (long long)(rng() % (unsigned)max_gap);
        sets[k].t = t;
        sets[k].has_delay = !(some_without_delay && rng() % 3 == 0);
        for (int i = 0; i < cn; ++i) {
            sets[k].gain.push_back(gain(rng));
            if (sets[k].has_delay) sets[k].delay.push_back(rng() % 5 == 0 ? std::floor(delay(rng)) : delay(rng));
        }
    }
    // as the kernel: one walk per parameter i = pair * 2 + kind, records [K + 1][cn][2]
    std::vector<SceneParam> rec((size_t)(K + 1) * cn * 2);
    for (int i = 0; i < 2 * cn; ++i) {
        const int kind = i & 1, pair = i >> 1;
        SceneParam q = p[i];
        rec[i] = q;
        for (int k = 0; k < K; ++k) {
            const bool changed = kind == 0 || sets[k].has_delay;
            const double to = changed ? (double)(kind == 0 ? sets[k].gain[pair] : sets[k].delay[pair]) : 0.0;
            q = ramp_next(q, to, changed, sets[k].t, R, any_set || k > 0);
            rec[(size_t)(k + 1) * cn * 2 + i] = q;
        }
    }
    // as the host between cut steps: one plain set after the other over all parameters, and the rule beside it
    std::vector<SceneParam> plain = p, rule = p;
    bool any = any_set;
    for (int k = 0; k < K; ++k) {
        for (int pair = 0; pair < cn; ++pair) {
            ramp_set(plain[2 * pair], sets[k].gain[pair], sets[k].t, R, any);
            rule[2 * pair] = by_the_rule(rule[2 * pair], sets[k].gain[pair], sets[k].t, R, !any);
            if (sets[k].has_delay) {
                ramp_set(plain[2 * pair + 1], sets[k].delay[pair], sets[k].t, R, any);
                rule[2 * pair + 1] = by_the_rule(rule[2 * pair + 1], sets[k].delay[pair], sets[k].t, R, !any);
            }
        }
        any = true;
        bool ok = true, untouched = true;
        for (int i = 0; i < 2 * cn; ++i) {
            const SceneParam &r = rec[(size_t)(k + 1) * cn * 2 + i];
            ok = ok && same(r, plain[i]) && same(r, rule[i]);
            if ((i & 1) && !sets[k].has_delay) untouched = untouched && same(r, rec[(size_t)k * cn * 2 + i]);
        }
        CHECK(ok);
        CHECK(untouched);                                // a set of gains only copies the delay records forward
    }
    // the value at any sample is that of the record in force there: the ramp is continuous across a set made during it
    for (int k = 1; k < K && R > 1; ++k)
        for (int i = 0; i < 2 * cn; ++i) {
            const SceneParam &before = rec[(size_t)k * cn * 2 + i], &after = rec[(size_t)(k + 1) * cn * 2 + i];
            const double v = ramp_value(before, sets[k].t - 1, R);
            CHECK(std::memcmp(&v, &after.from, 8) == 0 || same(before, after));
        }
}

int main() {
    std::mt19937_64 rng(20240607);
    const SceneParam silent{0.0, 0.0, 0, 0.0};
    for (int R : {0, 1, 7, 513, 2000})
        for (int round = 0; round < 6; ++round) {
            const int cn = 1 + (int)(rng() % 9), K = 1 + (int)(rng() % 40);
            const int max_gap = round % 2 ? 3000 : 600;  // sets that land during the ramp before them, and after it
            // after the enable: silence, the first set without a ramp
            schedule_case(rng, cn, K, R, 0, max_gap, std::vector<SceneParam>((size_t)cn * 2, silent), false, round >= 2);
            // in the middle of a run: from records that are themselves mid-ramp
            std::vector<SceneParam> p((size_t)cn * 2);
            std::uniform_real_distribution<double> val(-2.0, 2.0);
            for (SceneParam &q : p) {
                q = silent;
                ramp_set(q, (float)val(rng), 100, R, false);
                ramp_set(q, (float)val(rng), 5000, R, true);
            }
            schedule_case(rng, cn, K, R, 5000 + (long long)(rng() % 700), max_gap, p, true, round >= 2);
            // the first set after a reset: the targets kept, ramps finished, and no ramp at the first set
            for (SceneParam &q : p) ramp_settle(q);
            schedule_case(rng, cn, K, R, 0, max_gap, p, false, true);
        }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("scene schedule check ok\n");
    return 0;
}
