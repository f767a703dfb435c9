// Pins openpbso_amd/csrc/fir_schedule.h -- the work-strip table of a step of the scene filter mix with scheduled filter sets inside
// it, and the validation arithmetic of pbso_scene_fir_schedule -- against brute force: every sample of the step is labelled with
// the set in force, the set it fades from and whether its fade runs, by walking the sets sample by sample as the public header
// states the rule (the plain set's XFade of bus_clock.h between pieces cut at every t_set), and the table must say the same of
// every sample, cover every sample that has a filter exactly once, in order, with strips of at most `strip` samples that never
// cross a change point.  Strip lengths 512 and 2048; segments shorter than, equal to and longer than a strip; change points at
// 0, n - 1, k * 512 and k * 512 +- 1; R in {0, 1, 2, 7, 600}; t0 at 0 and near 2^40.
// Host compiler only, AddressSanitizer + UBSan (make -C openpbso_amd/csrc fir_schedule_check); tests/test_fir_schedule_check.py
// builds and runs it.  Prints "fir schedule check ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <random>
#include <vector>

#include "bus_clock.h"
#include "fir_schedule.h"

using namespace pbso;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 20) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

struct Label { int to, from; bool fading; long long t_set; };

// the step sample by sample: a plain set "between two steps cut at its sample" is XFade::swap_in at that sample
static std::vector<Label> brute(long long t0, long long n, const std::vector<long long> &ts, XFade f) {
    std::vector<Label> lab((size_t)n);
    int to = f.have_to ? 0 : -1, from = f.have_to && f.have_from ? 1 : -1;
    size_t k = 0;
    for (long long i = 0; i < n; ++i) {
        const long long t = t0 + i;
        if (k < ts.size() && ts[k] == t) {
            f.pending = true;
            f.swap_in(t);
            from = to;
            to = 2 + (int)k;
            ++k;
        }
        lab[(size_t)i] = Label{to, f.have_from ? from : -1, f.fading(t), f.t_set};
    }
    CHECK(k == ts.size());
    return lab;
}

static void check_step(long long t0, long long n, const std::vector<long long> &ts, const XFade &f0, int strip) {
    const std::vector<Label> lab = brute(t0, n, ts, f0);
    std::vector<FirSegment> segs;
    std::vector<FirStrip> strips;
    fir_segments(t0, n, (int)ts.size(), ts.data(), f0.have_to, f0.have_from, f0.t_set, segs);
    fir_strips(segs, t0, f0.R, strip, strips);
    // the segments tile the step, in order, and say of every sample what the labelling says
    long long at = 0;
    for (const FirSegment &g : segs) {
        CHECK(g.begin == at && g.end > g.begin && g.end <= n);
        for (long long i = g.begin; i < g.end && i < n; ++i) {
            const Label &l = lab[(size_t)i];
            CHECK(l.to == g.to);
            CHECK(!l.fading || (l.from == g.from && l.t_set == g.t_set));
            CHECK(fir_in_fade(g, t0, i, f0.R) == l.fading);
        }
        at = g.end;
    }
    CHECK(at == n);
    // the strips cover exactly the samples with a filter, once each and in order; none is longer than `strip` or crosses a change
    // point; set_from is there exactly for the strips that hold a sample of their segment's fade
    std::vector<int> seen((size_t)n, 0);
    long long last_end = 0;
    for (const FirStrip &e : strips) {
        CHECK(e.s_begin >= last_end && e.s_end > e.s_begin && e.s_end <= n && e.s_end - e.s_begin <= strip && e.set_to >= 0);
        last_end = e.s_end;
        bool any_fade = false;
        for (long long i = e.s_begin; i < e.s_end && i < n; ++i) {
            const Label &l = lab[(size_t)i];
            ++seen[(size_t)i];
            CHECK(l.to == e.set_to);
            CHECK(i == e.s_begin || l.t_set == lab[(size_t)i - 1].t_set);      // (no change point inside)
            if (l.fading) {
                any_fade = true;
                CHECK(e.set_from == l.from && e.set_from >= 0);
            }
        }
        CHECK((e.set_from >= 0) == any_fade);
    }
    for (long long i = 0; i < n; ++i) CHECK(seen[(size_t)i] == (lab[(size_t)i].to >= 0 ? 1 : 0));
}

// the validation arithmetic against the plain set's own rule: a set at t is accepted by pbso_scene_fir_set exactly when no fade
// runs at t (XFade::fading), and out[3] is the first t that passes
static void check_validation() {
    for (int R : {0, 1, 2, 7, 600})
        for (long long t_prev : {0ll, 5ll, (1ll << 40) + 3}) {
            XFade f;
            f.R = R;
            f.have_to = f.have_from = true;
            f.t_set = t_prev;
            for (long long d = 1; d <= 700; ++d) CHECK(fir_spacing_ok(t_prev + d, t_prev, R) == !f.fading(t_prev + d));
            for (long long floor : {t_prev + 1, t_prev + 3, t_prev + 599, t_prev + 2000}) {
                const long long m = fir_next_t_min(floor, true, t_prev, R);
                CHECK(m >= floor && fir_spacing_ok(m, t_prev, R));
                CHECK(m == floor || !fir_spacing_ok(m - 1, t_prev, R));
                CHECK(fir_next_t_min(floor, false, t_prev, R) == floor);
            }
        }
    // the issue's own two cases: spacing R - 2 refused, R - 1 accepted
    CHECK(!fir_spacing_ok(100 + 7 - 2, 100, 7) && fir_spacing_ok(100 + 7 - 1, 100, 7));
}

int main() {
    std::mt19937_64 rng(20261020);
    for (long long t0 : {0ll, 1ll << 40, (1ll << 40) + 777})
        for (int R : {0, 1, 2, 7, 600})
            for (int strip : {512, 2048}) {
                const long long n = (strip == 512 ? 6 : 16) * 513;
                // what the step begins with: nothing, a set without a predecessor, a finished fade, a fade that still runs
                for (int begin = 0; begin < 4; ++begin) {
                    XFade f;
                    f.R = R;
                    f.have_to = begin >= 1;
                    f.have_from = begin >= 2;
                    f.t_set = begin == 3 ? t0 - 3 : t0 - 5000;
                    if (begin >= 1 && t0 == 0) f.t_set = 0, f.have_from = false;     // (a set at sample 0 is the first: no fade)
                    // hand-made change points, thinned to the spacing rule (against the set in force too)
                    std::vector<long long> cands = {0, 1, 511, 512, 513, 1023, 1024, 1025, 1536, 1536 + 2048, 1536 + 2047, n - 2, n - 1};
                    for (int k = 0; k < 6; ++k) cands.push_back((long long)(rng() % (unsigned long long)n));
                    for (int pass = 0; pass < 3; ++pass) {
                        std::vector<long long> pick = cands, ts;
                        if (pass == 1) pick = {0, n - 1};
                        if (pass == 2) pick = {(long long)strip, 2ll * strip, 2ll * strip + (long long)strip + 1};   // segments of exactly a strip, and one more
                        std::sort(pick.begin(), pick.end());
                        bool have_prev = f.have_to;
                        long long t_prev = f.t_set;
                        for (long long c : pick) {
                            if (c >= n) continue;
                            const long long t = t0 + c;
                            if (have_prev && (t <= t_prev || !fir_spacing_ok(t, t_prev, R))) continue;
                            if (f.have_to && f.fading(t) && ts.empty()) continue;
                            ts.push_back(t);
                            have_prev = true;
                            t_prev = t;
                        }
                        check_step(t0, n, ts, f, strip);
                    }
                    check_step(t0, n, {}, f, strip);
                    check_step(t0, 1, {}, f, strip);
                }
            }
    check_validation();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("fir schedule check ok\n");
    return 0;
}
