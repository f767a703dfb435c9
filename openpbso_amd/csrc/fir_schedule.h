// The integer arithmetic of the scene filter mix's schedule (include/openpbso_amd.h "scene filter mix", SCHEDULE): when a
// scheduled filter set may take effect, and how a step with filter sets inside it is cut into the work strips that
// the scheduled scene_fir_stage1 (kernels_fir.hip) runs.  Integers only and no HIP call: scene_fir.cpp builds a step's table with it,
// the kernels read the entries, and tests/cpp/fir_schedule_check.cpp pins all of it against a per-sample labelling on the host
// compiler alone.
#pragma once

#include <vector>

namespace pbso {

// A filter set may not take effect while the fade of its predecessor runs (R >= 2: the fade of a set in force since t_prev
// covers t_prev .. t_prev + R - 2).  The rule of pbso_scene_fir_set, with t_set given by the caller.
inline bool fir_spacing_ok(long long t_set, long long t_prev, int R) { return R < 2 || t_set - t_prev + 1 >= (long long)R; }

// The smallest t_set the next scheduled filter set may have (pbso_scene_fir_schedule_info out[3]): not before `floor`, the next
// mixed sample or the sample behind the last pending set, and not inside the predecessor's fade where there is a predecessor.
inline long long fir_next_t_min(long long floor, bool have_prev, long long t_prev, int R) {
    if (!have_prev || R < 2) return floor;
    const long long after = t_prev + (long long)R - 1;
    return after > floor ? after : floor;
}

// One piece of a step between two filter change points, in samples of the step: [begin, end) runs under pool set `to` (-1:
// nothing set yet, silence), faded in from pool set `from` (-1: none) since the absolute sample t_set.
struct FirSegment { long long begin, end; int to, from; long long t_set; };

// One workgroup's samples [s_begin, s_end) of the step, all of one segment, at most `strip` of them: the pool sets to run.
// set_from >= 0 only where the strip intersects its segment's fade.
struct FirStrip { long long s_begin, s_end; int set_to, set_from; };

// Pool indices: 0 is the set in force when the step begins, 1 the set it is fading from, 2 + k the step's scheduled set k.
// The step [t0, t0 + n) with the S ascending times t_sets in it; what it began with: have_to / have_from / t_set0 (XFade).
inline void fir_segments(long long t0, long long n, int S, const long long *t_sets, bool have_to, bool have_from, long long t_set0,
                         std::vector<FirSegment> &out) {
    out.clear();
    long long begin = 0;
    int to = have_to ? 0 : -1, from = have_to && have_from ? 1 : -1;
    long long ts = t_set0;
    for (int k = 0; k <= S; ++k) {
        const long long end = k < S ? t_sets[k] - t0 : n;
        if (end > begin) out.push_back(FirSegment{begin, end, to, from, ts});
        if (k == S) break;
        from = to;                                       // (the first set after enable / reset has no predecessor: no fade)
        to = 2 + k;
        ts = t_sets[k];
        begin = end;
    }
}

// whether the local samples [b, e) of a segment touch its fade: t - t_set + 1 < R for t = t0 + b
inline bool fir_in_fade(const FirSegment &g, long long t0, long long b, int R) {
    return g.from >= 0 && R >= 2 && t0 + b - g.t_set + 1 < (long long)R;
}

// The step's work strips, in sample order; segments of silence (nothing set yet) have none: stage 2 writes their zeros.
inline void fir_strips(const std::vector<FirSegment> &segs, long long t0, int R, int strip, std::vector<FirStrip> &out) {
    out.clear();
    for (const FirSegment &g : segs) {
        if (g.to < 0) continue;
        for (long long b = g.begin; b < g.end; b += strip) {
            const long long e = b + strip < g.end ? b + strip : g.end;
            out.push_back(FirStrip{b, e, g.to, fir_in_fade(g, t0, b, R) ? g.from : -1});
        }
    }
}

}  // namespace pbso
