// The integer arithmetic of the EQ bus's schedule (include/openpbso_amd.h "The EQ bus's SCHEDULE"): when a scheduled set may take
// effect, and the plan of a step with sets inside it that the kernels of kernels_eq_schedule.hip read -- the segments of the step,
// one per set in force, and the two block lists the chain kernel walks.  Integers only and no HIP call: eq.cpp builds a step's plan
// with it, and tests/cpp/eq_schedule_check.cpp pins all of it against a per-sample labelling on the host compiler alone.  Compile
// with -ffp-contract=off as eq_block.h.
//
// Rows.  Every signal of a scheduled step lives in two extended rows of EQ_HIST + n doubles, index EQ_HIST + i = sample t + i:
//   V  the timeline in force: at every sample the value of the cascade of the newest set with t_set <= that sample;
//   F  the tails: while set g fades in (t_set_g .. t_set_g + R - 2) its predecessor's own values.  Tails never overlap, because
//      t_set_{g+1} >= t_set_g + R - 1.
// A block formula of a set refers to samples before its t_set at t_set - 1 and t_set - 2 only, and those are V.  A tail's formula
// reads V below the index `vs` of its segment and F from there on.
#pragma once

#include <climits>
#include <vector>

#include "eq_block.h"

namespace pbso {

constexpr int EQ_MAX_PENDING = 65536;                    // scheduled sets that may wait
constexpr int EQ_MAX_SETS_PER_STEP = 4096;               // ... and that may take effect inside one processed step

// A set may not take effect while the fade of its predecessor runs (R >= 2: the fade of a set in force since t_prev covers
// t_prev .. t_prev + R - 2).  The identity of enable / reset is a predecessor with t_prev = 0.
inline bool eq_spacing_ok(long long t_set, long long t_prev, int R) { return R < 2 || t_set - t_prev + 1 >= (long long)R; }

// The smallest t_set the next scheduled set may have (pbso_eq_schedule_info out[2]): not before the next processed sample, behind
// the last pending set when there is one, and not inside the predecessor's fade.
inline long long eq_next_t_min(long long t_next, bool prev_pending, long long t_prev, int R) {
    long long m = t_next;
    if (prev_pending && t_prev + 1 > m) m = t_prev + 1;
    if (R >= 2 && t_prev + (long long)R - 1 > m) m = t_prev + (long long)R - 1;
    return m;
}

// how many of the pending sets (ascending t_set) take effect inside the step [t, t + n)
inline int eq_sets_in_step(const long long *t_set, int n_pending, long long t, long long n) {
    int k = 0;
    while (k < n_pending && t_set[k] < t + n) ++k;
    return k;
}

// Table ids: 0 and 1 are the stage's two table slots, 2 + j the step's pool entry j.

// One set in force inside the step.  Record 0 stands for the cascade that is fading out when the step begins (only a and tab are
// read); record 1 + g is segment g: g = 0 the set in force when the step begins, g >= 1 the step's scheduled set g - 1.  All
// positions are row indices.
struct EqSeg {
    int s;                                               // first index of the segment (segment 0: EQ_HIST)
    int a;                                               // an origin of the set's block grid, a <= s: origins are a + m P
    int tab;                                             // table id
    int fe;                                              // the segment's fade covers [s, fe): its predecessor's tail (fe == s: none)
    int vs;                                              // the tail reads V below this index and F from it on
    int pad;
    long long d0;                                        // t - t_set + 1 at index s
};

// One block of a chain: the origin, how many of its samples belong to the chain (a block is cut short by the next set, by the end
// of a tail or by the end of the step), and where its two last samples come from.
struct EqBlk {
    int o, L;                                            // samples o .. o + L - 1, 1 <= L <= P; the pair is o + L - 2, o + L - 1
    int tab;                                             // table id
    int vs;                                              // stored values are read from V below this index, from F from it on
    int lo;                                              // samples below this index are stored already and not computed
    int flags;                                           // EQ_BLK_F: the block is a tail's; EQ_BLK_RESET: the chain starts here from o - 1, o - 2
};
constexpr int EQ_BLK_F = 1, EQ_BLK_RESET = 2;

struct EqPlan {
    std::vector<EqSeg> seg;                              // 2 + K records
    std::vector<EqBlk> vblk, fblk;                       // the chain of V, then the chains of the tails, in order
    int from_hist = 0;                                   // the fade of the last set runs past the step: From's history is written
    int vs_last = 0;                                     // ... from V below this index and from F from it on
};

// whether the plan fits the kernels' int indices
inline bool eq_plan_fits(long long n) { return n > 0 && n < (long long)INT_MAX - 4 * EQ_HIST; }

// The blocks of the grid `a + m P` that hold samples of [b, e), each cut at e; stored samples lie below lo.
inline void eq_blocks(int a, int b, int e, int tab, int vs, int lo, int flags, std::vector<EqBlk> &out) {
    bool first = true;
    for (long long o = a + (long long)((b - a) / EQ_BLOCK) * EQ_BLOCK; o < e; o += EQ_BLOCK) {
        const int L = (int)(e - o < EQ_BLOCK ? e - o : EQ_BLOCK);
        out.push_back(EqBlk{(int)o, L, tab, vs, lo, flags | (first ? EQ_BLK_RESET : 0)});
        first = false;
    }
}

// The plan of the step [t, t + n) with the K ascending t_set[] inside it.  What the step begins with: the set in force since
// t_to in table slot `to`, and -- while t - t_to + 1 < R -- its predecessor, on the grid of t_from, in the other slot.
inline void eq_plan(long long t, long long n, int R, int to, long long t_to, long long t_from, bool have_from, int K, const long long *t_set,
                    EqPlan &p) {
    const int H = EQ_HIST, N = (int)(H + n);
    p.seg.clear();
    p.vblk.clear();
    p.fblk.clear();
    const bool fading0 = have_from && R >= 2 && t - t_to + 1 < (long long)R;
    const long long fade0 = fading0 ? t_to + R - 1 - t : 0;
    p.seg.push_back(EqSeg{H, H - eq_block_offset(t, fading0 ? t_from : t), to ^ 1, H, 0, 0, 0});
    p.seg.push_back(EqSeg{H, H - eq_block_offset(t, t_to), to, (int)(H + (fade0 < n ? fade0 : n)), 0, 0, t - t_to + 1});
    for (int j = 0; j < K; ++j) {
        const int s = (int)(H + (t_set[j] - t));
        const long long fe = R >= 2 ? (long long)s + R - 1 : s;
        p.seg.push_back(EqSeg{s, s, 2 + j, (int)(fe < N ? fe : N), s, 0, 1});
    }
    for (int g = 0; g <= K; ++g) {
        const EqSeg &q = p.seg[1 + g], &f = p.seg[g];
        const int e = g < K ? p.seg[2 + g].s : N;
        if (e > q.s) eq_blocks(q.a, q.s, e, q.tab, INT_MAX, H, 0, p.vblk);
        if (q.fe > q.s) eq_blocks(f.a, q.s, q.fe, f.tab, q.vs, q.s, EQ_BLK_F, p.fblk);
    }
    // only the step's first block of V starts the chain from stored values; every later one continues it
    for (size_t i = 1; i < p.vblk.size(); ++i) p.vblk[i].flags &= ~EQ_BLK_RESET;
    const EqSeg &last = p.seg[1 + K];
    p.from_hist = K > 0 ? (R >= 2 && (long long)last.s + R - 1 > N) : (fade0 > n);
    p.vs_last = last.vs;
}

}  // namespace pbso
