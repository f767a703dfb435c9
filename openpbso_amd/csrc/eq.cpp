// The engine's side of the EQ bus (include/openpbso_amd.h "EQ bus"; kernels_eq.hip): at most two cascades of biquad sections, To
// in force since t_set and From faded out behind it, each with its block tables (eq_block.h) in one of two slots on the device and
// the last EQ_HIST samples of every signal in a double-buffered history; the cross-fade clock and the rule that every step is
// processed exactly once (bus_clock.h).  Its input is the caller's device buffer: of a step it reads the length only (last_nb_)
// and counts steps by tot_steps_.  It knows bus_state.h and nothing of the other buses.
#include "bus_state.h"
#include "eq_block.h"
#include "eq_schedule.h"

#include <cstdio>
#include <cstring>

namespace pbso {

struct Eq {
    int C = 0, S = 0;
    StepClock clock;
    XFade xf;                                            // xf.to_idx: the slot of To; To's grid starts at xf.t_set
    long long t_set_from = 0;                            // ... and From's here
    int64_t n_calls = 0, n_sets = 0;
    std::vector<double> tab[2];                          // [C][S][5][P] of either slot, as on the device
    DevMem<double> d_tab;                                // [2][C][S][5][P]
    DevMem<double> hist[2];                              // the pair; each [2 slots][C][S + 1][EQ_HIST]
    int at = 0;
    DevMem<double> work_to, work_from;
    UploadRing up;
    BusOut out;
    // the schedule (eq_schedule.h): the sets not yet in force as coefficients, ascending; the plain set that waits, as coefficients
    // too, because a step with scheduled sets inside it builds every table on the device
    std::vector<long long> sched_t;
    std::vector<double> sched_sos;                       // [sched_t.size()][C][S][5]
    std::vector<double> plain_sos;                       // [C][S][5] of the set eq_set left pending
    int64_t last_step_sets = 0;
    EqPlan plan;
    StagingRing stage;
    DevMem<char> d_plan;                                 // a step's coefficients, segments and block lists
    DevMem<double> d_pool, work_sched;                   // a step's tables [K][C][S][5][P]; its rows
    size_t set_words() const { return (size_t)C * S * 5; }
    void drop_schedule() {
        sched_t.clear();
        sched_sos.clear();
    }
    size_t tab_words() const { return (size_t)C * S * EQ_TABLES * EQ_BLOCK; }
    size_t hist_words() const { return (size_t)C * (S + 1) * EQ_HIST; }
    hipError_t silence(hipStream_t s) {
        for (DevMem<double> &b : hist) {
            const hipError_t e = hipMemsetAsync(b.p, 0, b.cap * sizeof(double), s);
            if (e != hipSuccess) return e;
        }
        at = 0;
        return hipSuccess;
    }
    // tab[slot] to the device, through the ring
    hipError_t upload(int slot, hipStream_t s) {
        char *b = nullptr;
        hipError_t e = up.acquire(b);
        if (e != hipSuccess) return e;
        const size_t bytes = tab_words() * sizeof(double);
        std::memcpy(b, tab[slot].data(), bytes);
        e = hipMemcpyAsync(d_tab.p + (size_t)slot * tab_words(), b, bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        return up.record(s);
    }
    // enable and reset: the identity cascade in slot 0, in force since sample 0, nothing pending and no fade
    hipError_t install_identity(hipStream_t s) {
        double c[5], one[EQ_TABLES * EQ_BLOCK];
        eq_identity(c);
        pbso::eq_tables(c, one);
        for (size_t i = 0; i < (size_t)C * S; ++i) std::memcpy(tab[0].data() + i * EQ_TABLES * EQ_BLOCK, one, sizeof(one));
        xf.reset();
        xf.have_to = true;
        xf.to_idx = 0;
        t_set_from = 0;
        drop_schedule();
        last_step_sets = 0;
        return upload(0, s);
    }
};

static const BusWords WORDS = {"eq", "processed", "the EQ bus", "signal", "processed step", "n_channels"};

void Engine::eq_release() {
    if (!eq_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete eq_;
    eq_ = nullptr;
}

int Engine::eq_enable(int C, int S, int xfade) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "eq_enable before finalize");
    if (C < 1 || C > SCENE_MAX_CHANNELS) return fail(PBSO_ERR_INVALID, "eq_enable: n_channels must be 1 .. 8");
    if (S < 1 || S > EQ_MAX_SECTIONS) return fail(PBSO_ERR_INVALID, "eq_enable: n_sections must be 1 .. 8");
    if (xfade < 0 || xfade > (1 << 20)) return fail(PBSO_ERR_INVALID, "eq_enable: xfade_samples must be 0 .. 1 << 20");
    HIPTRY(hipSetDevice(desc_.device));
    std::unique_ptr<Eq> q(new Eq());
    q->C = C;
    q->S = S;
    q->xf.R = xfade;
    q->tab[0].assign(q->tab_words(), 0.0);
    q->tab[1].assign(q->tab_words(), 0.0);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("eq_enable: cannot allocate ") + what);
    };
    if (q->d_tab.alloc(2 * q->tab_words()) != hipSuccess) return nomem("the tables");
    for (DevMem<double> &b : q->hist)
        if (b.alloc(2 * q->hist_words()) != hipSuccess) return nomem("the history");
    if (q->up.create(q->tab_words() * sizeof(double)) != UploadRing::OK) return nomem("the upload ring");
    if (q->silence(stream_) != hipSuccess || q->install_identity(stream_) != hipSuccess) return nomem("the state");
    eq_release();
    q->clock.arm(tot_steps_);
    eq_ = q.release();
    return PBSO_OK;
}

// takes effect at the first sample of the next processed step; replaces a set that no step has taken up yet
int Engine::eq_set(const double *sos) {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq_set: the EQ bus is not enabled");
    if (!sos) return fail(PBSO_ERR_INVALID, "eq_set: sos is NULL");
    Eq &q = *eq_;
    if (!q.sched_t.empty()) return fail(PBSO_ERR_STATE, "eq_set: scheduled sets are pending (pbso_eq_clear_schedule drops them)");
    if (const char *why = eq_refusal(sos, (long long)q.C * q.S)) return fail(PBSO_ERR_INVALID, std::string("eq_set: ") + why);
    if (q.xf.fading(q.clock.t)) return fail(PBSO_ERR_STATE, "eq_set: a cross-fade is still running");
    HIPTRY(hipSetDevice(desc_.device));
    const int slot = q.xf.incoming();
    for (size_t i = 0; i < (size_t)q.C * q.S; ++i) pbso::eq_tables(sos + 5 * i, q.tab[slot].data() + i * EQ_TABLES * EQ_BLOCK);
    HIPTRY(q.upload(slot, stream_));
    q.plain_sos.assign(sos, sos + q.set_words());
    q.xf.pending = true;
    ++q.n_sets;
    return PBSO_OK;
}

int Engine::eq(const void *d_in, void *d_out) {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq: the EQ bus is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "eq: d_in is NULL");
    Eq &q = *eq_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "eq: no step yet");
    if (const int order = q.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    const long long n = (long long)last_nb_ * B_, t = q.clock.t;
    if (d_out && d_out != d_in) {
        const char *a = (const char *)d_in, *b = (const char *)d_out;
        const size_t bytes = (size_t)q.C * n * sizeof(float);
        if (a < b + bytes && b < a + bytes) return fail(PBSO_ERR_INVALID, "eq: d_out overlaps d_in without being d_in");
    }
    if (eq_sets_in_step(q.sched_t.data(), (int)q.sched_t.size(), t, n) > 0) return eq_scheduled(d_in, d_out);
    HIPTRY(hipSetDevice(desc_.device));
    const int taken = q.xf.pending ? 1 : 0;
    // the sets in force in this step: a pending one takes effect at t
    XFade xf = q.xf;
    long long t_set_from = q.t_set_from;
    if (xf.pending) {
        t_set_from = xf.t_set;
        xf.swap_in(t);
    }
    const long long n_fade = xf.n_fade(t, n);
    float *out;
    GROWTRY(q.out.resolve(d_out, (size_t)q.C * n, stream_, out), "eq: output: cannot allocate", "eq: output");
    GROWTRY(grow(q.work_to, eq_work_doubles(q.C, n), stream_), "eq: work arrays: cannot allocate", "eq: work arrays");
    if (n_fade) GROWTRY(grow(q.work_from, eq_work_doubles(q.C, n_fade), stream_), "eq: work arrays: cannot allocate", "eq: work arrays");
    double *cur = q.hist[q.at].p, *next = q.hist[q.at ^ 1].p;
    const size_t hw = q.hist_words(), tw = q.tab_words();
    const int to = xf.to_idx, from = to ^ 1;
    // before t_set, To takes every signal's values from From: its history is From's
    if (q.xf.pending) HIPTRY(hipMemcpyAsync(cur + to * hw, cur + from * hw, hw * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    q.xf = xf;
    q.t_set_from = t_set_from;
    const double *y_to = nullptr, *y_from = nullptr;
    int lrc = launch_eq_cascade((const float *)d_in, n, q.C, q.S, n, eq_block_offset(t, xf.t_set), cur + to * hw, next + to * hw, q.d_tab.p + to * tw,
                                q.work_to, &y_to, stream_);
    if (lrc == 0 && n_fade)
        lrc = launch_eq_cascade((const float *)d_in, n, q.C, q.S, n_fade, eq_block_offset(t, t_set_from), cur + from * hw, next + from * hw,
                                q.d_tab.p + from * tw, q.work_from, &y_from, stream_);
    if (lrc == 0) lrc = launch_eq_output(y_to, y_from, q.C, n, n_fade, t - xf.t_set + 1, xf.R, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_eq");
    q.at ^= 1;
    q.clock.advance(n, tot_steps_);
    ++q.n_calls;
    q.last_step_sets = taken;
    q.out.wrote(out, last_nb_);
    return PBSO_OK;
}

// A step with scheduled sets inside it (eq_schedule.h; kernels_eq_schedule.hip): every allocation first, so that a refusal changes
// nothing; then the coefficients and the plan in one upload, the tables on the device, 2 + 3 S launches, and the stage left as the
// plain path keeps it: the last two sets in the two table slots, their histories in the pair, the fade clock at the last set.
int Engine::eq_scheduled(const void *d_in, void *d_out) {
    Eq &q = *eq_;
    const long long n = (long long)last_nb_ * B_, t = q.clock.t;
    const int Ks = eq_sets_in_step(q.sched_t.data(), (int)q.sched_t.size(), t, n), plain = q.xf.pending ? 1 : 0, K = Ks + plain;
    if (K > EQ_MAX_SETS_PER_STEP) return fail(PBSO_ERR_INVALID, "eq: more than 4096 sets take effect inside this step (step in shorter pieces, or clear the schedule)");
    if (!eq_plan_fits(n)) return fail(PBSO_ERR_INVALID, "eq: the step is too long for a schedule");
    HIPTRY(hipSetDevice(desc_.device));
    const size_t sw = q.set_words(), tw = q.tab_words(), hw = q.hist_words();
    std::vector<long long> ts((size_t)K);
    if (plain) ts[0] = t;
    for (int j = 0; j < Ks; ++j) ts[(size_t)plain + j] = q.sched_t[(size_t)j];
    eq_plan(t, n, q.xf.R, q.xf.to_idx, q.xf.t_set, q.t_set_from, q.xf.have_from, K, ts.data(), q.plan);
    const EqPlan &p = q.plan;
    const size_t b_sos = (size_t)K * sw * sizeof(double), b_seg = p.seg.size() * sizeof(EqSeg), b_v = p.vblk.size() * sizeof(EqBlk),
                 b_f = p.fblk.size() * sizeof(EqBlk), bytes = b_sos + b_seg + b_v + b_f;
    float *out;
    GROWTRY(q.out.resolve(d_out, (size_t)q.C * n, stream_, out), "eq: output: cannot allocate", "eq: output");
    GROWTRY(grow(q.d_pool, (size_t)K * tw, stream_), "eq: schedule tables: cannot allocate", "eq: schedule tables");
    GROWTRY(grow(q.work_sched, eq_sched_work_doubles(q.C, n), stream_), "eq: work arrays: cannot allocate", "eq: work arrays");
    GROWTRY(grow(q.d_plan, bytes, stream_), "eq: schedule plan: cannot allocate", "eq: schedule plan");
    char *b = nullptr;
    GROWTRY(q.stage.acquire(bytes, b), "eq: schedule staging: cannot allocate", "eq: schedule staging");
    if (plain) std::memcpy(b, q.plain_sos.data(), sw * sizeof(double));
    std::memcpy(b + (size_t)plain * sw * sizeof(double), q.sched_sos.data(), (size_t)Ks * sw * sizeof(double));
    std::memcpy(b + b_sos, p.seg.data(), b_seg);
    std::memcpy(b + b_sos + b_seg, p.vblk.data(), b_v);
    if (b_f) std::memcpy(b + b_sos + b_seg + b_v, p.fblk.data(), b_f);
    HIPTRY(hipMemcpyAsync(q.d_plan.p, b, bytes, hipMemcpyHostToDevice, stream_));
    HIPTRY(q.stage.record(stream_));
    // the stage behind the step: the last set in slot to2, the one before it in the other
    const int to = q.xf.to_idx, to2 = to ^ (K & 1);
    const double *last = (const double *)(b + (size_t)(K - 1) * sw * sizeof(double));
    for (size_t i = 0; i < (size_t)q.C * q.S; ++i) {
        if (K >= 2) pbso::eq_tables(last - sw + 5 * i, q.tab[to2 ^ 1].data() + i * EQ_TABLES * EQ_BLOCK);
        pbso::eq_tables(last + 5 * i, q.tab[to2].data() + i * EQ_TABLES * EQ_BLOCK);
    }
    const long long t_from2 = K >= 2 ? ts[(size_t)K - 2] : q.xf.t_set;
    q.xf.to_idx = to2;
    q.xf.have_to = q.xf.have_from = true;
    q.xf.pending = false;
    q.xf.t_set = ts[(size_t)K - 1];
    q.t_set_from = t_from2;
    q.sched_t.erase(q.sched_t.begin(), q.sched_t.begin() + Ks);
    q.sched_sos.erase(q.sched_sos.begin(), q.sched_sos.begin() + (size_t)Ks * sw);
    const double *cur = q.hist[q.at].p;
    double *next = q.hist[q.at ^ 1].p;
    const char *d = q.d_plan.p;
    int lrc = launch_eq_sched_tables((const double *)d, (long long)K * q.C * q.S, q.d_pool.p, stream_);
    if (lrc == 0)
        lrc = launch_eq_scheduled((const float *)d_in, q.C, q.S, n, q.xf.R, d + b_sos, K, d + b_sos + b_seg, (int)p.vblk.size(), d + b_sos + b_seg + b_v,
                                  (int)p.fblk.size(), q.d_tab.p, q.d_pool.p, cur + to * hw, cur + (to ^ 1) * hw, next + to2 * hw, next + (to2 ^ 1) * hw,
                                  p.from_hist, p.vs_last, q.work_sched.p, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_eq_scheduled");
    if (K >= 2)
        HIPTRY(hipMemcpyAsync(q.d_tab.p + (to2 ^ 1) * tw, q.d_pool.p + (size_t)(K - 2) * tw, tw * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    HIPTRY(hipMemcpyAsync(q.d_tab.p + to2 * tw, q.d_pool.p + (size_t)(K - 1) * tw, tw * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    if (host_profile_) std::fprintf(stderr, "eq: scheduled step: %d sets, %d kernel launches\n", K, 3 + 3 * q.S);
    q.at ^= 1;
    q.clock.advance(n, tot_steps_);
    ++q.n_calls;
    q.last_step_sets = K;
    q.out.wrote(out, last_nb_);
    return PBSO_OK;
}

// pbso_eq_set_at / pbso_eq_schedule: all of the sets are validated before any is taken
int Engine::eq_schedule(const char *name, int n_sets, const int64_t *t_set, const double *sos) {
    const std::string nm(name);
    if (!eq_) return fail(PBSO_ERR_STATE, nm + ": the EQ bus is not enabled");
    if (n_sets < 0) return fail(PBSO_ERR_INVALID, nm + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set || !sos) return fail(PBSO_ERR_INVALID, nm + ": t_set or sos is NULL");
    Eq &q = *eq_;
    if (q.sched_t.size() + (size_t)n_sets > (size_t)EQ_MAX_PENDING) return fail(PBSO_ERR_INVALID, nm + ": more than 65536 sets pending");
    const size_t sw = q.set_words();
    bool prev_pending = !q.sched_t.empty() || q.xf.pending;
    long long t_prev = !q.sched_t.empty() ? q.sched_t.back() : q.xf.pending ? q.clock.t : q.xf.t_set;
    for (int j = 0; j < n_sets; ++j) {
        if ((long long)t_set[j] < eq_next_t_min(q.clock.t, prev_pending, t_prev, q.xf.R))
            return fail(PBSO_ERR_INVALID, nm + ": t_set must be >= the next processed sample, ascending, and t_set - t_prev + 1 >= xfade_samples");
        if (const char *why = eq_refusal(sos + (size_t)j * sw, (long long)q.C * q.S)) return fail(PBSO_ERR_INVALID, nm + ": " + why);
        prev_pending = true;
        t_prev = t_set[j];
    }
    for (int j = 0; j < n_sets; ++j) q.sched_t.push_back(t_set[j]);
    q.sched_sos.insert(q.sched_sos.end(), sos, sos + (size_t)n_sets * sw);
    q.n_sets += n_sets;
    return PBSO_OK;
}

int Engine::eq_clear_schedule() {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq_clear_schedule: the EQ bus is not enabled");
    eq_->drop_schedule();
    return PBSO_OK;
}

int Engine::eq_schedule_info(int64_t out[4]) {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq_schedule_info: the EQ bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "eq_schedule_info: out is NULL");
    const Eq &q = *eq_;
    const bool prev_pending = !q.sched_t.empty() || q.xf.pending;
    const long long t_prev = !q.sched_t.empty() ? q.sched_t.back() : q.xf.pending ? q.clock.t : q.xf.t_set;
    out[0] = q.clock.t;
    out[1] = (int64_t)q.sched_t.size();
    out[2] = eq_next_t_min(q.clock.t, prev_pending, t_prev, q.xf.R);
    out[3] = q.last_step_sets;
    return PBSO_OK;
}

int Engine::read_eq(float *out, size_t n) { return read_bus(eq_ ? &eq_->out : nullptr, eq_ ? eq_->C : 0, WORDS, out, n); }

// the tables in force: To's, once its set has taken effect (a pending set's are not in force yet)
int Engine::eq_tables(double *out, size_t n) {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq_tables: the EQ bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "eq_tables: out is NULL");
    if (n != eq_->tab_words()) return fail(PBSO_ERR_INVALID, "eq_tables size mismatch (n = n_channels * n_sections * 5 * PBSO_EQ_BLOCK)");
    std::memcpy(out, eq_->tab[eq_->xf.to_idx].data(), n * sizeof(double));
    return PBSO_OK;
}

// the identity cascade again, every history silent, t = 0, no fade and nothing pending.  Armed for the next step.
int Engine::eq_reset() {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq_reset: the EQ bus is not enabled");
    Eq &q = *eq_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(q.silence(stream_));
    HIPTRY(q.install_identity(stream_));
    q.clock.reset(tot_steps_);
    return PBSO_OK;
}

int Engine::eq_info(int64_t out[4]) {
    if (!eq_) return fail(PBSO_ERR_STATE, "eq_info: the EQ bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "eq_info: out is NULL");
    const Eq &q = *eq_;
    out[0] = q.clock.t;
    out[1] = q.xf.fade_end(q.clock.t);
    out[2] = q.n_calls;
    out[3] = q.n_sets;
    return PBSO_OK;
}

}  // namespace pbso

// needs no engine; here and not in capi.cpp because this file is compiled without FMA contraction
extern "C" int pbso_eq_design(int kind, double rate, double f0, double q, double gain_db, double out[5]) {
    if (!out || pbso::eq_design_refusal(kind, rate, f0, q, gain_db)) return PBSO_ERR_INVALID;
    pbso::eq_design(kind, rate, f0, q, gain_db, out);
    return PBSO_OK;
}
