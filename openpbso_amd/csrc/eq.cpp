// The engine's side of the EQ bus (include/openpbso_amd.h "EQ bus"; kernels_eq.hip): at most two cascades of biquad sections, To
// in force since t_set and From faded out behind it, each with its block tables (eq_block.h) in one of two slots on the device and
// the last EQ_HIST samples of every signal in a double-buffered history; the cross-fade clock and the rule that every step is
// processed exactly once (bus_clock.h).  Its input is the caller's device buffer: of a step it reads the length only (last_nb_)
// and counts steps by tot_steps_.  It knows bus_state.h and nothing of the other buses.
#include "bus_state.h"
#include "eq_block.h"

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
    if (const char *why = eq_refusal(sos, (long long)q.C * q.S)) return fail(PBSO_ERR_INVALID, std::string("eq_set: ") + why);
    if (q.xf.fading(q.clock.t)) return fail(PBSO_ERR_STATE, "eq_set: a cross-fade is still running");
    HIPTRY(hipSetDevice(desc_.device));
    const int slot = q.xf.incoming();
    for (size_t i = 0; i < (size_t)q.C * q.S; ++i) pbso::eq_tables(sos + 5 * i, q.tab[slot].data() + i * EQ_TABLES * EQ_BLOCK);
    HIPTRY(q.upload(slot, stream_));
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
    HIPTRY(hipSetDevice(desc_.device));
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
    q.out.wrote(out, last_nb_);
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
