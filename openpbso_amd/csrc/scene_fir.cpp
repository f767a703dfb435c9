// The engine's side of the scene filter mix (include/openpbso_amd.h "scene filter mix"; kernels_fir.hip): the two filter sets (the
// one in force and the one faded out) with their onsets, the cross-fade's clock, the history of every object's last samples on
// the device, and the rule that every step is mixed exactly once.  It reads what a step left (last_audio_, last_nb_) and counts
// steps by tot_steps_.  It knows bus_state.h, which holds what the buses have in common (the cross-fade's clock among it), and
// nothing of the other buses.
// The schedule (pbso_scene_fir_schedule, pbso_scene_fir_delay_schedule): the filter and delay sets not yet in
// force wait on the host as given, each with its t_set; a mix takes those inside its step to the device in one staged block, cuts
// the step into work strips (fir_schedule.h) and launches the schedule's kernels.  A step without a scheduled set inside it is
// launched as it always was.
// The optional delay stage (pbso_scene_fir_delay_enable) puts the scene mix's ramped fractional delay per
// object in front of the filters: its records, the second history (of x: `hist` then holds z), and the other launch.
// The bank (pbso_scene_fir_bank_create): F filters that stay on the device; a bank set -- J (index, weight) pairs per object --
// waits on the host exactly as a taps set does, in the same pending list, and the mix that takes it has its taps built on the
// device (kernels_fir_bank.hip) where a taps set's are copied and reversed.  From there on nothing knows the difference.
#include "bus_state.h"
#include "fir_schedule.h"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <deque>

namespace pbso {

// the delay stage of a filter mix: a SceneParam per object, set and ramped by the scene mix's rule (bus_clock.h)
struct FirDelay {
    int max_delay = 0, ramp = 0, Hx = 0;                 // Hx = max_delay + 1 samples of x history per object
    std::vector<SceneParam> p;                           // [N]: the records in force, uploaded when they changed
    std::vector<float> pend;                             // a set call waits here for the next mix (a later one replaces it)
    bool have_pend = false, any_set = false, dirty = true, ramping = false;
    long long t_set = 0;                                 // of the last set that took effect (every object's)
    int64_t n_sets = 0;
    HistPair hist_x;                                     // [N][Hx]
    DevMem<SceneParam> d_p;
    UploadRing up;                                       // blocks of N records
    // the schedule: the delay sets not yet in force, ascending in t and none before the clock.  A mix expands those inside its step
    // into the step's records on the device (fir_delay_expand_kernel), and the last block becomes d_p; p then lags behind d_p
    // (p_stale) until the copy back, queued behind the mix, is taken over -- the scene mix's mechanism.
    struct Pending { long long t; std::vector<float> v; };
    std::deque<Pending> sched;
    DevMem<SceneParam> d_rec;                            // the step's records [K_d + 1][N]
    SceneParam *p_back = nullptr;                        // pinned: d_p after the last mix that took scheduled sets
    hipEvent_t ev_back = nullptr;
    bool p_stale = false;
    FirDelay() = default;
    FirDelay(const FirDelay &) = delete;
    FirDelay &operator=(const FirDelay &) = delete;
    ~FirDelay() {
        if (p_back) (void)hipHostFree(p_back);
        if (ev_back) (void)hipEventDestroy(ev_back);
    }
    // p as the device has it, before anything reads or changes it: waits for the mix that took the scheduled sets, not for more
    hipError_t refresh() {
        if (!p_stale) return hipSuccess;
        const hipError_t e = hipEventSynchronize(ev_back);
        if (e != hipSuccess) return e;
        std::memcpy(p.data(), p_back, p.size() * sizeof(SceneParam));
        p_stale = false;
        return hipSuccess;
    }
    // the first t at which every ramp is over; t itself when none runs
    long long ramp_end(long long t) const { return ramping && t - t_set + 1 < (long long)ramp ? t_set + ramp - 1 : t; }
};

struct SceneFir {
    int C = 0, N = 0, K = 0, max_onset = 0, H = 0, LP = 0;          // H = max_onset + K - 1 samples of history per object
    XFade fade;                                          // which set is in force, which is faded out, since when
    std::vector<int> onset_to, onset_from;
    // a set call waits here for the next mix (a later one replaces it): taps, or pend_J > 0 pairs per object into the bank
    std::vector<float> pend_taps;
    std::vector<int> pend_onset;
    int pend_J = 0;
    std::vector<int> pend_index;                         // [N][pend_J]
    std::vector<float> pend_weight;
    StepClock clock;
    int64_t n_mixes = 0, n_sets = 0;
    HistPair hist;                                       // [N][H]: of x, or of z = the delayed x once the delay stage is enabled
    std::unique_ptr<FirDelay> delay;                     // pbso_scene_fir_delay_enable
    BusOut out;                                          // [C][n]
    DevMem<float> parts;                                 // partial rows [2][C][groups][n]
    // on the device: the padded reversed taps [C][N][LP] and onsets [N] of both sets (fade.to_idx: the one in force), the raw
    // taps of an upload
    DevMem<float> d_P[2], d_raw;
    DevMem<int> d_onset[2];
    UploadRing up;                                       // blocks of taps [C][N][K] (or a bank set: bank_set_bytes), then onsets [N]
    // the bank [F][C][K]; A = max |tap| of it; where a plain bank set lies on the device: (slot, J) | index [N][J] | weight [N][J]
    DevMem<float> d_bank;
    int bank_F = 0;
    double bank_A = 0.0;
    int64_t n_bank_sets = 0;
    DevMem<char> d_bset;
    // the schedule: the filter sets not yet in force as given (onset NULL resolved to the predecessor's), ascending in t, none
    // before the clock and none inside its predecessor's fade
    // (a bank set: J > 0 pairs per object, index / weight [N][J], and no taps)
    struct Pending { long long t; std::vector<float> taps; std::vector<int> onset; int J = 0; std::vector<int> index; std::vector<float> weight; };
    std::deque<Pending> sched;
    StagingRing stage;                                   // a step's times, work strips, onsets, delays and taps
    DevMem<char> d_sets;                                 // ... on the device
    DevMem<float> d_pool;                                // the step's pool of padded reversed taps [S + 2][C][N][LP]
    DevMem<int> d_onpool;                                // ... and onsets [S + 2][N]

    size_t taps_floats() const { return (size_t)C * N * K; }
    static size_t bank_set_bytes(int n, int J) { return 2 * sizeof(int) + (size_t)n * J * (sizeof(int) + sizeof(float)); }
    size_t bank_sets_pending() const {
        size_t k = fade.pending && pend_J > 0 ? 1 : 0;
        for (const Pending &q : sched) k += q.J > 0 ? 1 : 0;
        return k;
    }
};

static const BusWords WORDS = {"scene_fir", "mixed", "the mixer", "audio", "mix", "n_channels"};

void Engine::scene_fir_release() {
    if (!fir_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete fir_;
    fir_ = nullptr;
}

int Engine::scene_fir_enable(int C, int K, int max_onset, int xfade) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "scene_fir_enable before finalize");
    if (C < 1 || C > SCENE_MAX_CHANNELS) return fail(PBSO_ERR_INVALID, "scene_fir_enable: n_channels must be 1 .. 8");
    if (K < 1 || K > SCENE_FIR_MAX_TAPS) return fail(PBSO_ERR_INVALID, "scene_fir_enable: n_taps must be 1 .. 1024");
    if (max_onset < 0 || max_onset > (1 << 20) || xfade < 0 || xfade > (1 << 20))
        return fail(PBSO_ERR_INVALID, "scene_fir_enable: max_onset and xfade_samples must be 0 .. 1 << 20");
    HIPTRY(hipSetDevice(desc_.device));
    scene_fir_release();
    std::unique_ptr<SceneFir> m(new SceneFir());
    m->C = C;
    m->N = n_objects();
    m->K = K;
    m->max_onset = max_onset;
    m->fade.R = xfade;
    m->H = max_onset + K - 1;
    m->LP = scene_fir_padded_taps(K);
    m->onset_to.assign(m->N, 0);
    m->onset_from.assign(m->N, 0);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("scene_fir_enable: cannot allocate ") + what);
    };
    if (m->hist.create((size_t)m->N * m->H, stream_) != hipSuccess) return nomem("the history");
    const size_t n = (size_t)std::max(last_nb_, 1) * B_;
    if (grow(m->out.own, (size_t)C * n, stream_) != hipSuccess) return nomem("the output");
    if (grow(m->parts, (size_t)2 * C * mix_objects_groups(m->N) * n, stream_) != hipSuccess) return nomem("the partial rows");
    const size_t cn = std::max<size_t>((size_t)C * m->N, 1), no = std::max(m->N, 1);
    for (int i = 0; i < 2; ++i) {
        if (m->d_P[i].alloc(cn * m->LP) != hipSuccess) return nomem("the taps");
        if (m->d_onset[i].alloc(no) != hipSuccess) return nomem("the onsets");
    }
    if (m->d_raw.alloc(cn * K) != hipSuccess) return nomem("the taps");
    switch (m->up.create(std::max(cn * K * sizeof(float), SceneFir::bank_set_bytes((int)no, SCENE_FIR_BANK_MAX_J)) + no * sizeof(int))) {
    case UploadRing::NO_MEMORY: return nomem("the upload ring");
    case UploadRing::NO_EVENT: return hip_fail(hipErrorInvalidValue, "scene_fir_enable: hipEventCreate");
    case UploadRing::OK: break;
    }
    m->clock.arm(tot_steps_);
    fir_ = m.release();
    return PBSO_OK;
}

int Engine::scene_fir_set(const float *taps, const int *onset) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_set: the scene filter mix is not enabled");
    if (!taps) return fail(PBSO_ERR_INVALID, "scene_fir_set: taps is NULL");
    SceneFir &m = *fir_;
    if (!m.sched.empty()) return fail(PBSO_ERR_STATE, "scene_fir_set: scheduled sets are pending (pbso_scene_fir_clear_schedule drops them)");
    if (m.fade.fading(m.clock.t))
        return fail(PBSO_ERR_STATE, "scene_fir_set: the cross-fade of the last set is still running (pbso_scene_fir_info tells when it ends)");
    const size_t nt = m.taps_floats();
    for (size_t i = 0; i < nt; ++i)
        if (!std::isfinite(taps[i])) return fail(PBSO_ERR_INVALID, "scene_fir_set: a tap is not finite");
    if (onset)
        for (int o = 0; o < m.N; ++o)
            if (onset[o] < 0 || onset[o] > m.max_onset) return fail(PBSO_ERR_INVALID, "scene_fir_set: an onset is outside [0, max_onset]");
    // takes effect at the first sample of the next mixed step; onset NULL keeps the onsets last set (0 at first)
    if (onset) m.pend_onset.assign(onset, onset + m.N);
    else if (!m.fade.pending) m.pend_onset = m.onset_to;
    m.pend_taps.assign(taps, taps + nt);
    m.pend_J = 0;
    m.fade.pending = true;
    ++m.n_sets;
    return PBSO_OK;
}

int Engine::scene_fir(void *d_out) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir: the scene filter mix is not enabled");
    SceneFir &m = *fir_;
    if (!last_audio_ || last_nb_ <= 0) return fail(PBSO_ERR_STATE, "scene_fir: no step yet");
    if (host_step_ == tot_steps_) return fail(PBSO_ERR_STATE, "scene_fir: the last step went to host memory (pbso_step_to_host): its rows are not on the device");
    if (const int order = m.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    HIPTRY(hipSetDevice(desc_.device));
    const long long n = (long long)last_nb_ * B_;
    const int groups = mix_objects_groups(m.N);
    // a step with scheduled sets inside it (none lies before it) goes to the schedule's kernels; any other is launched as ever
    if ((!m.sched.empty() && m.sched.front().t < m.clock.t + n) ||
        (m.delay && !m.delay->sched.empty() && m.delay->sched.front().t < m.clock.t + n))
        return scene_fir_scheduled_step(d_out);
    float *out;
    GROWTRY(m.out.resolve(d_out, (size_t)m.C * n, stream_, out), "scene_fir: cannot allocate the output", "scene_fir: output");
    GROWTRY(grow(m.parts, (size_t)2 * m.C * groups * n, stream_), "scene_fir: cannot allocate the partial rows", "scene_fir: partial rows");
    XFade &f = m.fade;
    const long long t = m.clock.t;
    if (f.pending) {
        // the new set goes where the predecessor of the set in force was (the device copies are ordered behind the previous mix
        // on the stream)
        char *h_up;
        HIPTRY(m.up.acquire(h_up));
        const size_t ob = (size_t)m.N * sizeof(int);
        const int dst = f.incoming();
        if (m.pend_J > 0) {
            // a bank set: its pairs go up instead of taps, and the taps are built where they are read (d_raw is not used)
            const int J = m.pend_J, hdr[2] = {0, J};
            const size_t ib = (size_t)m.N * J * sizeof(int), bb = SceneFir::bank_set_bytes(m.N, J);
            std::memcpy(h_up, hdr, sizeof(hdr));
            std::memcpy(h_up + sizeof(hdr), m.pend_index.data(), ib);
            std::memcpy(h_up + sizeof(hdr) + ib, m.pend_weight.data(), (size_t)m.N * J * sizeof(float));
            std::memcpy(h_up + bb, m.pend_onset.data(), ob);
            HIPTRY(hipMemcpyAsync(m.d_bset, h_up, bb, hipMemcpyHostToDevice, stream_));
            HIPTRY(hipMemcpyAsync(m.d_onset[dst], h_up + bb, ob, hipMemcpyHostToDevice, stream_));
            HIPTRY(m.up.record(stream_));
            const int prc = launch_scene_fir_bank_prepare(m.d_bank, (const int *)m.d_bset.p, (const int *)(m.d_bset.p + sizeof(hdr)),
                                                          (const float *)(m.d_bset.p + sizeof(hdr) + ib), 1, J, m.N, m.C, m.K, m.d_P[dst], stream_);
            if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_fir_bank_prepare");
        } else {
            const size_t tb = m.taps_floats() * sizeof(float);
            std::memcpy(h_up, m.pend_taps.data(), tb);
            std::memcpy(h_up + tb, m.pend_onset.data(), ob);
            HIPTRY(hipMemcpyAsync(m.d_raw, h_up, tb, hipMemcpyHostToDevice, stream_));
            HIPTRY(hipMemcpyAsync(m.d_onset[dst], h_up + tb, ob, hipMemcpyHostToDevice, stream_));
            HIPTRY(m.up.record(stream_));
            const int prc = launch_scene_fir_prepare(m.d_raw, (long long)m.C * m.N, m.K, m.d_P[dst], stream_);
            if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_fir_prepare");
        }
        m.onset_from.swap(m.onset_to);
        m.onset_to = m.pend_onset;
        f.swap_in(t);
    }
    const long long n_fade = f.n_fade(t, n);
    const int to = f.to_idx, from = to ^ 1;
    // (a set -- of filters above, of delays below -- is taken up before the launch: should the launch fail, the set has taken
    //  effect on the host and is not pending again; the caller's way on from a failed mix is the reset)
    FirDelay *d = m.delay.get();
    if (d && d->have_pend) {                             // the set takes effect at t, by the scene mix's rule
        HIPTRY(d->refresh());                            // (after a drained schedule: from the value it left, mid-ramp included)
        for (int o = 0; o < m.N; ++o) ramp_set(d->p[o], d->pend[o], t, d->ramp, d->any_set);
        d->ramping = d->any_set && d->ramp > 0;
        d->t_set = t;
        d->any_set = d->dirty = true;
        d->have_pend = false;
    }
    if (d && d->dirty) {
        char *h_p;
        HIPTRY(d->up.acquire(h_p));
        const size_t bytes = d->p.size() * sizeof(SceneParam);
        std::memcpy(h_p, d->p.data(), bytes);
        HIPTRY(hipMemcpyAsync(d->d_p, h_p, bytes, hipMemcpyHostToDevice, stream_));
        HIPTRY(d->up.record(stream_));
        d->dirty = false;
    }
    const float *P_to = f.have_to ? m.d_P[to].p : nullptr, *P_from = n_fade ? m.d_P[from].p : nullptr;
    const int *on_from = n_fade ? m.d_onset[from].p : nullptr;
    // a mixer without the delay stage is launched as it always was
    const int lrc = d ? launch_scene_fir_delay(last_audio_, m.N, n, m.hist.cur(), m.hist.next(), m.H, d->hist_x.cur(), d->hist_x.next(), d->Hx,
                                               d->d_p, d->ramp, P_to, P_from, m.d_onset[to], on_from, m.C, m.K, n_fade, t, f.t_set, f.R,
                                               m.parts, out, stream_)
                      : launch_scene_fir(last_audio_, m.N, n, m.hist.cur(), m.hist.next(), m.H, P_to, P_from, m.d_onset[to], on_from, m.C, m.K,
                                         n_fade, t, f.t_set, f.R, m.parts, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, d ? "launch_scene_fir_delay" : "launch_scene_fir");
    if (d) d->hist_x.flip();
    m.hist.flip();
    m.clock.advance(n, tot_steps_);
    ++m.n_mixes;
    m.out.wrote(out, last_nb_);
    return PBSO_OK;
}

int Engine::read_scene_fir(float *out, size_t n) { return read_bus(fir_ ? &fir_->out : nullptr, fir_ ? fir_->C : 0, WORDS, out, n); }

// the history back to silence, t back to 0, the filters gone: silence until the next set, which takes effect without a fade.
// Armed for the next step.
int Engine::scene_fir_reset() {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_reset: the scene filter mix is not enabled");
    SceneFir &m = *fir_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(m.hist.reset(stream_));
    m.sched.clear();                                     // (the schedule is dropped: the delays last IN FORCE stay)
    if (FirDelay *d = m.delay.get()) {                   // both histories; the delays stay at their targets, ramps finished
        HIPTRY(d->refresh());
        HIPTRY(d->hist_x.reset(stream_));
        d->sched.clear();
        if (d->have_pend)
            for (int o = 0; o < m.N; ++o) d->p[o].to = d->pend[o];
        for (SceneParam &q : d->p) ramp_settle(q);
        d->have_pend = d->any_set = d->ramping = false;
        d->dirty = true;
        d->t_set = 0;
    }
    m.onset_to.assign(m.N, 0);
    m.onset_from.assign(m.N, 0);
    m.fade.reset();
    m.clock.reset(tot_steps_);
    return PBSO_OK;
}

int Engine::scene_fir_info(int64_t out[4]) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_info: the scene filter mix is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_fir_info: out is NULL");
    const SceneFir &m = *fir_;
    out[0] = m.clock.t;
    out[1] = m.fade.fade_end(m.clock.t);
    out[2] = m.n_mixes;
    out[3] = m.n_sets;
    return PBSO_OK;
}

// The delay stage: before the first mix only (the history kept so far is of x, and becomes the history of z = x under the
// delays of 0 that hold until the first set).
int Engine::scene_fir_delay_enable(int max_delay, int ramp) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_delay_enable: the scene filter mix is not enabled");
    if (max_delay < 0 || max_delay > (1 << 20) || ramp < 0 || ramp > (1 << 20))
        return fail(PBSO_ERR_INVALID, "scene_fir_delay_enable: max_delay and ramp_samples must be 0 .. 1 << 20");
    SceneFir &m = *fir_;
    if (m.clock.t != 0) return fail(PBSO_ERR_STATE, "scene_fir_delay_enable: the mixer has mixed already (pbso_scene_fir_reset starts over)");
    HIPTRY(hipSetDevice(desc_.device));
    if (m.delay) {                                       // (a second enable replaces the first: nothing is in flight on its memory at t == 0 but a memset)
        if (stream_) (void)hipStreamSynchronize(stream_);
        m.delay.reset();
    }
    std::unique_ptr<FirDelay> d(new FirDelay());
    d->max_delay = max_delay;
    d->ramp = ramp;
    d->Hx = max_delay + 1;
    d->p.assign(std::max(m.N, 1), SceneParam{0.0, 0.0, 0, 0.0});
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("scene_fir_delay_enable: cannot allocate ") + what);
    };
    if (d->hist_x.create((size_t)m.N * d->Hx, stream_) != hipSuccess) return nomem("the history");
    if (d->d_p.alloc(d->p.size()) != hipSuccess) return nomem("the delays");
    switch (d->up.create(d->p.size() * sizeof(SceneParam))) {
    case UploadRing::NO_MEMORY: return nomem("the delays");
    case UploadRing::NO_EVENT: return hip_fail(hipErrorInvalidValue, "scene_fir_delay_enable: hipEventCreate");
    case UploadRing::OK: break;
    }
    if (hipHostMalloc((void **)&d->p_back, d->p.size() * sizeof(SceneParam), hipHostMallocDefault) != hipSuccess) {
        d->p_back = nullptr;
        return nomem("the delays");
    }
    if (hipEventCreateWithFlags(&d->ev_back, hipEventDisableTiming) != hipSuccess) {
        d->ev_back = nullptr;
        return hip_fail(hipErrorInvalidValue, "scene_fir_delay_enable: hipEventCreate");
    }
    m.delay = std::move(d);
    return PBSO_OK;
}

int Engine::scene_fir_set_delay(const float *delay) {
    if (!fir_ || !fir_->delay) return fail(PBSO_ERR_STATE, "scene_fir_set_delay: the delay stage is not enabled (pbso_scene_fir_delay_enable)");
    if (!delay) return fail(PBSO_ERR_INVALID, "scene_fir_set_delay: delay is NULL");
    FirDelay &d = *fir_->delay;
    if (!d.sched.empty()) return fail(PBSO_ERR_STATE, "scene_fir_set_delay: scheduled sets are pending (pbso_scene_fir_clear_schedule drops them)");
    for (int o = 0; o < fir_->N; ++o)
        if (!(std::isfinite(delay[o]) && delay[o] >= 0.f && delay[o] <= (float)d.max_delay))
            return fail(PBSO_ERR_INVALID, "scene_fir_set_delay: a delay is not finite or outside [0, max_delay]");
    // takes effect at the first sample of the next mixed step, whatever the filter sets' cross-fade is doing
    d.pend.assign(delay, delay + fir_->N);
    d.have_pend = true;
    ++d.n_sets;
    return PBSO_OK;
}

int Engine::scene_fir_delay_info(int64_t out[4]) {
    if (!fir_ || !fir_->delay) return fail(PBSO_ERR_STATE, "scene_fir_delay_info: the delay stage is not enabled (pbso_scene_fir_delay_enable)");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_fir_delay_info: out is NULL");
    const FirDelay &d = *fir_->delay;
    out[0] = d.max_delay;
    out[1] = d.ramp;
    out[2] = d.ramp_end(fir_->clock.t);
    out[3] = d.n_sets;
    return PBSO_OK;
}

// ---- the schedule

// what a scheduled filter set comes behind: the last pending one, else a plain set waiting for the next mix (it takes effect at
// the clock), else the set in force.  floor: the smallest t_set that is not before the clock and ascending.
struct FirPredecessor { bool have; long long t, floor; };
static FirPredecessor fir_predecessor(const SceneFir &m) {
    if (!m.sched.empty()) return {true, m.sched.back().t, m.sched.back().t + 1};
    if (m.fade.pending) return {true, m.clock.t, m.clock.t + 1};
    return {m.fade.have_to, m.fade.t_set, m.clock.t};
}
// why the times of n_sets scheduled filter sets (taps or bank sets: one kind, one pending list) are refused; nullptr: they pass
static const char *fir_times_refused(const SceneFir &m, int n_sets, const int64_t *t_set) {
    FirPredecessor prev = fir_predecessor(m);
    for (int k = 0; k < n_sets; ++k) {
        const long long t = (long long)t_set[k];
        if (t < m.clock.t) return ": a t_set lies before the next mixed sample";
        if (t < prev.floor) return ": the t_set are not ascending behind the last pending set's";
        if (prev.have && !fir_spacing_ok(t, prev.t, m.fade.R))
            return ": a t_set lies inside the cross-fade of the set before it (pbso_scene_fir_schedule_info tells the first that may follow)";
        prev = {true, t, t + 1};
    }
    return nullptr;
}
static long long fir_delay_floor(const SceneFir &m, const FirDelay &d) {
    return !d.sched.empty() ? d.sched.back().t + 1 : (d.have_pend ? m.clock.t + 1 : m.clock.t);
}

// n_sets filter sets at the absolute samples t_set, taps [n_sets][C][N][K], onset [n_sets][N] or NULL (unchanged by all of them);
// `call` names the entry point in the messages.  All of them are checked before the first is taken.
int Engine::scene_fir_schedule(const char *call, int n_sets, const int64_t *t_set, const float *taps, const int *onset) {
    const std::string name(call);
    if (!fir_) return fail(PBSO_ERR_STATE, name + ": the scene filter mix is not enabled");
    if (n_sets < 0) return fail(PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set) return fail(PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!taps) return fail(PBSO_ERR_INVALID, name + ": taps is NULL");
    SceneFir &m = *fir_;
    if (const char *why = fir_times_refused(m, n_sets, t_set)) return fail(PBSO_ERR_INVALID, name + why);
    const size_t nt = m.taps_floats();
    for (size_t i = 0; i < (size_t)n_sets * nt; ++i)
        if (!std::isfinite(taps[i])) return fail(PBSO_ERR_INVALID, name + ": a tap is not finite");
    if (onset)
        for (size_t i = 0; i < (size_t)n_sets * m.N; ++i)
            if (onset[i] < 0 || onset[i] > m.max_onset) return fail(PBSO_ERR_INVALID, name + ": an onset is outside [0, max_onset]");
    std::deque<SceneFir::Pending> taken;                 // (built apart: a failed allocation leaves the pending list as it was)
    // onset NULL keeps the onsets of the set before (0 at first)
    const std::vector<int> *on_prev = !m.sched.empty() ? &m.sched.back().onset : (m.fade.pending ? &m.pend_onset : &m.onset_to);
    for (int k = 0; k < n_sets; ++k) {
        SceneFir::Pending q{(long long)t_set[k], {}, {}};
        q.taps.assign(taps + (size_t)k * nt, taps + (size_t)(k + 1) * nt);
        if (onset) q.onset.assign(onset + (size_t)k * m.N, onset + (size_t)(k + 1) * m.N);
        else q.onset = *on_prev;
        taken.push_back(std::move(q));
        on_prev = &taken.back().onset;
    }
    for (SceneFir::Pending &q : taken) m.sched.push_back(std::move(q));
    m.n_sets += n_sets;
    return PBSO_OK;
}

int Engine::scene_fir_delay_schedule(const char *call, int n_sets, const int64_t *t_set, const float *delay) {
    const std::string name(call);
    if (!fir_ || !fir_->delay) return fail(PBSO_ERR_STATE, name + ": the delay stage is not enabled (pbso_scene_fir_delay_enable)");
    if (n_sets < 0) return fail(PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set) return fail(PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!delay) return fail(PBSO_ERR_INVALID, name + ": delay is NULL");
    SceneFir &m = *fir_;
    FirDelay &d = *m.delay;
    long long floor = fir_delay_floor(m, d);
    for (int k = 0; k < n_sets; ++k) {
        const long long t = (long long)t_set[k];
        if (t < m.clock.t) return fail(PBSO_ERR_INVALID, name + ": a t_set lies before the next mixed sample");
        if (t < floor) return fail(PBSO_ERR_INVALID, name + ": the t_set are not ascending behind the last pending set's");
        floor = t + 1;
    }
    for (size_t i = 0; i < (size_t)n_sets * m.N; ++i)
        if (!(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)d.max_delay))
            return fail(PBSO_ERR_INVALID, name + ": a delay is not finite or outside [0, max_delay]");
    std::deque<FirDelay::Pending> taken;
    for (int k = 0; k < n_sets; ++k) {
        FirDelay::Pending q{(long long)t_set[k], {}};
        q.v.assign(delay + (size_t)k * m.N, delay + (size_t)(k + 1) * m.N);
        taken.push_back(std::move(q));
    }
    for (FirDelay::Pending &q : taken) d.sched.push_back(std::move(q));
    d.n_sets += n_sets;
    return PBSO_OK;
}

int Engine::scene_fir_clear_schedule() {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_clear_schedule: the scene filter mix is not enabled");
    fir_->sched.clear();
    if (fir_->delay) fir_->delay->sched.clear();
    return PBSO_OK;
}

int Engine::scene_fir_schedule_info(int64_t out[4]) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_schedule_info: the scene filter mix is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_fir_schedule_info: out is NULL");
    const SceneFir &m = *fir_;
    const FirPredecessor prev = fir_predecessor(m);
    out[0] = m.clock.t;
    out[1] = (int64_t)m.sched.size();
    out[2] = m.delay ? (int64_t)m.delay->sched.size() : 0;
    out[3] = fir_next_t_min(prev.floor, prev.have, prev.t, m.fade.R);
    return PBSO_OK;
}

// ---- the bank

// F filters of [C][K] taps, on the device from here on.  A second create replaces the first, unless bank sets are waiting for it.
int Engine::scene_fir_bank_create(int F, const float *taps) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_bank_create: the scene filter mix is not enabled");
    if (F < 1 || F > SCENE_FIR_BANK_MAX_FILTERS) return fail(PBSO_ERR_INVALID, "scene_fir_bank_create: n_filters must be 1 .. 1 << 20");
    if (!taps) return fail(PBSO_ERR_INVALID, "scene_fir_bank_create: taps is NULL");
    SceneFir &m = *fir_;
    if ((long long)m.N * (m.LP / 4) > 0x7fffffffLL)
        return fail(PBSO_ERR_INVALID, "scene_fir_bank_create: n_objects * LP / 4 does not fit 31 bits");
    if (m.bank_sets_pending()) return fail(PBSO_ERR_STATE, "scene_fir_bank_create: bank sets are pending (pbso_scene_fir_clear_schedule drops the scheduled ones)");
    const size_t nf = (size_t)F * m.C * m.K;
    double A = 0.0;
    for (size_t i = 0; i < nf; ++i) {
        if (!std::isfinite(taps[i])) return fail(PBSO_ERR_INVALID, "scene_fir_bank_create: a tap is not finite");
        A = std::max(A, (double)std::fabs(taps[i]));
    }
    HIPTRY(hipSetDevice(desc_.device));
    auto nomem = [&]() {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, "scene_fir_bank_create: cannot allocate the bank");
    };
    DevMem<float> bank;
    if (bank.alloc(nf) != hipSuccess) return nomem();
    if (!m.d_bset.p && m.d_bset.alloc(SceneFir::bank_set_bytes(std::max(m.N, 1), SCENE_FIR_BANK_MAX_J)) != hipSuccess) return nomem();
    // (behind whatever still reads the bank replaced; it is freed once the stream is idle)
    HIPTRY(hipMemcpyAsync(bank.p, taps, nf * sizeof(float), hipMemcpyHostToDevice, stream_));
    HIPTRY(hipStreamSynchronize(stream_));
    std::swap(m.d_bank.p, bank.p);
    std::swap(m.d_bank.cap, bank.cap);
    m.bank_F = F;
    m.bank_A = A;
    return PBSO_OK;
}

int Engine::scene_fir_bank_info(int64_t out[4]) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_bank_info: the scene filter mix is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_fir_bank_info: out is NULL");
    const SceneFir &m = *fir_;
    out[0] = m.bank_F;
    out[1] = SCENE_FIR_BANK_MAX_J;
    out[2] = m.n_bank_sets;
    out[3] = (int64_t)((size_t)m.bank_F * m.C * m.K * sizeof(float));
    return PBSO_OK;
}

// n_sets bank sets: index / weight [n_sets][N][J], onset [n_sets][N] or NULL.  `plain`: the plain set (n_sets is 1, no t_set), which
// waits for the next mix by pbso_scene_fir_set's rules; else scheduled ones, by pbso_scene_fir_schedule's.  From the checks on a
// bank set is a filter set like any other.  All of them are checked before the first is taken.
int Engine::scene_fir_bank_sets(const char *call, bool plain, int n_sets, const int64_t *t_set, int J, const int *index, const float *weight, const int *onset) {
    const std::string name(call);
    if (!fir_) return fail(PBSO_ERR_STATE, name + ": the scene filter mix is not enabled");
    SceneFir &m = *fir_;
    if (!m.d_bank.p) return fail(PBSO_ERR_STATE, name + ": no bank (pbso_scene_fir_bank_create)");
    if (n_sets < 0) return fail(PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!plain && !t_set) return fail(PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!index) return fail(PBSO_ERR_INVALID, name + ": index is NULL");
    if (!weight) return fail(PBSO_ERR_INVALID, name + ": weight is NULL");
    if (J < 1 || J > SCENE_FIR_BANK_MAX_J) return fail(PBSO_ERR_INVALID, name + ": J must be 1 .. 8");
    if (plain) {
        if (!m.sched.empty()) return fail(PBSO_ERR_STATE, name + ": scheduled sets are pending (pbso_scene_fir_clear_schedule drops them)");
        if (m.fade.fading(m.clock.t))
            return fail(PBSO_ERR_STATE, name + ": the cross-fade of the last set is still running (pbso_scene_fir_info tells when it ends)");
    } else if (const char *why = fir_times_refused(m, n_sets, t_set))
        return fail(PBSO_ERR_INVALID, name + why);
    const size_t np = (size_t)m.N * J;                   // pairs of one set
    for (size_t r = 0; r < (size_t)n_sets * m.N; ++r) {  // one object of one set
        double sum = 0.0;
        for (int j = 0; j < J; ++j) {
            const int i = index[r * J + j];
            const float w = weight[r * J + j];
            if (i < 0 || i >= m.bank_F) return fail(PBSO_ERR_INVALID, name + ": an index is outside [0, n_filters)");
            if (!std::isfinite(w)) return fail(PBSO_ERR_INVALID, name + ": a weight is not finite");
            sum += std::fabs((double)w);
        }
        // every partial sum of the chain and every tap stay finite
        if (!(sum * m.bank_A <= (double)FLT_MAX))
            return fail(PBSO_ERR_INVALID, name + ": an object's sum of |weight| times the bank's largest |tap| exceeds FLT_MAX");
    }
    if (onset)
        for (size_t i = 0; i < (size_t)n_sets * m.N; ++i)
            if (onset[i] < 0 || onset[i] > m.max_onset) return fail(PBSO_ERR_INVALID, name + ": an onset is outside [0, max_onset]");
    if (plain) {
        // takes effect at the first sample of the next mixed step; onset NULL keeps the onsets last set (0 at first)
        if (onset) m.pend_onset.assign(onset, onset + m.N);
        else if (!m.fade.pending) m.pend_onset = m.onset_to;
        m.pend_index.assign(index, index + np);
        m.pend_weight.assign(weight, weight + np);
        m.pend_J = J;
        m.pend_taps.clear();
        m.fade.pending = true;
    } else {
        std::deque<SceneFir::Pending> taken;             // (built apart: a failed allocation leaves the pending list as it was)
        const std::vector<int> *on_prev = !m.sched.empty() ? &m.sched.back().onset : (m.fade.pending ? &m.pend_onset : &m.onset_to);
        for (int k = 0; k < n_sets; ++k) {
            SceneFir::Pending q{(long long)t_set[k], {}, {}};
            q.J = J;
            q.index.assign(index + (size_t)k * np, index + (size_t)(k + 1) * np);
            q.weight.assign(weight + (size_t)k * np, weight + (size_t)(k + 1) * np);
            if (onset) q.onset.assign(onset + (size_t)k * m.N, onset + (size_t)(k + 1) * m.N);
            else q.onset = *on_prev;
            taken.push_back(std::move(q));
            on_prev = &taken.back().onset;
        }
        for (SceneFir::Pending &q : taken) m.sched.push_back(std::move(q));
    }
    m.n_sets += n_sets;
    m.n_bank_sets += n_sets;
    return PBSO_OK;
}

// A step with scheduled sets inside it.  A plain set still waiting for this mix takes effect at the step's first sample: it goes
// in front of the scheduled ones (which lie behind it) as one more set of its kind.  Everything that can refuse comes before
// anything is taken or launched.
int Engine::scene_fir_scheduled_step(void *d_out) {
    SceneFir &m = *fir_;
    FirDelay *d = m.delay.get();
    XFade &f = m.fade;
    const long long n = (long long)last_nb_ * B_, t = m.clock.t;
    const int groups = mix_objects_groups(m.N);
    size_t Ss = 0, Ks = 0;                               // the scheduled sets inside the step
    while (Ss < m.sched.size() && m.sched[Ss].t < t + n) ++Ss;
    if (d) while (Ks < d->sched.size() && d->sched[Ks].t < t + n) ++Ks;
    const size_t S = Ss + (f.pending ? 1 : 0), Kd = Ks + (d && d->have_pend ? 1 : 0);
    if (S > (size_t)SCENE_FIR_MAX_SETS_PER_STEP)
        return fail(PBSO_ERR_INVALID, "scene_fir: more than 4096 filter sets take effect inside this step (step in shorter pieces, or pbso_scene_fir_clear_schedule)");
    if (Kd > (size_t)SCENE_MAX_SETS_PER_STEP)
        return fail(PBSO_ERR_INVALID, "scene_fir: more than 65536 delay sets take effect inside this step (step in shorter pieces, or pbso_scene_fir_clear_schedule)");
    // the step's times and its work strips
    std::vector<long long> t_f, t_d;
    if (f.pending) t_f.push_back(t);
    for (size_t k = 0; k < Ss; ++k) t_f.push_back(m.sched[k].t);
    if (d && d->have_pend) t_d.push_back(t);
    for (size_t k = 0; k < Ks; ++k) t_d.push_back(d->sched[k].t);
    const int strip = scene_fir_sched_strip(n, m.N);
    std::vector<FirSegment> segs;
    std::vector<FirStrip> strips;
    fir_segments(t, n, (int)S, t_f.data(), f.have_to, f.have_from, f.t_set, segs);
    fir_strips(segs, t, f.R, strip, strips);
    bool any_from = false;
    for (const FirStrip &e : strips) any_from = any_from || e.set_from >= 0;
    // which of the step's sets are bank sets (the others bring taps), and the widest of those
    std::vector<const SceneFir::Pending *> sets;         // of the step, in order; nullptr: the plain set waiting for this mix
    if (f.pending) sets.push_back(nullptr);
    for (size_t k = 0; k < Ss; ++k) sets.push_back(&m.sched[k]);
    auto J_of = [&](size_t k) { return sets[k] ? sets[k]->J : m.pend_J; };
    size_t Sb = 0;
    int Jmax = 0;
    for (size_t k = 0; k < S; ++k)
        if (J_of(k) > 0) {
            ++Sb;
            Jmax = std::max(Jmax, J_of(k));
        }
    const size_t St = S - Sb;
    // one staged block: filter times | delay times | strips | onsets [S][N] | delays [K_d][N] | of the S_b bank sets: (pool slot, J)
    // [S_b][2], index [S_b][N][Jmax], weight [S_b][N][Jmax] | taps [S_t][C][N][K] of the others
    const size_t cn = (size_t)m.C * m.N, nt = m.taps_floats(), set_floats = cn * m.LP, npair = (size_t)m.N * Jmax;
    const size_t off_td = S * sizeof(long long), off_strips = off_td + Kd * sizeof(long long),
                 off_on = off_strips + strips.size() * sizeof(FirStrip), off_dl = off_on + S * m.N * sizeof(int),
                 off_hdr = off_dl + Kd * m.N * sizeof(float), off_ix = off_hdr + Sb * 2 * sizeof(int), off_w = off_ix + Sb * npair * sizeof(int),
                 off_taps = off_w + Sb * npair * sizeof(float), set_bytes = off_taps + St * nt * sizeof(float);
    char *h_sets = nullptr;
    GROWTRY(grow(m.d_sets, set_bytes, stream_), "scene_fir: cannot allocate the step's scheduled sets", "scene_fir: scheduled sets");
    GROWTRY(grow(m.d_pool, (S + 2) * set_floats, stream_), "scene_fir: cannot allocate the step's pool of filter sets", "scene_fir: filter pool");
    GROWTRY(grow(m.d_onpool, (S + 2) * (size_t)m.N, stream_), "scene_fir: cannot allocate the step's pool of filter sets", "scene_fir: onset pool");
    if (d) GROWTRY(grow(d->d_rec, (Kd + 1) * d->p.size(), stream_), "scene_fir: cannot allocate the step's delay records", "scene_fir: delay records");
    GROWTRY(m.stage.acquire(set_bytes, h_sets), "scene_fir: cannot allocate the staging of the step's scheduled sets", "scene_fir: staging");
    float *out;
    GROWTRY(m.out.resolve(d_out, (size_t)m.C * n, stream_, out), "scene_fir: cannot allocate the output", "scene_fir: output");
    GROWTRY(grow(m.parts, (size_t)2 * m.C * groups * n, stream_), "scene_fir: cannot allocate the partial rows", "scene_fir: partial rows");
    if (d) HIPTRY(d->refresh());
    // nothing refuses from here on
    std::memcpy(h_sets, t_f.data(), S * sizeof(long long));
    std::memcpy(h_sets + off_td, t_d.data(), Kd * sizeof(long long));
    std::memcpy(h_sets + off_strips, strips.data(), strips.size() * sizeof(FirStrip));
    std::vector<const std::vector<int> *> onsets;        // of the step's sets, in order
    {
        size_t k = 0, kt = 0, kb = 0;                    // sets, and those with taps / from the bank among them
        for (; k < S; ++k) {
            const SceneFir::Pending *q = sets[k];
            onsets.push_back(q ? &q->onset : &m.pend_onset);
            const int J = J_of(k);
            if (J == 0) {
                std::memcpy(h_sets + off_taps + (kt++) * nt * sizeof(float), (q ? q->taps : m.pend_taps).data(), nt * sizeof(float));
                continue;
            }
            // pool slot 2 + k; the J pairs of an object in a row of Jmax (the rest is not read)
            const int hdr[2] = {(int)(2 + k), J}, *ix = (q ? q->index : m.pend_index).data();
            const float *w = (q ? q->weight : m.pend_weight).data();
            std::memcpy(h_sets + off_hdr + kb * sizeof(hdr), hdr, sizeof(hdr));
            int *h_ix = (int *)(h_sets + off_ix) + kb * npair;
            float *h_w = (float *)(h_sets + off_w) + kb * npair;
            for (int o = 0; o < m.N; ++o)
                for (int j = 0; j < Jmax; ++j) {
                    h_ix[(size_t)o * Jmax + j] = j < J ? ix[(size_t)o * J + j] : 0;
                    h_w[(size_t)o * Jmax + j] = j < J ? w[(size_t)o * J + j] : 0.f;
                }
            ++kb;
        }
        for (k = 0; k < S; ++k) std::memcpy(h_sets + off_on + k * m.N * sizeof(int), onsets[k]->data(), (size_t)m.N * sizeof(int));
        k = 0;
        if (d && d->have_pend) std::memcpy(h_sets + off_dl + (k++) * m.N * sizeof(float), d->pend.data(), (size_t)m.N * sizeof(float));
        for (size_t i = 0; i < Ks; ++i, ++k) std::memcpy(h_sets + off_dl + k * m.N * sizeof(float), d->sched[i].v.data(), (size_t)m.N * sizeof(float));
    }
    HIPTRY(hipMemcpyAsync(m.d_sets, h_sets, set_bytes, hipMemcpyHostToDevice, stream_));
    HIPTRY(m.stage.record(stream_));
    // the pool: 0 / 1 the sets the step begins with, 2 + k its own, prepared in one launch
    const int to = f.to_idx, from = to ^ 1;
    const size_t on_bytes = (size_t)m.N * sizeof(int);
    if (f.have_to) {
        HIPTRY(hipMemcpyAsync(m.d_pool, m.d_P[to], set_floats * sizeof(float), hipMemcpyDeviceToDevice, stream_));
        HIPTRY(hipMemcpyAsync(m.d_onpool, m.d_onset[to], on_bytes, hipMemcpyDeviceToDevice, stream_));
    }
    if (f.have_to && f.fading(t)) {
        HIPTRY(hipMemcpyAsync(m.d_pool.p + set_floats, m.d_P[from], set_floats * sizeof(float), hipMemcpyDeviceToDevice, stream_));
        HIPTRY(hipMemcpyAsync(m.d_onpool.p + m.N, m.d_onset[from], on_bytes, hipMemcpyDeviceToDevice, stream_));
    }
    if (S) {
        HIPTRY(hipMemcpyAsync(m.d_onpool.p + 2 * (size_t)m.N, m.d_sets.p + off_on, S * on_bytes, hipMemcpyDeviceToDevice, stream_));
        // the sets that brought taps: one launch per run of consecutive ones (a step without bank sets is one run: the launch
        // it always was); the bank sets: one launch for all of them, each to its slot
        for (size_t k = 0, kt = 0; k < S;) {
            size_t e = k;
            while (e < S && J_of(e) == 0) ++e;
            if (e > k) {
                const int prc = launch_scene_fir_prepare((const float *)(m.d_sets.p + off_taps) + kt * nt, (long long)((e - k) * cn), m.K,
                                                         m.d_pool.p + (2 + k) * set_floats, stream_);
                if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_fir_prepare");
                kt += e - k;
            }
            k = e + (e < S ? 1 : 0);
        }
        if (Sb) {
            const int prc = launch_scene_fir_bank_prepare(m.d_bank, (const int *)(m.d_sets.p + off_hdr), (const int *)(m.d_sets.p + off_ix),
                                                          (const float *)(m.d_sets.p + off_w), (int)Sb, Jmax, m.N, m.C, m.K, m.d_pool, stream_);
            if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_fir_bank_prepare");
        }
    }
    if (d && d->dirty) {
        char *h_p;
        HIPTRY(d->up.acquire(h_p));
        const size_t bytes = d->p.size() * sizeof(SceneParam);
        std::memcpy(h_p, d->p.data(), bytes);
        HIPTRY(hipMemcpyAsync(d->d_p, h_p, bytes, hipMemcpyHostToDevice, stream_));
        HIPTRY(d->up.record(stream_));
        d->dirty = false;
    }
    FirSchedStep a{};
    a.rows = last_audio_; a.n_obj = m.N; a.n = n;
    a.hist = m.hist.cur(); a.hist_next = m.hist.next(); a.H = m.H;
    if (d) {
        a.hist_x = d->hist_x.cur(); a.hist_x_next = d->hist_x.next(); a.Hx = d->Hx;
        a.params = d->d_p; a.rec = d->d_rec; a.t_d = (const long long *)(m.d_sets.p + off_td);
        a.targets = (const float *)(m.d_sets.p + off_dl); a.Kd = (int)Kd; a.Rd = d->ramp; a.any_set = d->any_set ? 1 : 0;
    }
    a.pool = m.d_pool; a.onpool = m.d_onpool; a.t_f = (const long long *)m.d_sets.p; a.S = (int)S;
    a.have_to0 = f.have_to ? 1 : 0; a.have_from0 = f.have_from ? 1 : 0; a.t_set0 = f.t_set;
    a.strips = (const FirStrip *)(m.d_sets.p + off_strips); a.n_strips = (int)strips.size(); a.strip = strip; a.any_from = any_from ? 1 : 0;
    a.C = m.C; a.K = m.K; a.R = f.R; a.t0 = t;
    a.parts = m.parts; a.out = out;
    const int lrc = launch_scene_fir_sched(a, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_fir_sched");
    if (S) {
        // what S plain sets between cut steps would have left: the last set in slot 0, in force; the one before it in slot 1
        const size_t i_to = S + 1, i_from = S >= 2 ? S : 0;
        const bool have_from = S >= 2 || f.have_to;
        HIPTRY(hipMemcpyAsync(m.d_P[0], m.d_pool.p + i_to * set_floats, set_floats * sizeof(float), hipMemcpyDeviceToDevice, stream_));
        HIPTRY(hipMemcpyAsync(m.d_onset[0], m.d_onpool.p + i_to * m.N, on_bytes, hipMemcpyDeviceToDevice, stream_));
        if (have_from) {
            HIPTRY(hipMemcpyAsync(m.d_P[1], m.d_pool.p + i_from * set_floats, set_floats * sizeof(float), hipMemcpyDeviceToDevice, stream_));
            HIPTRY(hipMemcpyAsync(m.d_onset[1], m.d_onpool.p + i_from * m.N, on_bytes, hipMemcpyDeviceToDevice, stream_));
        }
        const std::vector<int> on_to = *onsets[S - 1];
        m.onset_from = S >= 2 ? *onsets[S - 2] : m.onset_to;
        m.onset_to = on_to;
        f.to_idx = 0;
        f.have_from = have_from;
        f.have_to = true;
        f.t_set = t_f[S - 1];
        f.pending = false;
        m.sched.erase(m.sched.begin(), m.sched.begin() + (long)Ss);
    }
    if (d && Kd) {
        // d_p is now the block of the last set; the host's copy follows behind the mix, and is taken over by who next needs it
        HIPTRY(hipMemcpyAsync(d->p_back, d->d_p, d->p.size() * sizeof(SceneParam), hipMemcpyDeviceToHost, stream_));
        HIPTRY(hipEventRecord(d->ev_back, stream_));
        d->p_stale = true;
        d->ramping = (d->any_set || Kd > 1) && d->ramp > 0;
        d->t_set = t_d[Kd - 1];
        d->any_set = true;
        d->have_pend = false;
        d->sched.erase(d->sched.begin(), d->sched.begin() + (long)Ks);
    }
    if (d) d->hist_x.flip();
    m.hist.flip();
    m.clock.advance(n, tot_steps_);
    ++m.n_mixes;
    m.out.wrote(out, last_nb_);
    return PBSO_OK;
}

}  // namespace pbso
