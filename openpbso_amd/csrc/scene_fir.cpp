// The engine's side of the scene filter mix (include/openpbso_amd.h "scene filter mix"; kernels_fir.hip): the two filter sets (the
// one in force and the one faded out) with their onsets, the cross-fade's clock, the history of every object's last samples on
// the device, and the rule that every step is mixed exactly once.  It reads what a step left (last_audio_, last_nb_) and counts
// steps by tot_steps_.  It knows bus_state.h, which holds what the buses have in common (the cross-fade's clock among it), and
// nothing of the other buses.
// The optional delay stage (pbso_scene_fir_delay_enable; kernels_fir_delay.hip) puts the scene mix's ramped fractional delay per
// object in front of the filters: its records, the second history (of x: `hist` then holds z), and the other launch.
#include "bus_state.h"

#include <cmath>
#include <cstring>

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
    // the first t at which every ramp is over; t itself when none runs
    long long ramp_end(long long t) const { return ramping && t - t_set + 1 < (long long)ramp ? t_set + ramp - 1 : t; }
};

struct SceneFir {
    int C = 0, N = 0, K = 0, max_onset = 0, H = 0, LP = 0;          // H = max_onset + K - 1 samples of history per object
    XFade fade;                                          // which set is in force, which is faded out, since when
    std::vector<int> onset_to, onset_from;
    // a set call waits here for the next mix (a later one replaces it)
    std::vector<float> pend_taps;
    std::vector<int> pend_onset;
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
    UploadRing up;                                       // blocks of taps [C][N][K], then onsets [N]

    size_t taps_floats() const { return (size_t)C * N * K; }
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
    switch (m->up.create(cn * K * sizeof(float) + no * sizeof(int))) {
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
        const size_t tb = m.taps_floats() * sizeof(float), ob = (size_t)m.N * sizeof(int);
        std::memcpy(h_up, m.pend_taps.data(), tb);
        std::memcpy(h_up + tb, m.pend_onset.data(), ob);
        const int dst = f.incoming();
        HIPTRY(hipMemcpyAsync(m.d_raw, h_up, tb, hipMemcpyHostToDevice, stream_));
        HIPTRY(hipMemcpyAsync(m.d_onset[dst], h_up + tb, ob, hipMemcpyHostToDevice, stream_));
        HIPTRY(m.up.record(stream_));
        const int prc = launch_scene_fir_prepare(m.d_raw, (long long)m.C * m.N, m.K, m.d_P[dst], stream_);
        if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_fir_prepare");
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
    if (FirDelay *d = m.delay.get()) {                   // both histories; the delays stay at their targets, ramps finished
        HIPTRY(d->hist_x.reset(stream_));
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
    m.delay = std::move(d);
    return PBSO_OK;
}

int Engine::scene_fir_set_delay(const float *delay) {
    if (!fir_ || !fir_->delay) return fail(PBSO_ERR_STATE, "scene_fir_set_delay: the delay stage is not enabled (pbso_scene_fir_delay_enable)");
    if (!delay) return fail(PBSO_ERR_INVALID, "scene_fir_set_delay: delay is NULL");
    FirDelay &d = *fir_->delay;
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

}  // namespace pbso
