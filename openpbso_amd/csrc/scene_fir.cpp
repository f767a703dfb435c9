// The engine's side of the scene filter mix (include/openpbso_amd.h "scene filter mix"; kernels_fir.hip): the two filter sets (the
// one in force and the one faded out) with their onsets, the cross-fade's clock, the history of every object's last samples on
// the device, and the rule that every step is mixed exactly once.  As the scene mixer (scene_mix.cpp), of which it knows nothing,
// it reads what a step left (last_audio_, last_nb_) and counts steps by tot_steps_.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pbso {

struct SceneFir {
    int C = 0, N = 0, K = 0, max_onset = 0, R = 0, H = 0, LP = 0;   // H = max_onset + K - 1 samples of history per object
    // the sets in force: `to` since t_set, cross-faded from `from` over R samples when there was one
    std::vector<int> onset_to, onset_from;
    bool have_to = false, have_from = false;
    int64_t t_set = 0;
    // a set call waits here for the next mix (a later one replaces it)
    std::vector<float> pend_taps;
    std::vector<int> pend_onset;
    bool pending = false;
    int64_t t = 0;                                       // absolute sample of the next mixed step's first sample
    int64_t next_step = 0;                               // the tot_steps_ the next mix must find
    int64_t n_mixes = 0, n_sets = 0;
    float *hist[2] = {nullptr, nullptr};                 // [N][H] the samples before the next step, double-buffered
    int cur = 0;
    float *out = nullptr, *parts = nullptr;              // the engine-owned output [C][n]; partial rows [2][C][groups][n]
    size_t out_cap = 0, parts_cap = 0;
    // on the device: the padded reversed taps [C][N][LP] and onsets [N] of both sets (to = index to_idx), the raw taps of an upload
    float *d_P[2] = {nullptr, nullptr}, *d_raw = nullptr;
    int *d_onset[2] = {nullptr, nullptr};
    int to_idx = 0;
    // pinned staging of the uploads in a ring (taps [C][N][K], then onsets [N]): a caller that sets new filters every step waits
    // for nothing as long as it is less than UP_SLOTS steps ahead of the device
    static constexpr int UP_SLOTS = 3;
    char *h_up[UP_SLOTS] = {};
    hipEvent_t ev_up[UP_SLOTS] = {};
    bool up_used[UP_SLOTS] = {};
    int up_slot = 0;
    const float *last_out = nullptr;                     // where the last mix went
    int last_nb = 0;

    size_t taps_floats() const { return (size_t)C * N * K; }
    // the fade of the sets in force is still running at sample t
    bool fading(int64_t at) const { return have_from && at - t_set + 1 < (int64_t)R; }
};

namespace {

void free_fir(SceneFir *m) {
    for (float *h : m->hist)
        if (h) (void)hipFree(h);
    if (m->out) (void)hipFree(m->out);
    if (m->parts) (void)hipFree(m->parts);
    if (m->d_raw) (void)hipFree(m->d_raw);
    for (int i = 0; i < 2; ++i) {
        if (m->d_P[i]) (void)hipFree(m->d_P[i]);
        if (m->d_onset[i]) (void)hipFree(m->d_onset[i]);
    }
    for (int i = 0; i < SceneFir::UP_SLOTS; ++i) {
        if (m->h_up[i]) (void)hipHostFree(m->h_up[i]);
        if (m->ev_up[i]) (void)hipEventDestroy(m->ev_up[i]);
    }
    delete m;
}

// a device buffer of at least n floats; the old block may still be read by a mix in flight on the stream
hipError_t grow(float *&p, size_t &cap, size_t n, hipStream_t s) {
    if (p && n <= cap) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    e = hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return e;
    }
    cap = n;
    return hipSuccess;
}

}  // namespace

#define HIPTRY(expr)                                                   \
    do {                                                               \
        hipError_t _e = (expr);                                        \
        if (_e != hipSuccess) return hip_fail(_e, #expr);              \
    } while (0)

void Engine::scene_fir_release() {
    if (!fir_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    free_fir(fir_);
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
    SceneFir *m = new SceneFir();
    m->C = C;
    m->N = n_objects();
    m->K = K;
    m->max_onset = max_onset;
    m->R = xfade;
    m->H = max_onset + K - 1;
    m->LP = scene_fir_padded_taps(K);
    m->onset_to.assign(m->N, 0);
    m->onset_from.assign(m->N, 0);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        free_fir(m);
        return fail(PBSO_ERR_NOMEM, std::string("scene_fir_enable: cannot allocate ") + what);
    };
    const size_t hist_floats = std::max<size_t>((size_t)m->N * m->H, 1);
    for (float *&h : m->hist) {
        if (hipMalloc((void **)&h, hist_floats * sizeof(float)) != hipSuccess) { h = nullptr; return nomem("the history"); }
        if (hipMemsetAsync(h, 0, hist_floats * sizeof(float), stream_) != hipSuccess) return nomem("the history");
    }
    const size_t n = (size_t)std::max(last_nb_, 1) * B_;
    if (grow(m->out, m->out_cap, (size_t)C * n, stream_) != hipSuccess) return nomem("the output");
    if (grow(m->parts, m->parts_cap, (size_t)2 * C * mix_objects_groups(m->N) * n, stream_) != hipSuccess) return nomem("the partial rows");
    const size_t cn = std::max<size_t>((size_t)C * m->N, 1);
    for (int i = 0; i < 2; ++i) {
        if (hipMalloc((void **)&m->d_P[i], cn * m->LP * sizeof(float)) != hipSuccess) { m->d_P[i] = nullptr; return nomem("the taps"); }
        if (hipMalloc((void **)&m->d_onset[i], std::max(m->N, 1) * sizeof(int)) != hipSuccess) { m->d_onset[i] = nullptr; return nomem("the onsets"); }
    }
    if (hipMalloc((void **)&m->d_raw, cn * K * sizeof(float)) != hipSuccess) { m->d_raw = nullptr; return nomem("the taps"); }
    const size_t up_bytes = cn * K * sizeof(float) + std::max(m->N, 1) * sizeof(int);
    for (int i = 0; i < SceneFir::UP_SLOTS; ++i) {
        if (hipHostMalloc((void **)&m->h_up[i], up_bytes, hipHostMallocDefault) != hipSuccess) { m->h_up[i] = nullptr; return nomem("the upload ring"); }
        if (hipEventCreateWithFlags(&m->ev_up[i], hipEventDisableTiming) != hipSuccess) {
            m->ev_up[i] = nullptr;
            free_fir(m);
            return hip_fail(hipErrorInvalidValue, "scene_fir_enable: hipEventCreate");
        }
    }
    m->next_step = tot_steps_ + 1;                       // armed for the next step
    fir_ = m;
    return PBSO_OK;
}

int Engine::scene_fir_set(const float *taps, const int *onset) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_set: the scene filter mix is not enabled");
    if (!taps) return fail(PBSO_ERR_INVALID, "scene_fir_set: taps is NULL");
    SceneFir &m = *fir_;
    if (m.fading(m.t))
        return fail(PBSO_ERR_STATE, "scene_fir_set: the cross-fade of the last set is still running (pbso_scene_fir_info tells when it ends)");
    const size_t nt = m.taps_floats();
    for (size_t i = 0; i < nt; ++i)
        if (!std::isfinite(taps[i])) return fail(PBSO_ERR_INVALID, "scene_fir_set: a tap is not finite");
    if (onset)
        for (int o = 0; o < m.N; ++o)
            if (onset[o] < 0 || onset[o] > m.max_onset) return fail(PBSO_ERR_INVALID, "scene_fir_set: an onset is outside [0, max_onset]");
    // takes effect at the first sample of the next mixed step; onset NULL keeps the onsets last set (0 at first)
    if (onset) m.pend_onset.assign(onset, onset + m.N);
    else if (!m.pending) m.pend_onset = m.onset_to;
    m.pend_taps.assign(taps, taps + nt);
    m.pending = true;
    ++m.n_sets;
    return PBSO_OK;
}

int Engine::scene_fir(void *d_out) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir: the scene filter mix is not enabled");
    SceneFir &m = *fir_;
    if (!last_audio_ || last_nb_ <= 0) return fail(PBSO_ERR_STATE, "scene_fir: no step yet");
    if (host_step_ == tot_steps_) return fail(PBSO_ERR_STATE, "scene_fir: the last step went to host memory (pbso_step_to_host): its rows are not on the device");
    if (tot_steps_ < m.next_step) return fail(PBSO_ERR_STATE, "scene_fir: the last step is mixed already (or was taken before the mixer was enabled / reset)");
    if (tot_steps_ > m.next_step)
        return fail(PBSO_ERR_STATE, "scene_fir: a step was not mixed, the history is no longer the audio before this step (pbso_scene_fir_reset starts over)");
    HIPTRY(hipSetDevice(desc_.device));
    const long long n = (long long)last_nb_ * B_;
    const int groups = mix_objects_groups(m.N);
    float *out = (float *)d_out;
    if (!out) {
        hipError_t e = grow(m.out, m.out_cap, (size_t)m.C * n, stream_);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, "scene_fir: cannot allocate the output") : hip_fail(e, "scene_fir: output");
        out = m.out;
    }
    {
        hipError_t e = grow(m.parts, m.parts_cap, (size_t)2 * m.C * groups * n, stream_);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, "scene_fir: cannot allocate the partial rows") : hip_fail(e, "scene_fir: partial rows");
    }
    if (m.pending) {
        // the set in force becomes the one faded out; the new one goes where that one's predecessor was.  (A staging slot is
        // rewritten only once the copy that last read it is done; the device copies are ordered behind the previous mix on the stream.)
        const int k = m.up_slot;
        if (m.up_used[k]) HIPTRY(hipEventSynchronize(m.ev_up[k]));
        const size_t tb = m.taps_floats() * sizeof(float), ob = (size_t)m.N * sizeof(int);
        std::memcpy(m.h_up[k], m.pend_taps.data(), tb);
        std::memcpy(m.h_up[k] + tb, m.pend_onset.data(), ob);
        const int dst = m.have_to ? m.to_idx ^ 1 : m.to_idx;
        HIPTRY(hipMemcpyAsync(m.d_raw, m.h_up[k], tb, hipMemcpyHostToDevice, stream_));
        HIPTRY(hipMemcpyAsync(m.d_onset[dst], m.h_up[k] + tb, ob, hipMemcpyHostToDevice, stream_));
        HIPTRY(hipEventRecord(m.ev_up[k], stream_));
        m.up_used[k] = true;
        m.up_slot = (k + 1) % SceneFir::UP_SLOTS;
        const int prc = launch_scene_fir_prepare(m.d_raw, (long long)m.C * m.N, m.K, m.d_P[dst], stream_);
        if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_fir_prepare");
        m.have_from = m.have_to;                         // (the first set after enable / reset takes effect without a fade)
        m.onset_from.swap(m.onset_to);
        m.onset_to = m.pend_onset;
        m.to_idx = dst;
        m.have_to = true;
        m.t_set = m.t;
        m.pending = false;
    }
    long long n_fade = 0;
    if (m.fading(m.t)) n_fade = std::min<long long>(n, m.t_set + m.R - 1 - m.t);
    const int from = m.to_idx ^ 1;
    const int lrc = launch_scene_fir(last_audio_, m.N, n, m.hist[m.cur], m.hist[m.cur ^ 1], m.H, m.have_to ? m.d_P[m.to_idx] : nullptr,
                                     n_fade ? m.d_P[from] : nullptr, m.d_onset[m.to_idx], n_fade ? m.d_onset[from] : nullptr, m.C, m.K, n_fade,
                                     (long long)m.t, (long long)m.t_set, m.R, m.parts, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_fir");
    m.cur ^= 1;
    m.t += n;
    m.next_step = tot_steps_ + 1;
    ++m.n_mixes;
    m.last_out = out;
    m.last_nb = last_nb_;
    return PBSO_OK;
}

int Engine::read_scene_fir(float *out, size_t n) {
    if (!fir_ || !fir_->last_out) return fail(PBSO_ERR_STATE, "read_scene_fir: no mix yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_scene_fir: host_out is NULL");
    const size_t total = (size_t)fir_->C * fir_->last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_scene_fir size mismatch (n = n_channels * n_buffers * frames_per_buffer)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, fir_->last_out, total * sizeof(float), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

// the history back to silence, t back to 0, the filters gone: silence until the next set, which takes effect without a fade.
// Armed for the next step.
int Engine::scene_fir_reset() {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_reset: the scene filter mix is not enabled");
    SceneFir &m = *fir_;
    HIPTRY(hipSetDevice(desc_.device));
    for (float *h : m.hist) HIPTRY(hipMemsetAsync(h, 0, std::max<size_t>((size_t)m.N * m.H, 1) * sizeof(float), stream_));
    m.onset_to.assign(m.N, 0);
    m.onset_from.assign(m.N, 0);
    m.have_to = m.have_from = m.pending = false;
    m.t = 0;
    m.t_set = 0;
    m.cur = 0;
    m.next_step = tot_steps_ + 1;
    return PBSO_OK;
}

int Engine::scene_fir_info(int64_t out[4]) {
    if (!fir_) return fail(PBSO_ERR_STATE, "scene_fir_info: the scene filter mix is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_fir_info: out is NULL");
    const SceneFir &m = *fir_;
    out[0] = m.t;
    out[1] = m.fading(m.t) ? m.t_set + m.R - 1 : m.t;
    out[2] = m.n_mixes;
    out[3] = m.n_sets;
    return PBSO_OK;
}

}  // namespace pbso
