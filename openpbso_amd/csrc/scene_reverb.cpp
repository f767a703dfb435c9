// The engine's side of the scene reverb (include/openpbso_amd.h "scene reverb"; kernels_reverb.hip): the two tap sets (the one in
// force and the one faded out), the cross-fade's clock, the history of every input channel's last K - 1 samples on the device, and
// the rule that every step is processed exactly once.  Its input is the caller's device buffer, not the step's rows: of a step it
// reads the length only (last_nb_) and counts steps by tot_steps_.  It knows nothing of the two mixers (scene_mix.cpp, scene_fir.cpp).
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pbso {

struct SceneReverb {
    int n_in = 0, n_out = 0, K = 0, R = 0, H = 0, J = 0, LP = 0;     // H = K - 1 samples of history per input channel
    // the sets in force: `to` since t_set, cross-faded from `from` over R samples when there was one
    bool have_to = false, have_from = false;
    int64_t t_set = 0;
    std::vector<float> pend_taps;                        // a set call waits here for the next processed step (a later one replaces it)
    bool pending = false;
    int64_t t = 0;                                       // absolute sample of the next processed step's first sample
    int64_t next_step = 0;                               // the tot_steps_ the next call must find
    int64_t n_calls = 0, n_sets = 0;
    float *hist[2] = {nullptr, nullptr};                 // [n_in][H] the samples before the next step, double-buffered
    int cur = 0;
    float *out = nullptr, *parts = nullptr;              // the engine-owned output [n_out][n]; partial rows [2][n_out][n_in J][n]
    size_t out_cap = 0, parts_cap = 0;
    // on the device: the padded reversed taps [n_out][n_in][J][LP] of both sets (to = index to_idx), the raw taps of an upload
    float *d_P[2] = {nullptr, nullptr}, *d_raw = nullptr;
    int to_idx = 0;
    // pinned staging of the uploads in a ring, each block n_out n_in K floats
    static constexpr int UP_SLOTS = 3;
    float *h_up[UP_SLOTS] = {};
    hipEvent_t ev_up[UP_SLOTS] = {};
    bool up_used[UP_SLOTS] = {};
    int up_slot = 0;
    const float *last_out = nullptr;                     // where the last call wrote
    int last_nb = 0;

    size_t taps_floats() const { return (size_t)n_out * n_in * K; }
    size_t hist_floats() const { return std::max<size_t>((size_t)n_in * H, 1); }
    bool fading(int64_t at) const { return have_from && at - t_set + 1 < (int64_t)R; }
};

namespace {

void free_reverb(SceneReverb *m) {
    for (float *h : m->hist)
        if (h) (void)hipFree(h);
    if (m->out) (void)hipFree(m->out);
    if (m->parts) (void)hipFree(m->parts);
    if (m->d_raw) (void)hipFree(m->d_raw);
    for (float *p : m->d_P)
        if (p) (void)hipFree(p);
    for (int i = 0; i < SceneReverb::UP_SLOTS; ++i) {
        if (m->h_up[i]) (void)hipHostFree(m->h_up[i]);
        if (m->ev_up[i]) (void)hipEventDestroy(m->ev_up[i]);
    }
    delete m;
}

// a device buffer of at least n floats; the old block may still be read by a call in flight on the stream
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

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return x < y + nb && y < x + na;
}

}  // namespace

#define HIPTRY(expr)                                                   \
    do {                                                               \
        hipError_t _e = (expr);                                        \
        if (_e != hipSuccess) return hip_fail(_e, #expr);              \
    } while (0)

void Engine::scene_reverb_release() {
    if (!reverb_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    free_reverb(reverb_);
    reverb_ = nullptr;
}

int Engine::scene_reverb_enable(int n_in, int n_out, int K, int xfade) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "scene_reverb_enable before finalize");
    if (n_in < 1 || n_in > SCENE_MAX_CHANNELS || n_out < 1 || n_out > SCENE_MAX_CHANNELS)
        return fail(PBSO_ERR_INVALID, "scene_reverb_enable: n_in and n_out must be 1 .. 8");
    if (K < 1 || K > SCENE_REVERB_MAX_TAPS) return fail(PBSO_ERR_INVALID, "scene_reverb_enable: n_taps must be 1 .. 1 << 17");
    if (xfade < 0 || xfade > (1 << 20)) return fail(PBSO_ERR_INVALID, "scene_reverb_enable: xfade_samples must be 0 .. 1 << 20");
    HIPTRY(hipSetDevice(desc_.device));
    scene_reverb_release();
    SceneReverb *m = new SceneReverb();
    m->n_in = n_in;
    m->n_out = n_out;
    m->K = K;
    m->R = xfade;
    m->H = K - 1;
    m->J = scene_reverb_segments(K);
    m->LP = scene_reverb_padded_taps(K);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        free_reverb(m);
        return fail(PBSO_ERR_NOMEM, std::string("scene_reverb_enable: cannot allocate ") + what);
    };
    for (float *&h : m->hist) {
        if (hipMalloc((void **)&h, m->hist_floats() * sizeof(float)) != hipSuccess) { h = nullptr; return nomem("the history"); }
        if (hipMemsetAsync(h, 0, m->hist_floats() * sizeof(float), stream_) != hipSuccess) return nomem("the history");
    }
    const size_t rows = (size_t)n_out * n_in * m->J;
    for (float *&p : m->d_P)
        if (hipMalloc((void **)&p, rows * m->LP * sizeof(float)) != hipSuccess) { p = nullptr; return nomem("the taps"); }
    if (hipMalloc((void **)&m->d_raw, m->taps_floats() * sizeof(float)) != hipSuccess) { m->d_raw = nullptr; return nomem("the taps"); }
    for (int i = 0; i < SceneReverb::UP_SLOTS; ++i) {
        if (hipHostMalloc((void **)&m->h_up[i], m->taps_floats() * sizeof(float), hipHostMallocDefault) != hipSuccess) {
            m->h_up[i] = nullptr;
            return nomem("the upload ring");
        }
        if (hipEventCreateWithFlags(&m->ev_up[i], hipEventDisableTiming) != hipSuccess) {
            m->ev_up[i] = nullptr;
            free_reverb(m);
            return hip_fail(hipErrorInvalidValue, "scene_reverb_enable: hipEventCreate");
        }
    }
    m->next_step = tot_steps_ + 1;                       // armed for the next step
    reverb_ = m;
    return PBSO_OK;
}

int Engine::scene_reverb_set(const float *taps) {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb_set: the scene reverb is not enabled");
    if (!taps) return fail(PBSO_ERR_INVALID, "scene_reverb_set: taps is NULL");
    SceneReverb &m = *reverb_;
    if (m.fading(m.t))
        return fail(PBSO_ERR_STATE, "scene_reverb_set: the cross-fade of the last set is still running (pbso_scene_reverb_info tells when it ends)");
    const size_t nt = m.taps_floats();
    for (size_t i = 0; i < nt; ++i)
        if (!std::isfinite(taps[i])) return fail(PBSO_ERR_INVALID, "scene_reverb_set: a tap is not finite");
    m.pend_taps.assign(taps, taps + nt);                 // takes effect at the first sample of the next processed step
    m.pending = true;
    ++m.n_sets;
    return PBSO_OK;
}

int Engine::scene_reverb(const void *d_in, const void *d_add, void *d_out) {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb: the scene reverb is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "scene_reverb: d_in is NULL");
    SceneReverb &m = *reverb_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "scene_reverb: no step yet");
    if (tot_steps_ < m.next_step) return fail(PBSO_ERR_STATE, "scene_reverb: the last step is processed already (or was taken before the reverb was enabled / reset)");
    if (tot_steps_ > m.next_step)
        return fail(PBSO_ERR_STATE, "scene_reverb: a step was not processed, the history is no longer the input before this step (pbso_scene_reverb_reset starts over)");
    const long long n = (long long)last_nb_ * B_;
    if (d_out && overlap(d_in, (size_t)m.n_in * n * sizeof(float), d_out, (size_t)m.n_out * n * sizeof(float)))
        return fail(PBSO_ERR_INVALID, "scene_reverb: d_out overlaps d_in");
    HIPTRY(hipSetDevice(desc_.device));
    float *out = (float *)d_out;
    if (!out) {
        hipError_t e = grow(m.out, m.out_cap, (size_t)m.n_out * n, stream_);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, "scene_reverb: cannot allocate the output") : hip_fail(e, "scene_reverb: output");
        out = m.out;
    }
    {
        // (the rows of the set faded out only where fades are: R < 2 never blends)
        hipError_t e = grow(m.parts, m.parts_cap, (size_t)(m.R > 1 ? 2 : 1) * m.n_out * m.n_in * m.J * n, stream_);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, "scene_reverb: cannot allocate the partial rows") : hip_fail(e, "scene_reverb: partial rows");
    }
    if (m.pending) {
        // the set in force becomes the one faded out; the new one goes where that one's predecessor was.  (A staging slot is
        // rewritten only once the copy that last read it is done; the device copies are ordered behind the previous call on the stream.)
        const int k = m.up_slot;
        if (m.up_used[k]) HIPTRY(hipEventSynchronize(m.ev_up[k]));
        const size_t tb = m.taps_floats() * sizeof(float);
        std::memcpy(m.h_up[k], m.pend_taps.data(), tb);
        const int dst = m.have_to ? m.to_idx ^ 1 : m.to_idx;
        HIPTRY(hipMemcpyAsync(m.d_raw, m.h_up[k], tb, hipMemcpyHostToDevice, stream_));
        HIPTRY(hipEventRecord(m.ev_up[k], stream_));
        m.up_used[k] = true;
        m.up_slot = (k + 1) % SceneReverb::UP_SLOTS;
        const int prc = launch_scene_reverb_prepare(m.d_raw, m.n_out, m.n_in, m.K, m.d_P[dst], stream_);
        if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_reverb_prepare");
        m.have_from = m.have_to;                         // (the first set after enable / reset takes effect without a fade)
        m.to_idx = dst;
        m.have_to = true;
        m.t_set = m.t;
        m.pending = false;
    }
    long long n_fade = 0;
    if (m.fading(m.t)) n_fade = std::min<long long>(n, m.t_set + m.R - 1 - m.t);
    const int lrc = launch_scene_reverb((const float *)d_in, m.n_in, n, m.hist[m.cur], m.hist[m.cur ^ 1], m.have_to ? m.d_P[m.to_idx] : nullptr,
                                        n_fade ? m.d_P[m.to_idx ^ 1] : nullptr, m.n_out, m.K, n_fade, (long long)m.t, (long long)m.t_set, m.R,
                                        m.parts, (const float *)d_add, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_reverb");
    m.cur ^= 1;
    m.t += n;
    m.next_step = tot_steps_ + 1;
    ++m.n_calls;
    m.last_out = out;
    m.last_nb = last_nb_;
    return PBSO_OK;
}

int Engine::read_scene_reverb(float *out, size_t n) {
    if (!reverb_ || !reverb_->last_out) return fail(PBSO_ERR_STATE, "read_scene_reverb: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_scene_reverb: host_out is NULL");
    const size_t total = (size_t)reverb_->n_out * reverb_->last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_scene_reverb size mismatch (n = n_out * n_buffers * frames_per_buffer)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, reverb_->last_out, total * sizeof(float), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

// the history back to silence, t back to 0, the taps gone: silence until the next set, which takes effect without a fade.
// Armed for the next step.
int Engine::scene_reverb_reset() {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb_reset: the scene reverb is not enabled");
    SceneReverb &m = *reverb_;
    HIPTRY(hipSetDevice(desc_.device));
    for (float *h : m.hist) HIPTRY(hipMemsetAsync(h, 0, m.hist_floats() * sizeof(float), stream_));
    m.have_to = m.have_from = m.pending = false;
    m.t = 0;
    m.t_set = 0;
    m.cur = 0;
    m.next_step = tot_steps_ + 1;
    return PBSO_OK;
}

int Engine::scene_reverb_info(int64_t out[4]) {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb_info: the scene reverb is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_reverb_info: out is NULL");
    const SceneReverb &m = *reverb_;
    out[0] = m.t;
    out[1] = m.fading(m.t) ? m.t_set + m.R - 1 : m.t;
    out[2] = m.n_calls;
    out[3] = m.n_sets;
    return PBSO_OK;
}

}  // namespace pbso
