// The engine's side of the scene mixer (include/openpbso_amd.h "scene mix"; kernels_mix.hip): the gains and delays with their
// ramps, the history of every object's last samples on the device, and the rule that every step is mixed exactly once.  The
// mixer reads what a step left (last_audio_, last_nb_) and counts steps by tot_steps_; the step itself does not know about it.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pbso {

struct SceneMix {
    int C = 0, N = 0, max_delay = 0, ramp = 0, H = 0;   // H = max_delay + 1 samples of history per object
    std::vector<SceneParam> p;                           // [C][N][2] (gain, delay): the host's copy, uploaded when it changed
    bool any_set = false, dirty = true;
    int64_t t = 0;                                       // absolute sample of the next mixed step's first sample
    int64_t next_step = 0;                               // the tot_steps_ the next mix must find
    float *hist[2] = {nullptr, nullptr};                 // [N][H] the samples before the next step, double-buffered
    int cur = 0;
    float *out = nullptr, *parts = nullptr;              // the engine-owned output [C][n]; partial rows [C][groups][n]
    size_t out_cap = 0, parts_cap = 0;
    // the parameters on the device, and pinned staging of their uploads in a ring: a caller that sets new values every step (a
    // moving source) waits for nothing as long as it is less than UP_SLOTS steps ahead of the device
    static constexpr int UP_SLOTS = 3;
    SceneParam *d_p = nullptr, *h_p[UP_SLOTS] = {};
    hipEvent_t ev_up[UP_SLOTS] = {};                     // the upload from that slot has left it
    bool up_used[UP_SLOTS] = {};
    int up_slot = 0;
    const float *last_out = nullptr;                     // where the last mix went
    int last_nb = 0;
};

namespace {

// p(t) of include/openpbso_amd.h, in fp64 as the kernel evaluates it (kernels_mix.hip)
double ramp_value(const SceneParam &p, int64_t t, int R) {
    const int64_t k = t - p.t_set + 1;
    if (R == 0 || k >= R) return p.to;
    return p.from + p.slope * (double)k;
}

void free_scene(SceneMix *m) {
    for (float *h : m->hist)
        if (h) (void)hipFree(h);
    if (m->out) (void)hipFree(m->out);
    if (m->parts) (void)hipFree(m->parts);
    if (m->d_p) (void)hipFree(m->d_p);
    for (int i = 0; i < SceneMix::UP_SLOTS; ++i) {
        if (m->h_p[i]) (void)hipHostFree(m->h_p[i]);
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

void Engine::scene_mix_release() {
    if (!scene_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    free_scene(scene_);
    scene_ = nullptr;
}

int Engine::scene_mix_enable(int C, int max_delay, int ramp) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "scene_mix_enable before finalize");
    if (C < 1 || C > SCENE_MAX_CHANNELS) return fail(PBSO_ERR_INVALID, "scene_mix_enable: n_channels must be 1 .. 8");
    if (max_delay < 0 || max_delay > (1 << 20) || ramp < 0 || ramp > (1 << 20))
        return fail(PBSO_ERR_INVALID, "scene_mix_enable: max_delay and ramp_samples must be 0 .. 1 << 20");
    HIPTRY(hipSetDevice(desc_.device));
    scene_mix_release();
    SceneMix *m = new SceneMix();
    m->C = C;
    m->N = n_objects();
    m->max_delay = max_delay;
    m->ramp = ramp;
    m->H = max_delay + 1;
    m->p.assign((size_t)C * m->N * 2, SceneParam{0.0, 0.0, 0, 0.0});
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        free_scene(m);
        return fail(PBSO_ERR_NOMEM, std::string("scene_mix_enable: cannot allocate ") + what);
    };
    const size_t hist_floats = std::max<size_t>((size_t)m->N * m->H, 1);
    for (float *&h : m->hist) {
        if (hipMalloc((void **)&h, hist_floats * sizeof(float)) != hipSuccess) { h = nullptr; return nomem("the history"); }
        if (hipMemsetAsync(h, 0, hist_floats * sizeof(float), stream_) != hipSuccess) return nomem("the history");
    }
    const size_t n = (size_t)std::max(last_nb_, 1) * B_;
    if (grow(m->out, m->out_cap, (size_t)C * n, stream_) != hipSuccess) return nomem("the output");
    if (grow(m->parts, m->parts_cap, (size_t)C * mix_objects_groups(m->N) * n, stream_) != hipSuccess) return nomem("the partial rows");
    if (hipMalloc((void **)&m->d_p, m->p.size() * sizeof(SceneParam)) != hipSuccess) { m->d_p = nullptr; return nomem("the parameters"); }
    for (int i = 0; i < SceneMix::UP_SLOTS; ++i) {
        if (hipHostMalloc((void **)&m->h_p[i], m->p.size() * sizeof(SceneParam), hipHostMallocDefault) != hipSuccess) { m->h_p[i] = nullptr; return nomem("the parameters"); }
        if (hipEventCreateWithFlags(&m->ev_up[i], hipEventDisableTiming) != hipSuccess) {
            m->ev_up[i] = nullptr;
            free_scene(m);
            return hip_fail(hipErrorInvalidValue, "scene_mix_enable: hipEventCreate");
        }
    }
    m->next_step = tot_steps_ + 1;                       // armed for the next step
    scene_ = m;
    return PBSO_OK;
}

int Engine::scene_mix_set(const float *gain, const float *delay) {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_set: the scene mixer is not enabled");
    if (!gain) return fail(PBSO_ERR_INVALID, "scene_mix_set: gain is NULL");
    SceneMix &m = *scene_;
    const size_t cn = (size_t)m.C * m.N;
    for (size_t i = 0; i < cn; ++i) {
        if (!std::isfinite(gain[i])) return fail(PBSO_ERR_INVALID, "scene_mix_set: a gain is not finite");
        if (delay && !(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)m.max_delay))
            return fail(PBSO_ERR_INVALID, "scene_mix_set: a delay is not finite or outside [0, max_delay]");
    }
    // a set takes effect at the first sample of the next mixed step; during a ramp the new one starts from the current value
    auto set = [&](SceneParam &q, double v) {
        q.from = m.any_set ? ramp_value(q, m.t - 1, m.ramp) : v;
        q.to = v;
        q.t_set = m.t;
        q.slope = m.ramp ? (q.to - q.from) / (double)m.ramp : 0.0;
    };
    for (size_t i = 0; i < cn; ++i) {
        set(m.p[2 * i], gain[i]);
        if (delay) set(m.p[2 * i + 1], delay[i]);
    }
    m.any_set = true;
    m.dirty = true;
    return PBSO_OK;
}

int Engine::scene_mix(void *d_out) {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix: the scene mixer is not enabled");
    SceneMix &m = *scene_;
    if (!last_audio_ || last_nb_ <= 0) return fail(PBSO_ERR_STATE, "scene_mix: no step yet");
    if (host_step_ == tot_steps_) return fail(PBSO_ERR_STATE, "scene_mix: the last step went to host memory (pbso_step_to_host): its rows are not on the device");
    if (tot_steps_ < m.next_step) return fail(PBSO_ERR_STATE, "scene_mix: the last step is mixed already (or was taken before the mixer was enabled / reset)");
    if (tot_steps_ > m.next_step)
        return fail(PBSO_ERR_STATE, "scene_mix: a step was not mixed, the history is no longer the audio before this step (pbso_scene_mix_reset starts over)");
    HIPTRY(hipSetDevice(desc_.device));
    const long long n = (long long)last_nb_ * B_;
    const int groups = mix_objects_groups(m.N);
    float *out = (float *)d_out;
    if (!out) {
        hipError_t e = grow(m.out, m.out_cap, (size_t)m.C * n, stream_);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, "scene_mix: cannot allocate the output") : hip_fail(e, "scene_mix: output");
        out = m.out;
    }
    {
        hipError_t e = grow(m.parts, m.parts_cap, (size_t)m.C * groups * n, stream_);
        if (e != hipSuccess) return e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, "scene_mix: cannot allocate the partial rows") : hip_fail(e, "scene_mix: partial rows");
    }
    if (m.dirty) {
        // (a staging slot is rewritten only once the copy that last read it is done; the device copy itself is ordered behind the
        //  previous mix on the stream)
        const int k = m.up_slot;
        if (m.up_used[k]) HIPTRY(hipEventSynchronize(m.ev_up[k]));
        const size_t bytes = m.p.size() * sizeof(SceneParam);
        std::memcpy(m.h_p[k], m.p.data(), bytes);
        HIPTRY(hipMemcpyAsync(m.d_p, m.h_p[k], bytes, hipMemcpyHostToDevice, stream_));
        HIPTRY(hipEventRecord(m.ev_up[k], stream_));
        m.up_used[k] = true;
        m.up_slot = (k + 1) % SceneMix::UP_SLOTS;
        m.dirty = false;
    }
    const int lrc = launch_scene_mix(last_audio_, m.N, n, m.hist[m.cur], m.hist[m.cur ^ 1], m.H, m.d_p, m.C, m.ramp, (long long)m.t,
                                     m.parts, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_mix");
    m.cur ^= 1;
    m.t += n;
    m.next_step = tot_steps_ + 1;
    m.last_out = out;
    m.last_nb = last_nb_;
    return PBSO_OK;
}

int Engine::read_scene_mix(float *out, size_t n) {
    if (!scene_ || !scene_->last_out) return fail(PBSO_ERR_STATE, "read_scene_mix: no mix yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_scene_mix: host_out is NULL");
    const size_t total = (size_t)scene_->C * scene_->last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_scene_mix size mismatch (n = n_channels * n_buffers * frames_per_buffer)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, scene_->last_out, total * sizeof(float), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

// the history back to silence, t back to 0; the gains and delays stay at their targets (ramps finished), and the next set takes
// effect without a ramp.  Armed for the next step.
int Engine::scene_mix_reset() {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_reset: the scene mixer is not enabled");
    SceneMix &m = *scene_;
    HIPTRY(hipSetDevice(desc_.device));
    for (float *h : m.hist) HIPTRY(hipMemsetAsync(h, 0, std::max<size_t>((size_t)m.N * m.H, 1) * sizeof(float), stream_));
    for (SceneParam &q : m.p) {
        q.from = q.to;
        q.t_set = 0;
        q.slope = 0.0;
    }
    m.t = 0;
    m.cur = 0;
    m.any_set = false;
    m.dirty = true;
    m.next_step = tot_steps_ + 1;
    return PBSO_OK;
}

}  // namespace pbso
