// The engine's side of the scene mixer (include/openpbso_amd.h "scene mix"; kernels_mix.hip): the gains and delays with their
// ramps, the history of every object's last samples on the device, and the rule that every step is mixed exactly once.  The
// mixer reads what a step left (last_audio_, last_nb_) and counts steps by tot_steps_; the step itself does not know about it.
// What it has in common with the other buses -- memory that frees itself, the history pair, the upload ring, the step clock, the
// ramp -- is bus_state.h; here are its parameters, its buffer sizes, its upload and its launch.
#include "bus_state.h"

#include <cmath>
#include <cstring>

namespace pbso {

struct SceneMix {
    int C = 0, N = 0, max_delay = 0, ramp = 0, H = 0;   // H = max_delay + 1 samples of history per object
    std::vector<SceneParam> p;                           // [C][N][2] (gain, delay): the host's copy, uploaded when it changed
    bool any_set = false, dirty = true;
    StepClock clock;
    HistPair hist;                                       // [N][H]
    BusOut out;                                          // [C][n]
    DevMem<float> parts;                                 // partial rows [C][groups][n]
    DevMem<SceneParam> d_p;                              // the parameters on the device
    UploadRing up;                                       // blocks of p.size() parameters
};

static const BusWords WORDS = {"scene_mix", "mixed", "the mixer", "audio", "mix", "n_channels"};

void Engine::scene_mix_release() {
    if (!scene_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete scene_;
    scene_ = nullptr;
}

int Engine::scene_mix_enable(int C, int max_delay, int ramp) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "scene_mix_enable before finalize");
    if (C < 1 || C > SCENE_MAX_CHANNELS) return fail(PBSO_ERR_INVALID, "scene_mix_enable: n_channels must be 1 .. 8");
    if (max_delay < 0 || max_delay > (1 << 20) || ramp < 0 || ramp > (1 << 20))
        return fail(PBSO_ERR_INVALID, "scene_mix_enable: max_delay and ramp_samples must be 0 .. 1 << 20");
    HIPTRY(hipSetDevice(desc_.device));
    scene_mix_release();
    std::unique_ptr<SceneMix> m(new SceneMix());
    m->C = C;
    m->N = n_objects();
    m->max_delay = max_delay;
    m->ramp = ramp;
    m->H = max_delay + 1;
    m->p.assign((size_t)C * m->N * 2, SceneParam{0.0, 0.0, 0, 0.0});
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("scene_mix_enable: cannot allocate ") + what);
    };
    if (m->hist.create((size_t)m->N * m->H, stream_) != hipSuccess) return nomem("the history");
    const size_t n = (size_t)std::max(last_nb_, 1) * B_;
    if (grow(m->out.own, (size_t)C * n, stream_) != hipSuccess) return nomem("the output");
    if (grow(m->parts, (size_t)C * mix_objects_groups(m->N) * n, stream_) != hipSuccess) return nomem("the partial rows");
    if (m->d_p.alloc(m->p.size()) != hipSuccess) return nomem("the parameters");
    switch (m->up.create(m->p.size() * sizeof(SceneParam))) {
    case UploadRing::NO_MEMORY: return nomem("the parameters");
    case UploadRing::NO_EVENT: return hip_fail(hipErrorInvalidValue, "scene_mix_enable: hipEventCreate");
    case UploadRing::OK: break;
    }
    m->clock.arm(tot_steps_);
    scene_ = m.release();
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
    for (size_t i = 0; i < cn; ++i) {
        ramp_set(m.p[2 * i], gain[i], m.clock.t, m.ramp, m.any_set);
        if (delay) ramp_set(m.p[2 * i + 1], delay[i], m.clock.t, m.ramp, m.any_set);
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
    if (const int order = m.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    HIPTRY(hipSetDevice(desc_.device));
    const long long n = (long long)last_nb_ * B_;
    const int groups = mix_objects_groups(m.N);
    float *out;
    GROWTRY(m.out.resolve(d_out, (size_t)m.C * n, stream_, out), "scene_mix: cannot allocate the output", "scene_mix: output");
    GROWTRY(grow(m.parts, (size_t)m.C * groups * n, stream_), "scene_mix: cannot allocate the partial rows", "scene_mix: partial rows");
    if (m.dirty) {
        // (the device copy itself is ordered behind the previous mix on the stream)
        char *h_p;
        HIPTRY(m.up.acquire(h_p));
        const size_t bytes = m.p.size() * sizeof(SceneParam);
        std::memcpy(h_p, m.p.data(), bytes);
        HIPTRY(hipMemcpyAsync(m.d_p, h_p, bytes, hipMemcpyHostToDevice, stream_));
        HIPTRY(m.up.record(stream_));
        m.dirty = false;
    }
    const int lrc = launch_scene_mix(last_audio_, m.N, n, m.hist.cur(), m.hist.next(), m.H, m.d_p, m.C, m.ramp, m.clock.t, m.parts, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_mix");
    m.hist.flip();
    m.clock.advance(n, tot_steps_);
    m.out.wrote(out, last_nb_);
    return PBSO_OK;
}

int Engine::read_scene_mix(float *out, size_t n) { return read_bus(scene_ ? &scene_->out : nullptr, scene_ ? scene_->C : 0, WORDS, out, n); }

// the history back to silence, t back to 0; the gains and delays stay at their targets (ramps finished), and the next set takes
// effect without a ramp.  Armed for the next step.
int Engine::scene_mix_reset() {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_reset: the scene mixer is not enabled");
    SceneMix &m = *scene_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(m.hist.reset(stream_));
    for (SceneParam &q : m.p) ramp_settle(q);
    m.any_set = false;
    m.dirty = true;
    m.clock.reset(tot_steps_);
    return PBSO_OK;
}

}  // namespace pbso
