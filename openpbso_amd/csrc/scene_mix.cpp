// The engine's side of the scene mixer (include/openpbso_amd.h "scene mix"; kernels_mix.hip): the gains and delays with their
// ramps, the history of every object's last samples on the device, and the rule that every step is mixed exactly once.  The
// mixer reads what a step left (last_audio_, last_nb_) and counts steps by tot_steps_; the step itself does not know about it.
// What it has in common with the other buses -- memory that frees itself, the history pair, the upload ring, the step clock, the
// ramp -- is bus_state.h; here are its parameters, its buffer sizes, its upload and its launch.
#include "bus_state.h"

#include <cmath>
#include <cstring>
#include <deque>

namespace pbso {

// a scheduled set that is not in force yet: its targets in f32 as given, the gains [C][N], then the delays where it has any
struct PendingSet { long long t; bool has_delay; std::vector<float> v; };

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
    // the schedule (pbso_scene_mix_schedule): the sets not yet in force, ascending in t and none before clock.t; a mix takes those
    // inside its step to the device, where they are expanded into the step's records (scene_schedule_expand_kernel) and the last
    // one's block becomes d_p.  p then lags behind d_p (p_stale) until the copy back, queued behind the mix, is taken over.
    std::deque<PendingSet> pending;
    StagingRing stage;                                   // a step's times, has-delay flags and targets
    DevMem<char> d_sets;                                 // ... on the device
    DevMem<SceneParam> d_rec;                            // the step's records [K + 1][C][N][2]
    SceneParam *p_back = nullptr;                        // pinned: d_p after the last mix that took scheduled sets
    hipEvent_t ev_back = nullptr;
    bool p_stale = false;
    long long n_mixes = 0, n_sets = 0;                   // since the enable (pbso_scene_mix_info)
    SceneMix() = default;
    SceneMix(const SceneMix &) = delete;
    SceneMix &operator=(const SceneMix &) = delete;
    ~SceneMix() {
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
    if (hipHostMalloc((void **)&m->p_back, m->p.size() * sizeof(SceneParam), hipHostMallocDefault) != hipSuccess) {
        m->p_back = nullptr;
        return nomem("the parameters");
    }
    if (hipEventCreateWithFlags(&m->ev_back, hipEventDisableTiming) != hipSuccess) {
        m->ev_back = nullptr;
        return hip_fail(hipErrorInvalidValue, "scene_mix_enable: hipEventCreate");
    }
    m->clock.arm(tot_steps_);
    scene_ = m.release();
    return PBSO_OK;
}

int Engine::scene_mix_set(const float *gain, const float *delay) {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_set: the scene mixer is not enabled");
    if (!gain) return fail(PBSO_ERR_INVALID, "scene_mix_set: gain is NULL");
    SceneMix &m = *scene_;
    if (!m.pending.empty()) return fail(PBSO_ERR_STATE, "scene_mix_set: scheduled sets are pending (pbso_scene_mix_clear_schedule drops them)");
    const size_t cn = (size_t)m.C * m.N;
    for (size_t i = 0; i < cn; ++i) {
        if (!std::isfinite(gain[i])) return fail(PBSO_ERR_INVALID, "scene_mix_set: a gain is not finite");
        if (delay && !(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)m.max_delay))
            return fail(PBSO_ERR_INVALID, "scene_mix_set: a delay is not finite or outside [0, max_delay]");
    }
    HIPTRY(m.refresh());                                 // (after a drained schedule: from the value it left, mid-ramp included)
    // a set takes effect at the first sample of the next mixed step; during a ramp the new one starts from the current value
    for (size_t i = 0; i < cn; ++i) {
        ramp_set(m.p[2 * i], gain[i], m.clock.t, m.ramp, m.any_set);
        if (delay) ramp_set(m.p[2 * i + 1], delay[i], m.clock.t, m.ramp, m.any_set);
    }
    m.any_set = true;
    m.dirty = true;
    ++m.n_sets;
    return PBSO_OK;
}

// n_sets sets at the absolute samples t_set, gain / delay [n_sets][C][N] (delay NULL: unchanged by all of them); `call` names the
// entry point in the messages.  All of them are checked before the first is taken.
int Engine::scene_mix_schedule(const char *call, int n_sets, const int64_t *t_set, const float *gain, const float *delay) {
    const std::string name(call);
    if (!scene_) return fail(PBSO_ERR_STATE, name + ": the scene mixer is not enabled");
    if (n_sets < 0) return fail(PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set) return fail(PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!gain) return fail(PBSO_ERR_INVALID, name + ": gain is NULL");
    SceneMix &m = *scene_;
    const size_t cn = (size_t)m.C * m.N;
    long long after = m.pending.empty() ? m.clock.t - 1 : m.pending.back().t;       // every t_set lies behind this sample
    for (int k = 0; k < n_sets; ++k) {
        if ((long long)t_set[k] < m.clock.t) return fail(PBSO_ERR_INVALID, name + ": a t_set lies before the next mixed sample");
        if ((long long)t_set[k] <= after) return fail(PBSO_ERR_INVALID, name + ": the t_set are not ascending behind the last pending set's");
        after = (long long)t_set[k];
    }
    for (size_t i = 0; i < (size_t)n_sets * cn; ++i) {
        if (!std::isfinite(gain[i])) return fail(PBSO_ERR_INVALID, name + ": a gain is not finite");
        if (delay && !(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)m.max_delay))
            return fail(PBSO_ERR_INVALID, name + ": a delay is not finite or outside [0, max_delay]");
    }
    std::deque<PendingSet> taken;                        // (built apart: a failed allocation leaves the pending list as it was)
    for (int k = 0; k < n_sets; ++k) {
        PendingSet q{(long long)t_set[k], delay != nullptr, {}};
        q.v.assign(gain + (size_t)k * cn, gain + (size_t)(k + 1) * cn);
        if (delay) q.v.insert(q.v.end(), delay + (size_t)k * cn, delay + (size_t)(k + 1) * cn);
        taken.push_back(std::move(q));
    }
    for (PendingSet &q : taken) m.pending.push_back(std::move(q));
    m.n_sets += n_sets;
    return PBSO_OK;
}

int Engine::scene_mix_clear_schedule() {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_clear_schedule: the scene mixer is not enabled");
    scene_->pending.clear();
    return PBSO_OK;
}

int Engine::scene_mix_info(int64_t out[4]) {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_info: the scene mixer is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_mix_info: out is NULL");
    const SceneMix &m = *scene_;
    out[0] = m.clock.t;
    out[1] = (int64_t)m.pending.size();
    out[2] = m.n_mixes;
    out[3] = m.n_sets;
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
    // the scheduled sets that take effect inside this step (none lies before it); everything that can refuse comes before
    // anything is taken or launched
    size_t K = 0;
    while (K < m.pending.size() && m.pending[K].t < m.clock.t + n) ++K;
    if (K > (size_t)SCENE_MAX_SETS_PER_STEP)
        return fail(PBSO_ERR_INVALID, "scene_mix: more than 65536 scheduled sets take effect inside this step (step in shorter pieces, or pbso_scene_mix_clear_schedule)");
    const size_t cn = (size_t)m.C * m.N, off_flag = K * sizeof(long long), off_v = off_flag + K * sizeof(int),
                 set_bytes = off_v + K * 2 * cn * sizeof(float);
    char *h_sets = nullptr;
    if (K) {
        GROWTRY(grow(m.d_sets, set_bytes, stream_), "scene_mix: cannot allocate the step's scheduled sets", "scene_mix: scheduled sets");
        GROWTRY(grow(m.d_rec, (K + 1) * m.p.size(), stream_), "scene_mix: cannot allocate the step's records", "scene_mix: records");
        GROWTRY(m.stage.acquire(set_bytes, h_sets), "scene_mix: cannot allocate the staging of the step's scheduled sets", "scene_mix: staging");
    }
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
    if (K == 0) {
        const int lrc = launch_scene_mix(last_audio_, m.N, n, m.hist.cur(), m.hist.next(), m.H, m.d_p, m.C, m.ramp, m.clock.t, m.parts, out, stream_);
        if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_mix");
    } else {
        long long *h_t = (long long *)h_sets;
        int *h_flag = (int *)(h_sets + off_flag);
        float *h_v = (float *)(h_sets + off_v);
        for (size_t k = 0; k < K; ++k) {
            const PendingSet &q = m.pending[k];
            h_t[k] = q.t;
            h_flag[k] = q.has_delay ? 1 : 0;
            std::memcpy(h_v + k * 2 * cn, q.v.data(), q.v.size() * sizeof(float));       // (no delays: that half is never read)
        }
        HIPTRY(hipMemcpyAsync(m.d_sets, h_sets, set_bytes, hipMemcpyHostToDevice, stream_));
        HIPTRY(m.stage.record(stream_));
        const int lrc = launch_scene_mix_schedule(last_audio_, m.N, n, m.hist.cur(), m.hist.next(), m.H, m.d_p, m.C, m.ramp, m.clock.t, m.parts,
                                                  out, stream_, m.d_rec, (const long long *)m.d_sets.p, (const int *)(m.d_sets.p + off_flag),
                                                  (const float *)(m.d_sets.p + off_v), (int)K, m.any_set ? 1 : 0);
        if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_mix_schedule");
        // d_p is now the block of the last set; the host's copy follows behind the mix, and is taken over by who next needs it
        HIPTRY(hipMemcpyAsync(m.p_back, m.d_p, m.p.size() * sizeof(SceneParam), hipMemcpyDeviceToHost, stream_));
        HIPTRY(hipEventRecord(m.ev_back, stream_));
        m.p_stale = true;
        m.any_set = true;
        m.pending.erase(m.pending.begin(), m.pending.begin() + (long)K);
    }
    m.hist.flip();
    m.clock.advance(n, tot_steps_);
    m.out.wrote(out, last_nb_);
    ++m.n_mixes;
    return PBSO_OK;
}

int Engine::read_scene_mix(float *out, size_t n) { return read_bus(scene_ ? &scene_->out : nullptr, scene_ ? scene_->C : 0, WORDS, out, n); }

// the history back to silence, t back to 0; the gains and delays stay at the targets last in force (ramps finished), the scheduled
// sets still pending are dropped, and the next set takes effect without a ramp.  Armed for the next step.
int Engine::scene_mix_reset() {
    if (!scene_) return fail(PBSO_ERR_STATE, "scene_mix_reset: the scene mixer is not enabled");
    SceneMix &m = *scene_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(m.refresh());
    HIPTRY(m.hist.reset(stream_));
    m.pending.clear();
    for (SceneParam &q : m.p) ramp_settle(q);
    m.any_set = false;
    m.dirty = true;
    m.clock.reset(tot_steps_);
    return PBSO_OK;
}

}  // namespace pbso
