// The engine's side of the scene reverb (include/openpbso_amd.h "scene reverb"; kernels_reverb.hip): the two tap sets (the one in
// force and the one faded out), the cross-fade's clock, the history of every input channel's last K - 1 samples on the device, and
// the rule that every step is processed exactly once.  Its input is the caller's device buffer, not the step's rows: of a step it
// reads the length only (last_nb_) and counts steps by tot_steps_.  It knows bus_state.h, which holds what the buses have in common
// (the cross-fade's clock among it), and nothing of the other buses.
#include "bus_state.h"

#include <cmath>
#include <cstring>

namespace pbso {

struct SceneReverb {
    int n_in = 0, n_out = 0, K = 0, H = 0, J = 0, LP = 0;            // H = K - 1 samples of history per input channel
    XFade fade;                                          // which set is in force, which is faded out, since when
    std::vector<float> pend_taps;                        // a set call waits here for the next processed step (a later one replaces it)
    StepClock clock;
    int64_t n_calls = 0, n_sets = 0;
    HistPair hist;                                       // [n_in][H]
    BusOut out;                                          // [n_out][n]
    DevMem<float> parts;                                 // partial rows [2][n_out][n_in J][n]
    // on the device: the padded reversed taps [n_out][n_in][J][LP] of both sets (fade.to_idx: the one in force), the raw taps of
    // an upload
    DevMem<float> d_P[2], d_raw;
    UploadRing up;                                       // blocks of n_out n_in K floats

    size_t taps_floats() const { return (size_t)n_out * n_in * K; }
};

static const BusWords WORDS = {"scene_reverb", "processed", "the reverb", "input", "processed step", "n_out"};

namespace {
bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return x < y + nb && y < x + na;
}
}  // namespace

void Engine::scene_reverb_release() {
    if (!reverb_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete reverb_;
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
    std::unique_ptr<SceneReverb> m(new SceneReverb());
    m->n_in = n_in;
    m->n_out = n_out;
    m->K = K;
    m->fade.R = xfade;
    m->H = K - 1;
    m->J = scene_reverb_segments(K);
    m->LP = scene_reverb_padded_taps(K);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("scene_reverb_enable: cannot allocate ") + what);
    };
    if (m->hist.create((size_t)n_in * m->H, stream_) != hipSuccess) return nomem("the history");
    const size_t rows = (size_t)n_out * n_in * m->J;
    for (DevMem<float> &p : m->d_P)
        if (p.alloc(rows * m->LP) != hipSuccess) return nomem("the taps");
    if (m->d_raw.alloc(m->taps_floats()) != hipSuccess) return nomem("the taps");
    switch (m->up.create(m->taps_floats() * sizeof(float))) {
    case UploadRing::NO_MEMORY: return nomem("the upload ring");
    case UploadRing::NO_EVENT: return hip_fail(hipErrorInvalidValue, "scene_reverb_enable: hipEventCreate");
    case UploadRing::OK: break;
    }
    m->clock.arm(tot_steps_);
    reverb_ = m.release();
    return PBSO_OK;
}

int Engine::scene_reverb_set(const float *taps) {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb_set: the scene reverb is not enabled");
    if (!taps) return fail(PBSO_ERR_INVALID, "scene_reverb_set: taps is NULL");
    SceneReverb &m = *reverb_;
    if (m.fade.fading(m.clock.t))
        return fail(PBSO_ERR_STATE, "scene_reverb_set: the cross-fade of the last set is still running (pbso_scene_reverb_info tells when it ends)");
    const size_t nt = m.taps_floats();
    for (size_t i = 0; i < nt; ++i)
        if (!std::isfinite(taps[i])) return fail(PBSO_ERR_INVALID, "scene_reverb_set: a tap is not finite");
    m.pend_taps.assign(taps, taps + nt);                 // takes effect at the first sample of the next processed step
    m.fade.pending = true;
    ++m.n_sets;
    return PBSO_OK;
}

int Engine::scene_reverb(const void *d_in, const void *d_add, void *d_out) {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb: the scene reverb is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "scene_reverb: d_in is NULL");
    SceneReverb &m = *reverb_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "scene_reverb: no step yet");
    if (const int order = m.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    const long long n = (long long)last_nb_ * B_;
    if (d_out && overlap(d_in, (size_t)m.n_in * n * sizeof(float), d_out, (size_t)m.n_out * n * sizeof(float)))
        return fail(PBSO_ERR_INVALID, "scene_reverb: d_out overlaps d_in");
    HIPTRY(hipSetDevice(desc_.device));
    float *out;
    GROWTRY(m.out.resolve(d_out, (size_t)m.n_out * n, stream_, out), "scene_reverb: cannot allocate the output", "scene_reverb: output");
    XFade &f = m.fade;
    const long long t = m.clock.t;
    // (the rows of the set faded out only where fades are: R < 2 never blends)
    GROWTRY(grow(m.parts, (size_t)(f.R > 1 ? 2 : 1) * m.n_out * m.n_in * m.J * n, stream_), "scene_reverb: cannot allocate the partial rows",
            "scene_reverb: partial rows");
    if (f.pending) {
        // the new set goes where the predecessor of the set in force was (the device copies are ordered behind the previous call
        // on the stream)
        char *h_up;
        HIPTRY(m.up.acquire(h_up));
        const size_t tb = m.taps_floats() * sizeof(float);
        std::memcpy(h_up, m.pend_taps.data(), tb);
        const int dst = f.incoming();
        HIPTRY(hipMemcpyAsync(m.d_raw, h_up, tb, hipMemcpyHostToDevice, stream_));
        HIPTRY(m.up.record(stream_));
        const int prc = launch_scene_reverb_prepare(m.d_raw, m.n_out, m.n_in, m.K, m.d_P[dst], stream_);
        if (prc != 0) return hip_fail((hipError_t)prc, "launch_scene_reverb_prepare");
        f.swap_in(t);
    }
    const long long n_fade = f.n_fade(t, n);
    const int lrc = launch_scene_reverb((const float *)d_in, m.n_in, n, m.hist.cur(), m.hist.next(), f.have_to ? m.d_P[f.to_idx].p : nullptr,
                                        n_fade ? m.d_P[f.to_idx ^ 1].p : nullptr, m.n_out, m.K, n_fade, t, f.t_set, f.R, m.parts,
                                        (const float *)d_add, out, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_scene_reverb");
    m.hist.flip();
    m.clock.advance(n, tot_steps_);
    ++m.n_calls;
    m.out.wrote(out, last_nb_);
    return PBSO_OK;
}

int Engine::read_scene_reverb(float *out, size_t n) {
    return read_bus(reverb_ ? &reverb_->out : nullptr, reverb_ ? reverb_->n_out : 0, WORDS, out, n);
}

// the history back to silence, t back to 0, the taps gone: silence until the next set, which takes effect without a fade.
// Armed for the next step.
int Engine::scene_reverb_reset() {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb_reset: the scene reverb is not enabled");
    SceneReverb &m = *reverb_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(m.hist.reset(stream_));
    m.fade.reset();
    m.clock.reset(tot_steps_);
    return PBSO_OK;
}

int Engine::scene_reverb_info(int64_t out[4]) {
    if (!reverb_) return fail(PBSO_ERR_STATE, "scene_reverb_info: the scene reverb is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "scene_reverb_info: out is NULL");
    const SceneReverb &m = *reverb_;
    out[0] = m.clock.t;
    out[1] = m.fade.fade_end(m.clock.t);
    out[2] = m.n_calls;
    out[3] = m.n_sets;
    return PBSO_OK;
}

}  // namespace pbso
