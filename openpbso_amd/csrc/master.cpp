// The engine's side of the master bus (include/openpbso_amd.h "master bus"; kernels_master.hip): the ceiling, the look-ahead and
// hold, the smoothing window computed once at enable, the gain with its ramp, the history of the last 2 L + H samples of every
// channel on the device, and the rule that every step is processed exactly once.  Its input is the caller's device buffer, not the
// step's rows: of a step it reads the length only (last_nb_) and counts steps by tot_steps_.  It knows nothing of the mixers or the
// reverb.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pbso {

struct Master {
    int C = 0, L = 0, H = 0, R = 0, HL = 0;              // HL = 2 L + H samples of history per channel
    float T = 1.f;
    SceneParam gain{1.0, 1.0, 0, 0.0};                   // the scene mix's ramp of one parameter; passed to the kernel by value
    std::vector<float> w;                                // the L taps
    int64_t t = 0;                                       // absolute sample of the next processed step's first sample
    int64_t next_step = 0;                               // the tot_steps_ the next call must find
    int64_t n_calls = 0, n_sets = 0;
    float *hist[2] = {nullptr, nullptr};                 // [C][HL] the samples of v before the next step, double-buffered
    int cur = 0;
    float *d_w = nullptr;
    // work arrays of a call: V [C][HL + n] | Rb, M0, M1 [HL + n] | G [n] in one block; the engine-owned output; meters; PCM
    float *work = nullptr, *out = nullptr;
    size_t work_cap = 0, out_cap = 0;
    pbso_master_meter *meters = nullptr;
    size_t meters_cap = 0;
    int16_t *pcm = nullptr;
    size_t pcm_cap = 0;
    const float *last_out = nullptr;                     // where the last call wrote
    int last_nb = 0;

    bool ramping(int64_t at) const { return gain.from != gain.to && at - gain.t_set + 1 < (int64_t)R; }
};

static_assert(sizeof(pbso_master_meter) == 24, "pbso_master_meter is 24 bytes");

namespace {

// p(t) of include/openpbso_amd.h, in fp64 as the kernel evaluates it (kernels_master.hip)
double ramp_value(const SceneParam &p, int64_t t, int R) {
    const int64_t k = t - p.t_set + 1;
    if (R == 0 || k >= R) return p.to;
    return p.from + p.slope * (double)k;
}

void free_master(Master *m) {
    for (float *h : m->hist)
        if (h) (void)hipFree(h);
    if (m->d_w) (void)hipFree(m->d_w);
    if (m->work) (void)hipFree(m->work);
    if (m->out) (void)hipFree(m->out);
    if (m->meters) (void)hipFree(m->meters);
    if (m->pcm) (void)hipFree(m->pcm);
    delete m;
}

// a device buffer of at least n elements; the old block may still be read by a call in flight on the stream
template <typename E>
hipError_t grow(E *&p, size_t &cap, size_t n, hipStream_t s) {
    if (p && n <= cap) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    e = hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(E));
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
#define GROW(buf, cap, n, what)                                                                                   \
    do {                                                                                                          \
        hipError_t _e = grow(buf, cap, n, stream_);                                                               \
        if (_e != hipSuccess)                                                                                     \
            return _e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, what ": cannot allocate") : hip_fail(_e, what); \
    } while (0)

void Engine::master_release() {
    if (!master_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    free_master(master_);
    master_ = nullptr;
}

int Engine::master_enable(int C, float T, int L, int H, int ramp) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "master_enable before finalize");
    if (C < 1 || C > SCENE_MAX_CHANNELS) return fail(PBSO_ERR_INVALID, "master_enable: n_channels must be 1 .. 8");
    if (!(std::isfinite(T) && T > 0.f && T <= 1.f)) return fail(PBSO_ERR_INVALID, "master_enable: the ceiling must be finite, 0 < ceiling <= 1");
    if (L < 1 || L > MASTER_MAX_LOOKAHEAD) return fail(PBSO_ERR_INVALID, "master_enable: lookahead must be 1 .. 4096");
    if (H < 0 || H > MASTER_MAX_HOLD) return fail(PBSO_ERR_INVALID, "master_enable: hold must be 0 .. 65536");
    if (ramp < 0 || ramp > (1 << 20)) return fail(PBSO_ERR_INVALID, "master_enable: ramp_samples must be 0 .. 1 << 20");
    HIPTRY(hipSetDevice(desc_.device));
    master_release();
    Master *m = new Master();
    m->C = C;
    m->T = T;
    m->L = L;
    m->H = H;
    m->R = ramp;
    m->HL = 2 * L + H;
    // the smoothing window, in fp64: h_k = 1 - cos(2 pi (k + 1) / (L + 1)), summed in ascending k, w[k] = (float)(h_k / sum)
    {
        std::vector<double> h((size_t)L);
        double sum = 0.0;
        for (int k = 0; k < L; ++k) {
            h[k] = 1.0 - std::cos(2.0 * M_PI * (double)(k + 1) / (double)(L + 1));
            sum += h[k];
        }
        m->w.resize((size_t)L);
        for (int k = 0; k < L; ++k) m->w[k] = (float)(h[k] / sum);
    }
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        free_master(m);
        return fail(PBSO_ERR_NOMEM, std::string("master_enable: cannot allocate ") + what);
    };
    const size_t hist_bytes = (size_t)C * m->HL * sizeof(float);
    for (float *&h : m->hist) {
        if (hipMalloc((void **)&h, hist_bytes) != hipSuccess) { h = nullptr; return nomem("the history"); }
        if (hipMemsetAsync(h, 0, hist_bytes, stream_) != hipSuccess) return nomem("the history");
    }
    if (hipMalloc((void **)&m->d_w, (size_t)L * sizeof(float)) != hipSuccess) { m->d_w = nullptr; return nomem("the window"); }
    // (m->w outlives the copy: a Master is freed behind a synchronisation of the stream only)
    if (hipMemcpyAsync(m->d_w, m->w.data(), (size_t)L * sizeof(float), hipMemcpyHostToDevice, stream_) != hipSuccess) return nomem("the window");
    m->next_step = tot_steps_ + 1;                       // armed for the next step
    master_ = m;
    return PBSO_OK;
}

// takes effect at the first sample of the next processed step and ramps from the value in force one sample before it
int Engine::master_set_gain(float gain) {
    if (!master_) return fail(PBSO_ERR_STATE, "master_set_gain: the master bus is not enabled");
    if (!std::isfinite(gain)) return fail(PBSO_ERR_INVALID, "master_set_gain: the gain is not finite");
    Master &m = *master_;
    SceneParam &q = m.gain;
    q.from = ramp_value(q, m.t - 1, m.R);
    q.to = (double)gain;
    q.t_set = m.t;
    q.slope = m.R ? (q.to - q.from) / (double)m.R : 0.0;
    ++m.n_sets;
    return PBSO_OK;
}

int Engine::master(const void *d_in, void *d_out) {
    if (!master_) return fail(PBSO_ERR_STATE, "master: the master bus is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "master: d_in is NULL");
    Master &m = *master_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "master: no step yet");
    if (tot_steps_ < m.next_step) return fail(PBSO_ERR_STATE, "master: the last step is processed already (or was taken before the master bus was enabled / reset)");
    if (tot_steps_ > m.next_step)
        return fail(PBSO_ERR_STATE, "master: a step was not processed, the history is no longer the signal before this step (pbso_master_reset starts over)");
    HIPTRY(hipSetDevice(desc_.device));
    const size_t n = (size_t)last_nb_ * B_, N = (size_t)m.HL + n;
    float *out = (float *)d_out;
    if (!out) {
        GROW(m.out, m.out_cap, (size_t)m.C * n, "master: output");
        out = m.out;
    }
    GROW(m.work, m.work_cap, (size_t)(m.C + 3) * N + n, "master: work arrays");
    GROW(m.meters, m.meters_cap, (size_t)last_nb_ * m.C, "master: meters");
    float *V = m.work, *Rb = V + (size_t)m.C * N, *M0 = Rb + N, *M1 = M0 + N, *G = M1 + N;
    const int lrc = launch_master((const float *)d_in, m.C, (long long)n, B_, m.hist[m.cur], m.hist[m.cur ^ 1], m.L, m.H, m.T, m.gain, m.R,
                                  (long long)m.t, m.d_w, V, Rb, M0, M1, G, out, m.meters, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_master");
    m.cur ^= 1;
    m.t += (int64_t)n;
    m.next_step = tot_steps_ + 1;
    ++m.n_calls;
    m.last_out = out;
    m.last_nb = last_nb_;
    return PBSO_OK;
}

int Engine::read_master(float *out, size_t n) {
    if (!master_ || !master_->last_out) return fail(PBSO_ERR_STATE, "read_master: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_master: host_out is NULL");
    const size_t total = (size_t)master_->C * master_->last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_master size mismatch (n = n_channels * n_buffers * frames_per_buffer)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, master_->last_out, total * sizeof(float), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::read_master_pcm16(int16_t *out, size_t n) {
    if (!master_ || !master_->last_out) return fail(PBSO_ERR_STATE, "read_master_pcm16: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_master_pcm16: host_out is NULL");
    Master &m = *master_;
    const size_t total = (size_t)m.C * m.last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_master_pcm16 size mismatch (n = n_channels * n_buffers * frames_per_buffer)");
    HIPTRY(hipSetDevice(desc_.device));
    GROW(m.pcm, m.pcm_cap, total, "read_master_pcm16: PCM");
    const int lrc = launch_master_pcm16(m.last_out, m.C, (long long)m.last_nb * B_, (short *)m.pcm, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_master_pcm16");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, m.pcm, total * sizeof(int16_t), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::read_master_meters(pbso_master_meter *out, size_t n_records) {
    if (!master_ || !master_->last_out) return fail(PBSO_ERR_STATE, "read_master_meters: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_master_meters: out is NULL");
    const size_t total = (size_t)master_->C * master_->last_nb;
    if (n_records != total) return fail(PBSO_ERR_INVALID, "read_master_meters size mismatch (n_records = n_buffers * n_channels)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, master_->meters, total * sizeof(pbso_master_meter), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::master_window(float *out, size_t n) {
    if (!master_) return fail(PBSO_ERR_STATE, "master_window: the master bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "master_window: out is NULL");
    if (n != master_->w.size()) return fail(PBSO_ERR_INVALID, "master_window size mismatch (n = lookahead)");
    std::memcpy(out, master_->w.data(), n * sizeof(float));
    return PBSO_OK;
}

// the history back to silence, t back to 0; the gain stays at the value last set, its ramp finished.  Armed for the next step.
int Engine::master_reset() {
    if (!master_) return fail(PBSO_ERR_STATE, "master_reset: the master bus is not enabled");
    Master &m = *master_;
    HIPTRY(hipSetDevice(desc_.device));
    for (float *h : m.hist) HIPTRY(hipMemsetAsync(h, 0, (size_t)m.C * m.HL * sizeof(float), stream_));
    m.gain.from = m.gain.to;
    m.gain.t_set = 0;
    m.gain.slope = 0.0;
    m.t = 0;
    m.cur = 0;
    m.next_step = tot_steps_ + 1;
    return PBSO_OK;
}

int Engine::master_info(int64_t out[4]) {
    if (!master_) return fail(PBSO_ERR_STATE, "master_info: the master bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "master_info: out is NULL");
    const Master &m = *master_;
    out[0] = m.t;
    out[1] = m.ramping(m.t) ? m.gain.t_set + m.R - 1 : m.t;
    out[2] = m.n_calls;
    out[3] = m.n_sets;
    return PBSO_OK;
}

}  // namespace pbso
