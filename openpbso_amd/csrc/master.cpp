// The engine's side of the master bus (include/openpbso_amd.h "master bus"; kernels_master.hip): the ceiling, the look-ahead and
// hold, the smoothing window computed once at enable, the gain with its ramp, the history of the last 2 L + H samples of every
// channel on the device, and the rule that every step is processed exactly once.  Its input is the caller's device buffer, not the
// step's rows: of a step it reads the length only (last_nb_) and counts steps by tot_steps_.  It knows bus_state.h, which holds
// what the buses have in common (the ramp of one parameter among it), and nothing of the mixers or the reverb.
#include "bus_state.h"

#include <cmath>
#include <cstring>

namespace pbso {

struct Master {
    int C = 0, L = 0, H = 0, R = 0, HL = 0;              // HL = 2 L + H samples of history per channel
    float T = 1.f;
    SceneParam gain{1.0, 1.0, 0, 0.0};                   // one ramped parameter (scene_ramp.h); passed to the kernel by value
    std::vector<float> w;                                // the L taps
    StepClock clock;
    int64_t n_calls = 0, n_sets = 0;
    HistPair hist;                                       // [C][HL] the samples of v
    BusOut out;                                          // [C][n]
    DevMem<float> d_w;
    DevMem<float> work;                                  // of a call: V [C][HL + n] | Rb, M0, M1 [HL + n] | G [n] in one block
    DevMem<pbso_master_meter> meters;
    DevMem<int16_t> pcm;

    bool ramping(int64_t at) const { return gain.from != gain.to && at - gain.t_set + 1 < (int64_t)R; }
};

static_assert(sizeof(pbso_master_meter) == 24, "pbso_master_meter is 24 bytes");

static const BusWords WORDS = {"master", "processed", "the master bus", "signal", "processed step", "n_channels"};

void Engine::master_release() {
    if (!master_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete master_;
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
    std::unique_ptr<Master> m(new Master());
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
        return fail(PBSO_ERR_NOMEM, std::string("master_enable: cannot allocate ") + what);
    };
    if (m->hist.create((size_t)C * m->HL, stream_) != hipSuccess) return nomem("the history");
    if (m->d_w.alloc((size_t)L) != hipSuccess) return nomem("the window");
    // (m->w outlives the copy: a Master is freed behind a synchronisation of the stream only)
    if (hipMemcpyAsync(m->d_w, m->w.data(), (size_t)L * sizeof(float), hipMemcpyHostToDevice, stream_) != hipSuccess) return nomem("the window");
    m->clock.arm(tot_steps_);
    master_ = m.release();
    return PBSO_OK;
}

// takes effect at the first sample of the next processed step and ramps from the value in force one sample before it
int Engine::master_set_gain(float gain) {
    if (!master_) return fail(PBSO_ERR_STATE, "master_set_gain: the master bus is not enabled");
    if (!std::isfinite(gain)) return fail(PBSO_ERR_INVALID, "master_set_gain: the gain is not finite");
    Master &m = *master_;
    ramp_set(m.gain, (double)gain, m.clock.t, m.R, true);
    ++m.n_sets;
    return PBSO_OK;
}

int Engine::master(const void *d_in, void *d_out) {
    if (!master_) return fail(PBSO_ERR_STATE, "master: the master bus is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "master: d_in is NULL");
    Master &m = *master_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "master: no step yet");
    if (const int order = m.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    HIPTRY(hipSetDevice(desc_.device));
    const size_t n = (size_t)last_nb_ * B_, N = (size_t)m.HL + n;
    float *out;
    GROWTRY(m.out.resolve(d_out, (size_t)m.C * n, stream_, out), "master: output: cannot allocate", "master: output");
    GROWTRY(grow(m.work, (size_t)(m.C + 3) * N + n, stream_), "master: work arrays: cannot allocate", "master: work arrays");
    GROWTRY(grow(m.meters, (size_t)last_nb_ * m.C, stream_), "master: meters: cannot allocate", "master: meters");
    float *V = m.work, *Rb = V + (size_t)m.C * N, *M0 = Rb + N, *M1 = M0 + N, *G = M1 + N;
    const int lrc = launch_master((const float *)d_in, m.C, (long long)n, B_, m.hist.cur(), m.hist.next(), m.L, m.H, m.T, m.gain, m.R, m.clock.t,
                                  m.d_w, V, Rb, M0, M1, G, out, m.meters.p, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_master");
    m.hist.flip();
    m.clock.advance((long long)n, tot_steps_);
    ++m.n_calls;
    m.out.wrote(out, last_nb_);
    return PBSO_OK;
}

int Engine::read_master(float *out, size_t n) { return read_bus(master_ ? &master_->out : nullptr, master_ ? master_->C : 0, WORDS, out, n); }

int Engine::read_master_pcm16(int16_t *out, size_t n) {
    if (!master_ || !master_->out.last) return fail(PBSO_ERR_STATE, "read_master_pcm16: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_master_pcm16: host_out is NULL");
    Master &m = *master_;
    const size_t total = (size_t)m.C * m.out.last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_master_pcm16 size mismatch (n = n_channels * n_buffers * frames_per_buffer)");
    HIPTRY(hipSetDevice(desc_.device));
    GROWTRY(grow(m.pcm, total, stream_), "read_master_pcm16: PCM: cannot allocate", "read_master_pcm16: PCM");
    const int lrc = launch_master_pcm16(m.out.last, m.C, (long long)m.out.last_nb * B_, (short *)m.pcm.p, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_master_pcm16");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, m.pcm.p, total * sizeof(int16_t), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::read_master_meters(pbso_master_meter *out, size_t n_records) {
    if (!master_ || !master_->out.last) return fail(PBSO_ERR_STATE, "read_master_meters: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_master_meters: out is NULL");
    const size_t total = (size_t)master_->C * master_->out.last_nb;
    if (n_records != total) return fail(PBSO_ERR_INVALID, "read_master_meters size mismatch (n_records = n_buffers * n_channels)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, master_->meters.p, total * sizeof(pbso_master_meter), hipMemcpyDeviceToHost));
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
    HIPTRY(m.hist.reset(stream_));
    ramp_settle(m.gain);
    m.clock.reset(tot_steps_);
    return PBSO_OK;
}

int Engine::master_info(int64_t out[4]) {
    if (!master_) return fail(PBSO_ERR_STATE, "master_info: the master bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "master_info: out is NULL");
    const Master &m = *master_;
    out[0] = m.clock.t;
    out[1] = m.ramping(m.clock.t) ? m.gain.t_set + m.R - 1 : m.clock.t;
    out[2] = m.n_calls;
    out[3] = m.n_sets;
    return PBSO_OK;
}

}  // namespace pbso
