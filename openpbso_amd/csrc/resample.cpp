// The engine's side of the resampler bus (include/openpbso_amd.h "resampler bus"; kernels_resample.hip): the ratio L / M, the
// phase table designed once at enable, the history of the last T - 1 input samples of every channel on the device, the one number
// that carries the output clock from call to call (p0, resample_clock.h) and the rule that every step is processed exactly once.
// Its input is the caller's device buffer: of a step it reads the length only (last_nb_) and counts steps by tot_steps_.  Its
// output has a length of its own, n_out, which differs from call to call; hence its own read-backs and not read_bus.  It knows
// bus_state.h and nothing of the other buses.
#include "bus_state.h"
#include "resample_clock.h"

#include <cstring>

namespace pbso {

struct Resample {
    int C = 0, L = 1, M = 1, T = 1;
    std::vector<float> h;                                // [L][T]
    StepClock clock;                                     // of the input samples
    ResampleClock rc;                                    // t, m, p0 (rc.t == clock.t)
    int64_t n_calls = 0;
    HistPair hist;                                       // [C][T - 1]
    BusOut out;                                          // [C][stride]; of BusOut's bookkeeping only `last` is used
    long long last_n_out = 0, last_stride = 0;
    DevMem<float> d_h;
    DevMem<pbso_resample_meter> meters;                  // [C]
    DevMem<int16_t> pcm;
};

static_assert(sizeof(pbso_resample_meter) == 8, "pbso_resample_meter is 8 bytes");

static const BusWords WORDS = {"resample", "processed", "the resampler", "signal", "processed step", "n_channels"};

void Engine::resample_release() {
    if (!resample_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete resample_;
    resample_ = nullptr;
}

int Engine::resample_enable(int C, int rate_out, int taps, double beta, double cutoff) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "resample_enable before finalize");
    if (C < 1 || C > SCENE_MAX_CHANNELS) return fail(PBSO_ERR_INVALID, "resample_enable: n_channels must be 1 .. 8");
    if (const char *why = resample_refusal(rate_, rate_out, taps, beta, cutoff)) return fail(PBSO_ERR_INVALID, std::string("resample_enable: ") + why);
    HIPTRY(hipSetDevice(desc_.device));
    std::unique_ptr<Resample> r(new Resample());
    r->C = C;
    r->T = taps;
    resample_reduce(rate_, rate_out, r->L, r->M);
    resample_design(r->L, r->M, r->T, beta, cutoff, r->h);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("resample_enable: cannot allocate ") + what);
    };
    if (r->hist.create((size_t)C * (taps - 1), stream_) != hipSuccess) return nomem("the history");
    if (r->d_h.alloc(r->h.size()) != hipSuccess) return nomem("the phase table");
    if (r->meters.alloc((size_t)C) != hipSuccess) return nomem("the meters");
    // (r->h outlives the copy: a Resample is freed behind a synchronisation of the stream only)
    if (hipMemcpyAsync(r->d_h, r->h.data(), r->h.size() * sizeof(float), hipMemcpyHostToDevice, stream_) != hipSuccess) return nomem("the phase table");
    resample_release();
    r->clock.arm(tot_steps_);
    resample_ = r.release();
    return PBSO_OK;
}

int Engine::resample_max_out(int n_buffers, int64_t *out) {
    if (!resample_) return fail(PBSO_ERR_STATE, "resample_max_out: the resampler is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "resample_max_out: out is NULL");
    if (n_buffers < 1) return fail(PBSO_ERR_INVALID, "resample_max_out: n_buffers must be positive");
    *out = pbso::resample_max_out((long long)n_buffers * B_, resample_->L, resample_->M);
    return PBSO_OK;
}

int Engine::resample(const void *d_in, void *d_out, int64_t out_stride, int64_t *n_out_ret) {
    if (!resample_) return fail(PBSO_ERR_STATE, "resample: the resampler is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "resample: d_in is NULL");
    Resample &r = *resample_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "resample: no step yet");
    if (const int order = r.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    const long long n = (long long)last_nb_ * B_, n_out = r.rc.n_out(n, r.L, r.M);
    long long stride = n_out;
    if (d_out) {
        if (out_stride < pbso::resample_max_out(n, r.L, r.M)) return fail(PBSO_ERR_INVALID, "resample: out_stride is below ceil(n L / M)");
        if (out_stride > (1LL << 40)) return fail(PBSO_ERR_INVALID, "resample: out_stride is beyond 1 << 40");   // (the byte ranges below stay in 64 bits)
        stride = out_stride;
        const char *a = (const char *)d_in, *b = (const char *)d_out;
        const size_t na = (size_t)r.C * n * sizeof(float), nb = (size_t)r.C * stride * sizeof(float);
        if (a < b + nb && b < a + na) return fail(PBSO_ERR_INVALID, "resample: d_out overlaps d_in");
    }
    HIPTRY(hipSetDevice(desc_.device));
    float *out;
    GROWTRY(r.out.resolve(d_out, (size_t)r.C * stride, stream_, out), "resample: output: cannot allocate", "resample: output");
    const int lrc = launch_resample((const float *)d_in, r.C, n, r.hist.cur(), r.hist.next(), r.d_h, r.L, r.M, r.T, r.rc.p0, n_out, out, stride,
                                    r.meters.p, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_resample");
    r.hist.flip();
    r.clock.advance(n, tot_steps_);
    r.rc.advance(n, r.L, r.M);
    ++r.n_calls;
    r.out.wrote(out, last_nb_);
    r.last_n_out = n_out;
    r.last_stride = stride;
    if (n_out_ret) *n_out_ret = n_out;
    return PBSO_OK;
}

int Engine::read_resample(float *out, size_t n) {
    if (!resample_ || !resample_->out.last) return fail(PBSO_ERR_STATE, "read_resample: no processed step yet");
    const Resample &r = *resample_;
    const size_t total = (size_t)r.C * r.last_n_out;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_resample size mismatch (n = n_channels * n_out of the last call)");
    if (!out && total) return fail(PBSO_ERR_INVALID, "read_resample: host_out is NULL");
    { int src = sync(); if (src != PBSO_OK) return src; }
    if (total)
        HIPTRY(hipMemcpy2D(out, (size_t)r.last_n_out * sizeof(float), r.out.last, (size_t)r.last_stride * sizeof(float),
                           (size_t)r.last_n_out * sizeof(float), (size_t)r.C, hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::read_resample_pcm16(int16_t *out, size_t n) {
    if (!resample_ || !resample_->out.last) return fail(PBSO_ERR_STATE, "read_resample_pcm16: no processed step yet");
    Resample &r = *resample_;
    const size_t total = (size_t)r.C * r.last_n_out;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_resample_pcm16 size mismatch (n = n_channels * n_out of the last call)");
    if (!out && total) return fail(PBSO_ERR_INVALID, "read_resample_pcm16: host_out is NULL");
    if (!total) return sync();
    HIPTRY(hipSetDevice(desc_.device));
    GROWTRY(grow(r.pcm, total, stream_), "read_resample_pcm16: PCM: cannot allocate", "read_resample_pcm16: PCM");
    const int lrc = launch_resample_pcm16(r.out.last, r.C, r.last_n_out, r.last_stride, (short *)r.pcm.p, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_resample_pcm16");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, r.pcm.p, total * sizeof(int16_t), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::read_resample_meters(pbso_resample_meter *out, size_t n_channels) {
    if (!resample_ || !resample_->out.last) return fail(PBSO_ERR_STATE, "read_resample_meters: no processed step yet");
    if (!out) return fail(PBSO_ERR_INVALID, "read_resample_meters: out is NULL");
    if (n_channels != (size_t)resample_->C) return fail(PBSO_ERR_INVALID, "read_resample_meters size mismatch (n_channels as enabled)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, resample_->meters.p, n_channels * sizeof(pbso_resample_meter), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::resample_taps(float *out, size_t n) {
    if (!resample_) return fail(PBSO_ERR_STATE, "resample_taps: the resampler is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "resample_taps: out is NULL");
    if (n != resample_->h.size()) return fail(PBSO_ERR_INVALID, "resample_taps size mismatch (n = L * taps)");
    std::memcpy(out, resample_->h.data(), n * sizeof(float));
    return PBSO_OK;
}

// the history back to silence, t = m = p0 = 0.  Armed for the next step.
int Engine::resample_reset() {
    if (!resample_) return fail(PBSO_ERR_STATE, "resample_reset: the resampler is not enabled");
    Resample &r = *resample_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(r.hist.reset(stream_));
    r.rc.reset();
    r.clock.reset(tot_steps_);
    return PBSO_OK;
}

int Engine::resample_info(int64_t out[8]) {
    if (!resample_) return fail(PBSO_ERR_STATE, "resample_info: the resampler is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "resample_info: out is NULL");
    const Resample &r = *resample_;
    out[0] = r.rc.t;
    out[1] = r.rc.m;
    out[2] = r.n_calls;
    out[3] = r.L;
    out[4] = r.M;
    out[5] = r.T;
    out[6] = (int64_t)r.L * r.T - 1;
    out[7] = r.last_n_out;
    return PBSO_OK;
}

}  // namespace pbso
