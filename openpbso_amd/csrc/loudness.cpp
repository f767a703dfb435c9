// The engine's side of the loudness bus (include/openpbso_amd.h "Loudness bus"; kernels_loudness.hip): the K-weighting as one
// cascade of the EQ bus's block form (launch_eq_cascade with S = 2: its tables, its double-buffered history, its work rows), the
// true-peak phase table designed once at enable (resample_clock.h), the carries of an open sub-block, the log of records on the
// device, and the rule that every step is processed exactly once (bus_clock.h).  Its input is the caller's device buffer: of a
// step it reads the length only (last_nb_) and counts steps by tot_steps_.  The gating is host arithmetic (loudness_gate.h).  It
// knows bus_state.h and nothing of the other buses.
#include "bus_state.h"
#include "eq_block.h"
#include "loudness_gate.h"
#include "resample_clock.h"

#include <cstring>

namespace pbso {

struct Loudness {
    static constexpr int S = 2;                          // the shelf and the high-pass
    int C = 0, hs = 0, O = 0;
    bool true_peak = false;
    long long max_blocks = 0;
    std::vector<double> weight;                          // [C]
    std::vector<float> h;                                // [O][12]
    StepClock clock;
    int64_t n_calls = 0;
    DevMem<double> d_tab;                                // [C][S][5][P]
    DevMem<double> hist[2];                              // the pair; each [C][S + 1][EQ_HIST]
    DevMem<double> carry[2];                             // the pair; each [C][64]
    DevMem<unsigned> peaks[2];                           // the pair; each [C][2]
    int at = 0;
    HistPair tail;                                       // [C][11]
    DevMem<float> d_h;
    DevMem<pbso_loudness_block> log;                     // [max_blocks][C]
    DevMem<double> work;
    std::vector<double> tab;                             // as on the device
    size_t hist_words() const { return (size_t)C * (S + 1) * EQ_HIST; }
    long long logged() const { return clock.t / hs; }
    // every state silent; the log needs no clearing, a record is written before it counts as logged
    hipError_t silence(hipStream_t s) {
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipMemsetAsync(hist[i].p, 0, hist[i].cap * sizeof(double), s);
            if (e == hipSuccess) e = hipMemsetAsync(carry[i].p, 0, carry[i].cap * sizeof(double), s);
            if (e == hipSuccess) e = hipMemsetAsync(peaks[i].p, 0, peaks[i].cap * sizeof(unsigned), s);
            if (e != hipSuccess) return e;
        }
        at = 0;
        return tail.reset(s);
    }
};

static_assert(sizeof(pbso_loudness_block) == 16, "pbso_loudness_block is 16 bytes");
static_assert(sizeof(pbso_loudness_summary) == 80, "pbso_loudness_summary is 80 bytes");

static const BusWords WORDS = {"loudness", "measured", "the loudness bus", "signal", "measured step", "n_channels"};

void Engine::loudness_release() {
    if (!loudness_) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    delete loudness_;
    loudness_ = nullptr;
}

int Engine::loudness_enable(int C, const double *weight, int max_blocks, int true_peak) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "loudness_enable before finalize");
    if (const char *why = loudness_refusal(rate_, C, weight, max_blocks)) return fail(PBSO_ERR_INVALID, std::string("loudness_enable: ") + why);
    HIPTRY(hipSetDevice(desc_.device));
    std::unique_ptr<Loudness> q(new Loudness());
    q->C = C;
    q->hs = loudness_hop(rate_);
    q->O = loudness_oversampling(rate_);
    q->true_peak = true_peak != 0;
    q->max_blocks = max_blocks;
    q->weight.assign((size_t)C, 1.0);
    if (weight) q->weight.assign(weight, weight + C);
    resample_design(q->O, 1, LOUDNESS_TAPS, LOUDNESS_BETA, LOUDNESS_CUTOFF, q->h);
    double sos[2][5];
    loudness_design((double)rate_, sos);
    if (eq_refusal(&sos[0][0], 2)) return fail(PBSO_ERR_INVALID, "loudness_enable: the K-weighting is not stable at this sample rate");
    const size_t sec = (size_t)EQ_TABLES * EQ_BLOCK;
    q->tab.assign((size_t)C * Loudness::S * sec, 0.0);
    for (int c = 0; c < C; ++c)
        for (int s = 0; s < Loudness::S; ++s) pbso::eq_tables(sos[s], q->tab.data() + ((size_t)c * Loudness::S + s) * sec);
    auto nomem = [&](const char *what) {
        (void)hipGetLastError();
        return fail(PBSO_ERR_NOMEM, std::string("loudness_enable: cannot allocate ") + what);
    };
    if (q->d_tab.alloc(q->tab.size()) != hipSuccess) return nomem("the tables");
    for (int i = 0; i < 2; ++i)
        if (q->hist[i].alloc(q->hist_words()) != hipSuccess || q->carry[i].alloc((size_t)C * LOUDNESS_LANES) != hipSuccess ||
            q->peaks[i].alloc((size_t)C * 2) != hipSuccess)
            return nomem("the state");
    if (q->tail.create((size_t)C * LOUDNESS_TAIL, stream_) != hipSuccess) return nomem("the state");
    if (q->d_h.alloc(q->h.size()) != hipSuccess) return nomem("the phase table");
    if (q->log.alloc((size_t)max_blocks * C) != hipSuccess) return nomem("the log");
    // (q->tab and q->h outlive the copies: a Loudness is freed behind a synchronisation of the stream only)
    if (q->silence(stream_) != hipSuccess ||
        hipMemcpyAsync(q->d_tab, q->tab.data(), q->tab.size() * sizeof(double), hipMemcpyHostToDevice, stream_) != hipSuccess ||
        hipMemcpyAsync(q->d_h, q->h.data(), q->h.size() * sizeof(float), hipMemcpyHostToDevice, stream_) != hipSuccess)
        return nomem("the state");
    loudness_release();
    q->clock.arm(tot_steps_);
    loudness_ = q.release();
    return PBSO_OK;
}

int Engine::loudness(const void *d_in) {
    if (!loudness_) return fail(PBSO_ERR_STATE, "loudness: the loudness bus is not enabled");
    if (!d_in) return fail(PBSO_ERR_INVALID, "loudness: d_in is NULL");
    Loudness &q = *loudness_;
    if (last_nb_ <= 0) return fail(PBSO_ERR_STATE, "loudness: no step yet");
    if (const int order = q.clock.order(tot_steps_)) return fail(PBSO_ERR_STATE, step_refusal(order, WORDS));
    const long long n = (long long)last_nb_ * B_, t = q.clock.t;
    const LoudnessSpan sp = loudness_span(t, n, q.hs);
    if (sp.j0 + sp.n_complete > q.max_blocks)
        return fail(PBSO_ERR_STATE, "loudness: the log is full (max_blocks of the enable; pbso_loudness_reset starts over)");
    HIPTRY(hipSetDevice(desc_.device));
    GROWTRY(grow(q.work, eq_work_doubles(q.C, n), stream_), "loudness: work arrays: cannot allocate", "loudness: work arrays");
    const int at = q.at, nx = at ^ 1;
    // the first touched sub-block is below max_blocks unless nothing completes in this step; then no record is addressed
    pbso_loudness_block *log_j0 = q.log.p + (size_t)std::min(sp.j0, q.max_blocks - 1) * q.C;
    const double *z = nullptr;
    int lrc = launch_eq_cascade((const float *)d_in, n, q.C, Loudness::S, n, eq_block_offset(t, 0), q.hist[at].p, q.hist[nx].p, q.d_tab.p, q.work.p, &z, stream_);
    if (lrc == 0)
        lrc = launch_loudness_energy(z, EQ_HIST + n, EQ_HIST, q.C, n, q.hs, sp.k0, sp.n_touched, q.carry[at].p, q.carry[nx].p, q.peaks[at].p, q.peaks[nx].p,
                                     log_j0, stream_);
    if (lrc == 0 && q.true_peak)
        lrc = launch_loudness_peak((const float *)d_in, q.C, n, q.hs, sp.k0, q.O, q.tail.cur(), q.tail.next(), q.d_h.p, q.peaks[nx].p, log_j0, stream_);
    if (lrc != 0) return hip_fail((hipError_t)lrc, "launch_loudness");
    q.at = nx;
    if (q.true_peak) q.tail.flip();
    q.clock.advance(n, tot_steps_);
    ++q.n_calls;
    return PBSO_OK;
}

int Engine::read_loudness_blocks(int64_t first, int64_t n, pbso_loudness_block *out) {
    if (!loudness_) return fail(PBSO_ERR_STATE, "read_loudness_blocks: the loudness bus is not enabled");
    const Loudness &q = *loudness_;
    if (first < 0 || n < 0 || first > q.logged() || n > q.logged() - first)
        return fail(PBSO_ERR_INVALID, "read_loudness_blocks: first .. first + n must lie inside the logged blocks");
    if (n == 0) return PBSO_OK;
    if (!out) return fail(PBSO_ERR_INVALID, "read_loudness_blocks: out is NULL");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, q.log.p + (size_t)first * q.C, (size_t)n * q.C * sizeof(pbso_loudness_block), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

int Engine::loudness_report(pbso_loudness_summary *out) {
    if (!loudness_) return fail(PBSO_ERR_STATE, "loudness_report: the loudness bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "loudness_report: out is NULL");
    const Loudness &q = *loudness_;
    std::vector<pbso_loudness_block> blocks((size_t)q.logged() * q.C);
    if (const int rc = read_loudness_blocks(0, q.logged(), blocks.data())) return rc;
    if (!pbso::loudness_report(blocks.data(), q.logged(), q.C, q.weight.data(), q.hs, out)) return fail(PBSO_ERR_INVALID, "loudness_report");
    return PBSO_OK;
}

int Engine::loudness_taps(float *out, size_t n) {
    if (!loudness_) return fail(PBSO_ERR_STATE, "loudness_taps: the loudness bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "loudness_taps: out is NULL");
    if (n != loudness_->h.size()) return fail(PBSO_ERR_INVALID, "loudness_taps size mismatch (n = O * 12)");
    std::memcpy(out, loudness_->h.data(), n * sizeof(float));
    return PBSO_OK;
}

// the log empty, every state silent, t = 0.  Armed for the next step.
int Engine::loudness_reset() {
    if (!loudness_) return fail(PBSO_ERR_STATE, "loudness_reset: the loudness bus is not enabled");
    Loudness &q = *loudness_;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(q.silence(stream_));
    q.clock.reset(tot_steps_);
    return PBSO_OK;
}

int Engine::loudness_info(int64_t out[4]) {
    if (!loudness_) return fail(PBSO_ERR_STATE, "loudness_info: the loudness bus is not enabled");
    if (!out) return fail(PBSO_ERR_INVALID, "loudness_info: out is NULL");
    const Loudness &q = *loudness_;
    out[0] = q.clock.t;
    out[1] = q.logged();
    out[2] = q.n_calls;
    out[3] = q.max_blocks;
    return PBSO_OK;
}

}  // namespace pbso

// these need no engine; here and not in capi.cpp because this file is compiled without FMA contraction
extern "C" int pbso_loudness_design(double rate, double out[2][5]) {
    if (!out || pbso::loudness_design_refusal(rate)) return PBSO_ERR_INVALID;
    pbso::loudness_design(rate, out);
    return PBSO_OK;
}

extern "C" int pbso_loudness_report_from_blocks(const pbso_loudness_block *blocks, int64_t n_blocks, int n_channels, const double *weight, int hop,
                                                pbso_loudness_summary *out) {
    return pbso::loudness_report(blocks, n_blocks, n_channels, weight, hop, out) ? PBSO_OK : PBSO_ERR_INVALID;
}
