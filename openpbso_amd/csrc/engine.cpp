// Host engine: see engine.h.  Compiled by hipcc for the HIP runtime API only;
// there is no CPU compute path here -- every sample is produced by the HIP
// kernels in kernels_iir.hip / kernels_exact.hip.
#include "engine.h"
#include "plan_pool.h"
#include "submit_queue.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unordered_map>

#include <pthread.h>
#include <sched.h>

namespace pbso {

void PlanCtx::begin() {
    row_ptr.clear(); slot_idx.clear(); row_obj.clear(); stage_slot.clear(); chain_ptr.clear(); prow_obj.clear();
    tprof.clear(); prof_entries.clear(); prof_rows.clear(); stage.clear(); proj.clear(); proj_direct.clear(); ffat.clear();
    forced.clear(); freed_this_plan.clear(); freed_ar.clear(); strokes.clear();
    n_frows = n_prows = n_xfer = 0;
    n_stroke_rows = n_stroke_proj = 0;
    chain_obj = -1;
    rc = 0;
    err.clear();
}

// ---------------------------------------------------------------------------
// Blocks replaced by a larger one are not freed on the spot: launches already queued on either engine
// stream may still use them, and waiting for those would drain the whole device in the middle of a step --
// the caller's own work (torch, an RCCL gather) included.  They are parked here and freed the next time
// the engine is idle anyway (Engine::sync, destruction).
namespace {
std::mutex g_retired_mutex;
std::vector<void *> g_retired;
}  // namespace
void free_retired_blocks() {
    std::vector<void *> v;
    {
        std::lock_guard<std::mutex> lk(g_retired_mutex);
        v.swap(g_retired);
    }
    if (v.empty()) return;
    // the list is shared by the engines of a process (one per ModalSolver in the facade): another engine's
    // launches may still use a block parked here, so this rare path waits for the whole device
    (void)hipDeviceSynchronize();
    for (void *q : v) (void)hipFree(q);
}
// Does something in this process's environment let only ONE kernel run at a time?  Returns its name, or nullptr.
//   rocprofv3 --pmc (rocprofiler-sdk counter collection serialises dispatches): ROCPROF_COUNTER_COLLECTION / ROCPROF_COUNTERS
//   are set for the profiled process; the older rocprof sets ROCP_METRICS / ROCPROFILER_METRICS.  A kernel trace alone
//   does not serialise (the default command runs under --kernel-trace --stats with the gate).
//   AMD_SERIALIZE_KERNEL (HIP: wait before / after every kernel launch), HIP_LAUNCH_BLOCKING / CUDA_LAUNCH_BLOCKING.
//   PBSO_START_GATE=0 says so by hand (a tool this list does not know); PBSO_START_GATE=1 overrides the list.
static const char *serialising_environment() {
    if (const char *v = std::getenv("PBSO_START_GATE")) return std::atoi(v) ? nullptr : "PBSO_START_GATE=0";
    auto on = [](const char *name) {
        const char *v = std::getenv(name);
        return v && *v && std::strcmp(v, "0") != 0;
    };
    static const char *const names[] = {"ROCPROF_COUNTER_COLLECTION", "ROCPROF_COUNTERS", "ROCPROF_PMC", "ROCP_METRICS", "ROCPROFILER_METRICS",
                                        "ROCPROFILER_PC_SAMPLING_BETA_ENABLED", "AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "CUDA_LAUNCH_BLOCKING"};
    for (const char *n : names)
        if (on(n)) return n;
    return nullptr;
}
std::atomic<long long> g_alloc_events{0};       // buffer (re)allocations so far (PBSO_TIMELINE diagnostics)
template <class T>
hipError_t DevBuf<T>::ensure(size_t n, bool keep, hipStream_t s) {
    if (n <= cap) return hipSuccess;
    g_alloc_events += 1;
    // 25 % headroom: per-step demand (forced rows, slots) fluctuates by a few percent
    size_t ncap = std::max(n + n / 4, cap + cap / 2);
    T *np = nullptr;
    hipError_t e = hipMalloc((void **)&np, ncap * sizeof(T));
    if (e != hipSuccess) return e;
    if (p) {
        // `keep`: the contents move in stream order on s -- every writer and reader of a kept buffer is ordered
        // after s (the preparation stream, or an event chain from it), so nobody sees the new block before the copy
        if (keep && cap) {
            e = hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
        }
        std::lock_guard<std::mutex> lk(g_retired_mutex);
        g_retired.push_back(p);
    }
    p = np;
    cap = ncap;
    return hipSuccess;
}
template <class T>
void DevBuf<T>::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}
template <class T>
hipError_t PinBuf<T>::ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    size_t ncap = std::max(n + n / 4, cap + cap / 2);
    T *np = nullptr;
    hipError_t e = hipHostMalloc((void **)&np, ncap * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return e;
    if (p) (void)hipHostFree(p);
    p = np;
    cap = ncap;
    return hipSuccess;
}
// grows and keeps the first `keep` elements (the plan's fixed front part is written in place before the
// variable part is known)
template <class T>
hipError_t PinBuf<T>::ensure_keep(size_t n, size_t keep) {
    if (n <= cap) return hipSuccess;
    g_alloc_events += 1000;
    size_t ncap = std::max(n + n / 4, cap + cap / 2);
    T *np = nullptr;
    hipError_t e = hipHostMalloc((void **)&np, ncap * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return e;
    if (p) {
        if (keep) std::memcpy(np, p, std::min(keep, cap) * sizeof(T));
        (void)hipHostFree(p);
    }
    p = np;
    cap = ncap;
    return hipSuccess;
}
template <class T>
void PinBuf<T>::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

// every element type the engine's files use (the definitions above are in this file only)
template struct DevBuf<float>;
template struct DevBuf<double>;
template struct DevBuf<int>;
template struct DevBuf<unsigned>;
template struct DevBuf<long long>;
template struct DevBuf<unsigned long long>;
template struct DevBuf<unsigned char>;
template struct DevBuf<TeamDesc>;
template struct DevBuf<SplitObj>;
template struct DevBuf<FfatGeom>;
template struct DevBuf<FfatShared>;
template struct DevBuf<ArState>;
template struct DevBuf<ArRec>;
template struct DevBuf<ArFin>;
template struct PinBuf<unsigned char>;

void Engine::PlanSet::release() {
    h_arena.release(); d_arena.release(); d_tprof.release();
}

// ---------------------------------------------------------------------------
// forces.h
ForceProfile ForceProfile::make(int type, double gaussian_width_us, int sample_rate) {
    ForceProfile f;
    f.type = type;
    if (type == PBSO_GAUSSIAN_FORCE) {                       // forces.h:42-46
        f.width = gaussian_width_us;
        f.width_samples = std::max(1, (int)(f.width / 1000000. * sample_rate));
        f.center = (int)((f.cutoff - 0.5) * f.width_samples);
    }
    return f;
}

// the tiles that samples [first, first + n) of a buffer intersect, n > 0 (BufDesc::tile_mask)
static inline uint32_t tiles_of(int first, int n) {
    const int lo = first / TILE, hi = (first + n - 1) / TILE;
    return (hi >= 31 ? 0xFFFFFFFFu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
}

// TrackForce::Add's bookkeeping (include/openpbso_amd.h): `for i = o .. frames - 1, k = k0 + (i - o), while k < N`
bool ForceProfile::track_span(int frames, int *first_index, int *n_live, int64_t *k0) {
    Track &t = *track;
    if (t.k0 >= t.total) return false;
    const int o = t.offset;
    *first_index = o;
    *k0 = t.k0;
    *n_live = (int)std::min<int64_t>(frames - o, t.total - t.k0);
    t.k0 += frames - o;
    t.offset = 0;
    return true;
}

// x(p) of a track (include/openpbso_amd.h): the arithmetic of track_add in kernels_exact.hip, in its order (no FMA: see track_sample_at's
// callers -- the expression is written so that the compiler has nothing to contract)
static double track_value(const float *s, int64_t L, bool loop, double first, double rate, double gain, int64_t k) {
    volatile double prod = rate * (double)k;               // (volatile: the product and the sum round separately on every host compiler)
    const double p = first + prod;
    double x = 0.0;
    if (p >= 0.0 && p < 9.0e18) {
        const double fl = std::floor(p);
        const double f = p - fl;
        int64_t i0 = (int64_t)fl, i1;
        double s0 = 0.0, s1 = 0.0;
        if (loop) {
            i0 %= L;
            i1 = i0 + 1 == L ? 0 : i0 + 1;
            s0 = (double)s[i0];
            s1 = (double)s[i1];
        } else {
            i1 = i0 + 1;
            if (i0 < L) s0 = (double)s[i0];
            if (i1 < L) s1 = (double)s[i1];
        }
        volatile double d = f * (s1 - s0);
        x = s0 + d;
    }
    return gain * x;
}

bool ForceProfile::add(double *t, int frames, int *extent, uint32_t *live_tiles) {
    switch (type) {
    case PBSO_POINT_FORCE:                                   // forces.h:81-90
        if (used) return false;
        t[0] += 1.;
        used = true;
        *extent = std::max(*extent, 1);
        return true;
    case PBSO_GAUSSIAN_FORCE:                                // forces.h:92-105
        if (width == 0 || count >= cutoff * 2 * width_samples) return false;
        *extent = frames;
        for (int ii = 0; ii < frames; ++ii) {
            const double p = -0.5 * std::pow((double)(count + ii - center) / (double)width_samples, 2);
            t[ii] += std::exp(p);
        }
        count += frames;
        return true;
    case PBSO_AUTOREGRESSIVE_FORCE:                          // forces.h:107-128
        *extent = frames;
        for (int ii = 0; ii < frames; ++ii) {
            double mu_tilde = 0.0;
            for (int jj = 0; jj < 2; ++jj) mu_tilde += a[jj] * buf[(buf_idx + 3 - jj - 1) % 3];
            mu_tilde += sigma * distribution(generator);
            buf[buf_idx] = mu_tilde;
            buf_idx = (buf_idx + 1) % 3;
            t[ii] += mu + mu_tilde;
        }
        return true;
    case PBSO_TRACK_FORCE: {
        int o, n_live;
        int64_t k0;
        if (!track_span(frames, &o, &n_live, &k0)) return false;
        *extent = std::max(*extent, o + n_live);
        for (int j = 0; j < n_live; ++j)
            t[o + j] += track_value(track->samples, track->len, track->play.loop != 0, track->play.first, track->play.rate, track->play.gain, k0 + j);
        if (live_tiles && n_live > 0) *live_tiles |= tiles_of(o, n_live);
        return true;
    }
    }
    return false;
}

void ForceProfile::set_param(const double a_[2], double sigma_, double mu_) {   // forces.h:130-137
    buf[0] = buf[1] = buf[2] = 0;
    a[0] = a_[0];
    a[1] = a_[1];
    sigma = sigma_;
    mu = mu_;
}

// ---------------------------------------------------------------------------
Engine::Engine(const pbso_engine_desc &d) : desc_(d) {}

Engine::~Engine() {
    for (Object &o : objs_)
        while (!o.force_q.empty()) { std::free(o.force_q.front().ext); o.force_q.pop_front(); }
    if (host_profile_ && tot_steps_ > 0)
        std::fprintf(stderr, "pbso host profile, ms per step over %lld steps: wait-for-set %.3f | plan: fill %.3f objects %.3f merge %.3f | "
                             "submit (uploads + launches) %.3f = pack + upload %.3f, preparation launches %.3f, bank launches %.3f | step total %.3f\n",
                     (long long)tot_steps_, hprof_[0] / tot_steps_, hprof_[1] / tot_steps_, hprof_[2] / tot_steps_, hprof_[3] / tot_steps_,
                     hprof_[4] / tot_steps_, hprof_[6] / tot_steps_, hprof_[7] / tot_steps_, hprof_[8] / tot_steps_, hprof_[5] / tot_steps_);
    delete pool_;
    delete submit_;                                    // (the worker makes what it still holds, then ends)
    submit_ = nullptr;
    scene_mix_release();
    scene_fir_release();
    scene_reverb_release();
    master_release();
    resample_release();
    eq_release();
    loudness_release();
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (aux_stream_) (void)hipStreamSynchronize(aux_stream_);
    if (timeline_have_base_) {                         // (the reference launch's quad was kept out of the free list)
        for (hipEvent_t ev : {timeline_quad_.k0, timeline_quad_.k1, timeline_quad_.p0, timeline_quad_.p1, timeline_quad_.f0, timeline_quad_.f1})
            if (ev) (void)hipEventDestroy(ev);
    }
    if (prep_stream_) (void)hipStreamSynchronize(prep_stream_);
    for (int i = 0; i < N_SETS; ++i) {
        float ms = 0.f;
        if (stroke_ev_live_[i] && hipEventElapsedTime(&ms, stroke_ev_[i][0], stroke_ev_[i][1]) == hipSuccess) { stroke_kernel_ms_ += ms; stroke_kernel_n_ += 1; }
        for (int j = 0; j < 2; ++j)
            if (stroke_ev_[i][j]) (void)hipEventDestroy(stroke_ev_[i][j]);
    }
    if (host_profile_ && stroke_kernel_n_ > 0)
        std::fprintf(stderr, "pbso stroke kernel: %.4f ms per launch over %lld launches (HIP events)\n", stroke_kernel_ms_ / stroke_kernel_n_,
                     (long long)stroke_kernel_n_);
    free_retired_blocks();
    track_release();
    d_ca_.release(); d_cb_.release(); d_sq_.release(); d_sd_.release(); d_ss_.release(); d_c3_.release(); d_gq_.release();
    d_shapes_.release(); d_shape_off_.release(); d_g32_.release(); d_g32_off_.release(); d_n_modes_.release(); d_geom_.release();
    d_geom_off_.release(); d_psi_.release(); d_psi_t_.release(); d_ffat_k_.release(); d_ffat_valid_.release(); d_ffat_shared_.release(); d_slots_.release(); d_xfer_.release();
    d_pc_.release(); d_wtab_.release(); d_ftab_.release(); d_dump_row_.release(); d_xdump_.release(); d_xscale_.release(); d_wtab32_.release();
    d_ar_snaps_.release(); d_ar_vnorm_.release(); d_ar_cbuf_.release(); d_ar_vstate_.release(); d_ar_segcount_.release();
    d_ar_recs_.release(); d_ar_fins_.release();
    d_arstate_.release(); d_board_.release(); d_teams_.release(); d_split_.release(); d_ts_teams_.release(); d_ts_split_.release();
    d_audio_parts_.release(); d_audio_.release(); d_qnorm_.release(); d_mix_parts_.release();
    d_audio_host_[0].release(); d_audio_host_[1].release();
    if (copy_stream_) {
        (void)hipStreamSynchronize(copy_stream_);
        (void)hipStreamDestroy(copy_stream_);
        for (int i = 0; i < 2; ++i) { (void)hipEventDestroy(ev_host_bank_[i]); (void)hipEventDestroy(ev_host_copy_[i]); }
    }
    d_census_.release();
    h_retune_.release(); d_retune_.release();
    for (hipEvent_t ev : retune_ev_)
        if (ev) (void)hipEventDestroy(ev);
    d_scan_.release();
    for (int i = 0; i < N_SETS; ++i) { d_xs_[i].release(); d_xtrow_[i].release(); d_vinc_[i].release(); }
    for (TcSet &ts : tc_) { ts.d_teams.release(); ts.d_split.release(); }
    for (DevBuf<float> &g : d_grows_) g.release();
    for (int i = 0; i < N_SETS; ++i)
        for (hipEvent_t ev : {ev_prep_done_[i], ev_k1_done_[i], ev_set_[i], ev_aux_fork_[i], ev_aux_join_[i]})
            if (ev) (void)hipEventDestroy(ev);
    if (prep_stream_) (void)hipStreamDestroy(prep_stream_);
    if (aux_stream_) (void)hipStreamDestroy(aux_stream_);
    if (sig_prep_) (void)hipFree(sig_prep_);
    if (sig_start_) (void)hipFree(sig_start_);
    if (host_start_) (void)hipHostFree(host_start_);
    for (hipStream_t cs : class_stream_)
        if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
    if (ev_fork_) (void)hipEventDestroy(ev_fork_);
    for (hipEvent_t ev : ev_join_)
        if (ev) (void)hipEventDestroy(ev);
    for (PlanSet &ps : set_) ps.release();
    for (auto *v : {&ev_free_, &ev_pending_})
        for (EvQuad &q : *v)
            for (hipEvent_t ev : {q.k0, q.k1, q.p0, q.p1, q.f0, q.f1}) (void)hipEventDestroy(ev);
    if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

int Engine::fail(int code, const std::string &msg) {
    err_ = msg;
    return code;
}
int Engine::hip_fail(hipError_t e, const char *what) {
    err_ = std::string(what) + ": " + hipGetErrorString(e);
    return PBSO_ERR_HIP;
}
int Engine::init() {
    if (desc_.abi_version != PBSO_ABI_VERSION) return fail(PBSO_ERR_INVALID, "abi_version mismatch");
    if (desc_.frames_per_buffer > 0) B_ = desc_.frames_per_buffer;
    if (desc_.sample_rate > 0) rate_ = desc_.sample_rate;
    if (B_ % TILE != 0 || B_ / TILE > MAX_TILES)
        return fail(PBSO_ERR_INVALID, "frames_per_buffer must be a multiple of the 27-sample tile (at most 32 tiles); the reference uses 513");
    n_tiles_ = B_ / TILE;
    b_pad_ = (B_ + 15) / 16 * 16;
    if (desc_.recurrence_form != PBSO_FORM_BLOCK && desc_.recurrence_form != PBSO_FORM_BLOCK_BF16 && desc_.recurrence_form != PBSO_FORM_VELOCITY &&
        desc_.recurrence_form != PBSO_FORM_DIRECT)
        return fail(PBSO_ERR_INVALID, "recurrence_form");
    form_ = desc_.recurrence_form;
    // the block form tiles a buffer as 1 + 2 * 16 * 16 samples (the reference's 513); other lengths step per sample
    if (is_block() && B_ != 1 + 2 * BLOCK_J * BLOCK_N) form_ = PBSO_FORM_VELOCITY;
    // Launches that are mostly dense-profile buffers (sustained scraping): the f32 block kernel runs them in block form
    // itself (forced block path); the split-bf16 build has no such path and hands them to the per-sample kernel K1.
    // PBSO_DENSE_LAUNCHES=block|sample pins either; PBSO_FORCED_BLOCK=0 makes the block kernel step dense buffers per sample.
    dense_to_k1_ = form_ == PBSO_FORM_BLOCK_BF16;
    forced_block_ = desc_.forced_block >= 0;
    if (!forced_block_) dense_to_k1_ = true;
    if (desc_.dense_launches < 0 || desc_.dense_launches > 2) return fail(PBSO_ERR_INVALID, "dense_launches");
    if (desc_.dense_launches) dense_to_k1_ = desc_.dense_launches == 2;
    if (desc_.bank_kernel < PBSO_BANK_AUTO || desc_.bank_kernel > PBSO_BANK_PIPE) return fail(PBSO_ERR_INVALID, "bank_kernel");
    if (desc_.profile_kernel < 0 || desc_.profile_kernel > 2) return fail(PBSO_ERR_INVALID, "profile_kernel");
    if (desc_.pipe_consumers < 0 || desc_.pipe_consumers > 4) return fail(PBSO_ERR_INVALID, "pipe_consumers");
    if (desc_.profile_priority < 0 || desc_.profile_priority > 4) return fail(PBSO_ERR_INVALID, "profile_priority");
    if (desc_.stream_sync < 0 || desc_.stream_sync > 4) return fail(PBSO_ERR_INVALID, "stream_sync");
    latency_path_ = desc_.latency_path >= 0;
    fuse_short_ = desc_.fuse_short_launches >= 0;
    if (desc_.submit_thread > 0 && desc_.stream_sync == 4)
        return fail(PBSO_ERR_INVALID, "submit_thread with stream_sync = 4: the host-side gate would make the caller wait for the worker's launches");
    if (desc_.qnorm_mode < PBSO_QNORM_OFF || desc_.qnorm_mode > PBSO_QNORM_CLOSED)
        return fail(PBSO_ERR_INVALID, "qnorm_mode");
    {
        const int r = desc_.modes_per_lane;
        if (r != 0 && r != 1 && r != 2 && r != 3 && r != 4 && r != 8) return fail(PBSO_ERR_INVALID, "modes_per_lane must be 0,1,2,3,4,8");
    }
    int ndev = 0;
    HIPTRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(PBSO_ERR_HIP, "no HIP device: this engine has no CPU fallback");
    if (desc_.device < 0 || desc_.device >= ndev) return fail(PBSO_ERR_INVALID, "device ordinal out of range");
    HIPTRY(hipSetDevice(desc_.device));
    {
        // sizes of the chip (or of the partition this ordinal is: a CPX / NPS slice has fewer CUs)
        hipDeviceProp_t prop;
        HIPTRY(hipGetDeviceProperties(&prop, desc_.device));
        n_cus_ = std::max(1, prop.multiProcessorCount);
    }
    if (desc_.stream) {
        stream_ = (hipStream_t)desc_.stream;
    } else {
        HIPTRY(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        own_stream_ = true;
    }
    for (int i = 0; i < N_SETS; ++i) HIPTRY(hipEventCreateWithFlags(&ev_set_[i], hipEventDisableTiming));
    // preparation of step k+1 (plan upload, projection, FFAT lookup, force combination)
    // runs on its own stream beside the oscillator bank of step k
    // High priority: its kernels are small, the oscillator bank waits for them, and the runtime maps
    // streams of different priority to different hardware queues -- with equal priority the two
    // engine streams can land on ONE queue when the process owns many streams (torch + RCCL under
    // torch.distributed.run did exactly that: no overlap, +12 % per step).
    {
        int least = 0, greatest = 0;
        HIPTRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPTRY(hipStreamCreateWithPriority(&prep_stream_, hipStreamNonBlocking, greatest));
        prep_priority_ = greatest;
    }
    // A start gate that waits ON THE DEVICE is a kernel spinning on a memory word another kernel stores when it starts.  Anything that
    // lets only one kernel run at a time can dispatch the waiting kernel first -- it then never ends (round 6: every rocprofv3 --pmc
    // pass of the headline launch hung until its time limit with the gate and finished in 11 s without; profiles/NOTES.md).  Under the
    // policy (stream_sync = 0) such an environment gets no gate; 2 / 3 stay the caller's explicit choice.
    const char *serial_env = serialising_environment();
    if (desc_.stream_sync == 0 && serial_env) {
        gate_choice_ = -1;
        if (std::getenv("PBSO_TIMELINE")) std::fprintf(stderr, "openpbso_amd: no start gate: %s serialises kernel dispatches\n", serial_env);
    }
    if (desc_.stream_sync != 1 && gate_choice_ != -1) {
        // the HOST form of the start gate (stream_sync = 4, an option: see step_chunk): a word of pinned host memory the bank's first
        // workgroup writes and the submitting thread reads -- no waiting kernel on the device
        void *dptr = nullptr;
        if (hipHostMalloc((void **)&host_start_, sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer(&dptr, host_start_, 0) == hipSuccess) {
            *host_start_ = 0;
            host_start_dev_ = static_cast<unsigned long long *>(dptr);
        } else {
            if (host_start_) (void)hipHostFree(host_start_);
            host_start_ = nullptr;
            (void)hipGetLastError();
        }
        int can = 0;
        auto signal_word = [&](unsigned long long **p) {
            if (hipExtMallocWithFlags((void **)p, sizeof(unsigned long long), hipMallocSignalMemory) != hipSuccess) { *p = nullptr; return false; }
            return hipMemset(*p, 0, sizeof(unsigned long long)) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        };
        if (hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, desc_.device) == hipSuccess && can) {
            start_gate_ = signal_word(&sig_start_);
            if (desc_.stream_sync == 2 || desc_.stream_sync == 0) sync_values_ = signal_word(&sig_prep_);      // (0: for short launches, step_chunk)
        }
        (void)hipGetLastError();
        if ((desc_.stream_sync == 2 || desc_.stream_sync == 3) && !(desc_.stream_sync == 2 ? sync_values_ : start_gate_))
            return fail(PBSO_ERR_HIP, "stream_sync = 2 / 3: the device has no hipStreamWaitValue64");
        if (desc_.stream_sync == 4 && !host_start_)
            return fail(PBSO_ERR_HIP, "stream_sync = 4: no pinned host memory for the gate's word");
        gate_choice_ = desc_.stream_sync == 4 ? 2 : start_gate_ ? 1 : 0;
    }
    // (waited for by the engine's own streams only, never by the host or another device: without the system-scope fence
    //  a record costs the stream nothing -- 4 us with it, scripts/microbench/wait_value.hip; +0.4 % per step at 1024 x 512)
    constexpr unsigned device_event_flags = hipEventDisableTiming | hipEventDisableSystemFence;
    for (int i = 0; i < N_SETS; ++i) {
        HIPTRY(hipEventCreateWithFlags(&ev_prep_done_[i], device_event_flags));
        HIPTRY(hipEventCreateWithFlags(&ev_k1_done_[i], device_event_flags));
        HIPTRY(hipEventCreateWithFlags(&ev_aux_fork_[i], device_event_flags));
        HIPTRY(hipEventCreateWithFlags(&ev_aux_join_[i], device_event_flags));
    }
    plan_threads_ = std::min(16, std::max(1, desc_.plan_threads));
    ctx_.resize(plan_threads_);
    for (PlanCtx &c : ctx_) c.tbuf.assign(B_, 0.0);
    // which build of the oscillator bank to launch (see kernels_iir.hip)
    if (const char *v = std::getenv("PBSO_CENSUS")) census_ = std::atoi(v) != 0;
    if (const char *v = std::getenv("PBSO_ROTATE_PRIO")) rotate_prio_ = std::min(2, std::max(0, std::atoi(v)));
    if (const char *v = std::getenv("PBSO_TIMELINE")) timeline_ = std::atoi(v) != 0;
    if (const char *v = std::getenv("PBSO_PREP_SPLIT")) prep_split_ = std::min(2, std::max(0, std::atoi(v)));
    host_profile_ = std::getenv("PBSO_HOST_PROFILE") != nullptr;
    if (host_profile_)
        for (int i = 0; i < N_SETS; ++i)
            for (int j = 0; j < 2; ++j) HIPTRY(hipEventCreate(&stroke_ev_[i][j]));
    // which kernels run and how: per engine, from the descriptor (ABI 4); the environment only switches diagnostics on
    device_profiles_ = desc_.device_profiles >= 0;
    k2_rows_ = desc_.profile_kernel == 0;
    ar_serial_ = desc_.profile_kernel == 2;
    if (desc_.profile_margin_pct > 0) k2_margin_pct_ = std::min(400, desc_.profile_margin_pct);
    if (desc_.profile_priority > 0) { k2_prio_ = desc_.profile_priority - 1; k2_prio_auto_ = false; }
    direct_hits_ = desc_.direct_hits >= 0;
    timing_every_ = desc_.timing_every < 0 ? 0 : std::max(1, desc_.timing_every);
    if (desc_.chunk_buffers > 0) chunk_buffers_ = desc_.chunk_buffers;
    tc_mode_ = desc_.time_chunks;
    tc_shape_ = desc_.time_chunk_shape;
    if (desc_.scan_kernel < 0 || desc_.scan_kernel > 2) return fail(PBSO_ERR_INVALID, "scan_kernel");
    return PBSO_OK;
}

// ---------------------------------------------------------------------------
// ModalSolver::enqueueForceMessage, modal_solver.h:329-333
int Engine::enqueue_force_impl(int obj, const pbso_force_msg &m, int64_t not_before, const char **why, const pbso_track_play *play,
                               int64_t track_total) {
    if (!finalized_) { *why = "enqueue_force before finalize"; return PBSO_ERR_STATE; }
    if (!valid_obj(obj)) { *why = "object id"; return PBSO_ERR_INVALID; }
    Object &o = objs_[obj];
    if (m.force_type < PBSO_POINT_FORCE || m.force_type > (play ? PBSO_TRACK_FORCE : PBSO_AUTOREGRESSIVE_FORCE))
        { *why = m.force_type == PBSO_TRACK_FORCE ? "a track force needs a play record: pbso_enqueue_track_force" : "unrecognized force type";
          return PBSO_ERR_INVALID; }                                               // assert modal_solver.h:73
    HostForceMsg h;
    h.force_type = m.force_type;
    h.sustained_start = m.sustained_force_start != 0;
    h.sustained_end = m.sustained_force_end != 0;
    h.clear_all = m.clear_all_forces != 0;
    h.data_kind = m.data_kind;
    h.not_before = not_before;
    // (the Force object itself is built when the message is dequeued)
    const bool need_ext = play || m.data_kind == PBSO_DATA_FACE || m.gaussian_width_us != 0.0 ||
                          (m.data_kind == PBSO_DATA_EXPLICIT && !h.clear_all);
    auto make_ext = [&](int n_data) {
        MsgExt *x = (MsgExt *)std::malloc(sizeof(MsgExt) + sizeof(double) * (size_t)(n_data > 0 ? n_data - 1 : 0) + (play ? sizeof(TrackExt) : 0));
        x->coords[0] = m.coords[0]; x->coords[1] = m.coords[1]; x->coords[2] = m.coords[2];
        x->gaussian_width_us = m.gaussian_width_us;
        x->n_data = n_data;
        if (play) { track_ext(x)->play = *play; track_ext(x)->total = track_total; }
        return x;
    };
    switch (m.data_kind) {
    case PBSO_DATA_EXPLICIT:
        // a clearAllForces message returns from step() before any dimension check (modal_solver.h:186-189):
        // the GUI sends it with an empty data vector (tools/real_time_modal_sound.cpp:745-747)
        if (h.clear_all) { h.data_kind = PBSO_DATA_ZERO; break; }
        if (!m.data || m.n_data != o.n_modes)
            { *why = "dimension of force message incorrect"; return PBSO_ERR_INVALID; }   // assert :258
        h.ext = make_ext(m.n_data);
        if (m.n_data) std::memcpy(h.ext->data, m.data, sizeof(double) * (size_t)m.n_data);
        break;
    case PBSO_DATA_VERTEX:
    case PBSO_DATA_FACE: {
        if (!o.n_dof) { *why = "object has no mode shapes for on-device projection"; return PBSO_ERR_INVALID; }
        const int nv = o.n_dof / 3;
        const int cnt = m.data_kind == PBSO_DATA_VERTEX ? 1 : 3;
        for (int j = 0; j < cnt; ++j)
            if (m.vids[j] < 0 || m.vids[j] >= nv) { *why = "vertex id out of range"; return PBSO_ERR_INVALID; }
        for (int j = 0; j < 3; ++j) {
            h.vids[j] = m.vids[j];
            h.vn[j] = m.vn[j];
        }
        break;
    }
    case PBSO_DATA_ZERO:
        break;
    default:
        { *why = "data_kind"; return PBSO_ERR_INVALID; }
    }
    if (o.force_q.size() >= 1023) { std::free(h.ext); return 0; }      // ReaderWriterQueue(512): ceilToPow2(513)-1 usable slots
    if (need_ext && !h.ext) h.ext = make_ext(0);
    // keep arrival order monotone: a message cannot overtake an earlier one (FIFO)
    if (!o.force_q.empty()) h.not_before = std::max(h.not_before, o.force_q.back().not_before);
    o.force_q.push_back(std::move(h));
    return 1;
}

// pbso_enqueue_vertex_hits: a step's plain vertex hits as borrowed parallel arrays, object by object.
int Engine::enqueue_vertex_hits(int n, const int *objs, const int *vids, const double *vn, const int64_t *stamps) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "enqueue_vertex_hits before finalize");
    if (script_.n > 0) return fail(PBSO_ERR_STATE, "a hit script is already pending (one per step)");
    if (n == 0) return 0;
    const int N = (int)objs_.size();
    hit_off_.assign((size_t)N + 1, 0);
    int prev = 0;
    for (int i = 0; i < n; ++i) {
        const int o = objs[i];
        if (o < prev || o >= N) return fail(PBSO_ERR_INVALID, "enqueue_vertex_hits: object ids must be valid and ascending");
        const int n_dof = objs_[o].n_dof;
        if (vids[i] < 0 || 3 * vids[i] + 2 >= n_dof)
            return fail(PBSO_ERR_INVALID, n_dof ? "vertex id out of range" : "object has no mode shapes for on-device projection");
        prev = o;
        hit_off_[(size_t)o + 1] = i + 1;
    }
    for (int o = 0; o < N; ++o)                       // objects without hits: an empty range at the running offset
        if (hit_off_[(size_t)o + 1] < hit_off_[o]) hit_off_[(size_t)o + 1] = hit_off_[o];
    script_ = HitScript();
    script_.n = n; script_.objs = objs; script_.vids = vids; script_.vn = vn; script_.stamps = stamps;
    return n;
}

// pbso_enqueue_strokes: a step's stroke entries (face data or the dummy start / stop messages, with the sustained flags) as
// borrowed parallel arrays, object by object -- the vertex-hit script's rules word for word.
int Engine::enqueue_strokes(int n, const int *objs, const int *vids, const double *coords, const double *vn, const int64_t *stamps,
                            const unsigned char *flags, int force_type) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "enqueue_strokes before finalize");
    if (script_.n > 0) return fail(PBSO_ERR_STATE, "a hit script is already pending (one per step)");
    if (force_type != PBSO_POINT_FORCE && force_type != PBSO_AUTOREGRESSIVE_FORCE)
        return fail(PBSO_ERR_INVALID, "enqueue_strokes: force_type must be point or autoregressive (a Gaussian needs a width per message)");
    if (n == 0) return 0;
    const int N = (int)objs_.size();
    hit_off_.assign((size_t)N + 1, 0);
    int prev = 0;
    for (int i = 0; i < n; ++i) {
        const int o = objs[i];
        if (o < prev || o >= N) return fail(PBSO_ERR_INVALID, "enqueue_strokes: object ids must be valid and ascending");
        if (!(flags && (flags[i] & STROKE_ZERO))) {
            const int n_dof = objs_[o].n_dof;
            if (!n_dof) return fail(PBSO_ERR_INVALID, "object has no mode shapes for on-device projection");
            for (int j = 0; j < 3; ++j) {
                const int v = vids[3 * (size_t)i + j];
                if (v < 0 || v >= n_dof / 3) return fail(PBSO_ERR_INVALID, "vertex id out of range");
            }
        }
        prev = o;
        hit_off_[(size_t)o + 1] = i + 1;
    }
    for (int o = 0; o < N; ++o)
        if (hit_off_[(size_t)o + 1] < hit_off_[o]) hit_off_[(size_t)o + 1] = hit_off_[o];
    script_ = HitScript();
    script_.n = n; script_.objs = objs; script_.vids = vids; script_.vn = vn; script_.stamps = stamps;
    script_.strokes = true; script_.coords = coords; script_.flags = flags; script_.force_type = force_type;
    return n;
}

void Engine::stroke_stats(int64_t out[4]) const {
    out[0] = stroke_direct_.load();
    out[1] = stroke_queued_.load();
    out[2] = stroke_dropped_.load();
    out[3] = tot_stroke_launches_;
}

// hits h0 .. h1 - 1 of the script (all of object oi) enter the object's queue exactly as pbso_enqueue_force would put them: a
// full queue (1023 slots, modal_solver.h:105) REJECTS a message -- try_enqueue returns false, modal_solver.h:329-333, and the tool
// ignores it (tools/real_time_modal_sound.cpp:610) -- so the hits that do not fit are dropped and counted, nothing fails
int Engine::script_to_queue(int oi, int h0, int h1, const char **why) {
    (void)why;
    Object &o = objs_[oi];
    if (script_.strokes) {
        // entry h as pbso_enqueue_force would queue it (enqueue_force_impl: the same fields, the same heap block for a face)
        for (int h = h0; h < h1; ++h) {
            if (o.force_q.size() >= 1023) { dropped_hits_.fetch_add(h1 - h); stroke_dropped_.fetch_add(h1 - h); break; }
            const int fl = script_.flags ? script_.flags[h] : 0;
            HostForceMsg m;
            m.force_type = (int8_t)script_.force_type;
            m.sustained_start = (fl & STROKE_START) != 0;
            m.sustained_end = (fl & STROKE_END) != 0;
            m.not_before = script_.stamps[h];
            if (fl & STROKE_ZERO) {
                m.data_kind = PBSO_DATA_ZERO;
            } else {
                m.data_kind = PBSO_DATA_FACE;
                m.ext = (MsgExt *)std::malloc(sizeof(MsgExt));
                m.ext->gaussian_width_us = 0.0;
                m.ext->n_data = 0;
                for (int j = 0; j < 3; ++j) {
                    m.vids[j] = script_.vids[3 * (size_t)h + j];
                    m.vn[j] = script_.vn[3 * (size_t)h + j];
                    m.ext->coords[j] = script_.coords[3 * (size_t)h + j];
                }
            }
            if (!o.force_q.empty()) m.not_before = std::max(m.not_before, o.force_q.back().not_before);
            o.force_q.push_back(std::move(m));
            stroke_queued_.fetch_add(1);
        }
        return PBSO_OK;
    }
    for (int h = h0; h < h1; ++h) {
        if (o.force_q.size() >= 1023) { dropped_hits_.fetch_add(h1 - h); break; }
        HostForceMsg m;
        m.force_type = PBSO_POINT_FORCE;
        m.data_kind = PBSO_DATA_VERTEX;
        m.not_before = script_.stamps[h];
        m.vids[0] = script_.vids[h];
        for (int j = 0; j < 3; ++j) m.vn[j] = script_.vn[3 * (size_t)h + j];
        if (!o.force_q.empty()) m.not_before = std::max(m.not_before, o.force_q.back().not_before);
        o.force_q.push_back(std::move(m));
    }
    return PBSO_OK;
}

int Engine::flush_script() {
    if (script_.n <= 0) return PBSO_OK;
    const int N = (int)objs_.size();
    const char *why = "";
    for (int o = 0; o < N; ++o) {
        int rc = script_to_queue(o, hit_off_[o], hit_off_[(size_t)o + 1], &why);
        if (rc != PBSO_OK) { script_.n = 0; return fail(rc, why); }
    }
    script_.n = 0;
    return PBSO_OK;
}

// Planner, before an object's buffers are planned: its share of the pending hit script.  An object that is idle -- no live
// force, nothing queued, no pending listener / parameter call -- takes its hits straight into the descriptors of this launch:
// hit after hit at buffer max(stamp, previous hit's buffer + 1), which is where ModalSolver::step would have dequeued it
// (at most one message per buffer, modal_solver.h:184), each a DESC_DIRECT impulse.  Everything else goes through the queue.
int Engine::consume_script(PlanCtx &c, int oi, int nb) {
    if (script_.n <= 0) return PBSO_OK;
    const int h0 = hit_off_[oi], h1 = hit_off_[(size_t)oi + 1];
    if (h0 >= h1) return PBSO_OK;
    Object &o = objs_[oi];
    const bool idle = o.force_q.empty() && o.active.empty() && !o.sustained && o.pending.empty() && !o.trans_full &&
                      !(!o.use_transfer && o.latest_row != XFER_UNIT) && !o.arprm_full;
    int h = h0;
    if (idle && device_profiles_ && direct_hits_) {
        int next_b = 0;
        for (; h < h1; ++h) {
            const int64_t rel = script_.stamps[h] - buffers_done_;
            const int b = (int)std::max<int64_t>(rel, next_b);
            if (b >= nb) break;
            BufDesc &d = plan_desc_[(size_t)oi * nb + b];
            const double *vnd = script_.vn + 3 * (size_t)h;
            const float vn[3] = {(float)vnd[0], (float)vnd[1], (float)vnd[2]};
            d.frow = 3 * script_.vids[h];
            std::memcpy(&d.prow, &vn[0], 4);
            std::memcpy(&d.tile_mask, &vn[1], 4);
            std::memcpy(&d.pad[0], &vn[2], 4);
            d.flags |= DESC_IMPULSE | DESC_DIRECT;
            d.amp = 1.f;
            next_b = b + 1;
        }
    }
    const char *why = "";
    int rc = script_to_queue(oi, h, h1, &why);       // what is left: beyond this launch, or the object is busy
    if (rc != PBSO_OK) return cfail(c, rc, why);
    return PBSO_OK;
}

// Planner, before an object's buffers are planned: its share of a pending STROKE script.  The object is eligible when taking the
// entries out of the arrays cannot be told from the queue: nothing queued, no stamped call due inside the launch (AR parameters
// already in the 1-slot queue are taken by the first dense row, modal_solver.h:226-236), no transfer work, and either no live force
// -- then the entries that land in this launch open with sustainedForceStart -- or exactly the one sustained AR force.  The shapes
// taken are  [start] data* [end]  with an AutoregressiveForce: the scraping of tools/real_time_modal_sound.cpp:754-776, 1127-1160.
// For those the host reserves ranges and writes one StrokeRec; stroke_expand_kernel does the rest (kernels_stroke.hip).  Anything
// else -- a PointForce, a second start, a stroke interrupted by clearAllForces (sustained with an empty list: plan_object reports
// PBSO_ERR_ASSERT for it), listeners enabled, a launch of one buffer -- and the entries beyond the launch go through the queue.
int Engine::consume_strokes(PlanCtx &c, int oi, int nb, bool *taken) {
    *taken = false;
    if (script_.n <= 0) return PBSO_OK;
    const int h0 = hit_off_[oi], h1 = hit_off_[(size_t)oi + 1];
    if (h0 >= h1) return PBSO_OK;
    Object &o = objs_[oi];
    const char *why = "";
    const int64_t horizon = buffers_done_ + nb;
    bool ok = device_profiles_ && nb >= 2 && nb <= STROKE_MAX_BUFFERS && script_.force_type == PBSO_AUTOREGRESSIVE_FORCE &&
              o.force_q.empty() && !o.trans_full &&
              !(o.path_left() && o.path[o.path_head].stamp < horizon) && (n_dump_ == 0 || dump_row_[oi] < 0);
    if (ok && o.sustained)
        ok = o.active.size() == 1 && o.active.front().force_type == PBSO_AUTOREGRESSIVE_FORCE && o.active.front().ar_state >= 0 &&
             o.active.front().slot >= 0;
    else if (ok)
        ok = o.active.empty();
    if (ok) {
        // calls stamped for the launch's first buffer or earlier take effect there (plan_object's first lines): AR parameters enter
        // the 1-slot queue, setUseTransfer switches; a listener move, or anything stamped later inside the launch, needs the planner
        size_t due = 0;
        bool full = o.arprm_full, use_t = o.use_transfer;
        while (due < o.pending.size() && o.pending[due].not_before <= buffers_done_) {
            const TimedEvent &ev = o.pending[due];
            if (ev.kind == TimedEvent::ARPRM && !full) full = true;
            else if (ev.kind == TimedEvent::USE_TRANSFER) use_t = ev.flag != 0;
            else break;
            ++due;
        }
        ok = (due == o.pending.size() || o.pending[due].not_before >= horizon) && !(!use_t && o.latest_row != XFER_UNIT);
        if (ok) {
            for (size_t i = 0; i < due; ++i) {
                const TimedEvent &ev = o.pending.front();
                if (ev.kind == TimedEvent::ARPRM) { o.arprm_full = true; std::memcpy(o.arprm, ev.v, sizeof(o.arprm)); }
                else o.use_transfer = ev.flag != 0;
                o.pending.pop_front();
            }
        }
    }
    // the entries that land inside the launch, one per buffer; their flags decide
    int K = 0, n_face = 0, b_first = 0, b_last = -1;
    bool has_end = false;
    if (ok) {
        int next_b = 0;
        for (int h = h0; h < h1; ++h) {
            const int64_t rel = script_.stamps[h] - buffers_done_;
            const int b = (int)std::max<int64_t>(std::min<int64_t>(rel, nb), next_b);
            if (b >= nb) break;
            const int fl = script_.flags ? script_.flags[h] : 0;
            const bool first = h == h0;
            if (has_end || ((fl & STROKE_START) != 0) != (first && !o.sustained) || ((fl & STROKE_START) && (fl & STROKE_END))) { ok = false; break; }
            has_end = (fl & STROKE_END) != 0;
            if (!(fl & STROKE_ZERO)) ++n_face;
            if (first) b_first = b;
            b_last = b;
            next_b = b + 1;
            ++K;
        }
        ok = ok && K > 0;
    }
    if (!ok) {
        int rc = script_to_queue(oi, h0, h1, &why);
        return rc != PBSO_OK ? cfail(c, rc, why) : PBSO_OK;
    }
    // ---- one record
    StrokeRec r;
    std::memset(&r, 0, sizeof(r));
    r.obj = oi;
    r.e0 = h0;
    r.n_ent = K;
    if (K > o.stroke_cap) {
        // (a larger pair of ranges; the old ones are not reused -- the row in force may still live there)
        o.stroke_cap = (std::max(K, o.stroke_cap + o.stroke_cap / 2) + 7) & ~7;
        o.stroke_base = (int)n_slots_.fetch_add((size_t)2 * o.stroke_cap);
        o.stroke_half = 0;
    }
    r.slot0 = o.stroke_base + o.stroke_half * o.stroke_cap;
    o.stroke_half ^= 1;
    r.sustained0 = o.sustained ? 1 : 0;
    if (!o.sustained) {                                    // sustainedForceStart (modal_solver.h:190-194): a fresh force
        ActiveForce af;
        af.force_type = PBSO_AUTOREGRESSIVE_FORCE;
        af.force = ForceProfile::make(PBSO_AUTOREGRESSIVE_FORCE, 0.0, rate_);
        if (!c.free_ar.empty()) { af.ar_state = c.free_ar.back(); c.free_ar.pop_back(); }
        else af.ar_state = (int)n_ar_states_.fetch_add(1);
        r.flags0 |= 1;
        o.active.push_back(af);
        o.sustained = true;
        r.carry_slot = -1;
    } else {
        r.carry_slot = o.active.front().slot;
        free_slot(c, o.active.front());                    // replaced by the first entry (:197-200)
    }
    ActiveForce &af = o.active.front();
    af.slot = r.slot0 + K - 1;
    af.slot_pinned = true;
    r.ar_state = af.ar_state;
    const int first_dense = r.sustained0 ? 0 : b_first, end_dense = has_end ? b_last : nb;
    r.n_dense = end_dense - first_dense;
    if (r.n_dense > 0 && o.arprm_full) {                   // :226-236, at the first profile row
        o.arprm_full = false;
        r.flags0 |= 2;
        std::memcpy(r.arprm, o.arprm, sizeof(r.arprm));
    }
    if (r.n_dense <= 0) r.flags0 = 0;                      // (start and end within ... never: start + end in one launch needs two entries, one buffer apart)
    r.row0 = c.n_stroke_rows;
    r.proj0 = c.n_stroke_proj;
    r.stream = -1;
    c.n_stroke_rows += r.n_dense;
    c.n_stroke_proj += n_face;
    c.strokes.push_back(r);
    if (has_end) {                                         // :201-204
        for (ActiveForce &x : o.active) release(c, x);
        o.active.clear();
        o.sustained = false;
    }
    stroke_direct_.fetch_add(K);
    int rc = script_to_queue(oi, h0 + K, h1, &why);        // what falls beyond this launch
    if (rc != PBSO_OK) return cfail(c, rc, why);
    *taken = true;
    return PBSO_OK;
}

int Engine::enqueue_force(int obj, const pbso_force_msg &m, int64_t not_before) {
    if (script_.n > 0) { int frc = flush_script(); if (frc != PBSO_OK) return frc; }
    const char *why = "";
    const int rc = enqueue_force_impl(obj, m, not_before, &why);
    return rc < 0 ? fail(rc, why) : rc;
}

// pbso_enqueue_track_force: the message of pbso_enqueue_force with force_type PBSO_TRACK_FORCE and its play record, validated here.
// The number of output samples the play lasts is fixed here too, with the fp64 expression the kernel and the host profile use.
int Engine::enqueue_track_force(int obj, const pbso_force_msg &m, const pbso_track_play &play, int64_t not_before) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "enqueue_track_force before finalize");
    if (m.force_type != PBSO_TRACK_FORCE) return fail(PBSO_ERR_INVALID, "enqueue_track_force: force_type must be PBSO_TRACK_FORCE");
    const int64_t L = track_length(play.track);
    if (L < 0) return fail(PBSO_ERR_INVALID, "pbso_track_play: track is not an id pbso_track_create returned");
    if (play.start_sample < 0 || play.start_sample >= B_) return fail(PBSO_ERR_INVALID, "pbso_track_play: start_sample must be 0 .. frames - 1");
    if (play.reserved != 0) return fail(PBSO_ERR_INVALID, "pbso_track_play: reserved must be 0");
    if (play.n_samples < 0) return fail(PBSO_ERR_INVALID, "pbso_track_play: n_samples must be >= 0");
    if (!std::isfinite(play.first) || play.first < 0.0) return fail(PBSO_ERR_INVALID, "pbso_track_play: first must be finite and >= 0");
    if (!std::isfinite(play.rate) || !(play.rate > 0.0)) return fail(PBSO_ERR_INVALID, "pbso_track_play: rate must be finite and > 0");
    if (!std::isfinite(play.gain)) return fail(PBSO_ERR_INVALID, "pbso_track_play: gain must be finite");
    int64_t N;
    if (play.n_samples > 0) N = play.n_samples;
    else if (play.loop) N = INT64_MAX;
    else if (play.first >= (double)L) N = 0;
    else {
        // the number of k with first + rate * k < L: an estimate, then a step up or down with that very expression
        auto pos = [&](int64_t k) { volatile double prod = play.rate * (double)k; return play.first + prod; };
        const double est = ((double)L - play.first) / play.rate;
        N = est < 9.0e18 ? (int64_t)est : (int64_t)9.0e18;
        if (N < 1) N = 1;
        while (N > 0 && !(pos(N - 1) < (double)L)) --N;
        while (N < INT64_MAX - 1 && pos(N) < (double)L) ++N;
    }
    if (script_.n > 0) { int frc = flush_script(); if (frc != PBSO_OK) return frc; }
    const char *why = "";
    const int rc = enqueue_force_impl(obj, m, not_before, &why, &play, N);
    return rc < 0 ? fail(rc, why) : rc;
}

// A whole step of a force script.  Messages of one object keep their order.  With planner threads
// (PBSO_PLAN_THREADS > 1) every thread enqueues the messages of its own range of objects.
int Engine::enqueue_force_batch(int n, const int *objs, const pbso_force_msg *msgs, const int64_t *stamps,
                                unsigned char *accepted) {
    if (script_.n > 0) { int frc = flush_script(); if (frc != PBSO_OK) return frc; }
    const int N = (int)objs_.size();
    const int T = (plan_threads_ > 1 && n >= 4096 && N >= 64) ? plan_threads_ : 1;
    std::vector<int> taken(T, 0), rcs(T, 0);
    std::vector<const char *> whys(T, "");
    // A script given object by object (ids ascending; each object's messages in their own order) is cut at the threads'
    // object ranges by binary search: no thread walks messages that are not its own, and an object's queue takes its
    // messages back to back (one ring's tail stays in the core's cache).  Any other order: every thread walks the batch.
    bool by_object = n > 0 && objs[0] >= 0 && objs[n - 1] < N;
    for (int i = 1; i < n && by_object; ++i) by_object = objs[i - 1] <= objs[i];
    auto job = [&](int t) {
        const int lo = (int)((long long)N * t / T), hi = (int)((long long)N * (t + 1) / T);
        int i0 = 0, i1 = n;
        if (by_object) {
            i0 = (int)(std::lower_bound(objs, objs + n, lo) - objs);
            i1 = (int)(std::lower_bound(objs, objs + n, hi) - objs);
        }
        for (int i = i0; i < i1; ++i) {
            const int o = objs[i];
            const bool mine = by_object || (o >= lo && o < hi) || (t == 0 && (o < 0 || o >= N));   // bad ids: reported by thread 0
            if (!mine) continue;
            const int rc = enqueue_force_impl(o, msgs[i], stamps[i], &whys[t]);
            if (rc < 0) { rcs[t] = rc; return; }
            if (accepted) accepted[i] = rc ? 1 : 0;
            taken[t] += rc ? 1 : 0;
        }
    };
    if (T > 1) {
        if (!pool_) {
            pool_ = new PlanPool(plan_threads_ - 1, desc_.plan_pin ? sched_getcpu() : -1);
        }
        pool_->run(T, job);
    } else {
        job(0);
    }
    int total = 0;
    for (int t = 0; t < T; ++t) {
        if (rcs[t] < 0) return fail(rcs[t], whys[t]);
        total += taken[t];
    }
    return total;
}

static void push_timed(std::deque<TimedEvent> &q, const TimedEvent &ev) {
    auto it = q.end();
    while (it != q.begin() && (it - 1)->not_before > ev.not_before) --it;
    q.insert(it, ev);
}

// ModalSolver::enqueueArprmMessageNoFail, modal_solver.h:382-393
int Engine::enqueue_arprm(int obj, const double a[2], double sigma, double mu, int64_t not_before) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "enqueue_arprm before finalize");
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    path_to_pending(objs_[obj], INT64_MAX);              // (a parameter message that waits for its slot holds the events behind it back)
    TimedEvent ev;
    ev.kind = TimedEvent::ARPRM;
    ev.not_before = not_before;
    ev.v[0] = a[0]; ev.v[1] = a[1]; ev.v[2] = sigma; ev.v[3] = mu;
    ev.flag = 0;
    push_timed(objs_[obj].pending, ev);
    return 1;
}

// what ModalSolver::enqueueArprmMessage's try_enqueue would find (modal_solver.h:378-381): the slot taken, or a message waiting for it
int Engine::arprm_pending(int obj) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "arprm_pending before finalize");
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    const Object &o = objs_[obj];
    if (o.arprm_full) return 1;
    for (const TimedEvent &ev : o.pending)
        if (ev.kind == TimedEvent::ARPRM) return 1;
    return 0;
}

// ModalSolver::computeTransfer(pos), modal_solver.h:286-300
int Engine::compute_transfer(int obj, const double pos[3], int64_t not_before) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "compute_transfer before finalize");
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    Object &o = objs_[obj];
    path_to_pending(o, INT64_MAX);                                // (a path given earlier: its positions are in front of this one)
    if (!o.have_maps) return 0;                                   // :290-291
    if (!o.maps_cover_modes)                                      // (the maps are fixed at finalize: checked once, there)
        return fail(PBSO_ERR_MISSING_MAP, "FFAT map for a modeId in 0..N_modes-1 is missing (std::map::at throws)");
    if (not_before <= buffers_done_ && o.pending.empty() && o.trans_full) return 0;   // try_enqueue on a full 1-slot queue
    TimedEvent ev;
    ev.kind = TimedEvent::TRANSFER;
    ev.not_before = not_before;
    ev.v[0] = pos[0]; ev.v[1] = pos[1]; ev.v[2] = pos[2]; ev.v[3] = 0;
    ev.flag = 0;
    push_timed(o.pending, ev);
    return 1;
}

// a listener PATH: n computeTransfer(pos) calls (modal_solver.h:286-300) in one -- what the tool's camera callback issues frame
// after frame (tools/real_time_modal_sound.cpp:844, 1172), pre-scheduled as the throughput harness has it
int Engine::compute_transfer_path(int n, const int *objs, const double *pos, const int64_t *stamps, unsigned char *accepted) {
    if (n < 0 || (n > 0 && (!objs || !pos || !stamps))) return fail(PBSO_ERR_INVALID, "compute_transfer_path arguments");
    if (!finalized_) return fail(PBSO_ERR_STATE, "compute_transfer before finalize");
    // Runs of ONE object with ascending stamps -- the shape a camera path and the throughput harness have -- are kept as an array
    // with a cursor (Object::path) for the planner; anything else goes call by call.
    int taken = 0;
    const int N = (int)objs_.size();
    for (int i = 0; i < n;) {
        const int o = objs[i];
        int j = i + 1;
        while (j < n && objs[j] == o && stamps[j] > stamps[j - 1]) ++j;
        bool run = o >= 0 && o < N && j - i >= 4;
        if (run) {
            Object &ob = objs_[o];
            // every call of the run must be one pbso_compute_transfer accepts and appends: maps there, behind what the object's path
            // already holds, and the first not an immediate call that finds the 1-slot queue taken
            run = ob.have_maps && ob.maps_cover_modes && (!ob.path_left() || stamps[i] > ob.path.back().stamp) &&
                  !(stamps[i] <= buffers_done_ && ob.pending.empty() && !ob.path_left() && ob.trans_full);
            if (run) {
                if (!ob.path_left()) { ob.path.clear(); ob.path_head = 0; }
                for (int e = i; e < j; ++e) ob.path.push_back(Object::PathEv{stamps[e], {pos[3 * (size_t)e], pos[3 * (size_t)e + 1], pos[3 * (size_t)e + 2]}});
                if (accepted) std::memset(accepted + i, 1, (size_t)(j - i));
                taken += j - i;
            }
        }
        if (!run) {
            for (int e = i; e < j; ++e) {
                const int rc = compute_transfer(objs[e], pos + 3 * (size_t)e, stamps[e]);
                if (rc < 0) return rc;
                if (accepted) accepted[e] = rc ? 1 : 0;
                taken += rc ? 1 : 0;
            }
        }
        i = j;
    }
    return taken;
}

// the positions of the object's path stamped below `before` enter its pending list as pbso_compute_transfer puts them
void Engine::path_to_pending(Object &o, int64_t before) {
    while (o.path_left() && o.path[o.path_head].stamp < before) {
        const Object::PathEv &pe = o.path[o.path_head++];
        TimedEvent ev;
        ev.kind = TimedEvent::TRANSFER;
        ev.not_before = pe.stamp;
        ev.v[0] = pe.pos[0]; ev.v[1] = pe.pos[1]; ev.v[2] = pe.pos[2]; ev.v[3] = 0;
        ev.flag = 0;
        push_timed(o.pending, ev);
    }
    if (!o.path_left()) { o.path.clear(); o.path_head = 0; }
}

// Planner, before an object's buffers are planned: the positions of its path that fall into this launch.  For an object with
// nothing else going on -- no live force, no message or stamped call due, the transfer in use, the 1-slot queue free -- a position
// stamped s is what plan_object makes of it: try_enqueue into _queue_trans at the first buffer t >= s (modal_solver.h:286-300),
// dequeued by the same step (:242-256) -- one lookup event and that buffer's transfer row; a second position that falls into the
// same buffer finds the queue full and is dropped.  Otherwise they go through the pending list.
int Engine::consume_path(PlanCtx &c, int oi, int nb) {
    Object &o = objs_[oi];
    if (!o.path_left()) return PBSO_OK;
    const int64_t horizon = buffers_done_ + nb;
    if (o.path[o.path_head].stamp >= horizon) return PBSO_OK;
    const bool quiet = o.pending.empty() && (o.force_q.empty() || o.force_q.front().not_before >= horizon) && o.active.empty() &&
                       !o.sustained && o.use_transfer && !o.trans_full && !o.arprm_full;
    if (!quiet) {
        path_to_pending(o, horizon);
        return PBSO_OK;
    }
    int last_b = -1;
    for (; o.path_left(); ++o.path_head) {
        const Object::PathEv &pe = o.path[o.path_head];
        const int64_t rel = pe.stamp - buffers_done_;
        if (rel >= nb) break;
        const int b = rel > 0 ? (int)rel : 0;
        if (b == last_b) continue;                       // the queue still holds the position before it: try_enqueue fails, the move is lost
        FfatEvent fe;
        fe.obj = oi;
        fe.row = c.xfer_base + c.n_xfer++;
        fe.pos[0] = pe.pos[0]; fe.pos[1] = pe.pos[1]; fe.pos[2] = pe.pos[2];
        c.ffat.push_back(fe);
        o.trans_row = fe.row;
        o.latest_row = fe.row;
        plan_desc_[(size_t)oi * nb + b].trow = fe.row;
        last_b = b;
    }
    if (!o.path_left()) { o.path.clear(); o.path_head = 0; }
    return PBSO_OK;
}

// ModalSolver::setUseTransfer, modal_solver.h:148-152
int Engine::set_use_transfer(int obj, int use, int64_t not_before) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "set_use_transfer before finalize");
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    path_to_pending(objs_[obj], INT64_MAX);
    TimedEvent ev;
    ev.kind = TimedEvent::USE_TRANSFER;
    ev.not_before = not_before;
    ev.v[0] = ev.v[1] = ev.v[2] = ev.v[3] = 0;
    ev.flag = use ? 1 : 0;
    push_timed(objs_[obj].pending, ev);
    return PBSO_OK;
}

void Engine::release(PlanCtx &c, ActiveForce &af) {
    free_slot(c, af);                                            // (negative: an on-the-fly projection, no pool row)
    if (af.ar_state >= 0) c.freed_ar.push_back(af.ar_state);
    af.ar_state = -1;
}

int Engine::alloc_slot(PlanCtx &c) {
    if (!c.free_slots.empty()) {
        int s = c.free_slots.back();
        c.free_slots.pop_back();
        return s;
    }
    return (int)n_slots_.fetch_add(1);
}

// ---------------------------------------------------------------------------
// One object, one buffer: ModalSolver::step lines 184-256.
int Engine::plan_object(PlanCtx &c, int oi, int b, int nb, int64_t t) {
    Object &o = objs_[oi];
    BufDesc &d = plan_desc_[(size_t)oi * nb + b];

    // GUI-thread calls stamped for this buffer or earlier
    while (!o.pending.empty() && o.pending.front().not_before <= t) {
        const TimedEvent ev = o.pending.front();
        if (ev.kind == TimedEvent::ARPRM) {
            if (o.arprm_full) break;              // NoFail: the caller spins until the 1-slot queue drains
            o.arprm_full = true;
            std::memcpy(o.arprm, ev.v, sizeof(o.arprm));
        } else if (ev.kind == TimedEvent::TRANSFER) {
            if (!o.trans_full) {                  // try_enqueue; a full queue drops the update
                FfatEvent fe;
                fe.obj = oi;
                fe.row = c.xfer_base + c.n_xfer++;
                fe.pos[0] = ev.v[0]; fe.pos[1] = ev.v[1]; fe.pos[2] = ev.v[2];
                c.ffat.push_back(fe);
                o.trans_full = true;
                o.trans_row = fe.row;
            }
        } else {
            o.use_transfer = ev.flag != 0;
        }
        o.pending.pop_front();
    }

    // :184 dequeue at most one force message
    const bool due_msg = !o.force_q.empty() && o.force_q.front().not_before <= t;
    bool plain_hit = false;
    if (due_msg && device_profiles_ && o.active.empty() && !o.sustained) {
        const HostForceMsg &m0 = o.force_q.front();
        plain_hit = m0.force_type == PBSO_POINT_FORCE && !m0.clear_all && !m0.sustained_start && !m0.sustained_end &&
                    (m0.data_kind == PBSO_DATA_VERTEX || m0.data_kind == PBSO_DATA_FACE);
    }
    if (plain_hit && direct_hits_ && o.force_q.front().data_kind == PBSO_DATA_VERTEX && 3 * o.force_q.front().vids[0] + 2 < o.n_dof) {
        // ... and when the hit is at a vertex, not even a row: the oscillator bank dots the hit's normal with three rows
        // of the object's (float)(c3 * shape) table itself (DESC_DIRECT).  No work for any preparation kernel.
        const HostForceMsg &m0 = o.force_q.front();
        const float vn[3] = {(float)m0.vn[0], (float)m0.vn[1], (float)m0.vn[2]};
        d.frow = 3 * m0.vids[0];
        std::memcpy(&d.prow, &vn[0], 4);
        std::memcpy(&d.tile_mask, &vn[1], 4);
        std::memcpy(&d.pad[0], &vn[2], 4);
        d.flags |= DESC_IMPULSE | DESC_DIRECT;
        d.amp = 1.f;
        std::free(m0.ext);
        o.force_q.pop_front();
    } else if (plain_hit) {
        const HostForceMsg &m0 = o.force_q.front();
        {
            // The common case in one go -- the hit of a plain PointForce on an object with no live force: what the
            // general path below does for it (active list of one, Force::Add -> 1 at sample 0, erased next step,
            // modal_solver.h:195-221, forces.h:81-90) comes to one impulse row whose spatial vector is the
            // projection of this hit, evaluated by the combine kernel.
            ProjectEvent pe;
            pe.obj = oi;
            pe.kind = m0.data_kind;
            pe.slot = -1;
            for (int j = 0; j < 3; ++j) {
                pe.vids[j] = m0.vids[j];
                pe.coords[j] = m0.coord(j);
                pe.vn[j] = m0.vn[j];
            }
            c.slot_idx.push_back(-((int)c.proj_direct.size() + 1));
            c.proj_direct.push_back(pe);
            std::free(m0.ext);
            o.force_q.pop_front();
            d.frow = c.n_frows++;
            c.forced.push_back(&d);
            c.row_obj.push_back(oi);
            c.row_ptr.push_back((int)c.slot_idx.size());
            d.flags |= DESC_IMPULSE;
            d.tile_mask = 1u;
            d.amp = 1.f;
        }
    } else if (due_msg) {
        const HostForceMsg mess = o.force_q.front();
        o.force_q.pop_front();
        struct FreeExt { MsgExt *p; ~FreeExt() { std::free(p); } } free_ext{mess.ext};
        if (mess.clear_all) {                                           // :186-189
            for (ActiveForce &af : o.active) release(c, af);
            o.active.clear();
            d.flags |= DESC_SKIP;
            emitted_[(size_t)oi * plan_nb_total_ + plan_b0_ + b] = 0;
            return PBSO_OK;
        }
        // the message's modal data becomes one immutable row of the slot pool -- except for the hit of a plain
        // PointForce (forces.h:81-90: alive for exactly one buffer), whose projection the combine kernel
        // evaluates on the fly: slot -(event + 1) refers to the event, no pool row is written or read back
        const bool direct = device_profiles_ && mess.force_type == PBSO_POINT_FORCE && !mess.sustained_start && !mess.sustained_end &&
                            !o.sustained && (mess.data_kind == PBSO_DATA_VERTEX || mess.data_kind == PBSO_DATA_FACE);
        const int slot = direct ? -((int)c.proj_direct.size() + 1) : alloc_slot(c);
        if (mess.data_kind == PBSO_DATA_EXPLICIT || mess.data_kind == PBSO_DATA_ZERO) {
            const size_t off = c.stage.size();
            c.stage.resize(off + m_pad_, 0.0);
            if (mess.data_kind == PBSO_DATA_EXPLICIT)
                std::copy(mess.ext->data, mess.ext->data + mess.ext->n_data, c.stage.begin() + off);
            c.stage_slot.push_back(slot);
        } else {
            ProjectEvent pe;
            pe.obj = oi;
            pe.kind = mess.data_kind;
            pe.slot = slot;
            for (int j = 0; j < 3; ++j) {
                pe.vids[j] = mess.vids[j];
                pe.coords[j] = mess.coord(j);
                pe.vn[j] = mess.vn[j];
            }
            (direct ? c.proj_direct : c.proj).push_back(pe);
        }
        ActiveForce af;
        af.slot = slot;
        af.force_type = mess.force_type;
        af.force = ForceProfile::make(mess.force_type, mess.gaussian_width_us(), rate_);   // fresh Force, tools/...:281-294
        if (mess.force_type == PBSO_TRACK_FORCE) {
            const TrackExt &te = *track_ext(mess.ext);
            af.force.track = std::make_shared<ForceProfile::Track>(ForceProfile::Track{
                te.play, te.total, 0, te.play.start_sample, device_profiles_ ? nullptr : track_host_samples(te.play.track),
                track_length(te.play.track)});
            track_msgs_.fetch_add(1, std::memory_order_relaxed);
        }
        bool slot_used = false;
        if (mess.sustained_start) {                                     // :190-194
            for (ActiveForce &x : o.active) release(c, x);
            o.active.clear();
            o.sustained = true;
            o.active.push_back(af);
            slot_used = true;
        }
        if (!o.sustained) {                                             // :195-196
            o.active.push_back(af);
            slot_used = true;
        } else {                                                        // :197-200 data only
            if (o.active.empty())
                return cfail(c, PBSO_ERR_ASSERT, "sustained force list is empty (reference dereferences begin() of an empty list)");
            if (o.active.front().slot != slot) {
                free_slot(c, o.active.front());
                o.active.front().slot = slot;
                o.active.front().slot_pinned = false;
                slot_used = true;
            }
        }
        if (mess.sustained_end) {                                       // :201-204
            for (ActiveForce &x : o.active) release(c, x);
            o.active.clear();
            o.sustained = false;
            slot_used = true;   // freed through the list (or below)
        }
        if (!slot_used && slot >= 0) c.freed_this_plan.push_back(slot);
    }

    // :206-240 time profile and spatial sum
    if ((!o.active.empty() || o.sustained) && device_profiles_) {
        // Force::Add bookkeeping only (who is alive, _count, PointForce::used); the samples
        // of Gaussian / AR profiles are generated on the device (K2, kernels_exact.hip)
        const int row_begin = (int)c.slot_idx.size();
        const int entry_begin = (int)c.prof_entries.size();
        int n_point = 0;
        bool dense = false, dense_all_tiles = false;
        uint32_t track_tiles = 0;
        auto emit = [&](ActiveForce &af, bool set_param) -> bool {
            ForceProfile &f = af.force;
            ProfEntry e;
            std::memset(&e, 0, sizeof(e));
            e.kind = f.type;
            e.state = -1;
            switch (f.type) {
            case PBSO_POINT_FORCE:                                   // forces.h:81-90
                if (f.used) return false;
                f.used = true;
                ++n_point;
                break;
            case PBSO_GAUSSIAN_FORCE:                                // forces.h:92-105
                if (f.width == 0 || f.count >= f.cutoff * 2 * f.width_samples) return false;
                e.count = f.count;
                e.center = f.center;
                e.width_samples = f.width_samples;
                f.count += B_;
                dense = dense_all_tiles = true;
                break;
            case PBSO_TRACK_FORCE: {                                 // include/openpbso_amd.h, pbso_track_play; ProfEntry's track layout
                int o_first, n_live;
                int64_t k0;
                if (!f.track_span(B_, &o_first, &n_live, &k0)) return false;
                e.state = f.track->play.track;
                e.flags = f.track->play.loop ? 1 : 0;
                e.count = o_first;
                e.center = n_live;
                e.a0 = f.track->play.first; e.a1 = f.track->play.rate; e.sigma = f.track->play.gain;
                e.mu = track_k0_bits(k0);
                if (n_live > 0) track_tiles |= tiles_of(o_first, n_live);
                dense = true;
                c.prof_entries.push_back(e);
                return true;
            }
            default:                                                 // forces.h:107-137
                if (af.ar_state < 0) {
                    if (!c.free_ar.empty()) { af.ar_state = c.free_ar.back(); c.free_ar.pop_back(); }
                    else af.ar_state = (int)n_ar_states_.fetch_add(1);
                    e.flags |= 1;
                }
                if (set_param) {
                    e.flags |= 2;
                    e.a0 = o.arprm[0]; e.a1 = o.arprm[1]; e.sigma = o.arprm[2]; e.mu = o.arprm[3];
                }
                e.state = af.ar_state;
                dense = dense_all_tiles = true;
                break;
            }
            c.prof_entries.push_back(e);
            return true;
        };
        if (!o.sustained) {
            size_t w = 0;
            for (size_t r = 0; r < o.active.size(); ++r) {
                ActiveForce &af = o.active[r];
                if (!emit(af, false)) {
                    release(c, af);                                            // erase
                } else {
                    c.slot_idx.push_back(af.slot);
                    if (af.force.type == PBSO_POINT_FORCE) {
                        // a PointForce adds its one sample and is erased by the NEXT step()'s Add (forces.h:84-85,
                        // modal_solver.h:212-215); nothing can observe it in between, so it leaves the list now
                        // and an object with no other live force needs no bookkeeping for the next buffer
                        release(c, af);
                    } else {
                        if (w != r) o.active[w] = std::move(af);
                        ++w;
                    }
                }
            }
            o.active.resize(w);
        } else {
            if (o.active.size() != 1)
                return cfail(c, PBSO_ERR_ASSERT, "Should only have 1 concurrent sustained force");   // assert :223
            ActiveForce &af = o.active.front();
            bool sp = false;
            if (af.force_type == PBSO_AUTOREGRESSIVE_FORCE && o.arprm_full) {   // :226-236
                o.arprm_full = false;
                sp = true;
            }
            emit(af, sp);                        // the return value is ignored, modal_solver.h:238
            c.slot_idx.push_back(af.slot);
        }
        if ((int)c.slot_idx.size() > row_begin && (dense || n_point)) {
            d.frow = c.n_frows++;
            c.forced.push_back(&d);
            c.row_obj.push_back(oi);
            c.row_ptr.push_back((int)c.slot_idx.size());
            if (!dense) {
                d.flags |= DESC_IMPULSE;          // PointForce(s) only: n * delta[0], no profile row
                d.tile_mask = 1u;
                d.amp = (float)n_point;
                c.prof_entries.resize(entry_begin);
            } else {
                d.prow = c.n_prows++;
                c.prow_obj.push_back(oi);
                // (a row of track entries only: the tiles its live samples intersect, and tile 0 for a PointForce beside them)
                d.tile_mask = dense_all_tiles ? (n_tiles_ >= 32 ? 0xFFFFFFFFu : ((1u << n_tiles_) - 1u)) : (track_tiles | (n_point ? 1u : 0u));
                if (track_tiles) track_rows_.fetch_add(1, std::memory_order_relaxed);
                ProfRow pr = {d.prow, entry_begin, (int)c.prof_entries.size()};
                c.prof_rows.push_back(pr);
                if (c.chain_obj != oi) {           // rows of one object are contiguous (object-major plan)
                    c.chain_ptr.push_back((int)c.prof_rows.size() - 1);
                    c.chain_obj = oi;
                }
            }
        } else {
            c.slot_idx.resize(row_begin);          // nothing active produced samples: a force-free buffer
            c.prof_entries.resize(entry_begin);
        }
    } else if (!o.active.empty() || o.sustained) {
        double *T = c.tbuf.data();
        std::fill(T, T + c.t_extent, 0.0);
        c.t_extent = 0;
        c.t_live_tiles = 0;
        bool track_added = false;
        const int row_begin = (int)c.slot_idx.size();
        if (!o.sustained) {
            size_t w = 0;
            for (size_t r = 0; r < o.active.size(); ++r) {
                ActiveForce &af = o.active[r];
                const bool added = af.force.add(T, B_, &c.t_extent, &c.t_live_tiles);
                track_added = track_added || (added && af.force.type == PBSO_TRACK_FORCE);
                if (!added) {
                    release(c, af);                                            // erase
                } else {
                    c.slot_idx.push_back(af.slot);
                    if (w != r) o.active[w] = std::move(af);
                    ++w;
                }
            }
            o.active.resize(w);
        } else {
            if (o.active.size() != 1)
                return cfail(c, PBSO_ERR_ASSERT, "Should only have 1 concurrent sustained force");   // assert :223
            ActiveForce &af = o.active.front();
            if (af.force_type == PBSO_AUTOREGRESSIVE_FORCE && o.arprm_full) {   // :226-236
                o.arprm_full = false;
                af.force.set_param(o.arprm, o.arprm[2], o.arprm[3]);
            }
            if (af.force.add(T, B_, &c.t_extent, &c.t_live_tiles) && af.force.type == PBSO_TRACK_FORCE) track_added = true;
            c.slot_idx.push_back(af.slot);
        }
        if (track_added) track_rows_.fetch_add(1, std::memory_order_relaxed);
        uint32_t mask = 0;
        int last_nz = -1;
        for (int i = 0; i < c.t_extent; ++i)
            if (T[i] != 0.0) { mask |= 1u << (i / TILE); last_nz = i; }
        if ((int)c.slot_idx.size() > row_begin && mask) {
            d.frow = c.n_frows++;
            c.forced.push_back(&d);
            d.tile_mask = mask | c.t_live_tiles;               // (the mask the device-profile path gives a row of track entries)
            c.row_obj.push_back(oi);
            c.row_ptr.push_back((int)c.slot_idx.size());
            if (last_nz == 0) {
                d.flags |= DESC_IMPULSE;                  // PointForce(s): amp * delta[0], no profile row
                d.amp = (float)T[0];
            } else {
                d.prow = c.n_prows++;
                c.prow_obj.push_back(oi);
                const size_t off = c.tprof.size();
                c.tprof.resize(off + b_pad_, 0.f);
                for (int i = 0; i <= last_nz; ++i) c.tprof[off + i] = (float)T[i];
            }
        } else {
            c.slot_idx.resize(row_begin);          // S * 0 == 0: a force-free buffer
        }
    }

    // :242-256 transfer selection (single caller thread: try_lock always succeeds)
    if (o.use_transfer) {
        if (o.trans_full) {
            o.latest_row = o.trans_row;
            d.trow = o.trans_row;
            o.trans_full = false;
        }
    } else if (o.latest_row != XFER_UNIT) {
        o.latest_row = XFER_UNIT;
        d.trow = XFER_UNIT;
    }
    return PBSO_OK;
}

// All buffers of one object.  Objects are independent, and between stamped
// messages an idle object needs no bookkeeping at all: jump to the next stamp.
int Engine::plan_object_span(PlanCtx &c, int oi, int nb) {
    Object &o = objs_[oi];
    {
        bool taken = false;
        int rc = script_.strokes ? consume_strokes(c, oi, nb, &taken) : consume_script(c, oi, nb);
        if (rc != PBSO_OK || taken) return rc;
        rc = consume_path(c, oi, nb);
        if (rc != PBSO_OK) return rc;
    }
    int b = 0;
    while (b < nb) {
        const int64_t t = buffers_done_ + b;
        // The buffer of a listener PATH in one step: nothing is due but one computeTransfer (a camera move per frame,
        // tools/real_time_modal_sound.cpp:844, 1172), no force is alive, the 1-slot queue is free -- what plan_object does for it
        // (try_enqueue into _queue_trans, modal_solver.h:286-300; dequeued at :242-256 in the same step) comes to one lookup event
        // and this buffer's transfer row.
        if (!o.pending.empty() && o.pending.front().kind == TimedEvent::TRANSFER && o.pending.front().not_before <= t &&
            o.active.empty() && !o.sustained && o.use_transfer && !o.trans_full &&
            (o.force_q.empty() || o.force_q.front().not_before > t) && (o.pending.size() == 1 || o.pending[1].not_before > t)) {
            const TimedEvent &ev = o.pending.front();
            FfatEvent fe;
            fe.obj = oi;
            fe.row = c.xfer_base + c.n_xfer++;
            fe.pos[0] = ev.v[0]; fe.pos[1] = ev.v[1]; fe.pos[2] = ev.v[2];
            c.ffat.push_back(fe);
            o.pending.pop_front();
            o.trans_row = fe.row;
            o.latest_row = fe.row;
            plan_desc_[(size_t)oi * nb + b].trow = fe.row;
            ++b;
            continue;
        }
        const bool due = (!o.pending.empty() && o.pending.front().not_before <= t) ||
                         (!o.force_q.empty() && o.force_q.front().not_before <= t);
        const bool live = !o.active.empty() || o.sustained || (o.trans_full && o.use_transfer) ||
                          (!o.use_transfer && o.latest_row != XFER_UNIT);
        if (!due && !live) {
            int64_t next = INT64_MAX;
            if (!o.pending.empty()) next = std::min(next, o.pending.front().not_before);
            if (!o.force_q.empty()) next = std::min(next, o.force_q.front().not_before);
            if (next >= buffers_done_ + nb) break;
            b = (int)(next - buffers_done_);
            continue;
        }
        int rc = plan_object(c, oi, b, nb, t);
        if (rc != PBSO_OK) return rc;
        ++b;
    }
    return PBSO_OK;
}

int Engine::plan(int nb) {
    const int N = (int)objs_.size();
    PlanSet &ps = set_[cur_set_];
    // one pinned arena per plan set, uploaded with ONE copy: [descriptors | xfer_init | everything the planner emits]
    ps.off_xfer_init = arena_align((size_t)N * nb * sizeof(BufDesc));
    ps.front_bytes = ps.off_xfer_init + arena_align((size_t)N * sizeof(int));
    HIPTRY(ps.h_arena.ensure_keep(std::max(ps.front_bytes, ps.last_bytes), 0));
    plan_desc_ = reinterpret_cast<BufDesc *>(ps.h_arena.p);
    int *h_xfer_init = reinterpret_cast<int *>(ps.h_arena.p + ps.off_xfer_init);
    const auto tp0 = std::chrono::steady_clock::now();
    const BufDesc dflt = {-1, -1, 0u, 0.f, XFER_KEEP, 0u, {0, 0}};
    std::fill(plan_desc_, plan_desc_ + (size_t)N * nb, dflt);
    busy_.clear();
    for (int i = 0; i < N; ++i) {
        const Object &o = objs_[i];
        h_xfer_init[i] = o.latest_row;
        if (!o.force_q.empty() || !o.active.empty() || !o.pending.empty() || o.trans_full ||
            o.sustained || (!o.use_transfer && o.latest_row != XFER_UNIT) ||
            (script_.n > 0 && hit_off_[(size_t)i + 1] > hit_off_[i]) || (o.path_left() && o.path[o.path_head].stamp < buffers_done_ + nb))
            busy_.push_back(i);
    }
    // contiguous shares of the busy objects, one planning context (host thread) each
    const int nbusy = (int)busy_.size();
    const int T = std::max(1, std::min(plan_threads_, nbusy / plan_grain_));      // at least plan_grain_ objects per thread
    std::vector<int> lo(T + 1);
    for (int t = 0; t <= T; ++t) lo[t] = (int)((long long)nbusy * t / T);
    // every stamped computeTransfer that can fire in this batch may need one scratch row
    std::vector<size_t> need(T, 0);
    size_t need_all = 0;
    for (int t = 0; t < T; ++t) {
        for (int k = lo[t]; k < lo[t + 1]; ++k) {
            for (const TimedEvent &ev : objs_[busy_[k]].pending) {
                if (ev.not_before >= buffers_done_ + nb) break;      // sorted by stamp (push_timed): the rest is later
                if (ev.kind == TimedEvent::TRANSFER) ++need[t];
            }
            // (the object's path: at most one position fires per buffer)
            need[t] += std::min<size_t>(objs_[busy_[k]].path.size() - objs_[busy_[k]].path_head, (size_t)nb);
        }
        need_all += need[t];
    }
    if ((int)need_all > xfer_cap_) {
        const int ncap = std::max<int>((int)need_all, 2 * xfer_cap_ + 16);
        // rows [2N + s*cap, ...) change meaning with cap: nothing may be in flight (ensure() drains) -- nor still waiting in the
        // submitting thread's queue: its recorded launches hold the old block's address, and the keep-copy must come behind them
        {
            int drc = drain_submit();
            if (drc != PBSO_OK) return drc;
        }
        HIPTRY(d_xfer_.ensure((size_t)(2 * N + N_SETS * ncap) * m_pad_, true, stream_));
        HIPTRY(hipDeviceSynchronize());
        xfer_cap_ = ncap;
    }
    {
        int xb = 2 * N + cur_set_ * xfer_cap_;
        for (int t = 0; t < T; ++t) {
            ctx_[t].begin();
            ctx_[t].xfer_base = xb;
            xb += (int)need[t];
        }
    }
    auto job = [&](int t) {
        PlanCtx &c = ctx_[t];
        for (int k = lo[t]; k < lo[t + 1]; ++k) {
            c.rc = plan_object_span(c, busy_[k], nb);
            if (c.rc != PBSO_OK) return;
        }
    };
    const auto tp1 = std::chrono::steady_clock::now();
    if (T > 1) {
        if (!pool_) {
            pool_ = new PlanPool(plan_threads_ - 1, desc_.plan_pin ? sched_getcpu() : -1);
        }
        pool_->run(T, job);
    } else {
        job(0);
    }
    const auto tp2 = std::chrono::steady_clock::now();
    script_.n = 0;                                   // (every object with hits was busy: all of the script is consumed)
    for (int t = 0; t < T; ++t)
        if (ctx_[t].rc != PBSO_OK) return fail(ctx_[t].rc, ctx_[t].err);

    // merge in object order: the numbering is the one a single context would have produced
    row_ptr_.assign(1, 0);
    slot_idx_.clear(); row_obj_.clear(); tprof_.clear(); stage_.clear(); stage_slot_.clear();
    proj_.clear(); proj_direct_.clear(); ffat_.clear(); prof_entries_.clear(); prof_rows_.clear(); chain_ptr_.clear(); prow_obj_.clear();
    n_frows_ = 0;
    n_prows_ = 0;
    for (int t = 0; t < T; ++t) {
        PlanCtx &c = ctx_[t];
        const int base_f = n_frows_, base_p = n_prows_, base_s = (int)slot_idx_.size();
        const int base_e = (int)prof_entries_.size(), base_r = (int)prof_rows_.size();
        if (t > 0) {
            for (BufDesc *d : c.forced) {
                d->frow += base_f;
                if (d->prow >= 0) d->prow += base_p;
            }
        }
        for (int e : c.row_ptr) row_ptr_.push_back(base_s + e);
        const int base_d = (int)proj_direct_.size();
        if (base_d == 0) slot_idx_.insert(slot_idx_.end(), c.slot_idx.begin(), c.slot_idx.end());
        else for (int e : c.slot_idx) slot_idx_.push_back(e >= 0 ? e : e - base_d);     // on-the-fly projections: global event index
        proj_direct_.insert(proj_direct_.end(), c.proj_direct.begin(), c.proj_direct.end());
        row_obj_.insert(row_obj_.end(), c.row_obj.begin(), c.row_obj.end());
        prow_obj_.insert(prow_obj_.end(), c.prow_obj.begin(), c.prow_obj.end());
        tprof_.insert(tprof_.end(), c.tprof.begin(), c.tprof.end());
        prof_entries_.insert(prof_entries_.end(), c.prof_entries.begin(), c.prof_entries.end());
        for (ProfRow r : c.prof_rows) {
            r.prow += base_p;
            r.entry_begin += base_e;
            r.entry_end += base_e;
            prof_rows_.push_back(r);
        }
        for (int ci : c.chain_ptr) chain_ptr_.push_back(base_r + ci);
        stage_.insert(stage_.end(), c.stage.begin(), c.stage.end());
        stage_slot_.insert(stage_slot_.end(), c.stage_slot.begin(), c.stage_slot.end());
        proj_.insert(proj_.end(), c.proj.begin(), c.proj.end());
        ffat_.insert(ffat_.end(), c.ffat.begin(), c.ffat.end());
        n_frows_ += c.n_frows;
        n_prows_ += c.n_prows;
        // what this pass released becomes reusable from the next plan on (this launch still reads it)
        c.free_slots.insert(c.free_slots.end(), c.freed_this_plan.begin(), c.freed_this_plan.end());
        c.free_ar.insert(c.free_ar.end(), c.freed_ar.begin(), c.freed_ar.end());
    }
    // stroke records: their rows and events are numbered behind everything the host planned, context after context
    stroke_recs_.clear();
    n_stroke_rows_ = n_stroke_proj_ = 0;
    for (int t = 0; t < T; ++t) {
        PlanCtx &c = ctx_[t];
        for (StrokeRec r : c.strokes) {
            r.row0 += n_stroke_rows_;
            r.proj0 += n_stroke_proj_;
            if (r.n_dense > 0) chain_ptr_.push_back((int)prof_rows_.size() + r.row0);
            stroke_recs_.push_back(r);
        }
        n_stroke_rows_ += c.n_stroke_rows;
        n_stroke_proj_ += c.n_stroke_proj;
    }
    n_frows_ += n_stroke_rows_;
    n_prows_ += n_stroke_rows_;
    build_ar_tables();
    const auto tp3 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    hprof_[1] += ms(tp0, tp1);
    hprof_[2] += ms(tp1, tp2);
    hprof_[3] += ms(tp2, tp3);
    return PBSO_OK;
}

// ---------------------------------------------------------------------------
// The row-parallel form of K2 (kernels_exact.hip): which AR forces add samples in this launch, in which rows, and how many
// candidate pairs of each force's engine to evaluate.  A force needs ceil(n_uses * frames / 2) accepted pairs (one more when a
// cached variate is not there to start with: counted); a candidate is accepted with probability pi / 4, so
// pairs / 0.7854 + 8 sigma of the binomial + one batch is asked for -- ar_zero_state_kernel continues the sequence by itself
// should that ever fall short.
void Engine::build_ar_tables() {
    ar_streams_.clear(); ar_uses_.clear(); seg_stream_.clear();
    ar_max_segs_ = 0;
    k2_rows_launch_ = device_profiles_ && k2_rows_ && !ar_serial_ && B_ >= 3 && (!prof_rows_.empty() || n_stroke_rows_ > 0);
    if (!k2_rows_launch_) return;
    const size_t n_states = n_ar_states_.load();
    if (ar_stream_of_state_.size() < n_states) ar_stream_of_state_.resize(n_states, -1);
    ar_last_use_.clear(); ar_epoch_.clear(); ar_param_.clear();
    for (size_t ei = 0; ei < prof_entries_.size(); ++ei) {
        ProfEntry &e = prof_entries_[ei];
        if (e.kind != PBSO_AUTOREGRESSIVE_FORCE) continue;
        int &si = ar_stream_of_state_[(size_t)e.state];
        if (si < 0) {
            si = (int)ar_streams_.size();
            ArStream S;
            std::memset(&S, 0, sizeof(S));
            S.state = e.state;
            S.reset = (e.flags & 1) ? 1 : 0;
            ar_streams_.push_back(S);
            ar_last_use_.push_back(-1); ar_epoch_.push_back(-1); ar_param_.push_back(-1);
        } else if (e.flags & 1) {
            k2_rows_launch_ = false;                 // a slot constructed twice within one launch: the planner never does this
            break;
        }
        ArUse U;
        std::memset(&U, 0, sizeof(U));
        U.entry = (int)ei;
        U.stream = si;
        U.u = ar_streams_[(size_t)si].n_uses++;
        if (e.flags & 3) { ar_epoch_[(size_t)si] = U.u; ar_param_[(size_t)si] = (int)ei; }
        U.epoch_u = ar_epoch_[(size_t)si];
        U.param_entry = ar_param_[(size_t)si];
        e.count = (int)ar_uses_.size();
        ar_last_use_[(size_t)si] = (int)ar_uses_.size();
        ar_uses_.push_back(U);
    }
    // the forces of stroke records: one stream each, its uses the record's dense rows in order (stroke_expand_kernel writes them)
    const size_t n_host_streams = ar_streams_.size();
    for (StrokeRec &r : stroke_recs_) {
        r.stream = -1;
        if (!k2_rows_launch_ || r.n_dense <= 0) continue;
        r.stream = (int)ar_streams_.size();
        ArStream S;
        std::memset(&S, 0, sizeof(S));
        S.state = r.ar_state;
        S.reset = (r.flags0 & 1) ? 1 : 0;
        S.n_uses = r.n_dense;
        ar_streams_.push_back(S);
    }
    int use0 = 0, seg0 = 0;
    for (size_t si = 0; si < ar_streams_.size(); ++si) {
        ArStream &S = ar_streams_[si];
        ar_stream_of_state_[(size_t)S.state] = -1;
        if (!k2_rows_launch_) continue;
        if (si < n_host_streams) ar_uses_[(size_t)ar_last_use_[si]].last = 1;
        S.use0 = use0;
        use0 += S.n_uses;
        const double pairs = 0.5 * ((double)S.n_uses * B_ + 1.0);
        const double want = (pairs / 0.78539 + 8.0 * std::sqrt(pairs) + 256.0) * (k2_margin_pct_ / 100.0);
        S.n_seg = std::max(1, (int)std::ceil(want / K2_SEG));
        S.seg_base = seg0;
        seg0 += S.n_seg;
        ar_max_segs_ = std::max(ar_max_segs_, S.n_seg);
        seg_stream_.insert(seg_stream_.end(), (size_t)S.n_seg, (int)si);
    }
    if (ar_max_segs_ > 8192) k2_rows_launch_ = false;     // (the prefix table of a stream's segments lives in LDS: > 8 M candidates per force and launch)
    if (!k2_rows_launch_) {
        ar_streams_.clear(); ar_uses_.clear(); seg_stream_.clear();
        for (StrokeRec &r : stroke_recs_) r.stream = -1;
    }
}

int Engine::sync() {
    {
        int drc = drain_submit();
        if (drc != PBSO_OK) return drc;
    }
    HIPTRY(hipSetDevice(desc_.device));      // the caller's thread may have another device current
    if (aux_stream_) HIPTRY(hipStreamSynchronize(aux_stream_));
    if (prep_stream_) HIPTRY(hipStreamSynchronize(prep_stream_));
    if (stream_) HIPTRY(hipStreamSynchronize(stream_));
    if (copy_stream_) HIPTRY(hipStreamSynchronize(copy_stream_));
    for (hipStream_t cs : class_stream_)
        if (cs) HIPTRY(hipStreamSynchronize(cs));
    free_retired_blocks();                   // nothing of this engine is in flight any more
    return PBSO_OK;
}

int Engine::read_audio(float *out, size_t n) {
    { int src = sync(); if (src != PBSO_OK) return src; }      // (results come from two streams: the bank's, and the scan's state on the preparation stream)
    if (!last_audio_) return fail(PBSO_ERR_STATE, "no step yet");
    const size_t total = (size_t)objs_.size() * last_nb_ * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, "read_audio size mismatch");
    HIPTRY(hipMemcpyAsync(out, last_audio_, total * sizeof(float), hipMemcpyDeviceToHost, stream_));
    return sync();
}

// some objects' rows of the last step's audio: out[n_rows][n_buffers * B]
int Engine::read_audio_rows(const int *rows, int n_rows, float *out) {
    if (!last_audio_) return fail(PBSO_ERR_STATE, "no step yet");
    if (n_rows < 0 || (n_rows > 0 && (!rows || !out))) return fail(PBSO_ERR_INVALID, "read_audio_rows arguments");
    { int src = sync(); if (src != PBSO_OK) return src; }
    const size_t row = (size_t)last_nb_ * B_;
    for (int i = 0; i < n_rows; ++i) {
        if (!valid_obj(rows[i])) return fail(PBSO_ERR_INVALID, "read_audio_rows: object id out of range");
        HIPTRY(hipMemcpy(out + (size_t)i * row, last_audio_ + (size_t)rows[i] * row, row * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PBSO_OK;
}

int Engine::read_census(unsigned long long *out, size_t n) {
    { int src = sync(); if (src != PBSO_OK) return src; }      // (results come from two streams: the bank's, and the scan's state on the preparation stream)
    if (!census_ || !d_census_.p) return fail(PBSO_ERR_STATE, "census not enabled (PBSO_CENSUS=1) or no step yet");
    // (n_teams rows; for the pipeline kernel its own table's rows; for a time-chunked launch (teams of its shape) x (chunks) rows,
    //  chunk-major: any whole number of rows the launch can have written)
    if (n == 0 || n % CENSUS_WORDS || n > d_census_.cap)
        return fail(PBSO_ERR_INVALID, "read_census size mismatch (12 words per team, at most the rows of the last launch)");
    HIPTRY(hipMemcpyAsync(out, d_census_.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
    return sync();
}

int Engine::read_emitted(unsigned char *out, size_t n) {
    if (n != emitted_.size()) return fail(PBSO_ERR_INVALID, "read_emitted size mismatch");
    std::memcpy(out, emitted_.data(), n);
    return PBSO_OK;
}

int Engine::read_qnorm(int obj, int buffer, float *out, int n) {
    { int src = sync(); if (src != PBSO_OK) return src; }      // (results come from two streams: the bank's, and the scan's state on the preparation stream)
    if (desc_.qnorm_mode == PBSO_QNORM_OFF) return fail(PBSO_ERR_STATE, "qnorm_mode is OFF");
    if (!valid_obj(obj) || buffer < 0 || buffer >= last_nb_ || n < 0 || n > m_pad_)
        return fail(PBSO_ERR_INVALID, "read_qnorm arguments");
    HIPTRY(hipMemcpyAsync(out, d_qnorm_.p + ((size_t)obj * last_nb_ + buffer) * m_pad_, (size_t)n * sizeof(float),
                          hipMemcpyDeviceToHost, stream_));
    return sync();
}

int Engine::read_state(int obj, double *q1, double *q2, int n) {
    { int src = sync(); if (src != PBSO_OK) return src; }      // (results come from two streams: the bank's, and the scan's state on the preparation stream)
    if (!finalized_) return fail(PBSO_ERR_STATE, "read_state before finalize");
    if (!valid_obj(obj) || n < 0 || n > m_pad_) return fail(PBSO_ERR_INVALID, "read_state arguments");
    // the arrays hold (scale x state) and the scale (kernels_iir.hip, "scaled state")
    std::vector<float> a(n), b(n), sc(n);
    HIPTRY(hipMemcpyAsync(a.data(), d_sq_.p + (size_t)obj * m_pad_, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIPTRY(hipMemcpyAsync(b.data(), d_sd_.p + (size_t)obj * m_pad_, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIPTRY(hipMemcpyAsync(sc.data(), d_ss_.p + (size_t)obj * m_pad_, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
    int rc = sync();
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const double qa = (double)a[i] / (double)sc[i], qb = (double)b[i] / (double)sc[i];
        q1[i] = qa;
        q2[i] = form_ != PBSO_FORM_DIRECT ? qa - qb : qb;
    }
    return PBSO_OK;
}

// Restore of the integrator state (the pair pbso_read_state returns): stored unscaled (scale 1), in the form's
// own variables -- (q_{k-1}, q_{k-1} - q_{k-2}) for the velocity and block forms, (q_{k-1}, q_{k-2}) for the direct form.
int Engine::write_state(int obj, const double *q1, const double *q2, int n) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "write_state before finalize");
    if (!valid_obj(obj) || n < 0 || n > objs_[obj].n_modes) return fail(PBSO_ERR_INVALID, "write_state arguments");
    if (failed_) return fail(PBSO_ERR_STATE, "an earlier step failed half-way: create a new engine");
    HIPTRY(hipSetDevice(desc_.device));
    int rc = sync();
    if (rc) return rc;
    std::vector<float> a(n), b(n), sc(n, 1.f);
    for (int i = 0; i < n; ++i) {
        a[i] = (float)q1[i];
        b[i] = form_ != PBSO_FORM_DIRECT ? (float)(q1[i] - q2[i]) : (float)q2[i];
    }
    const size_t off = (size_t)obj * m_pad_;
    HIPTRY(hipMemcpyAsync(d_sq_.p + off, a.data(), n * sizeof(float), hipMemcpyHostToDevice, stream_));
    HIPTRY(hipMemcpyAsync(d_sd_.p + off, b.data(), n * sizeof(float), hipMemcpyHostToDevice, stream_));
    HIPTRY(hipMemcpyAsync(d_ss_.p + off, sc.data(), n * sizeof(float), hipMemcpyHostToDevice, stream_));
    return sync();
}

// ModalSolver::getLatestTransfer, modal_solver.h:145-147
int Engine::get_latest_transfer(int obj, double *out) {
    { int src = sync(); if (src != PBSO_OK) return src; }      // (results come from two streams: the bank's, and the scan's state on the preparation stream)
    if (!finalized_) return fail(PBSO_ERR_STATE, "get_latest_transfer before finalize");
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    const Object &o = objs_[obj];
    if (o.latest_row == XFER_UNIT) {
        for (int i = 0; i < o.n_modes; ++i) { out[i] = 1.0; out[i] *= 1E7; }     // setToUnit :89-92
        return PBSO_OK;
    }
    int src = sync();
    if (src) return src;
    HIPTRY(hipMemcpyAsync(out, d_xfer_.p + (size_t)o.latest_row * m_pad_, (size_t)o.n_modes * sizeof(double),
                          hipMemcpyDeviceToHost, stream_));
    return sync();
}

// ModalSolver::computeTransfer(pos, T *trans), modal_solver.h:302-315, batched
// Multi-listener output: from the next step on the block kernel keeps this object's block-start states.
int Engine::listeners_enable(int obj) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "listeners_enable before finalize");
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    if (!is_block()) return fail(PBSO_ERR_STATE, "the multi-listener mix needs one of the block forms (frames_per_buffer = 513)");
    if (dump_row_.empty()) { dump_row_.assign(objs_.size(), -1); dump_valid_.assign(objs_.size(), 0); }
    if (dump_row_[obj] >= 0) return PBSO_OK;
    const Object &o = objs_[obj];
    // this object's f32 operand table (the engine's own table may hold the split-bf16 form)
    std::vector<float> wt((size_t)m_pad_ / 2 * 64, 0.f);
    // (pbso_set_material rebuilds it from the object's new c1 / c2: retune.cpp)
    for (int m = 0; m < o.n_modes; ++m) mode_walk(o.c1[m], o.c2[m], 0, (size_t)m, 0, W_F32, wt.data(), nullptr, nullptr);
    HIPTRY(hipSetDevice(desc_.device));
    int rc = sync();
    if (rc) return rc;
    // the build of the bank that keeps block-start states evaluates the closed-form qnorm rows whatever qnorm_mode says
    // (a PBSO_QNORM_OFF engine has no G planes yet: the kernel would read through a null pointer)
    rc = build_gq();
    if (rc) return rc;
    HIPTRY(d_wtab32_.ensure((size_t)(n_dump_ + 1) * wt.size(), true, stream_));
    HIPTRY(hipMemcpyAsync(d_wtab32_.p + (size_t)n_dump_ * wt.size(), wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice, stream_));
    HIPTRY(hipStreamSynchronize(stream_));
    dump_row_[obj] = n_dump_++;
    dump_rows_dirty_ = true;
    return PBSO_OK;
}

// out[n_listeners][last_nb * frames]: the last step's audio of `obj` as heard at each position
int Engine::mix_listeners(int obj, const double *pos, int n_listeners, float *out, size_t n_out) {
    { int src = sync(); if (src != PBSO_OK) return src; }      // (results come from two streams: the bank's, and the scan's state on the preparation stream)
    HIPTRY(hipSetDevice(desc_.device));
    if (!finalized_) return fail(PBSO_ERR_STATE, "mix_listeners before finalize");
    if (!valid_obj(obj) || n_listeners <= 0 || !pos || !out) return fail(PBSO_ERR_INVALID, "mix_listeners arguments");
    if (dump_row_.empty() || dump_row_[obj] < 0) return fail(PBSO_ERR_STATE, "pbso_listeners_enable was not called for this object");
    if (dump_nb_ <= 0 || dump_nb_ != last_nb_) return fail(PBSO_ERR_STATE, "no step since pbso_listeners_enable");
    if (!dump_valid_[obj])
        return fail(PBSO_ERR_STATE, "the last step has buffers of this object without block states (dense force profile or per-sample launch)");
    if (n_out != (size_t)n_listeners * last_nb_ * B_) return fail(PBSO_ERR_INVALID, "mix_listeners output size");
    Object &o = objs_[obj];
    DevBuf<double> rows;
    DevBuf<float> dout;
    int rc = PBSO_OK;
    hipError_t e = rows.ensure((size_t)n_listeners * m_pad_, false, stream_);
    if (e == hipSuccess) e = dout.ensure(n_out, false, stream_);
    if (e == hipSuccess && o.have_maps && o.n_maps > 0) {
        // ModalSolver::computeTransfer(pos, T*) per listener (modal_solver.h:302-315)
        if (o.n_maps < o.n_modes) { rows.release(); dout.release(); return fail(PBSO_ERR_MISSING_MAP, "FFAT maps do not cover the audible modes"); }
        std::vector<FfatEvent> evs(n_listeners);
        for (int i = 0; i < n_listeners; ++i) {
            evs[i].obj = obj;
            evs[i].row = i;
            for (int j = 0; j < 3; ++j) evs[i].pos[j] = pos[3 * i + j];
        }
        DevBuf<FfatEvent> dev;
        e = dev.ensure(n_listeners, false, stream_);
        if (e == hipSuccess) e = hipMemcpyAsync(dev.p, evs.data(), n_listeners * sizeof(FfatEvent), hipMemcpyHostToDevice, stream_);
        if (e == hipSuccess) {
            // (the object's modes share one map geometry: every listener located once, lane = mode -- kernels_exact.hip, round 6)
            int le = (!ffat_shared_h_.empty() && ffat_shared_h_[obj])
                         ? launch_ffat_lookup_shared(dev.p, n_listeners, d_ffat_shared_.p, d_geom_.p, d_geom_off_.p, d_n_modes_.p, d_ffat_k_.p,
                                                     d_ffat_valid_.p, d_psi_t_.p, rows.p, m_pad_, stream_)
                         : launch_ffat_lookup(dev.p, n_listeners, d_geom_.p, d_geom_off_.p, d_n_modes_.p, d_psi_.p, rows.p, m_pad_, stream_);
            if (le) e = (hipError_t)le;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        dev.release();
    } else if (e == hipSuccess) {
        std::vector<double> unit((size_t)n_listeners * m_pad_, 1E7);          // no maps: TransMessage::setToUnit (modal_solver.h:89-92)
        e = hipMemcpyAsync(rows.p, unit.data(), unit.size() * sizeof(double), hipMemcpyHostToDevice, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    }
    if (e == hipSuccess) {
        // a buffer whose waves left the scaled-state representation (a transfer weight outside [2^-20, 2^40]) was stepped
        // per sample inside the block kernel and kept no block states: its scale row says 0.  The planner cannot know.
        std::vector<float> sc((size_t)last_nb_ * m_pad_);
        e = hipMemcpyAsync(sc.data(), d_xscale_.p + (size_t)dump_row_[obj] * last_nb_ * m_pad_, sc.size() * sizeof(float), hipMemcpyDeviceToHost, stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        if (e == hipSuccess)
            for (int b = 0; b < last_nb_ && rc == PBSO_OK; ++b)
                for (int m = 0; m < o.n_modes; ++m)
                    if (sc[(size_t)b * m_pad_ + m] == 0.f) {
                        rc = fail(PBSO_ERR_STATE, "the last step has a buffer of this object that was stepped per sample (a transfer weight outside "
                                                  "the scaled-state range): no block states to mix");
                        break;
                    }
    }
    if (rc != PBSO_OK) { rows.release(); dout.release(); return rc; }
    if (e == hipSuccess) {
        const size_t row = (size_t)dump_row_[obj];
        int le = iir_block::launch_listener_mix(d_xdump_.p + row * last_nb_ * 32 * m_pad_ * 2, d_xscale_.p + row * last_nb_ * m_pad_,
                                                d_wtab32_.p + row * ((size_t)m_pad_ / 2 * 64), rows.p, dout.p, last_nb_, m_pad_, o.n_modes,
                                                n_listeners, (long long)last_nb_ * B_, stream_);
        if (le) e = (hipError_t)le;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.p, n_out * sizeof(float), hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) rc = hip_fail(e, "mix_listeners");
    rows.release();
    dout.release();
    return rc;
}

int Engine::host_wait() {
    if (host_last_ < 0) return PBSO_OK;
    HIPTRY(hipSetDevice(desc_.device));
    HIPTRY(hipEventSynchronize(ev_host_copy_[host_last_]));
    return PBSO_OK;
}

// The step's audio summed over the objects, on the device, in a fixed order (what one output stream plays when the scene's
// objects sound together; the per-rank half of the device group's PBSO_GATHER_MIX).  Asynchronous on the engine's stream.
int Engine::mix_objects(void *d_out) {
    if (!last_audio_ || !d_out) return fail(PBSO_ERR_STATE, "mix_objects: no step yet (or a null output)");
    HIPTRY(hipSetDevice(desc_.device));
    const int N = (int)objs_.size();
    const long long n = (long long)last_nb_ * B_;
    HIPTRY(d_mix_parts_.ensure((size_t)mix_objects_groups(N) * n, false, stream_));
    LAUNCHTRY(launch_mix_objects(last_audio_, N, n, n, d_mix_parts_.p, (float *)d_out, stream_));
    return PBSO_OK;
}

int Engine::object_n_maps(int obj) {
    if (!valid_obj(obj)) return fail(PBSO_ERR_INVALID, "object id");
    return objs_[obj].have_maps ? objs_[obj].n_maps : 0;
}

int Engine::compute_transfer_batch(int obj, const double *pos, int n_pos, double *out, int out_cols) {
    HIPTRY(hipSetDevice(desc_.device));      // the caller's thread may have another device current
    if (!finalized_) return fail(PBSO_ERR_STATE, "compute_transfer_batch before finalize");
    if (!valid_obj(obj) || n_pos < 0 || (n_pos && (!pos || !out))) return fail(PBSO_ERR_INVALID, "arguments");
    Object &o = objs_[obj];
    if (!o.have_maps) return 0;
    const int nmap = o.n_maps;
    if (nmap > o.n_modes) return fail(PBSO_ERR_INVALID, "more FFAT maps than audible modes is not supported");
    if (out_cols < nmap) return fail(PBSO_ERR_INVALID, "compute_transfer_batch: out_cols is smaller than the object's map count (pbso_object_n_maps)");
    for (int m = 0; m < nmap; ++m)
        if (m >= (int)o.geom.size() || !o.geom[m].valid)
            return fail(PBSO_ERR_MISSING_MAP, "FFAT map ids are not 0..size-1 (std::map::at throws)");
    if (!n_pos) return 1;
    // Positions go up once; the lookups run in chunks (one workgroup per mode and 1024 positions, the mode's map
    // staged in LDS) into two row buffers, and the copy of chunk c to the caller's memory (the copy stream) runs beside
    // the kernel of chunk c + 1.
    const int CH = 16384;
    const int n_chunks = (n_pos + CH - 1) / CH;
    DevBuf<double> rows, dpos;
    hipEvent_t ev_k[2] = {nullptr, nullptr};
    int rc = PBSO_OK;
    hipError_t e = rows.ensure((size_t)2 * std::min(n_pos, CH) * m_pad_, false, stream_);
    if (e == hipSuccess) e = dpos.ensure((size_t)3 * n_pos, false, stream_);
    if (e == hipSuccess) e = hipMemcpyAsync(dpos.p, pos, (size_t)3 * n_pos * sizeof(double), hipMemcpyHostToDevice, stream_);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev_k[i], hipEventDisableTiming);
    const FfatGeom *g0 = d_geom_.p + geom_off_h_[obj];
    // (round 6) an object whose modes share one map geometry: the positions as lookup events of the shared-geometry kernel -- located
    // once per position, lane = mode, the maps read cell-major (kernels_exact.hip) -- instead of one workgroup per (mode, 1024 positions)
    const bool shared = !ffat_shared_h_.empty() && ffat_shared_h_[obj] && e == hipSuccess;
    DevBuf<FfatEvent> dev_ev;
    if (shared) {
        std::vector<FfatEvent> evs((size_t)n_pos);
        for (int p = 0; p < n_pos; ++p) {
            evs[p].obj = obj;
            evs[p].row = (p % CH) + ((p / CH) & 1) * CH;          // (its row in the two-chunk row buffer)
            for (int j = 0; j < 3; ++j) evs[p].pos[j] = pos[3 * (size_t)p + j];
        }
        e = dev_ev.ensure((size_t)n_pos, false, stream_);
        if (e == hipSuccess) e = hipMemcpy(dev_ev.p, evs.data(), (size_t)n_pos * sizeof(FfatEvent), hipMemcpyHostToDevice);
    }
    auto launch_chunk = [&](int c) -> hipError_t {
        const int p0 = c * CH, n = std::min(CH, n_pos - p0);
        int le = shared ? launch_ffat_lookup_shared(dev_ev.p + p0, n, d_ffat_shared_.p, d_geom_.p, d_geom_off_.p, d_n_modes_.p, d_ffat_k_.p,
                                                    d_ffat_valid_.p, d_psi_t_.p, rows.p, m_pad_, stream_)
                        : launch_ffat_batch(dpos.p + 3 * (size_t)p0, n, g0, nmap, d_psi_.p, rows.p + (size_t)(c & 1) * CH * m_pad_, m_pad_, stream_);
        if (le) return (hipError_t)le;
        return hipEventRecord(ev_k[c & 1], stream_);
    };
    if (e == hipSuccess) e = launch_chunk(0);
    for (int c = 0; c < n_chunks && e == hipSuccess; ++c) {
        if (c + 1 < n_chunks) e = launch_chunk(c + 1);          // (its row buffer was copied out two chunks ago: the copy below is synchronous)
        const int p0 = c * CH, n = std::min(CH, n_pos - p0);
        if (e == hipSuccess) e = hipStreamWaitEvent(prep_stream_, ev_k[c & 1], 0);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(out + (size_t)p0 * out_cols, (size_t)out_cols * sizeof(double), rows.p + (size_t)(c & 1) * CH * m_pad_,
                                 (size_t)m_pad_ * sizeof(double), (size_t)nmap * sizeof(double), n, hipMemcpyDeviceToHost, prep_stream_);
        if (e == hipSuccess) e = hipStreamSynchronize(prep_stream_);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    if (e != hipSuccess) rc = hip_fail(e, "compute_transfer_batch");
    for (hipEvent_t ev : ev_k)
        if (ev) (void)hipEventDestroy(ev);
    rows.release();
    dpos.release();
    dev_ev.release();
    return rc == PBSO_OK ? 1 : rc;
}

int Engine::info(pbso_engine_info *out) {
    std::memset(out, 0, sizeof(*out));
    out->n_objects = (int)objs_.size();
    out->frames_per_buffer = B_;
    out->modes_padded = m_pad_;
    out->modes_per_lane = R_;
    out->waves_per_object = W_;
    out->n_teams = n_teams_;
    out->lds_bytes_per_workgroup = !finalized_ ? 0 : is_block() ? (int)block_lds_bytes(W_, R_) : (int)iir_lds_bytes(W_, n_tiles_);
    out->recurrence_form = form_;
    out->total_block_launches = tot_block_launches_;
    out->total_sample_launches = tot_sample_launches_;
    out->total_split_launches = tot_split_launches_;
    out->total_time_chunk_launches = tot_tc_launches_;
    out->total_dense_increment_launches = tot_tc_dense_launches_;
    out->total_segmented_scans = tot_seg_scans_;
    out->last_time_chunk_shape = last_tc_shape_;
    out->last_time_chunk_buffers = last_tc_cb_;
    out->last_time_chunk_teams = last_tc_teams_;
    out->total_dropped_hits = dropped_hits_.load();
    out->total_one_stream_launches = tot_one_stream_launches_;
    out->start_gate = gate_choice_;
    out->total_gate_timeouts = gate_timeouts_;
    out->total_host_submit_ms = hprof_[4];
    out->total_ffat_shared_events = tot_ffat_shared_events_;
    out->total_ffat_general_events = tot_ffat_general_events_;
    out->buffers_done = buffers_done_;
    out->last_step_host_plan_ms = last_plan_ms_;
    out->last_step_forced_rows = last_frows_;
    out->last_step_transfer_rows = last_trows_;
    int rc = harvest_timing(true);
    if (rc) return rc;
    out->last_step_kernel_ms = last_kernel_ms_;
    out->last_step_device_ms = last_device_ms_;
    out->total_kernel_ms = tot_kernel_ms_;
    out->total_device_ms = tot_device_ms_;
    out->total_timed_launches = tot_timed_launches_;
    out->total_host_plan_ms = tot_plan_ms_;
    out->total_steps = tot_steps_;
    return PBSO_OK;
}

// Reads the HIP-event pairs of finished launches into the totals.  blocking: waits for everything in flight (pbso_get_info);
// otherwise only the launches whose last event has already completed are read (called once per launch: keeps the number of live
// events small and lets the K2 priority follow the workload without ever stalling the host).
int Engine::harvest_timing(bool blocking) {
    if (ev_pending_.empty()) return PBSO_OK;
    if (blocking) {
        int rc = sync();
        if (rc) return rc;
    }
    size_t done = 0;
    for (; done < ev_pending_.size(); ++done) {
        EvQuad &q = ev_pending_[done];
        if (submit_ && q.batch > submit_->done()) break;      // (its events are not recorded yet: an unrecorded event reads as complete)
        if (!blocking && hipEventQuery(q.p1) != hipSuccess) break;
        float ms = 0, ms2 = 0;
        HIPTRY(hipEventElapsedTime(&ms, q.k0, q.k1));
        HIPTRY(hipEventElapsedTime(&ms2, q.p0, q.p1));
        if (timeline_) {                            // PBSO_TIMELINE=1: where each timed launch's events fall (ms since the first one)
            float a = 0, b = 0, c = 0, d = 0;
            if (!timeline_have_base_) { timeline_ref_ = q.p0; timeline_quad_ = q; timeline_have_base_ = true; timeline_keep_ = true; timeline_h0_ = q.h_prep; }
            HIPTRY(hipEventElapsedTime(&a, timeline_ref_, q.p0));
            HIPTRY(hipEventElapsedTime(&b, timeline_ref_, q.k0));
            HIPTRY(hipEventElapsedTime(&c, timeline_ref_, q.k1));
            HIPTRY(hipEventElapsedTime(&d, timeline_ref_, q.p1));
            std::fprintf(stderr, "pbso timeline: step %lld device: prep starts %.3f | bank starts %.3f ends %.3f | launch done %.3f || host: step entered %.3f, "
                                 "prep submitted from %.3f (upload call returned %.3f), bank submitted at %.3f, all submitted %.3f\n", (long long)q.step_id, a, b, c, d,
                         q.h_enter - timeline_h0_, q.h_prep - timeline_h0_, q.h_copy - timeline_h0_, q.h_bank - timeline_h0_, q.h_done - timeline_h0_);
        }
        if (q.step_id != harvest_step_) {          // "last step" sums the launches of one step
            harvest_step_ = q.step_id;
            last_kernel_ms_ = 0;
            last_device_ms_ = 0;
        }
        if (q.has_k2) {
            float msf = 0;
            HIPTRY(hipEventElapsedTime(&msf, q.f0, q.f1));
            // exponential averages over the last few timed launches
            k2_ms_avg_ = k2_ms_n_ ? 0.75 * k2_ms_avg_ + 0.25 * msf : msf;
            k2_bank_ms_avg_ = k2_ms_n_ ? 0.75 * k2_bank_ms_avg_ + 0.25 * ms : ms;
            k2_ms_n_ += 1;
        }
        last_kernel_ms_ += ms;
        tot_kernel_ms_ += ms;
        tot_timed_launches_ += 1;
        last_device_ms_ += ms2;
        tot_device_ms_ += ms2;
        if (timeline_keep_) timeline_keep_ = false;      // (the reference launch's events stay out of the free list)
        else ev_free_.push_back(q);
    }
    ev_pending_.erase(ev_pending_.begin(), ev_pending_.begin() + (long)done);
    if (k2_prio_auto_ && k2_ms_n_ >= 2) {
        // the longer of the two kernels that run side by side gets the SIMDs they share (with hysteresis)
        const int want = k2_ms_avg_ > (k2_prio_ ? 0.85 : 0.95) * k2_bank_ms_avg_ ? 3 : 0;
        if (want != k2_prio_ && host_profile_)
            std::fprintf(stderr, "pbso: force-profile kernel %.3f ms, oscillator bank %.3f ms per timed launch: K2 wave priority %d -> %d\n",
                         k2_ms_avg_, k2_bank_ms_avg_, k2_prio_, want);
        k2_prio_ = want;
    }
    return PBSO_OK;
}

}  // namespace pbso