// Engine::step: one launch (step_chunk) as its stages, in the order the streams see them.  See engine.h.
#include "engine.h"
#include "submit_queue.h"

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cstring>
#include <thread>
#include <unordered_map>

namespace pbso {

// Engine::step_chunk's stream calls: made at once, or -- with the second submitting thread (submit_queue.h) -- recorded with their
// arguments evaluated HERE and made by the worker.  `L` is the stage's Launch.
#define QHIP(fn, ...)                                                                      \
    do {                                                                                   \
        if (L.defer) L.ops.push_back(make_submit_op(#fn, fn, __VA_ARGS__));                \
        else HIPTRY(fn(__VA_ARGS__));                                                      \
    } while (0)
#define QLAUNCH(fn, ...)                                                                   \
    do {                                                                                   \
        if (L.defer) L.ops.push_back(make_submit_op(#fn, fn, __VA_ARGS__));                \
        else LAUNCHTRY(fn(__VA_ARGS__));                                                   \
    } while (0)
// a device buffer that has to GROW while recorded calls are still waiting: its keep-copy and the retirement of the old block are
// immediate calls and must come behind them in their streams -- wait for the worker first (rare: the first steps of an engine)
#define GROWTRY(buf, n, keep, s)                                                           \
    do {                                                                                   \
        if (submit_ && (size_t)(n) > (buf).cap) {                                          \
            int _d = drain_submit();                                                       \
            if (_d != PBSO_OK) return _d;                                                  \
        }                                                                                  \
        HIPTRY((buf).ensure((n), (keep), (s)));                                            \
    } while (0)

// ---------------------------------------------------------------------------
// One step = nb buffers for every object.  Long steps are cut into launches of at most
// chunk_buffers_ buffers so that the host plans chunk c+1 while the device runs chunk c (the same
// overlap consecutive steps have); results do not depend on the cut (state, force lists and queues
// carry over exactly as between steps).
int Engine::step(int nb, void *d_audio_user) {
    HIPTRY(hipSetDevice(desc_.device));      // the caller's thread may have another device current
    if (!finalized_) return fail(PBSO_ERR_STATE, "step before finalize");
    if (nb <= 0) return fail(PBSO_ERR_INVALID, "n_buffers must be > 0");
    if (failed_) return fail(PBSO_ERR_STATE, "an earlier step failed half-way (" + failed_why_ + "): queues and force lists are no "
                                             "longer consistent, create a new engine");
    const int N = (int)objs_.size();
    const bool defer = submit_ != nullptr;             // (GROWTRY: a buffer that grows waits for the recorded calls first)
    float *audio = (float *)d_audio_user;
    // outputs of the whole step (growth drains the device first, see DevBuf::ensure)
    if (!audio) {
        GROWTRY(d_audio_, (size_t)N * nb * B_, false, stream_);
        audio = d_audio_.p;
    }
    if (desc_.qnorm_mode != PBSO_QNORM_OFF || n_dump_ > 0) GROWTRY(d_qnorm_, (size_t)N * nb * m_pad_, false, stream_);
    if (n_dump_ > 0) {
        // block-start states of the objects a multi-listener mix was asked for (pbso_listeners_enable)
        GROWTRY(d_xdump_, (size_t)n_dump_ * nb * 32 * m_pad_ * 2, false, stream_);
        GROWTRY(d_xscale_, (size_t)n_dump_ * nb * m_pad_, false, stream_);
        if (dump_rows_dirty_) {
            if (defer) { int drc = drain_submit(); if (drc != PBSO_OK) return drc; }
            GROWTRY(d_dump_row_, N, false, stream_);
            HIPTRY(hipMemcpyAsync(d_dump_row_.p, dump_row_.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, stream_));
            HIPTRY(hipStreamSynchronize(stream_));           // (dump_row_ is pageable host memory)
            dump_rows_dirty_ = false;
        }
        dump_nb_ = nb;
        std::fill(dump_valid_.begin(), dump_valid_.end(), 1);
    }
    {
        // (a step's launches may run on different kernels: room for either kind's partial rows)
        int rows = std::max(use_split() ? n_ts_part_rows_ : 0, n_part_rows_);
        if (tc_ok_) for (const TcSet &ts : tc_) rows = std::max(rows, ts.n_part_rows);
        if (rows) GROWTRY(d_audio_parts_, (size_t)rows * nb * B_, false, stream_);
    }
    emitted_.assign((size_t)N * nb, 1);
    const int64_t step_id = tot_steps_;
    double plan_ms = 0;
    for (int b0 = 0; b0 < nb; b0 += chunk_buffers_) {
        int rc = step_chunk(std::min(chunk_buffers_, nb - b0), b0, nb, audio, step_id);
        if (rc != PBSO_OK) {
            // the reference would have aborted here (assert) or be equally stuck (device error)
            failed_ = true;
            failed_why_ = err_;
            return rc;
        }
        plan_ms += last_plan_ms_;
    }
    last_plan_ms_ = plan_ms;
    tot_plan_ms_ += plan_ms;
    tot_steps_ += 1;
    last_audio_ = audio;
    last_nb_ = nb;
    return PBSO_OK;
}

// The plan arena behind the descriptors: every table of a launch is added ONCE -- element type, host source, count, and the
// rows behind the host's that the device fills itself (stroke_expand_kernel, in the device copy) -- and the handle it gets back
// gives its place in the pinned arena and, typed, in the device copy.  The order of the add calls is the layout.
template <class T>
struct ArenaTable {
    size_t off = 0;
    T *host(unsigned char *ha) const { return reinterpret_cast<T *>(ha + off); }
    T *dev(unsigned char *da) const { return reinterpret_cast<T *>(da + off); }
};
struct PlanArena {
    size_t off;                                          // the next free byte
    static constexpr int MAX_TABLES = 32;              // (24 today; add() asserts the bound)
    struct Copy { size_t off; const void *src; size_t bytes; } copies[MAX_TABLES];
    int n = 0;
    explicit PlanArena(size_t front) : off(front) {}
    template <class T>
    ArenaTable<T> add(const T *src, size_t count, size_t device_rows = 0) {
        ArenaTable<T> t;
        t.off = off;
        assert(n < MAX_TABLES);
        copies[n++] = Copy{off, src, count * sizeof(T)};
        off += arena_align((count + device_rows) * sizeof(T));
        return t;
    }
    void fill(unsigned char *ha) const {
        for (int i = 0; i < n; ++i)
            if (copies[i].bytes) std::memcpy(ha + copies[i].off, copies[i].src, copies[i].bytes);
    }
};

// One launch, from step_chunk's first line to its last: what its stages hand to each other.  Lives on step_chunk's stack.
struct Engine::Launch {
    int nb, b0, nb_total, N;
    int64_t step_id;
    float *audio;
    PlanSet *ps;
    DevBuf<float> *grows;
    // the second submitting thread: this launch's stream calls are recorded (QHIP / QLAUNCH) and handed over at the end
    bool defer = false;
    std::vector<SubmitOp> ops;
    hipStream_t sk = nullptr, sp = nullptr, sa = nullptr;      // bank, preparation, the preparation's fork (or sp)
    // decisions (launch_policy.h)
    PolicyScene scene;
    PolicySettings set;
    PolicyLaunch pl;
    bool one_stream = false, tc_launch = false, fuse_combine = false, rows_and_combine = false, split_prep = false, split_launch = false;
    bool dense_heavy = false, timed = false, qn = false;
    int tc_set = -1, tc_cb = 0;
    EvQuad evq;
    IirParams kp;
    // counts
    int n_chains = 0, n_srows = 0, n_srecs = 0, n_prof_rows = 0, n_ar_uses = 0, n_frows = 0, n_proj = 0, n_cl = 0, n_cq = 0;
    int n_ffat_sh = 0, n_ffat_gen = 0, s_lo = 0, s_n = 0;
    std::vector<int> cp;                                 // rows to re-park: [src...] then [dst...]
    // the plan arena
    unsigned char *da = nullptr;
    ArenaTable<int> row_ptr, slot_idx, row_obj, prow_obj, chain, arseg, stage_slot, svids, copy;
    ArenaTable<ProfEntry> pent;
    ArenaTable<ProfRow> prow;
    ArenaTable<ArUse> aruse;
    ArenaTable<ArStream> arstream;
    ArenaTable<float> tprof;
    ArenaTable<double> stage, scoords, svn;
    ArenaTable<ProjectEvent> proj, projd;
    ArenaTable<StrokeRec> srec;
    ArenaTable<int64_t> sstamp;
    ArenaTable<unsigned char> sflags;
    ArenaTable<FfatEvent> ffat;
    ArenaTable<FfatRun> ffat_runs;
    const float *d_tprof = nullptr;
    std::chrono::steady_clock::time_point tw0, t0, tsub0, tsub1, tsub2;
};
static double host_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

PolicyScene Engine::policy_scene() const {
    PolicyScene s;
    s.n_obj = (long long)objs_.size();
    s.m_pad = m_pad_;
    s.n_cus = n_cus_;
    for (int k = 0; k < 3; ++k) s.shape[k] = PolicyShape{tc_[k].waves, tc_[k].cover, tc_[k].waves_per_cu};
    s.pipe_teams = n_ts_teams_;
    return s;
}
PolicySettings Engine::policy_settings() const {
    PolicySettings s;
    s.block = is_block();
    s.tc_ok = tc_ok_; s.have_scan = d_scan_.p != nullptr; s.have_ftab = d_ftab_.p != nullptr; s.ftab_forced = ftab_forced_;
    s.listeners = n_dump_ > 0;
    s.use_split = use_split(); s.split_always = split_always_;
    s.dense_to_k1 = dense_to_k1_;
    s.qnorm_off = desc_.qnorm_mode == PBSO_QNORM_OFF;
    s.device_profiles = device_profiles_; s.have_aux_stream = aux_stream_ != nullptr; s.sync_values = sync_values_;
    s.tc_mode = tc_mode_; s.tc_shape = tc_shape_;
    s.scan_kernel = desc_.scan_kernel; s.stream_sync = desc_.stream_sync; s.pipe_consumers = desc_.pipe_consumers; s.prep_split = prep_split_;
    return s;
}
static_assert(POLICY_SCAN_SEG_MAX == SCAN_SEG_MAX, "launch_policy.h has no kernels.h: the constant is written out there");

int Engine::step_chunk(int nb, int b0, int nb_total, float *audio, int64_t step_id) {
    Launch L;
    L.nb = nb; L.b0 = b0; L.nb_total = nb_total; L.N = (int)objs_.size();
    L.audio = audio;
    L.ps = &set_[cur_set_];
    L.grows = &d_grows_[cur_set_];
    L.step_id = step_id;
    plan_b0_ = b0;
    plan_nb_total_ = nb_total;
    int rc;
    if ((rc = launch_wait_set(L)) != PBSO_OK) return rc;
    if ((rc = launch_plan(L)) != PBSO_OK) return rc;
    if ((rc = launch_open(L)) != PBSO_OK) return rc;
    if ((rc = launch_pack(L)) != PBSO_OK) return rc;
    if ((rc = launch_upload_and_gate(L)) != PBSO_OK) return rc;
    if ((rc = launch_expand_strokes(L)) != PBSO_OK) return rc;
    if ((rc = launch_bank_params(L)) != PBSO_OK) return rc;
    if ((rc = launch_prepare(L)) != PBSO_OK) return rc;
    if (L.tc_launch && (rc = launch_scan(L)) != PBSO_OK) return rc;
    if ((rc = launch_hand_over(L)) != PBSO_OK) return rc;
    if ((rc = launch_bank(L)) != PBSO_OK) return rc;
    return launch_finish(L);
}

// stage 1: the plan set is free -- its last launch has been made, its uploads are done
int Engine::launch_wait_set(Launch &L) {
    L.tw0 = std::chrono::steady_clock::now();
    L.defer = submit_ != nullptr;
    if (L.defer) {
        L.ops.reserve(48);
        submit_->wait(set_batch_[cur_set_]);             // the launch that last used this plan set has been MADE (its events recorded) ...
        std::string why;
        if (submit_->error(&why)) return fail(PBSO_ERR_HIP, "a launch of an earlier step failed on the submitting thread: " + why);
    }
    HIPTRY(hipEventSynchronize(ev_set_[cur_set_]));      // ... and this set's previous uploads are done
    if (stroke_ev_live_[cur_set_]) {                     // PBSO_HOST_PROFILE=1: the stroke kernel of the launch that last used this set
        float ms = 0.f;
        HIPTRY(hipEventSynchronize(stroke_ev_[cur_set_][1]));
        HIPTRY(hipEventElapsedTime(&ms, stroke_ev_[cur_set_][0], stroke_ev_[cur_set_][1]));
        stroke_kernel_ms_ += ms;
        stroke_kernel_n_ += 1;
        stroke_ev_live_[cur_set_] = false;
    }
    L.t0 = std::chrono::steady_clock::now();
    hprof_[0] += std::chrono::duration<double, std::milli>(L.t0 - L.tw0).count();
    return PBSO_OK;
}

// stage 2: the planner, and the rows that keep _latest_transfer / the transfer queue in their persistent rows after the launch
int Engine::launch_plan(Launch &L) {
    const int N = L.N;
    int rc = plan(L.nb);
    if (rc != PBSO_OK) return rc;
    std::vector<int> copy_latest, copy_queued;
    for (int i : busy_) {
        Object &o = objs_[i];
        if (o.latest_row >= 0 && o.latest_row != i) {
            copy_latest.push_back(o.latest_row);
            copy_latest.push_back(i);
            o.latest_row = i;
        }
        if (o.trans_full && o.trans_row != N + i) {
            copy_queued.push_back(o.trans_row);
            copy_queued.push_back(N + i);
            o.trans_row = N + i;
        }
    }
    const int n_cl = L.n_cl = (int)copy_latest.size() / 2, n_cq = L.n_cq = (int)copy_queued.size() / 2;
    // layout: [src...] then [dst...]
    L.cp.resize((size_t)2 * (n_cl + n_cq));
    for (int i = 0; i < n_cl; ++i) { L.cp[i] = copy_latest[2 * i]; L.cp[n_cl + n_cq + i] = copy_latest[2 * i + 1]; }
    for (int i = 0; i < n_cq; ++i) { L.cp[n_cl + i] = copy_queued[2 * i]; L.cp[n_cl + n_cq + n_cl + i] = copy_queued[2 * i + 1]; }
    L.n_chains = (int)chain_ptr_.size();
    L.n_srows = n_stroke_rows_;
    L.n_srecs = (int)stroke_recs_.size();
    L.n_prof_rows = (int)prof_rows_.size() + L.n_srows;          // (stroke rows: written on the device, behind the host's)
    L.n_ar_uses = (int)ar_uses_.size() + (k2_rows_launch_ ? L.n_srows : 0);
    chain_ptr_.push_back(L.n_prof_rows);
    last_plan_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - L.t0).count();
    L.tsub0 = std::chrono::steady_clock::now();
    L.n_frows = n_frows_;
    last_frows_ = L.n_frows;
    last_trows_ = (int64_t)ffat_.size();
    return PBSO_OK;
}

// The launch's streams and kind, its timing events, and the preparation stream's wait for this set's device buffers.
int Engine::launch_open(Launch &L) {
    const int nb = L.nb;
    L.scene = policy_scene();
    L.set = policy_settings();
    L.pl = PolicyLaunch{nb, n_prows_, k2_rows_launch_};
    // Latency path: a short single-launch step submitted while the device is idle (the real-time facade: step, wait, step) has
    // nothing to run beside -- its preparation goes on the bank's own stream, and the 11 us an event takes to hand a launch
    // from one stream to the other (profiles/r04_stream_sync.txt) are saved.  Ordering only: same kernels, same arguments.
    if (latency_path_ && nb == L.nb_total && nb <= 4 && !L.defer) {      // (the query below needs the previous launch's events recorded)
        L.one_stream = last_set_ < 0 || hipEventQuery(ev_k1_done_[last_set_]) == hipSuccess;      // (the previous bank, hence its preparation)
        (void)hipGetLastError();
    }
    // K5: a launch without (many) dense-profile buffers on a chip the scene cannot fill runs the block kernel as (team, chunk of
    // buffers) workgroups behind a scan of the buffer-start states (kernels_scan.hip)
    L.tc_launch = is_block() && !split_always_ && choose_time_chunks(L.scene, L.set, L.pl, &L.tc_set, &L.tc_cb);
    L.sk = stream_;
    L.sp = L.one_stream ? L.sk : prep_stream_;
    hipStream_t sp = L.sp;
    // (the preparation stream takes over again behind a launch that went without it: behind that launch's bank)
    if (!L.one_stream && last_one_stream_ && last_set_ >= 0) QHIP(hipStreamWaitEvent, sp, ev_k1_done_[last_set_], 0);
    // device arenas (growth drains the device first, see DevBuf::ensure)
    GROWTRY(d_slots_, std::max<size_t>(1, n_slots_.load()) * m_pad_, true, sp);
    GROWTRY(*L.grows, std::max<size_t>(1, (size_t)L.n_frows) * m_pad_, false, sp);
    L.qn = desc_.qnorm_mode != PBSO_QNORM_OFF;
    {
        int hrc = harvest_timing(ev_pending_.size() >= 256);      // (what has finished; everything when too many events are live)
        if (hrc != PBSO_OK) return hrc;
    }
    EvQuad &evq = L.evq;
    if (!ev_free_.empty()) {
        evq = ev_free_.back();
        ev_free_.pop_back();
    } else {
        HIPTRY(hipEventCreate(&evq.k0));
        HIPTRY(hipEventCreate(&evq.k1));
        HIPTRY(hipEventCreate(&evq.p0));
        HIPTRY(hipEventCreate(&evq.p1));
        HIPTRY(hipEventCreate(&evq.f0));
        HIPTRY(hipEventCreate(&evq.f1));
    }
    evq.step_id = L.step_id;
    evq.has_k2 = false;
    evq.h_enter = std::chrono::duration<double, std::milli>(L.t0.time_since_epoch()).count();
    // (two timing events before and three after the bank cost the stream ~15 us per launch -- 2 % of a 0.7 ms step)
    L.timed = timing_every_ > 0 && (launch_seq_ % (unsigned)timing_every_) == 0;
    // ---- preparation stream: this set's device buffers are free once the oscillator bank that last read them (N_SETS
    //      launches ago) has finished.  (The upload stays on this stream: on one of its own the next launch's scan starts as soon
    //      as this launch's has finished -- beside the START of a bank, whose workgroups then wait for the slots it holds:
    //      512 x 512 x 86 0.51 -> 0.59 ms per step, scripts/debug/r04_sync.sh.)
    QHIP(hipStreamWaitEvent, sp, ev_k1_done_[cur_set_], 0);
    if (L.timed) QHIP(hipEventRecord, evq.p0, sp);
    evq.h_prep = host_ms();
    return PBSO_OK;
}

// A launch of ONE buffer (the real-time step): the rows of explicit data and the projections whose vectors outlive the buffer are
// taken by the combine kernel itself -- every slot filled now is read by exactly one row of this launch -- instead of a scatter and
// a projection launch in front of it (kernels_exact.hip: force_combine_kernel).  Any slot that is NOT read exactly once (a force
// whose profile is all zero in this buffer leaves its row out) keeps the separate launches.
bool Engine::fuse_one_buffer_combine(int nb, int n_frows) {
    bool fuse_combine = fuse_short_ && nb == 1 && n_frows > 0 && (!stage_slot_.empty() || !proj_.empty());
    if (!fuse_combine) return false;
    const int n_ev = (int)(proj_direct_.size() + proj_.size());
    std::unordered_map<int, std::pair<int, int>> code;      // slot -> (entry, references)
    for (size_t e = 0; e < proj_.size(); ++e) code[proj_[e].slot] = {-((int)(proj_direct_.size() + e) + 1), 0};
    for (size_t r = 0; r < stage_slot_.size(); ++r) code[stage_slot_[r]] = {-(n_ev + (int)r + 1), 0};
    fuse_combine = code.size() == proj_.size() + stage_slot_.size();      // (a slot filled twice in one launch: never, but not fused)
    for (int si : slot_idx_) {
        if (si < 0) continue;
        auto it = code.find(si);
        if (it != code.end()) ++it->second.second;
    }
    for (const auto &kv : code) fuse_combine = fuse_combine && kv.second.second == 1;
    if (fuse_combine) {
        for (int &si : slot_idx_) {
            if (si < 0) continue;
            auto it = code.find(si);
            if (it != code.end()) si = it->second.first;
        }
        proj_direct_.insert(proj_direct_.end(), proj_.begin(), proj_.end());
        proj_.clear();
    }
    return fuse_combine;
}

// stage 3: everything the planner produced, behind the descriptors in the set's pinned arena
int Engine::launch_pack(Launch &L) {
    PlanSet &ps = *L.ps;
    hipStream_t sp = L.sp;
    L.fuse_combine = fuse_one_buffer_combine(L.nb, L.n_frows);
    L.n_proj = (int)proj_.size() + n_stroke_proj_;      // (behind the fusion above, which may have emptied proj_)
    // the listener events as runs of one object each (the planner lists them object by object): one geometry read per (run, mode)
    // (events of objects whose modes share one map geometry first: they go to the kernel that locates a position once per event)
    if (n_ffat_shared_ > 0 && !ffat_.empty()) {
        auto mid = std::stable_partition(ffat_.begin(), ffat_.end(), [&](const FfatEvent &e) { return ffat_shared_h_[e.obj] != 0; });
        L.n_ffat_sh = (int)(mid - ffat_.begin());
    }
    L.n_ffat_gen = (int)ffat_.size() - L.n_ffat_sh;
    tot_ffat_shared_events_ += L.n_ffat_sh;
    tot_ffat_general_events_ += L.n_ffat_gen;
    ffat_runs_.clear();
    for (size_t i = (size_t)L.n_ffat_sh; i < ffat_.size(); ++i) {
        if (ffat_runs_.empty() || ffat_runs_.back().obj != ffat_[i].obj) ffat_runs_.push_back(FfatRun{ffat_[i].obj, (int)i, 0, 0});
        ffat_runs_.back().count += 1;
    }
    // (every table with stroke rows: room for them behind the host's part; stroke_expand_kernel fills it in the device copy)
    const size_t n_srows = (size_t)L.n_srows, dp = device_profiles_ ? 1 : 0;
    PlanArena a(ps.front_bytes);
    L.row_ptr = a.add(row_ptr_.data(), row_ptr_.size(), n_srows);
    L.slot_idx = a.add(slot_idx_.data(), slot_idx_.size(), n_srows);
    L.row_obj = a.add(row_obj_.data(), row_obj_.size(), n_srows);
    L.prow_obj = a.add(prow_obj_.data(), prow_obj_.size(), n_srows);
    L.pent = a.add(prof_entries_.data(), dp * prof_entries_.size(), dp * n_srows);
    L.prow = a.add(prof_rows_.data(), dp * prof_rows_.size(), dp * n_srows);
    L.chain = a.add(chain_ptr_.data(), dp * chain_ptr_.size());
    L.aruse = a.add(ar_uses_.data(), ar_uses_.size(), k2_rows_launch_ ? n_srows : 0);
    L.arstream = a.add(ar_streams_.data(), ar_streams_.size());
    L.arseg = a.add(seg_stream_.data(), seg_stream_.size());
    L.tprof = a.add(tprof_.data(), (1 - dp) * tprof_.size());
    L.stage = a.add(stage_.data(), stage_.size());
    L.stage_slot = a.add(stage_slot_.data(), stage_slot_.size());
    L.proj = a.add(proj_.data(), proj_.size(), (size_t)n_stroke_proj_);
    L.projd = a.add(proj_direct_.data(), proj_direct_.size());
    // the stroke records and the part of the caller's arrays they refer to, as given (the arrays are borrowed only until the step returns)
    const int n_srecs = L.n_srecs;
    const int s_lo = L.s_lo = n_srecs ? stroke_recs_.front().e0 : 0;
    const size_t s_n = L.s_n = n_srecs ? stroke_recs_.back().e0 + stroke_recs_.back().n_ent - s_lo : 0;
    L.srec = a.add((const StrokeRec *)nullptr, 0, (size_t)n_srecs);      // (written below, rebased by s_lo)
    L.sstamp = a.add(s_n ? script_.stamps + s_lo : nullptr, s_n);
    L.svids = a.add(s_n ? script_.vids + 3 * (size_t)s_lo : nullptr, s_n * 3);
    L.scoords = a.add(s_n ? script_.coords + 3 * (size_t)s_lo : nullptr, s_n * 3);
    L.svn = a.add(s_n ? script_.vn + 3 * (size_t)s_lo : nullptr, s_n * 3);
    L.sflags = a.add(script_.flags && s_n ? script_.flags + s_lo : nullptr, script_.flags ? s_n : 0);
    L.ffat = a.add(ffat_.data(), ffat_.size());
    L.copy = a.add(L.cp.data(), L.cp.size());
    L.ffat_runs = a.add(ffat_runs_.data(), ffat_runs_.size());
    HIPTRY(ps.h_arena.ensure_keep(a.off, ps.front_bytes));
    plan_desc_ = reinterpret_cast<BufDesc *>(ps.h_arena.p);      // (the arena may have moved)
    ps.last_bytes = a.off;
    a.fill(ps.h_arena.p);
    for (int i = 0; i < n_srecs; ++i) {
        StrokeRec &r = L.srec.host(ps.h_arena.p)[i];
        r = stroke_recs_[(size_t)i];
        r.e0 -= s_lo;
    }
    if (device_profiles_) {
        if (k2_rows_launch_) {
            const size_t ns = std::max<size_t>(1, ar_streams_.size()), nu = std::max<size_t>(1, (size_t)L.n_ar_uses);
            const size_t ng = std::max<size_t>(1, seg_stream_.size());
            GROWTRY(d_ar_snaps_, ns, false, sp);
            GROWTRY(d_ar_fins_, ns, false, sp);
            GROWTRY(d_ar_recs_, nu, false, sp);
            GROWTRY(d_ar_cbuf_, nu * (size_t)b_pad_, false, sp);
            GROWTRY(d_ar_vnorm_, ng * 2 * K2_SEG, false, sp);
            GROWTRY(d_ar_vstate_, ng * K2_SEG, false, sp);
            GROWTRY(d_ar_segcount_, ng, false, sp);
        }
        GROWTRY(ps.d_tprof, std::max<size_t>(1, (size_t)n_prows_) * b_pad_, false, sp);
        GROWTRY(d_arstate_, std::max<size_t>(1, n_ar_states_.load()), true, sp);
    }
    GROWTRY(ps.d_arena, a.off, false, sp);
    L.da = ps.d_arena.p;
    L.d_tprof = device_profiles_ ? ps.d_tprof.p : L.tprof.dev(L.da);
    return PBSO_OK;
}

// stage 4: ONE upload, and the start gate.
// (Twelve separate copies cost the host 0.1 ms of API calls per step, and the small ones went through
// blit kernels that cannot start while the oscillator bank fills the register file.)
int Engine::launch_upload_and_gate(Launch &L) {
    PlanSet &ps = *L.ps;
    hipStream_t sp = L.sp;
    unsigned char *ha = ps.h_arena.p;
    const size_t off = ps.last_bytes;
    QHIP(hipMemcpyAsync, ps.d_arena.p, ha, off, hipMemcpyHostToDevice, sp);
    QHIP(hipEventRecord, ev_set_[cur_set_], sp);          // this set's pinned arena is reusable
    // the start gate: this launch's preparation kernels behind the START of the previous launch's bank (engine.h).  By policy
    // for LONG launches only: there the gate's few microseconds are nothing, and what it prevents is expensive -- a scan of 860
    // buffers that the preparation stream runs TWO launches ahead trails the bank it was squeezed beside by 0.2 ms, holds LDS
    // while the next bank starts, and that bank's left-over workgroups wait a whole workgroup's length (512 x 512 x 860: every
    // other launch 9 instead of 4.6 ms in one run of four).  Gated, a scan is never more than one launch ahead, and the bank
    // that needs it waits for it.
    // (stream_sync = 4, round 5: the gate as a wait of the SUBMITTING thread on a word of pinned host memory the previous bank's
    //  first workgroup writes.  Built because hipStreamWaitValue64 runs on this stack as a kernel that waits -- `__amd_rocclr_streamOpsWait`
    //  sits 1.1 of a 1.28 ms bank until workgroups retire, scripts/debug/r05_timeline_share.sh -- and was suspected behind the share's
    //  outlier runs; those came from the planner's helper threads (PlanPool::run), both forms show them alike, and the host form
    //  costs the host its second launch of run-ahead: an option, not the policy.)
    const bool gated = gate_now(L.set, L.pl, L.one_stream, last_bank_seq_ > 0);
    host_gate_used_ = false;
    if (gated && host_start_ && desc_.stream_sync == 4) {
        const auto tg0 = std::chrono::steady_clock::now();
        volatile unsigned long long *w = host_start_;
        while (*w < last_bank_seq_) {
            std::this_thread::yield();
            // (fail-safe: a bank that never starts -- a device fault -- must not hang the caller; the launch then goes ungated)
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - tg0).count() > 2.0) {
                ++gate_timeouts_;                         // (pbso_engine_info::total_gate_timeouts)
                break;
            }
        }
        host_gate_used_ = true;
    } else if (gated && start_gate_) {
        QHIP(hipStreamWaitValue64, sp, sig_start_, last_bank_seq_, hipStreamWaitValueGte, ~0ull);
    }
    L.evq.h_copy = host_ms();
    L.tsub1 = std::chrono::steady_clock::now();
    return PBSO_OK;
}

// stage 5, first kernel: stroke records -> descriptors, events, profile rows: behind the upload (it overwrites the eligible
// objects' default rows in the device copy), in front of everything that reads the plan
int Engine::launch_expand_strokes(Launch &L) {
    if (!L.n_srecs) return PBSO_OK;
    hipStream_t sp = L.sp;
    unsigned char *da = L.da;
    StrokeTables st;
    std::memset(&st, 0, sizeof(st));
    st.recs = L.srec.dev(da);
    st.stamps = L.sstamp.dev(da);
    st.vids = L.svids.dev(da);
    st.coords = L.scoords.dev(da);
    st.vn = L.svn.dev(da);
    st.flags = script_.flags ? L.sflags.dev(da) : nullptr;
    st.buffers_done = buffers_done_;
    st.nb = L.nb;
    st.tile_mask = n_tiles_ >= 32 ? 0xFFFFFFFFu : ((1u << n_tiles_) - 1u);
    st.desc = reinterpret_cast<BufDesc *>(da);
    st.row_ptr = L.row_ptr.dev(da);
    st.slot_idx = L.slot_idx.dev(da);
    st.row_obj = L.row_obj.dev(da);
    st.prow_obj = L.prow_obj.dev(da);
    st.prof_rows = L.prow.dev(da);
    st.prof_entries = L.pent.dev(da);
    st.ar_uses = k2_rows_launch_ ? L.aruse.dev(da) : nullptr;
    st.proj = L.proj.dev(da);
    st.slots = d_slots_.p;
    st.frow_base = L.n_frows - L.n_srows;
    st.prow_base = n_prows_ - L.n_srows;
    st.sidx_base = (int)slot_idx_.size();
    st.entry_base = (int)prof_entries_.size();
    st.prof_row_base = (int)prof_rows_.size();
    st.use_base = (int)ar_uses_.size();
    st.proj_base = (int)proj_.size();
    st.m_pad = m_pad_;
    if (host_profile_ && stroke_ev_[cur_set_][0]) QHIP(hipEventRecord, stroke_ev_[cur_set_][0], sp);
    QLAUNCH(launch_stroke_expand, st, L.n_srecs, sp);
    if (host_profile_ && stroke_ev_[cur_set_][0]) { QHIP(hipEventRecord, stroke_ev_[cur_set_][1], sp); stroke_ev_live_[cur_set_] = true; }
    tot_stroke_launches_ += 1;
    return PBSO_OK;
}

// the bank's arguments (the scan reads them too)
int Engine::launch_bank_params(Launch &L) {
    const int N = L.N, nb = L.nb;
    hipStream_t sk = L.sk;
    L.dense_heavy = dense_heavy(L.scene, L.set, L.pl);
    IirParams &kp = L.kp;
    kp.ca = d_ca_.p; kp.cb = d_cb_.p; kp.sq = d_sq_.p; kp.sd = d_sd_.p; kp.ss = d_ss_.p;
    kp.desc = reinterpret_cast<const BufDesc *>(L.da);
    kp.grows = L.grows->p;
    kp.g32 = d_g32_.p;
    kp.g32_off = d_g32_off_.p;
    kp.tprof = L.d_tprof;
    kp.xfer_rows = d_xfer_.p;
    kp.xfer_init = reinterpret_cast<const int *>(L.da + L.ps->off_xfer_init);
    kp.audio = L.audio + (size_t)L.b0 * B_;
    kp.qnorm = (L.qn || n_dump_ > 0) ? d_qnorm_.p : nullptr;
    kp.xdump = n_dump_ > 0 ? d_xdump_.p : nullptr;
    kp.xscale = d_xscale_.p;
    kp.dump_row = d_dump_row_.p;
    kp.qn_nb = L.nb_total;
    kp.qn_b0 = L.b0;
    kp.gq = d_gq_.p;
    kp.gq_plane = (long long)N * m_pad_;
    kp.census = nullptr;
    if (census_) {
        size_t rows = (size_t)std::max(n_teams_, use_split() ? n_ts_teams_ : 0);
        if (tc_ok_) for (const TcSet &ts : tc_) rows = std::max(rows, (size_t)ts.n_teams * nb);
        GROWTRY(d_census_, rows * CENSUS_WORDS, false, sk);
        kp.census = d_census_.p;
    }
    kp.nb = nb; kp.n_tiles = n_tiles_; kp.m_pad = m_pad_; kp.b_pad = b_pad_;
    kp.audio_stride = (long long)L.nb_total * B_;
    // the per-CU progress feedback only pays when several teams compete for every SIMD
    kp.rotate_prio = (rotate_prio_ == 2 && total_team_waves_ < 12LL * n_cus_) ? 1 : rotate_prio_;
    kp.board = d_board_.p;
    kp.launch_seq = ++launch_seq_;
    kp.start_flag = (host_start_ && desc_.stream_sync == 4) ? host_start_dev_ : (start_gate_ ? sig_start_ : nullptr);
    kp.start_seq = ++bank_seq_;
    kp.pc = d_pc_.p;
    kp.wtab = d_wtab_.p;
    kp.frames = B_;
    kp.ftab = ftab_forced_ ? d_ftab_.p : nullptr;
    kp.forced_block = (forced_block_ && n_prows_ > 0) ? 1 : 0;      // (the build with the forced block path only when a buffer needs it)
    return PBSO_OK;
}

// stage 5: K2 -> time-profile rows ; K3 / scatter -> data slots ; K4 -> transfer rows ; combine -> g rows
// (the fork of launches with many dense-profile rows: launch_policy.h, split_prep)
int Engine::launch_prepare(Launch &L) {
    PlanSet &ps = *L.ps;
    DevBuf<float> &grows = *L.grows;
    unsigned char *da = L.da;
    EvQuad &evq = L.evq;
    hipStream_t sp = L.sp;
    const int n_frows = L.n_frows, n_prof_rows = L.n_prof_rows, n_ar_uses = L.n_ar_uses, n_ffat_sh = L.n_ffat_sh, n_ffat_gen = L.n_ffat_gen;
    const int *d_row_ptr = L.row_ptr.dev(da), *d_slot_idx = L.slot_idx.dev(da), *d_row_obj = L.row_obj.dev(da), *d_chain = L.chain.dev(da);
    const ProfEntry *d_pent = L.pent.dev(da);
    const ProfRow *d_prow = L.prow.dev(da);
    const double *d_stage = L.stage.dev(da);
    const int *d_stage_slot = L.stage_slot.dev(da);
    const ProjectEvent *d_proj = L.proj.dev(da), *d_projd = L.projd.dev(da);
    const FfatEvent *d_ffat = L.ffat.dev(da);
    const ArUse *d_aruse = L.aruse.dev(da);
    const ArStream *d_arstream = L.arstream.dev(da);

    L.split_prep = split_prep(L.set, L.pl, L.one_stream, n_frows > 0 || !proj_.empty() || !ffat_.empty() || !stage_slot_.empty());
    hipStream_t sa = L.sa = L.split_prep ? aux_stream_ : sp;
    if (L.split_prep) {
        tot_prep_splits_ += 1;
        QHIP(hipEventRecord, ev_aux_fork_[cur_set_], sp);         // (behind the upload and, for gated launches, the start gate)
        QHIP(hipStreamWaitEvent, sa, ev_aux_fork_[cur_set_], 0);
    }
    if (device_profiles_ && L.timed && L.n_chains > 0) { QHIP(hipEventRecord, evq.f0, sp); evq.has_k2 = true; }
    // (round 6, second half) a one-buffer launch whose profile rows go through the fused kernel and whose combine takes its rows itself:
    // both in ONE launch -- they touch different arrays (kernels_exact.hip, force_rows_combine_kernel)
    L.rows_and_combine = device_profiles_ && k2_rows_launch_ && L.fuse_combine && sa == sp && !prof_rows_.empty() && n_frows > 0 &&
                         fuse_short_ && !ar_uses_.empty() && ar_uses_.size() == ar_streams_.size();
    if (L.rows_and_combine)
        QLAUNCH(launch_force_rows_combine, d_prow, n_prof_rows, d_pent, d_aruse,
                                            d_arstream, ar_max_segs_, d_arstate_.p, d_ar_snaps_.p,
                                            d_ar_vnorm_.p, d_ar_vstate_.p, d_ar_segcount_.p, d_ar_cbuf_.p, d_ar_recs_.p, d_ar_fins_.p,
                                            ps.d_tprof.p, track_device_pool(), track_device_table(), B_, b_pad_, b_pad_, d_row_ptr, d_slot_idx,
                                            d_row_obj, n_frows, d_slots_.p, d_c3_.p,
                                            grows.p, d_projd, d_shapes_.p, d_shape_off_.p, d_n_modes_.p, m_pad_, (int)proj_direct_.size(),
                                            d_stage, d_stage_slot, sp);
    else if (device_profiles_ && k2_rows_launch_)
        QLAUNCH(launch_force_rows, d_prow, n_prof_rows, d_pent, d_aruse, n_ar_uses,
                                    d_arstream, L.arseg.dev(da),
                                    (int)seg_stream_.size(), ar_max_segs_, d_arstate_.p, d_ar_snaps_.p, d_ar_vnorm_.p, d_ar_vstate_.p,
                                    d_ar_segcount_.p, d_ar_cbuf_.p, d_ar_recs_.p, d_ar_fins_.p, ps.d_tprof.p, track_device_pool(),
                                    track_device_table(), B_, b_pad_, b_pad_,
                                    /* every AR force adds its samples once (a launch of one buffer): one launch instead of three */
                                    fuse_short_ && n_ar_uses > 0 && (size_t)n_ar_uses == ar_streams_.size(), sp);
    else if (device_profiles_)
        QLAUNCH(launch_force_profiles, d_chain, L.n_chains, d_prow, d_pent, d_arstate_.p, ps.d_tprof.p, track_device_pool(), track_device_table(),
                                        B_, b_pad_, ar_serial_ ? 1 : 0, k2_prio_, sp);
    if (evq.has_k2) QHIP(hipEventRecord, evq.f1, sp);
    if (!L.fuse_combine) QLAUNCH(launch_scatter_rows, d_stage, d_stage_slot, (int)stage_slot_.size(), d_slots_.p, m_pad_, sa);
    QLAUNCH(launch_modal_project, d_proj, L.n_proj, d_shapes_.p, d_shape_off_.p, d_n_modes_.p, d_slots_.p, m_pad_, sa);
    // (a few events: one thread per (event, mode); listener paths -- many events per object -- by runs)
    if (n_ffat_sh > 0)
        QLAUNCH(launch_ffat_lookup_shared, d_ffat, n_ffat_sh, d_ffat_shared_.p, d_geom_.p, d_geom_off_.p, d_n_modes_.p, d_ffat_k_.p,
                                            d_ffat_valid_.p, d_psi_t_.p, d_xfer_.p, m_pad_, sa);
    if ((size_t)n_ffat_gen >= 4 * ffat_runs_.size() && !ffat_runs_.empty())
        QLAUNCH(launch_ffat_lookup_runs, d_ffat, L.ffat_runs.dev(da), (int)ffat_runs_.size(), d_geom_.p,
                                          d_geom_off_.p, d_n_modes_.p, d_psi_.p, d_xfer_.p, m_pad_, sa);
    else
        QLAUNCH(launch_ffat_lookup, d_ffat + n_ffat_sh, n_ffat_gen, d_geom_.p, d_geom_off_.p, d_n_modes_.p, d_psi_.p, d_xfer_.p, m_pad_, sa);
    // (the combine stays on the preparation stream even when the bank fills the register file: its workgroups
    //  move in as the bank's retire, so most of it is done when the last one leaves -- queued behind the bank in
    //  the bank's own stream it would start only then: 0.785 instead of 0.735 ms per step at 1024 x 512)
    if (!L.rows_and_combine)
        QLAUNCH(launch_force_combine, d_row_ptr, d_slot_idx, d_row_obj, n_frows, d_slots_.p, d_c3_.p, grows.p, d_projd, d_shapes_.p,
                                       d_shape_off_.p, d_n_modes_.p, m_pad_, (int)proj_direct_.size(), d_stage, d_stage_slot, sa);
    if (L.split_prep) QHIP(hipEventRecord, ev_aux_join_[cur_set_], sa);
    if (L.split_prep && !L.tc_launch) QHIP(hipStreamWaitEvent, sp, ev_aux_join_[cur_set_], 0);
    return PBSO_OK;
}

// stage 6 (time-chunked launches): the scan hands the state from launch to launch by itself (the chunked bank launches never
// write it), so it runs HERE, on the preparation stream, beside the previous launch's oscillator bank -- behind a launch of
// another kind it waits for that launch's bank, which wrote the state it starts from.
int Engine::launch_scan(Launch &L) {
    const int N = L.N, nb = L.nb, tc_cb = L.tc_cb;
    hipStream_t sp = L.sp;
    const int n_chunks = (nb + tc_cb - 1) / tc_cb;
    GROWTRY(d_xs_[cur_set_], (size_t)N * n_chunks * m_pad_ * 2, false, sp);
    GROWTRY(d_xtrow_[cur_set_], (size_t)N * n_chunks, false, sp);
    // dense-profile buffers (Gaussian / AR, forces.h:92-128): what each leaves in the state per unit gain, all of them at once
    const float *vinc = nullptr;
    if (n_prows_ > 0) {
        GROWTRY(d_vinc_[cur_set_], (size_t)n_prows_ * m_pad_ * 2, false, sp);
        QLAUNCH(launch_dense_increments, d_pc_.p, d_ftab_.p, (long long)N * m_pad_, L.d_tprof, L.prow_obj.dev(L.da),
                                          d_n_modes_.p, n_prows_, m_pad_, b_pad_, B_, d_vinc_[cur_set_].p, sp);
        vinc = d_vinc_[cur_set_].p;
        tot_tc_dense_launches_ += 1;
    }
    if (!last_launch_tc_ && last_set_ >= 0) QHIP(hipStreamWaitEvent, sp, ev_k1_done_[last_set_], 0);
    if (L.split_prep) QHIP(hipStreamWaitEvent, sp, ev_aux_join_[cur_set_], 0);      // (the increments above did not need the gains; the scan does)
    const bool seg = segmented_scan(L.scene, L.set, tc_cb, n_chunks, vinc != nullptr);
    if (seg) tot_seg_scans_ += 1;
    QLAUNCH(launch_iir_scan, L.kp, N, d_scan_.p, tc_cb, n_chunks, d_xs_[cur_set_].p, d_xtrow_[cur_set_].p, direct_hits_, vinc, seg, sp);
    return PBSO_OK;
}

// stage 7: the bank after its preparation (and, stream order, after the previous bank)
int Engine::launch_hand_over(Launch &L) {
    hipStream_t sk = L.sk, sp = L.sp;
    if (L.one_stream) {
        tot_one_stream_launches_ += 1;
    } else if (value_handover(L.set, L.pl)) {
        QLAUNCH(launch_signal_value, sig_prep_, ++prep_seq_, sp);
        QHIP(hipStreamWaitValue64, sk, sig_prep_, prep_seq_, hipStreamWaitValueGte, ~0ull);
    } else {
        QHIP(hipEventRecord, ev_prep_done_[cur_set_], sp);
        QHIP(hipStreamWaitEvent, sk, ev_prep_done_[cur_set_], 0);
    }
    L.tsub2 = std::chrono::steady_clock::now();
    if (L.timed) QHIP(hipEventRecord, L.evq.k0, sk);
    L.evq.h_bank = host_ms();
    return PBSO_OK;
}

// stage 8: the oscillator bank in its kind (launch_policy.h, bank_kind), then the partial sums and the re-parked rows
int Engine::launch_bank(Launch &L) {
    const int N = L.N, nb = L.nb, tc_cb = L.tc_cb, n_cl = L.n_cl, n_cq = L.n_cq;
    const bool tc_launch = L.tc_launch, dense_heavy = L.dense_heavy;
    hipStream_t sk = L.sk;
    IirParams &kp = L.kp;
    kp.audio_parts = d_audio_parts_.p ? d_audio_parts_.p + (size_t)L.b0 * B_ : nullptr;
    const BankKind kind = bank_kind(L.scene, L.set, L.pl, tc_launch);
    const bool split_launch = L.split_launch = kind == BankKind::Pipeline;
    (kind == BankKind::Sample ? tot_sample_launches_ : tot_block_launches_) += 1;
    if (split_launch) tot_split_launches_ += 1;
    if (tc_launch) {
        tot_tc_launches_ += 1;
        last_tc_shape_ = tc_[L.tc_set].R;
        last_tc_cb_ = tc_cb;
        last_tc_teams_ = tc_[L.tc_set].n_teams;
    }
    if (n_dump_ > 0) {
        // the mix needs block states: a launch on the per-sample kernel leaves none, a dense-profile buffer neither
        for (int i = 0; i < N; ++i) {
            if (dump_row_[i] < 0) continue;
            if (!tc_launch && (dense_heavy || !is_block())) { dump_valid_[i] = 0; continue; }
            for (int b = 0; b < nb; ++b)
                if (!(plan_desc_[(size_t)i * nb + b].flags & DESC_DIRECT) && plan_desc_[(size_t)i * nb + b].prow >= 0) { dump_valid_[i] = 0; break; }
        }
    }
    bool used[N_CLASS_STREAMS] = {false, false, false};
    if (tc_launch) {
        TcSet &ts = tc_[L.tc_set];
        kp.tc_cb = tc_cb;
        kp.tc_xs = d_xs_[cur_set_].p;
        kp.tc_xtrow = d_xtrow_[cur_set_].p;
        kp.census_stride = ts.n_teams;
        // The priority rotation (kernels_block.hip) assumes the teams of a CU walk their buffers in step.  A launch of several
        // ROUNDS of workgroups does not: a team that arrives when another retires starts at its own chunk's first buffer, two
        // teams of a CU then hold the same priority and the oldest-first arbitration is back -- 1024 x 512 forced into two
        // chunks: 1.33 ms against 1.07 without the rotation; 700 x 512: 0.751 against 0.742 (scripts/debug/r04_tcrounds.py).
        // (A phase taken from the wall clock instead of the team's buffer count does not help: 0.752 ms at 700 x 512.)
        kp.rotate_prio = (rotate_prio_ && ts.waves * (long long)((nb + tc_cb - 1) / tc_cb) <= 8LL * n_cus_) ? 1 : 0;
        for (const SizeClass &c : ts.classes) {
            kp.teams = ts.d_teams.p + c.first;
            QLAUNCH(iir_block::launch_iir_block, kp, c.count, ts.R, c.W, desc_.qnorm_mode, form_ == PBSO_FORM_BLOCK_BF16 ? 1 : 0, sk);
        }
    }
    if (split_launch) {
        kp.teams = d_ts_teams_.p;
        const int nc = pipe_consumer_waves(L.scene, L.set, L.pl);
        QLAUNCH(iir_pipe::launch_iir_pipe, kp, n_ts_teams_, nc, desc_.qnorm_mode, sk);
    }
    // Side by side only while everything is resident at once (largest teams first, on the engine's
    // stream); an engine that needs several rounds of workgroups runs its classes one after the other
    // (512 x 512 + 4096 x 64: 3.1 ms in sequence, 3.7 ms side by side -- teams of different size fragment
    // the CUs' LDS and wave slots).
    const bool fork = !tc_launch && !split_launch && classes_.size() > 1 && ev_fork_ && total_team_waves_ <= 16LL * n_cus_;
    if (fork) QHIP(hipEventRecord, ev_fork_, sk);
    for (size_t ci = 0; ci < (tc_launch || split_launch ? 0 : classes_.size()); ++ci) {
        const SizeClass &c = classes_[ci];
        hipStream_t s = sk;
        if (fork && ci > 0) {
            const int j = (int)((ci - 1) % N_CLASS_STREAMS);
            s = class_stream_[j];
            if (!used[j]) {
                QHIP(hipStreamWaitEvent, s, ev_fork_, 0);
                used[j] = true;
            }
        }
        kp.teams = d_teams_.p + c.first;
        if (kind == BankKind::Block)
            QLAUNCH(iir_block::launch_iir_block, kp, c.count, R_, c.W, desc_.qnorm_mode, form_ == PBSO_FORM_BLOCK_BF16 ? 1 : 0, s);
        else
            QLAUNCH(iir_scalar::launch_iir_bank, kp, c.count, R_, c.W, form_ == PBSO_FORM_DIRECT ? 1 : 0, desc_.qnorm_mode, s);
    }
    for (int j = 0; j < N_CLASS_STREAMS; ++j) {
        if (!used[j]) continue;
        QHIP(hipEventRecord, ev_join_[j], class_stream_[j]);
        QHIP(hipStreamWaitEvent, sk, ev_join_[j], 0);
    }
    // objects stepped by several teams: the teams' partial sums of this launch's buffers, added in team order
    // ... and _latest_transfer = trans (modal_solver.h:251) in the same launch; then re-park a still-queued transfer
    const int *d_copy = L.copy.dev(L.da);
    QLAUNCH(launch_sum_parts_copy_rows, tc_launch ? tc_[L.tc_set].d_split.p : split_launch ? d_ts_split_.p : d_split_.p,
                                         tc_launch ? tc_[L.tc_set].n_split : split_launch ? n_ts_split_ : n_split_, kp.audio_parts,
                                         L.audio + (size_t)L.b0 * B_, (long long)L.nb_total * B_, (long long)nb * B_, d_copy, d_copy + (n_cl + n_cq), n_cl,
                                         d_xfer_.p, m_pad_, sk);
    if (L.timed) QHIP(hipEventRecord, L.evq.k1, sk);
    QLAUNCH(launch_copy_rows, d_copy + n_cl, d_copy + (n_cl + n_cq) + n_cl, n_cq, d_xfer_.p, m_pad_, sk);
    if (L.timed) QHIP(hipEventRecord, L.evq.p1, sk);
    L.evq.h_done = host_ms();
    QHIP(hipEventRecord, ev_k1_done_[cur_set_], sk);
    return PBSO_OK;
}

// stage 9: the recorded calls go to the worker; what the next launch needs to know about this one; the host's times
int Engine::launch_finish(Launch &L) {
    if (L.defer) {
        L.evq.batch = submit_->pushed() + 1;
        set_batch_[cur_set_] = submit_->push(std::move(L.ops));     // (from here on the worker makes the calls; the caller goes on to plan)
    }
    if (L.timed) ev_pending_.push_back(L.evq);
    else ev_free_.push_back(L.evq);
    buffers_done_ += L.nb;
    last_launch_tc_ = L.tc_launch;
    last_one_stream_ = L.one_stream;
    last_bank_seq_ = L.kp.start_seq;
    last_set_ = cur_set_;
    cur_set_ = (cur_set_ + 1) % N_SETS;
    hprof_[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - L.t0).count() - last_plan_ms_;
    hprof_[6] += std::chrono::duration<double, std::milli>(L.tsub1 - L.tsub0).count();
    hprof_[7] += std::chrono::duration<double, std::milli>(L.tsub2 - L.tsub1).count();
    hprof_[8] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - L.tsub2).count();
    hprof_[5] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - L.tw0).count();
    return PBSO_OK;
}

// the second submitting thread has made every recorded call (NOT a device synchronisation); a call that failed there surfaces here
int Engine::drain_submit() {
    if (!submit_) return PBSO_OK;
    submit_->drain();
    std::string why;
    if (submit_->error(&why)) {
        failed_ = true;
        failed_why_ = why;
        return fail(PBSO_ERR_HIP, "a launch failed on the submitting thread: " + why);
    }
    return PBSO_OK;
}

// Host delivery (the reference's consumer is a host queue of SoundMessages, modal_solver.h:79-82, 346-363): a step whose audio
// of ALL objects lands in caller memory.  Pinned host memory (pbso_host_alloc, hipHostMalloc, hipHostRegister) is mapped into
// the device's address space: the oscillator bank writes its samples STRAIGHT into it over PCIe -- every sample is stored
// exactly once, coalesced -- so delivery needs no second pass and the step runs at the link's rate (1024 x 512 x 86: 3.5 ms per
// step against 3.2 ms for the bare copy of the same 181 MB; scripts/debug/r04_d2h.py).  What was tried first -- the bank into
// device memory, then hipMemcpyAsync on a copy stream beside the next step's bank -- does NOT overlap on this stack: the runtime
// runs the device-to-host copy as a blit KERNEL, which finds no free registers while the bank's two 256-register waves per SIMD
// are resident (4.35 ms per step waited one by one, 4.65 ms "pipelined").  That staged path remains for pageable memory.
int Engine::step_to_host(int nb, float *host_out, size_t n) {
    HIPTRY(hipSetDevice(desc_.device));
    if (!finalized_) return fail(PBSO_ERR_STATE, "step before finalize");
    const size_t total = (size_t)objs_.size() * (size_t)std::max(nb, 0) * B_;
    if (!host_out || nb <= 0 || n != total) return fail(PBSO_ERR_INVALID, "step_to_host arguments (n_floats = n_objects * n_buffers * frames_per_buffer)");
    if (!copy_stream_) {
        {
            // (highest priority: should the runtime run the copy as a blit kernel, its workgroups take the CUs the retiring
            //  bank frees before the next bank's do)
            int least = 0, greatest = 0;
            HIPTRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPTRY(hipStreamCreateWithPriority(&copy_stream_, hipStreamNonBlocking, greatest));
        }
        for (int i = 0; i < 2; ++i) {
            HIPTRY(hipEventCreateWithFlags(&ev_host_bank_[i], hipEventDisableTiming));
            HIPTRY(hipEventCreateWithFlags(&ev_host_copy_[i], hipEventDisableTiming));
        }
    }
    const int slot = host_slot_;
    {
        hipPointerAttribute_t attr;
        std::memset(&attr, 0, sizeof(attr));
        if (hipPointerGetAttributes(&attr, host_out) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer) {
            int rc = step(nb, attr.devicePointer);
            if (rc != PBSO_OK) return rc;
            host_step_ = tot_steps_;
            if ((rc = drain_submit()) != PBSO_OK) return rc;          // (the event below goes behind the step's launches)
            HIPTRY(hipEventRecord(ev_host_copy_[slot], stream_));      // "delivered" = the bank (and what follows it) has finished
            host_last_ = slot;
            host_slot_ ^= 1;
            return PBSO_OK;
        }
        (void)hipGetLastError();                         // (a pageable pointer is not an error here)
    }
    HIPTRY(d_audio_host_[slot].ensure(total, false, stream_));
    HIPTRY(hipStreamWaitEvent(stream_, ev_host_copy_[slot], 0));          // the copy that last read this buffer is done
    int rc = step(nb, d_audio_host_[slot].p);
    if (rc != PBSO_OK) return rc;
    host_step_ = tot_steps_;
    if ((rc = drain_submit()) != PBSO_OK) return rc;
    HIPTRY(hipEventRecord(ev_host_bank_[slot], stream_));
    HIPTRY(hipStreamWaitEvent(copy_stream_, ev_host_bank_[slot], 0));
    HIPTRY(hipMemcpyAsync(host_out, d_audio_host_[slot].p, total * sizeof(float), hipMemcpyDeviceToHost, copy_stream_));
    HIPTRY(hipEventRecord(ev_host_copy_[slot], copy_stream_));
    host_last_ = slot;
    host_slot_ ^= 1;
    return PBSO_OK;
}

}  // namespace pbso
