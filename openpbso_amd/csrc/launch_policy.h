// The decisions Engine::step_chunk takes per launch, as functions of plain numbers: which kernel takes the bank, whether the
// launch is cut along the time axis and how, whether its preparation forks, how it is gated and handed over.  Host only, no
// HIP in here: the engine calls them directly, and tests/cpp/engine_tables_check.cpp calls them without a GPU.
#pragma once
#include <algorithm>
#include <cmath>

namespace pbso {

constexpr int POLICY_SCAN_SEG_MAX = 8;                   // == SCAN_SEG_MAX (kernels.h; asserted in engine_launch.cpp)

struct PolicyShape { long long waves, cover; int waves_per_cu; };      // one team shape of the time-chunked launches (TcSet)
struct PolicyScene {
    long long n_obj;
    int m_pad, n_cus;
    PolicyShape shape[3];                                // R = 1, 2, 4
    int pipe_teams;                                      // teams of the pipeline kernel's table
};
// the engine's settings that matter (descriptor and what finalize made of it)
struct PolicySettings {
    bool block;                                          // the block form runs
    bool tc_ok, have_scan, have_ftab, ftab_forced;       // K5 can run; the scan table / the F table exist; the bank's forced block path may use F
    bool listeners;                                      // objects keep their block-start states for a listener mix
    bool use_split, split_always;                        // the pipeline kernel can run / takes every launch it can
    bool dense_to_k1;                                    // dense-heavy launches run on the per-sample kernel K1
    bool qnorm_off;
    bool device_profiles, have_aux_stream, sync_values;
    int tc_mode, tc_shape;                               // pbso_engine_desc::time_chunks, time_chunk_shape
    int scan_kernel, stream_sync, pipe_consumers, prep_split;
};
struct PolicyLaunch {
    int nb, n_dense_rows;
    bool k2_rows;                                        // the profiles come from K2's row-parallel form
};

inline bool dense_majority(const PolicyScene &sc, const PolicyLaunch &l) { return (long long)l.n_dense_rows * 2 > sc.n_obj * l.nb; }
// Block form: a launch in which most (object, buffer) pairs carry a dense force profile -- sustained
// scraping, forces.h:107-128 -- has nothing for the matrix pipe to do (every sample is forced) and runs on the
// per-sample kernel K1, whose inner loop is built for exactly that; state layout, teams and scaled-state
// rules are shared, so the two kernels hand over at any launch boundary.  (Audio then is bit-identical
// across different cuts of a step only while both cuts pick the same kernel; always within tolerance.)
// PBSO_DENSE_LAUNCHES=block keeps every launch on the block kernel (bit-identical audio for any cut of a step).
inline bool dense_heavy(const PolicyScene &sc, const PolicySettings &s, const PolicyLaunch &l) {
    return s.block && s.dense_to_k1 && dense_majority(sc, l);
}

// K5: does this launch run time-chunked, with which team shape and how many buffers per chunk?  Auto: only while the scene
// leaves SIMDs idle (fewer than two waves per SIMD in its largest shape) and few of the launch's (object, buffer) pairs
// carry a dense force profile (the scan steps those per sample, serially per object).  The shape: the most modes per lane
// that still fills the chip when every buffer is its own chunk (a wave of four modes per lane amortises its operand table
// over more work), unless the padding to whole waves wastes columns; the chunk length minimises rounds x (length + start-up).
inline bool choose_time_chunks(const PolicyScene &sc, const PolicySettings &s, const PolicyLaunch &l, int *set, int *cb) {
    const int nb = l.nb, n_dense_rows = l.n_dense_rows, tc_mode_ = s.tc_mode;
    const PolicyShape *tc_ = sc.shape;
    if (!s.tc_ok || !s.have_scan || (nb < 2 && tc_mode_ <= 0)) return false;
    if (s.listeners) return false;                       // (objects that keep their block-start states for a listener mix: the walk in buffer order, as K1p)
    const long long N = sc.n_obj;
    // Dense-profile buffers (Gaussian / AR, sustained contact: forces.h:92-128, modal_solver.h:222-240) take their place in the scan
    // through their increments (dense_increment_kernel); the bank steps them in its forced block path.
    if (n_dense_rows > 0 && !s.have_ftab) return false;
    // (engines whose bank steps dense buffers per sample -- the split-bf16 projection, forced_block < 0 -- keep their launches with
    //  many of them on the kernels that walk the buffers in order, as before round 5)
    if (tc_mode_ == 0 && !s.ftab_forced && (long long)n_dense_rows * 8 > N * nb) return false;
    // (every dense row costs m_pad x 8 bytes of increments per plan set: a launch whose rows would take more than 1 GiB walks its
    //  buffers in order instead -- 1024 x 512 sustained scraping in ten-second steps is 880 640 rows = 3.6 GB)
    if ((long long)n_dense_rows * sc.m_pad * 8 > (1LL << 30)) return false;
    const bool dense_majority = (long long)n_dense_rows * 2 > N * nb;
    // (a scene small enough for the pipeline kernel keeps its mostly-dense launches WITHOUT qnorm rows there: teams of five waves per
    //  64 modes walk the buffers in order and evaluate every increment once -- cut in time they are evaluated twice, for the scan and
    //  in the bank: 8 x 4096 x 86 scraping 0.25 ms per step against 0.27.  With qnorm rows the re-stepped samples are the long stage
    //  and want the whole chip's vector ALUs at three waves per SIMD: cut in time 0.33 ms, five-wave teams 0.49, three-wave teams 0.45)
    if (dense_majority && tc_mode_ == 0 && s.use_split && s.ftab_forced && l.k2_rows && s.qnorm_off) return false;
    int k = 0;
    for (int c = 2; c >= 1; --c)
        if (tc_[c].cover * 100 <= tc_[0].cover * 115 && tc_[c].waves * nb >= (long long)tc_[c].waves_per_cu * sc.n_cus) { k = c; break; }
    // a launch of mostly dense buffers: ONE mode per lane -- the only shape whose registers hold the increment table F next to the
    // operand table W, so that the state moves a block at a time (F . T_n on the matrix pipe) instead of a sample at a time, and
    // whose per-sample chain for the qnorm rows has three waves per SIMD to hide behind
    if (dense_majority && s.ftab_forced) k = 0;
    if (s.tc_shape == 1 || s.tc_shape == 2 || s.tc_shape == 4) k = s.tc_shape == 4 ? 2 : s.tc_shape - 1;
    const long long capacity = (long long)tc_[k].waves_per_cu * sc.n_cus;
    const long long waves = tc_[k].waves;
    int best = nb;
    if (tc_mode_ > 0) {
        best = std::min(tc_mode_, nb);
    } else {
        // cost of a launch in buffer times: rounds of workgroups x (chunk length + 0.3 for a workgroup's start-up: operand table,
        // coefficients, state).  A scene LARGER than the chip, whose walk is a launch of several rounds of full-length
        // workgroups, does not pack perfectly -- a CU may be handed a ninth workgroup while another gets seven
        // (scripts/census.py 2048: a third, nearly empty round; 1100 / 1536 / 2048 x 512 walk 1.68 / 2.04 / 2.72 ms: half a round
        // more than their 1.07 / 1.5 / 2 rounds) -- and the shorter the workgroups, the cheaper that tail: such scenes are cut in
        // time too (1.22 / 1.66 / 2.21 ms).  A scene that fills the chip exactly (1024 x 512: one round) is not.
        const bool over_full = waves > capacity;
        // (round 6, ADVICE r05: a mostly-dense scene that fills the chip anyway gains nothing from the cut -- its increments are
        //  evaluated twice, for the scan and in the bank: 1024 x 512 sustained scraping 7.90 ms per second of audio cut in time against
        //  7.37 for the walk, profiles/r06_bench_c4scr_*.json -- so the cut is for dense scenes that leave wave slots free)
        if (dense_majority && waves >= capacity) return false;
        if (over_full && !dense_majority) {
            // measured, in rounds of the exactly-full chip (scripts/debug/r04_tcrounds.py): the walk of 1100 / 1536 / 2048 / 3000
            // objects x 512 modes takes 1.57 / 1.90 / 2.54 / 3.07 -- whole rounds + a last, partly filled one that runs faster the
            // emptier it is (0.57 + 0.54 x its fill), or half a round of stragglers when the rounds are exactly full -- and the
            // same scenes cut in time 1.07 x their share of the chip (1.14 / 1.57 / 2.12 / 3.17): at 3000 the walk wins
            const double frac = (double)waves / (double)capacity, whole = std::floor(frac), fill = frac - whole;
            const double walk = whole + (fill > 1e-9 ? 0.57 + 0.54 * fill : 0.5);
            if (frac * 1.07 >= walk) return false;
        }
        double best_cost = 0;
        for (int c = nb; c >= 1; --c) {
            const long long chunks = (nb + c - 1) / c;
            const long long rounds = (waves * chunks + capacity - 1) / capacity;
            const double cost = ((double)rounds + (over_full ? 0.5 : 0.0)) * (c + 0.3);
            if (c == nb || cost < best_cost - 1e-9) { best = c; best_cost = cost; }
        }
    }
    if ((nb + best - 1) / best < 2 && tc_mode_ <= 0) return false;       // (forced: every launch, so that any cut of a step runs the same arithmetic)
    *set = k;
    *cb = best;
    return true;
}

// The scan cut along the time axis itself -- one wave per chunk (kernels_scan.hip, SEG) -- in three cases.  (a) The whole scan is a
// handful of waves: it halves the latency of a scan that has the device to itself (1 x 512 x 86: 11.3 -> 5.7 us).  (b) LONG
// chunks of a scene whose serial scan is at most two waves per SIMD: that scan can only start as the previous bank's
// workgroups retire (the bank holds every register), so the waves placed last start when the bank ends and what the next
// bank waits for is ONE WAVE'S walk over all buffers of the launch -- 82 us for 860 buffers; cut into the bank's own
// chunks a wave walks 108 and the whole scan is 45 us of a throughput-bound kernel, most of it beside the bank's tail:
// 128 x 512 x 860 1.31 -> 1.27 ms per step, 256 x 512 x 860 2.45 -> 2.42 (scripts/debug/r05_scan_seg2.sh).  NOT for
// four serial waves per SIMD (512 x 512: the serial scan is throughput-bound already and does less work: 4.79 against
// 4.87 ms) and not for short chunks (86-buffer steps, 11 buffers per chunk: 0.156 against 0.160 ms -- eight times the
// waves for one batch each).  (c) A DENSE scan (every buffer a hit with a row of increments: 64 hits per serial batch,
// sixteen in flight) of at most two waves per CU: 8 x 4096 x 86 sustained scraping with qnorm rows 0.320 -> 0.312 ms per
// step (scripts/debug/r05_seg_short.sh).  One buffer per chunk keeps the serial scan, whose arithmetic does not depend
// on where a step is cut.
inline bool segmented_scan(const PolicyScene &sc, const PolicySettings &s, int tc_cb, int n_chunks, bool have_increments) {
    const bool seg_fits = n_chunks >= 2 && n_chunks <= POLICY_SCAN_SEG_MAX;
    const long long scan_waves = sc.n_obj * (sc.m_pad / 64);
    return seg_fits && s.scan_kernel != 1 &&
           (s.scan_kernel == 2 || (tc_cb > 1 && scan_waves * n_chunks <= 2LL * sc.n_cus) || (tc_cb >= 32 && scan_waves <= 8LL * sc.n_cus) ||
            (tc_cb > 1 && have_increments && scan_waves <= 2LL * sc.n_cus));
}

// The pipeline kernel of under-filled engines (K1p) takes the launch -- also one whose (object, buffer)
// pairs mostly carry a dense force profile (sustained scraping) when the profiles come from K2's row-parallel form
// (8 x 4096 x 86: 0.30 ms against K1b's 0.43 without qnorm rows, 0.48 against 0.74 with).  Beside K2's CHAIN form -- then
// the step's critical chain, which a wave on every SIMD slows 2.7 x (1.28 ms against 0.48 for 8 chains of 86 rows beside
// K1b's 512 waves) -- K1b's forced block path keeps those launches (state and teams hand over at any launch boundary).
// Without the F table of the forced block path (PBSO_FORCED_BLOCK=0) and without qnorm rows they go to K1b as well.
inline bool split_launch(const PolicyScene &sc, const PolicySettings &s, const PolicyLaunch &l, bool tc_launch) {
    const bool split_dense_ok = l.k2_rows && (!s.qnorm_off || s.ftab_forced);
    return !tc_launch && s.use_split && (s.split_always || !dense_majority(sc, l) || split_dense_ok);      // (PBSO_SPLIT=2: always)
}
// which bank kernel takes the launch
enum class BankKind { TimeChunked, Pipeline, Block, Sample };
inline BankKind bank_kind(const PolicyScene &sc, const PolicySettings &s, const PolicyLaunch &l, bool tc_launch) {
    if (tc_launch) return BankKind::TimeChunked;
    if (split_launch(sc, s, l, tc_launch)) return BankKind::Pipeline;
    return s.block && !dense_heavy(sc, s, l) ? BankKind::Block : BankKind::Sample;
}
// consumer waves of a pipeline team
inline int pipe_consumer_waves(const PolicyScene &sc, const PolicySettings &s, const PolicyLaunch &l) {
    const bool dm = dense_majority(sc, l);
    // two consumers (one group each) also where that puts a second wave on some SIMDs: 8 x 4096 scraping -- 512 teams, 1536
    // waves -- runs 3120 x against 2800 with one consumer (no qnorm rows) and 1700 x against 1590 (with them)
    int nc = 2;
    // qnorm rows of a mostly-dense launch: the consumers re-step every sample for the sums and are the long stage -- a third
    // consumer wave that only steps (half of the chains) when that still leaves at most two waves per SIMD
    if (dm && !s.qnorm_off && s.ftab_forced && 4LL * sc.pipe_teams <= 8LL * sc.n_cus) nc = 3;
    // round 5: a mostly-dense launch as teams of FIVE -- the block increments F . T_n come from two waves of their own, a buffer
    // ahead of the producer, which is left with the 32 coarse steps (kernels_pipe.hip, iir_pipe5_kernel)
    if (dm && s.ftab_forced && s.qnorm_off) nc = 4;
    if (s.pipe_consumers > 0) nc = s.pipe_consumers;
    return nc;
}

// Round 5: a launch with many dense-profile rows FORKS its preparation.  The force profiles (variates -> zero-state chains ->
// rows) and the dense increments that need them are one dependent chain, projection -> combine another, and nothing connects
// the two before the scan; in one stream they ran one after the other BESIDE the previous bank -- 8 x 4096 x 86 sustained
// scraping with qnorm rows: 31 + 54 + 73 (profiles) + 29 + 15 (project, combine) + 78 (increments) = 280 us beside a bank of
// 283, then the scan: the preparation, not the bank, set the step (scripts/debug/r05_timeline_c5.sh).  Forked, projection +
// FFAT + combine run on the second preparation stream behind the upload and join the preparation stream in front of the scan
// (or of the hand-over to the bank): every later reader is ordered behind the preparation stream as before.
inline bool split_prep(const PolicySettings &s, const PolicyLaunch &l, bool one_stream, bool anything_to_fork) {
    return !one_stream && s.have_aux_stream && s.prep_split > 0 && s.device_profiles && l.n_dense_rows > 0 &&
           (s.prep_split == 2 || l.n_dense_rows >= 64) && anything_to_fork;
}
// The start gate, by policy for LONG launches only (stream_sync = 3 / 4: every launch); see Engine::launch_upload_and_gate (engine_launch.cpp)
inline bool gate_now(const PolicySettings &s, const PolicyLaunch &l, bool one_stream, bool bank_before) {
    return !one_stream && bank_before && (s.stream_sync == 3 || s.stream_sync == 4 || l.nb >= 256);
}
// the hand-over preparation -> bank through a value in signal memory instead of an event
// (round 6: by policy for launches of fewer than 256 buffers -- a step of 86 buffers: 64 x 256 with a listener move per buffer
//  0.0765 -> 0.0717 ms, 16 / 128 / 256 / 512 x 512 impulses 4 / 2.7 / 1.7 / 1.5 % per step, 64 x 512 and 1 x 512 unchanged,
//  profiles/r06_value_handover.txt; long launches keep the event: nothing to gain there, and their numbers stand as measured)
inline bool value_handover(const PolicySettings &s, const PolicyLaunch &l) { return s.sync_values && (s.stream_sync == 2 || l.nb < 256); }

}  // namespace pbso
