// Engine::finalize and what leads up to it: objects, FFAT maps, the tables of engine_tables.h uploaded, streams.  See engine.h.
#include "engine.h"
#include "submit_queue.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace pbso {

// ModalIntegrator<double>::Build + ctor, modal_integrator.h:63-99: the one copy, for add_object and for pbso_set_material (retune.cpp)
void integrator_coefs(double omega_squared, double density, double alpha, double beta, double h, double &c1, double &c2, double &c3_out) {
    const double omega0 = std::sqrt(omega_squared / density);                 // :63
    const double xi = 0.5 * (alpha / omega0 + beta * omega0);                 // :64
    const double a = 2.0 * xi * omega0;                                       // :65
    const double b = std::pow(omega0, 2);                                     // :66
    const double epsilon = std::exp(-a / 2 * h);                              // :89
    const double theta = h * std::sqrt(b - a * a / 4.0);                      // :90
    const double gamma = std::asin(a / (2.0 * std::sqrt(b)));                 // :91
    const double omega = std::sqrt(b);                                        // :92
    const double omega_d = std::sqrt(b - std::pow(a, 2) / 4.0);               // :93
    c1 = 2.0 * epsilon * std::cos(theta);                                     // :95
    c2 = -std::pow(epsilon, 2);                                               // :96
    double c3 = 2.0 * (epsilon * std::cos(theta + gamma)
                       - std::pow(epsilon, 2) * std::cos(2.0 * theta + gamma));  // :97
    c3 /= (3.0 * omega * omega_d);                                            // :98
    c3 *= 1E9;                                                                // :99
    c3_out = c3;
}

// BuildSolver -> ModalIntegrator<double>::Build + ctor, modal_integrator.h:47-101
int Engine::add_object(const pbso_object_desc &d, int *id) {
    if (finalized_) return fail(PBSO_ERR_STATE, "add_object after finalize");
    if (d.n_modes < 0 || d.n_omega < d.n_modes || (d.n_modes > 0 && !d.omega_squared))
        return fail(PBSO_ERR_INVALID, "N for modal integrator invalid");         // assert :56
    Object o;
    o.n_modes = d.n_modes;
    o.c1.resize(d.n_modes);
    o.c2.resize(d.n_modes);
    o.c3.resize(d.n_modes);
    o.omega_squared.assign(d.omega_squared, d.omega_squared + d.n_modes);
    o.material = pbso_material{d.density, d.alpha, d.beta};
    const double h = 1.0 / (double)rate_;
    for (int ii = 0; ii < d.n_modes; ++ii) integrator_coefs(d.omega_squared[ii], d.density, d.alpha, d.beta, h, o.c1[ii], o.c2[ii], o.c3[ii]);
    if (d.mode_shapes && d.n_dof > 0) {
        o.n_dof = d.n_dof;
        o.shapes.assign(d.mode_shapes, d.mode_shapes + (size_t)d.n_modes * d.n_dof);
    }
    objs_.push_back(std::move(o));
    if (id) *id = (int)objs_.size() - 1;
    return PBSO_OK;
}

// ModalSolver::readFFATMaps, modal_solver.h:278-284 (std::map keyed by modeId)
int Engine::set_ffat_maps(int obj, const pbso_ffat_map *maps, int n) {
    if (finalized_) return fail(PBSO_ERR_STATE, "set_ffat_maps after finalize");
    if (!valid_obj(obj) || n < 0 || (n > 0 && !maps)) return fail(PBSO_ERR_INVALID, "set_ffat_maps arguments");
    Object &o = objs_[obj];
    o.have_maps = true;               // LoadAll returns a non-null (possibly empty) map, SURVEY Q12
    o.geom.clear();
    o.psi.clear();
    o.n_maps = 0;
    for (int i = 0; i < n; ++i) {
        const pbso_ffat_map &m = maps[i];
        if (m.mode_id < 0) return fail(PBSO_ERR_INVALID, "negative modeId");
        if ((int)o.geom.size() <= m.mode_id) {
            FfatGeom z;
            std::memset(&z, 0, sizeof(z));
            o.geom.resize(m.mode_id + 1, z);
        }
        FfatGeom &g = o.geom[m.mode_id];
        if (!g.valid) o.n_maps++;
        // every index GetMapVal can form must be inside psi
        for (int f = 0; f < 6; ++f) {
            if (m.n_elements[f][0] < 1 || m.n_elements[f][1] < 1 || m.strides[f] < 0 ||
                (long long)m.strides[f] + (long long)m.n_elements[f][0] * m.n_elements[f][1] > m.n_psi)
                return fail(PBSO_ERR_INVALID, "FFAT map strides/n_elements exceed psi");
        }
        g.k = m.k;
        g.cell_size = m.cell_size;
        for (int j = 0; j < 3; ++j) {
            g.center3[j] = m.center3[j];
            g.center[j] = m.center[j];
            g.bbox_low[j] = m.bbox_low[j];
            g.bbox_top[j] = m.bbox_top[j];
        }
        for (int f = 0; f < 6; ++f) {
            for (int j = 0; j < 3; ++j) g.low_corners[f][j] = m.low_corners[f][j];
            g.n_elements[f][0] = m.n_elements[f][0];
            g.n_elements[f][1] = m.n_elements[f][1];
            g.strides[f] = m.strides[f];
        }
        g.n_psi = m.n_psi;
        g.valid = 1;
        g.psi_off = (long long)o.psi.size();       // a replaced map leaves its old psi unused
        o.psi.insert(o.psi.end(), m.psi, m.psi + m.n_psi);
    }
    return PBSO_OK;
}

static std::vector<int> modes_of(const std::vector<Object> &objs) {
    std::vector<int> n(objs.size());
    for (size_t i = 0; i < objs.size(); ++i) n[i] = objs[i].n_modes;
    return n;
}
static std::vector<ModeCoefs> coefs_of(const std::vector<Object> &objs) {
    std::vector<ModeCoefs> c(objs.size());
    for (size_t i = 0; i < objs.size(); ++i) c[i] = ModeCoefs{objs[i].c1.data(), objs[i].c2.data(), objs[i].c3.data(), objs[i].n_modes};
    return c;
}

// Closed-form qnorm matrices (engine_tables.h, build_gq_table).  Built by finalize() for the engines that report qnorm rows in
// closed form, and by listeners_enable() for a block engine created with PBSO_QNORM_OFF (the build of the bank that keeps
// block-start states always evaluates the rows).
int Engine::build_gq() {
    if (d_gq_.p) return PBSO_OK;
    const size_t nm = (size_t)objs_.size() * m_pad_;
    const std::vector<float> gq = build_gq_table(coefs_of(objs_), m_pad_, B_);
    HIPTRY(d_gq_.ensure(3 * nm));
    HIPTRY(hipMemcpy(d_gq_.p, gq.data(), 3 * nm * sizeof(float), hipMemcpyHostToDevice));
    return PBSO_OK;
}

int Engine::finalize() {
    HIPTRY(hipSetDevice(desc_.device));      // the caller's thread may have another device current
    if (finalized_) return fail(PBSO_ERR_STATE, "finalize called twice");
    if (objs_.empty()) return fail(PBSO_ERR_STATE, "no objects");
    const int N = (int)objs_.size();
    const std::vector<int> n_modes = modes_of(objs_);
    {
        // The second preparation stream (round 5, step_chunk's fork), for engines large enough for the fork to matter.  Created
        // HERE, not with the engine and not at the first fork: every stream a process owns shifts which hardware queue the next
        // one lands on -- created with every engine it doubled the cross-stream hand-over of one-buffer steps of small engines
        // (58 -> 112 us, scripts/latency.py, latency_path = -1: any third stream does, whatever its priority class), created at
        // the first fork it came to share a queue with the bank (8 x 4096 x 86 scraping: 0.30 -> 0.40 ms per step;
        // scripts/debug/r05_aux_queue.sh).  Large OBJECTS: that is where projection and combine are long enough to be worth a
        // stream (64 x 256 with a moving listener, host-bound, 0.13 - 0.15 ms per step without the third stream and 0.15 - 0.19
        // with it).  PBSO_PREP_SPLIT=2 creates it for any engine (tests), 0 never.
        long long modes = 0;
        for (int n : n_modes) modes += n;
        if (prep_split_ == 2 || (prep_split_ == 1 && modes >= 32768 && modes >= 1024LL * N))
            HIPTRY(hipStreamCreateWithPriority(&aux_stream_, hipStreamNonBlocking, prep_priority_));
    }
    // Team shape: R oscillators per lane; an object of n modes needs ceil(n / 64R) waves, cut into
    // teams (workgroups) of at most MAX_WAVES_PER_TEAM waves.  The VALU issue rate needs ~4 waves per
    // SIMD (4096 on the chip, profiles/r01_microbench.txt).
    int R = desc_.modes_per_lane;
    if (R != 0 && R != 1 && R != 2 && R != 3 && R != 4 && R != 8) return fail(PBSO_ERR_INVALID, "modes_per_lane must be 0,1,2,3,4,8");
    const bool block = is_block();
    // (round 6: the block form's eight-modes-per-lane builds -- one wave per SIMD, 300 - 460 bytes of scratch per lane -- were never a
    //  policy's choice and are gone)
    if (block && (R == 3 || R == 8)) return fail(PBSO_ERR_INVALID, "modes_per_lane must be 0,1,2,4 in the block form");
    if (R == 0) R = choose_modes_per_lane(n_modes, block, n_cus_);
    int wmax = 1;
    for (int n : n_modes) wmax = std::max(wmax, waves_of(n, R));
    R_ = R;
    m_pad_ = 64 * R * wmax;
    // K5 (kernels_scan.hip): launches cut along the time axis pick their team shape per launch, up to four modes per lane: rows
    // padded to whole 256-column waves of that shape (padding columns are dead: zero coefficients, zero state)
    tc_ok_ = block && tc_mode_ >= 0;
    if (tc_ok_) m_pad_ = (m_pad_ + 255) / 256 * 256;

    int rc;
    if ((rc = finalize_teams(n_modes)) != PBSO_OK) return rc;
    if ((rc = finalize_coefs()) != PBSO_OK) return rc;
    if ((rc = finalize_shapes()) != PBSO_OK) return rc;
    if ((rc = finalize_ffat(n_modes)) != PBSO_OK) return rc;
    HIPTRY(hipMemcpy(d_n_modes_.p, n_modes.data(), N * sizeof(int), hipMemcpyHostToDevice));
    HIPTRY(d_board_.ensure(4096));
    HIPTRY(hipMemset(d_board_.p, 0, 4096 * sizeof(unsigned)));
    // transfer rows: [0,N) _latest_transfer, [N,2N) the 1-slot transfer queue, then per-launch scratch
    HIPTRY(d_xfer_.ensure((size_t)2 * N * m_pad_));
    HIPTRY(hipMemset(d_xfer_.p, 0, (size_t)2 * N * m_pad_ * sizeof(double)));
    (void)warm_copy_engines();
    if (desc_.submit_thread > 0) submit_ = new SubmitQueue(desc_.device);
    finalized_ = true;
    return PBSO_OK;
}

int Engine::upload_team_table(const TeamTable &t, DevBuf<TeamDesc> &d_teams, DevBuf<SplitObj> &d_split) {
    HIPTRY(d_teams.ensure(t.teams.size()));
    HIPTRY(hipMemcpy(d_teams.p, t.teams.data(), t.teams.size() * sizeof(TeamDesc), hipMemcpyHostToDevice));
    if (!t.split.empty()) {
        HIPTRY(d_split.ensure(t.split.size()));
        HIPTRY(hipMemcpy(d_split.p, t.split.data(), t.split.size() * sizeof(SplitObj), hipMemcpyHostToDevice));
    }
    return PBSO_OK;
}

// The three kinds of team table (engine_tables.h), grouped into size classes: one launch of the oscillator bank per team
// size, largest first.
int Engine::finalize_teams(const std::vector<int> &n_modes) {
    const bool block = is_block();
    int rc;
    {
        // the engine's own shape
        // (the per-sample kernel's LDS grows with the buffer length: no team larger than a CU's LDS holds at this n_tiles)
        const int team_max = block ? MAX_WAVES_PER_BLOCK_TEAM : iir_team_cap_by_lds(n_tiles_, MAX_WAVES_PER_TEAM);
        if (!block && iir_lds_bytes(team_max, n_tiles_) > IIR_LDS_LIMIT)
            return fail(PBSO_ERR_INVALID, "frames_per_buffer: the per-sample kernel's tile ring does not fit the LDS");
        total_team_waves_ = total_waves(n_modes, R_);
        const int team_cap = engine_team_cap(total_team_waves_, n_cus_, team_max, desc_.team_waves);
        const TeamTable t = build_team_table(waves_per_object(n_modes, R_), R_, std::vector<int>(n_modes.size(), team_cap), MAX_WAVES_PER_TEAM);
        classes_ = t.classes;
        W_ = t.w_max;
        n_teams_ = (int)t.teams.size();
        n_split_ = (int)t.split.size();
        n_part_rows_ = t.n_part_rows;
        if (classes_.size() > 1 && !ev_fork_) {
            HIPTRY(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
            for (int i = 0; i < N_CLASS_STREAMS; ++i) {
                HIPTRY(hipStreamCreateWithFlags(&class_stream_[i], hipStreamNonBlocking));
                HIPTRY(hipEventCreateWithFlags(&ev_join_[i], hipEventDisableTiming));
            }
        }
        if ((rc = upload_team_table(t, d_teams_, d_split_)) != PBSO_OK) return rc;
    }
    if (tc_ok_) {
        // the time-chunked launches, one table per shape
        const int shapes[3] = {1, 2, 4};
        for (int k = 0; k < 3; ++k) {
            TcSet &ts = tc_[k];
            const TcShapeTable s = build_tc_shape(n_modes, shapes[k], desc_.team_waves);
            ts.R = shapes[k];
            ts.classes = s.table.classes;
            ts.n_teams = (int)s.table.teams.size();
            ts.n_split = (int)s.table.split.size();
            ts.n_part_rows = s.table.n_part_rows;
            ts.waves = s.waves;
            ts.cover = s.cover;
            ts.waves_per_cu = s.waves_per_cu;
            if ((rc = upload_team_table(s.table, ts.d_teams, ts.d_split)) != PBSO_OK) return rc;
        }
    }
    // K1p: fewer than one wave of oscillators per SIMD even with one mode per lane -- a team of several waves per 64
    // modes instead (kernels_pipe.hip: a producer and two consumers).  f32 block form only; desc.bank_kernel = BLOCK keeps
    // the one-wave-per-64-modes kernel (and its time chunks, K5) for every launch.
    split_ok_ = false;
    const long long max_chunks = desc_.pipe_max_teams > 0 ? desc_.pipe_max_teams : 2LL * n_cus_;
    if (block && form_ == PBSO_FORM_BLOCK && R_ == 1 && pipe_chunks(n_modes) <= max_chunks && desc_.bank_kernel != PBSO_BANK_BLOCK) {
        const TeamTable t = build_pipe_table(n_modes);
        n_ts_teams_ = (int)t.teams.size();
        n_ts_split_ = (int)t.split.size();
        n_ts_part_rows_ = t.n_part_rows;
        if ((rc = upload_team_table(t, d_ts_teams_, d_ts_split_)) != PBSO_OK) return rc;
        split_ok_ = true;
        split_always_ = desc_.bank_kernel == PBSO_BANK_PIPE;
    }
    return PBSO_OK;
}

// the coefficient tables (engine_tables.h) and the state planes
int Engine::finalize_coefs() {
    const int N = (int)objs_.size();
    const size_t nm = (size_t)N * m_pad_;
    const bool block = is_block();
    const std::vector<ModeCoefs> coefs = coefs_of(objs_);
    std::vector<float> ca, cb;
    std::vector<double> c3;
    build_bank_coefs(coefs, m_pad_, form_ == PBSO_FORM_DIRECT, ca, cb, c3);
    HIPTRY(d_ca_.ensure(nm));
    HIPTRY(d_cb_.ensure(nm));
    HIPTRY(d_sq_.ensure(nm));
    HIPTRY(d_sd_.ensure(nm));
    HIPTRY(d_ss_.ensure(nm));
    HIPTRY(d_c3_.ensure(nm));
    HIPTRY(d_n_modes_.ensure(N));
    HIPTRY(hipMemcpy(d_ca_.p, ca.data(), nm * sizeof(float), hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(d_cb_.p, cb.data(), nm * sizeof(float), hipMemcpyHostToDevice));
    HIPTRY(hipMemset(d_sq_.p, 0, nm * sizeof(float)));
    HIPTRY(hipMemset(d_sd_.p, 0, nm * sizeof(float)));
    HIPTRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d_ss_.p), 0x3F800000, nm));      // scale 1.0f: state stored unscaled
    HIPTRY(hipMemcpy(d_c3_.p, c3.data(), nm * sizeof(double), hipMemcpyHostToDevice));
    if (desc_.qnorm_mode == PBSO_QNORM_CLOSED || (block && desc_.qnorm_mode != PBSO_QNORM_OFF)) {
        int rc = build_gq();
        if (rc != PBSO_OK) return rc;
    }
    if (!block) return PBSO_OK;
    std::vector<float> pc, wt;
    build_wp_tables(coefs, m_pad_, pc, wt);
    if (form_ == PBSO_FORM_BLOCK_BF16) wtab_to_split_bf16(wt, nm);
    HIPTRY(d_pc_.ensure(4 * nm));
    HIPTRY(hipMemcpy(d_pc_.p, pc.data(), 4 * nm * sizeof(float), hipMemcpyHostToDevice));
    if (tc_ok_) {
        const std::vector<float> sc = build_scan_table(coefs, m_pad_, B_);
        HIPTRY(d_scan_.ensure(6 * nm));
        HIPTRY(hipMemcpy(d_scan_.p, sc.data(), 6 * nm * sizeof(float), hipMemcpyHostToDevice));
    }
    // (a time-chunked launch picks its own team shape: one or two modes per lane use the table; K5's dense_increment_kernel
    //  uses it whatever the projection and the bank's own path for dense buffers are)
    // Engines with more than two modes per lane keep the per-sample path (no registers left for 32 constants per mode).
    ftab_forced_ = form_ == PBSO_FORM_BLOCK && (R_ <= 2 || tc_ok_) && forced_block_;
    if (ftab_forced_ || tc_ok_) {
        const std::vector<float> ft = build_f_table(coefs, m_pad_);
        HIPTRY(d_ftab_.ensure(ft.size()));
        HIPTRY(hipMemcpy(d_ftab_.p, ft.data(), ft.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    HIPTRY(d_wtab_.ensure(wt.size()));
    HIPTRY(hipMemcpy(d_wtab_.p, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
    return PBSO_OK;
}

// mode shapes: mode-major (ModeData.h:24) -> vertex-major [dof][m_pad]
int Engine::finalize_shapes() {
    const int N = (int)objs_.size();
    std::vector<long long> off(N, 0);
    size_t total = 0;
    for (int i = 0; i < N; ++i) {
        off[i] = (long long)total;
        total += (size_t)objs_[i].n_dof * m_pad_;
    }
    HIPTRY(d_shape_off_.ensure(N));
    HIPTRY(hipMemcpy(d_shape_off_.p, off.data(), N * sizeof(long long), hipMemcpyHostToDevice));
    std::vector<long long> row_off(N, 0);
    for (int i = 0; i < N; ++i) row_off[i] = off[i] / m_pad_;
    HIPTRY(d_g32_off_.ensure(N));
    HIPTRY(hipMemcpy(d_g32_off_.p, row_off.data(), N * sizeof(long long), hipMemcpyHostToDevice));
    HIPTRY(d_g32_.ensure(std::max<size_t>(total, 1)));
    if (!total) return PBSO_OK;
    HIPTRY(d_shapes_.ensure(total));
    std::vector<double> vm;
    std::vector<float> vg;
    for (int i = 0; i < N; ++i) {
        Object &o = objs_[i];
        if (!o.n_dof) continue;
        transpose_shapes(o.shapes, o.c3.data(), o.n_modes, o.n_dof, m_pad_, vm, vg);
        HIPTRY(hipMemcpy(d_shapes_.p + off[i], vm.data(), vm.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPTRY(hipMemcpy(d_g32_.p + off[i], vg.data(), vg.size() * sizeof(float), hipMemcpyHostToDevice));
        std::vector<double>().swap(o.shapes);
    }
    return PBSO_OK;
}

// FFAT maps: the objects' maps packed, and once more, transposed, for the objects whose modes share one geometry
// (engine_tables.h, build_ffat_shared; PBSO_FFAT_SHARED=0: never)
int Engine::finalize_ffat(const std::vector<int> &n_modes) {
    const int N = (int)objs_.size();
    std::vector<long long> goff(N, 0);
    std::vector<FfatGeom> geom;
    std::vector<double> psi;
    for (int i = 0; i < N; ++i) {
        Object &o = objs_[i];
        o.maps_cover_modes = true;
        for (int m = 0; m < o.n_modes; ++m)
            if (m >= (int)o.geom.size() || !o.geom[m].valid) { o.maps_cover_modes = false; break; }
        goff[i] = (long long)geom.size();
        const int ng = std::min((int)o.geom.size(), m_pad_);
        for (int m = 0; m < ng; ++m) {
            FfatGeom g = o.geom[m];
            g.psi_off += (long long)psi.size();
            geom.push_back(g);
        }
        // pad so that every mode < n_modes has an entry
        for (int m = ng; m < o.n_modes; ++m) {
            FfatGeom z;
            std::memset(&z, 0, sizeof(z));
            geom.push_back(z);
        }
        psi.insert(psi.end(), o.psi.begin(), o.psi.end());
        std::vector<double>().swap(o.psi);
    }
    HIPTRY(d_geom_off_.ensure(N));
    HIPTRY(hipMemcpy(d_geom_off_.p, goff.data(), N * sizeof(long long), hipMemcpyHostToDevice));
    geom_off_h_ = goff;
    if (!geom.empty()) {
        HIPTRY(d_geom_.ensure(geom.size()));
        HIPTRY(hipMemcpy(d_geom_.p, geom.data(), geom.size() * sizeof(FfatGeom), hipMemcpyHostToDevice));
    }
    if (!psi.empty()) {
        HIPTRY(d_psi_.ensure(psi.size()));
        HIPTRY(hipMemcpy(d_psi_.p, psi.data(), psi.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const char *env = std::getenv("PBSO_FFAT_SHARED");
    const FfatSharedTables t = build_ffat_shared(n_modes, geom, goff, psi, !(env && std::atoi(env) == 0));
    ffat_shared_h_ = t.is_shared;
    n_ffat_shared_ = t.n_shared;
    if (n_ffat_shared_ > 0) {
        HIPTRY(d_ffat_shared_.ensure(N));
        HIPTRY(hipMemcpy(d_ffat_shared_.p, t.shared.data(), N * sizeof(FfatShared), hipMemcpyHostToDevice));
        HIPTRY(d_ffat_k_.ensure(t.mode_k.size()));
        HIPTRY(hipMemcpy(d_ffat_k_.p, t.mode_k.data(), t.mode_k.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPTRY(d_ffat_valid_.ensure(t.mode_valid.size()));
        HIPTRY(hipMemcpy(d_ffat_valid_.p, t.mode_valid.data(), t.mode_valid.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPTRY(d_psi_t_.ensure(t.psi_t.size()));
        HIPTRY(hipMemcpy(d_psi_t_.p, t.psi_t.data(), t.psi_t.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return PBSO_OK;
}

// One-time work of the runtime that would otherwise block a step's submission, done here, untimed (PBSO_WARM_COPIES=0: not).
// Found with PBSO_TIMELINE=1 / scripts/debug/r03_stalls.py: an engine's first ~30 launches contained two hipMemcpyAsync calls
// (the step's ONE upload) that took 6 - 7 ms each whatever their size, with no buffer growing -- in the middle of a real-time run,
// or of a 20-step timed region (64 x 256 with a listener move per buffer measured 2800 x or 4900 x run to run, depending on
// whether one fell into the 40 timed steps).  (1) The runtime opens its copy queues lazily: a few overlapping uploads and
// read-backs on both streams remove the first.  (2) The other comes with the first upload whose stream is still WAITING for an
// event of the other stream when the call is made -- which is what a step's upload looks like as soon as the host runs a whole
// plan set ahead of the oscillator bank (the wait for ev_k1_done_ in front of it); it happened at a random launch, whenever the
// host first got that far ahead.  Issuing exactly that pattern here removes it.
int Engine::warm_copy_engines() {
    if (desc_.warm_copies < 0) return PBSO_OK;
    // Best effort: a failure here costs a slow first launch, never the engine (errors are swallowed, everything is released).
    // A caller's stream is not touched: the second pattern only needs SOME stream the preparation stream waits for.
    constexpr size_t chunk = (size_t)1 << 20;
    const int n = 6;
    PinBuf<unsigned char> h;
    DevBuf<unsigned char> d;
    hipStream_t other = own_stream_ ? stream_ : nullptr;
    hipEvent_t ev = nullptr, ev2 = nullptr;
    auto body = [&]() -> hipError_t {
        hipError_t e;
        if (!other && (e = hipStreamCreateWithFlags(&other, hipStreamNonBlocking)) != hipSuccess) return e;
        if ((e = h.ensure(chunk * n)) != hipSuccess) return e;
        if ((e = d.ensure(chunk * n)) != hipSuccess) return e;
        std::memset(h.p, 0, chunk * n);
        for (int rep = 0; rep < 2; ++rep) {           // (1) the copy queues, both directions, both streams
            for (int i = 0; i < n; ++i)
                if ((e = hipMemcpyAsync(d.p + chunk * i, h.p + chunk * i, chunk, hipMemcpyHostToDevice, (i & 1) ? other : prep_stream_)) != hipSuccess) return e;
            for (int i = 0; i < n; ++i)
                if ((e = hipMemcpyAsync(h.p + chunk * i, d.p + chunk * i, chunk, hipMemcpyDeviceToHost, (i & 1) ? prep_stream_ : other)) != hipSuccess) return e;
        }
        if ((e = hipStreamSynchronize(prep_stream_)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(other)) != hipSuccess) return e;
        // (2) uploads behind a wait for an event that has not happened yet
        if ((e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&ev2, hipEventDisableTiming)) != hipSuccess) return e;
        for (int rep = 0; rep < 4; ++rep) {
            for (int i = 0; i < n; ++i)
                if ((e = hipMemcpyAsync(d.p + chunk * i, h.p + chunk * i, chunk, hipMemcpyHostToDevice, other)) != hipSuccess) return e;
            if ((e = hipEventRecord(ev, other)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(prep_stream_, ev, 0)) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(d.p, h.p, (size_t)384 << 10, hipMemcpyHostToDevice, prep_stream_)) != hipSuccess) return e;
            if ((e = hipEventRecord(ev2, prep_stream_)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(other, ev2, 0)) != hipSuccess) return e;
        }
        if ((e = hipStreamSynchronize(prep_stream_)) != hipSuccess) return e;
        return hipStreamSynchronize(other);
    };
    (void)body();
    (void)hipGetLastError();
    if (prep_stream_) (void)hipStreamSynchronize(prep_stream_);
    if (other) (void)hipStreamSynchronize(other);
    if (ev) (void)hipEventDestroy(ev);
    if (ev2) (void)hipEventDestroy(ev2);
    if (other && other != stream_) (void)hipStreamDestroy(other);
    h.release();
    d.release();
    return PBSO_OK;
}

}  // namespace pbso
