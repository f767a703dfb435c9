// pbso_set_material (include/openpbso_amd.h, "retune"): validation, the upload of (c1, c2, c3) per mode of the named objects, the
// ordering against launches in flight, and the launch of the kernels that rebuild the tables (kernels_retune.hip, mode_tables.h).
#include "engine.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pbso {

// Everything that can refuse a call, with no side effect.  coefs (may be null): the new (c1, c2, c3) of every mode of every
// named object, in call order.
static const char *material_fault(const std::vector<Object> &objs, int rate, int n, const int *ids, const pbso_material *mats,
                                  std::vector<double> *coefs) {
    if (n < 0) return "set_material: n < 0";
    if (n > 0 && (!ids || !mats)) return "set_material: NULL array";
    std::vector<unsigned char> named(objs.size(), 0);
    const double h = 1.0 / (double)rate;
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= (int)objs.size()) return "set_material: object id out of range";
        if (named[ids[i]]) return "set_material: an object id is named twice";
        named[ids[i]] = 1;
        const pbso_material &mt = mats[i];
        if (!std::isfinite(mt.density) || !std::isfinite(mt.alpha) || !std::isfinite(mt.beta)) return "set_material: a value is not finite";
        if (!(mt.density > 0)) return "set_material: density <= 0";
        const Object &o = objs[ids[i]];
        for (int m = 0; m < o.n_modes; ++m) {
            double c[3];
            integrator_coefs(o.omega_squared[m], mt.density, mt.alpha, mt.beta, h, c[0], c[1], c[2]);
            if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
                return "set_material: a mode's c1, c2 or c3 is not finite (over-damped for this material)";
            if (coefs) coefs->insert(coefs->end(), c, c + 3);
        }
    }
    return nullptr;
}

int Engine::check_material(int n, const int *ids, const pbso_material *mats) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "set_material before finalize");
    if (failed_) return fail(PBSO_ERR_STATE, "an earlier step failed half-way: create a new engine");
    const char *why = material_fault(objs_, rate_, n, ids, mats, nullptr);
    return why ? fail(PBSO_ERR_INVALID, why) : PBSO_OK;
}

int Engine::get_material(int obj, pbso_material *out) {
    if (!valid_obj(obj) || !out) return fail(PBSO_ERR_INVALID, "get_material arguments");
    *out = objs_[obj].material;
    return PBSO_OK;
}

void Engine::material_stats(int64_t out[4]) const {
    out[0] = retune_calls_; out[1] = retune_objects_; out[2] = retune_modes_; out[3] = retune_g32_;
}

int Engine::set_material(int n, const int *ids, const pbso_material *mats, int keep_state) {
    if (!finalized_) return fail(PBSO_ERR_STATE, "set_material before finalize");
    if (failed_) return fail(PBSO_ERR_STATE, "an earlier step failed half-way: create a new engine");
    std::vector<double> coefs;
    if (const char *why = material_fault(objs_, rate_, n, ids, mats, &coefs)) return fail(PBSO_ERR_INVALID, why);
    if (n == 0) { retune_calls_ += 1; return PBSO_OK; }
    HIPTRY(hipSetDevice(desc_.device));
    // the upload, staged before anything of the engine changes: [RetuneObj records | coefficients]
    const size_t rec_bytes = arena_align((size_t)n * sizeof(RetuneObj)), bytes = rec_bytes + std::max<size_t>(coefs.size(), 1) * sizeof(double);
    HIPTRY(h_retune_.ensure(bytes));
    RetuneObj *recs = reinterpret_cast<RetuneObj *>(h_retune_.p);
    long long off = 0, max_elems = 0, g32_elems = 0, modes = 0;
    {
        long long shape_off = 0;
        std::vector<long long> shape_off_of(objs_.size());
        for (size_t i = 0; i < objs_.size(); ++i) { shape_off_of[i] = shape_off; shape_off += (long long)objs_[i].n_dof * m_pad_; }
        for (int i = 0; i < n; ++i) {
            const Object &o = objs_[ids[i]];
            recs[i] = RetuneObj{ids[i], o.n_modes, o.n_dof, 0, off, shape_off_of[ids[i]]};
            off += 3LL * o.n_modes;
            modes += o.n_modes;
            max_elems = std::max(max_elems, (long long)o.n_dof * m_pad_);
            g32_elems += (long long)o.n_dof * m_pad_;
        }
    }
    if (!coefs.empty()) std::memcpy(h_retune_.p + rec_bytes, coefs.data(), coefs.size() * sizeof(double));
    // Order against everything in flight: the submitting thread's queue, every stream, the launch in flight.  From here on the
    // state planes hold the state pbso_read_state returns, and no kernel reads a table.
    { int rc = sync(); if (rc != PBSO_OK) return rc; }
    HIPTRY(d_retune_.ensure(bytes));
    HIPTRY(hipMemcpyAsync(d_retune_.p, h_retune_.p, bytes, hipMemcpyHostToDevice, stream_));
    const RetuneObj *d_recs = reinterpret_cast<const RetuneObj *>(d_retune_.p);
    const double *d_coefs = reinterpret_cast<const double *>(d_retune_.p + rec_bytes);
    RetuneTables t;
    std::memset(&t, 0, sizeof(t));
    t.ca = d_ca_.p; t.cb = d_cb_.p; t.c3 = d_c3_.p;
    t.gq = d_gq_.p;                                      // (where the engine built it: finalize, or listeners_enable)
    if (is_block()) {
        t.pc = d_pc_.p; t.wtab = d_wtab_.p;
        t.sc = tc_ok_ ? d_scan_.p : nullptr;
        t.ftab = (ftab_forced_ || tc_ok_) ? d_ftab_.p : nullptr;
        t.w_kind = form_ == PBSO_FORM_BLOCK_BF16 ? W_SPLIT_BF16 : W_F32;
    }
    // keep_state != 0: the planes hold (scale x state) and the scale in the form's own variables, none of which is made from a
    // coefficient -- what pbso_read_state returns is what it returned.  0: as finalize leaves them (scale 1: stored unscaled)
    if (!keep_state) { t.sq = d_sq_.p; t.sd = d_sd_.p; t.ss = d_ss_.p; }
    t.plane = (long long)objs_.size() * m_pad_;
    t.m_pad = m_pad_; t.frames = B_; t.direct_form = form_ == PBSO_FORM_DIRECT;
    static const bool timing = [] { const char *v = std::getenv("PBSO_RETUNE_TIMING"); return v && std::atoi(v) != 0; }();
    if (timing)
        for (hipEvent_t &ev : retune_ev_)
            if (!ev) HIPTRY(hipEventCreate(&ev));
    if (timing) HIPTRY(hipEventRecord(retune_ev_[0], stream_));
    LAUNCHTRY(launch_retune_tables(t, d_recs, n, d_coefs, stream_));
    if (timing) HIPTRY(hipEventRecord(retune_ev_[1], stream_));
    if (max_elems > 0) LAUNCHTRY(launch_retune_g32(d_recs, n, d_coefs, d_shapes_.p, d_g32_.p, m_pad_, max_elems, stream_));
    if (timing) HIPTRY(hipEventRecord(retune_ev_[2], stream_));
    // the host's copies: pbso_listeners_enable reads c1 / c2, and the objects that keep block-start states have an f32 operand
    // table of their own
    const size_t wt_floats = (size_t)m_pad_ / 2 * 64;
    std::vector<float> wt;
    const double *c = coefs.data();
    for (int i = 0; i < n; ++i) {
        Object &o = objs_[ids[i]];
        for (int m = 0; m < o.n_modes; ++m, c += 3) { o.c1[m] = c[0]; o.c2[m] = c[1]; o.c3[m] = c[2]; }
        o.material = mats[i];
        if (!dump_row_.empty() && dump_row_[ids[i]] >= 0) {
            wt.assign(wt_floats, 0.f);
            for (int m = 0; m < o.n_modes; ++m) mode_walk(o.c1[m], o.c2[m], 0, (size_t)m, 0, W_F32, wt.data(), nullptr, nullptr);
            HIPTRY(hipMemcpyAsync(d_wtab32_.p + (size_t)dump_row_[ids[i]] * wt_floats, wt.data(), wt_floats * sizeof(float), hipMemcpyHostToDevice, stream_));
            HIPTRY(hipStreamSynchronize(stream_));       // (wt is reused)
            dump_valid_[ids[i]] = 0;                     // the last step's states were stepped with the old material
        }
    }
    HIPTRY(hipStreamSynchronize(stream_));
    if (timing) {
        (void)hipEventElapsedTime(&retune_ms_[0], retune_ev_[0], retune_ev_[1]);
        (void)hipEventElapsedTime(&retune_ms_[1], retune_ev_[1], retune_ev_[2]);
        std::fprintf(stderr, "pbso retune: tables kernel %.4f ms, g32 kernel %.4f ms (%lld elements), %d objects, %lld modes\n", retune_ms_[0],
                     retune_ms_[1], max_elems > 0 ? g32_elems : 0LL, n, modes);
    }
    retune_calls_ += 1; retune_objects_ += n; retune_modes_ += modes; retune_g32_ += g32_elems;
    return PBSO_OK;
}

}  // namespace pbso
