// The per-lane bodies of the retune kernels (csrc/mode_tables.h: retune_lane, retune_g32_lane) against the vector builders of
// csrc/engine_tables.h, bit for bit: every lane is called as the grid of kernels_retune.hip would, on tables that first hold
// ANOTHER material's values (so a lane that writes nothing is caught), then every table is compared with what finalize builds
// from the same c1, c2, c3.  Host compiler, -fsanitize=address,undefined, -ffp-contract=off; no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "engine_tables.h"

using namespace pbso;

static int g_fail = 0;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
            g_fail += 1;                                              \
        }                                                             \
    } while (0)

struct ObjCoefs { std::vector<double> c1, c2, c3; };

// modal_integrator.h:63-99 for a plausible spread of modes; the material enters through alpha / beta / density
static ObjCoefs make_coefs(int n, int obj, double density, double alpha, double beta, int rate) {
    ObjCoefs o;
    const double h = 1.0 / rate;
    for (int m = 0; m < n; ++m) {
        const double f = 60.0 + 17000.0 * (m + 0.37 * obj) / (n + 1.0);
        const double lam = std::pow(2.0 * M_PI * f, 2) * 2700.0;
        const double omega0 = std::sqrt(lam / density), xi = 0.5 * (alpha / omega0 + beta * omega0), a = 2.0 * xi * omega0, b = omega0 * omega0;
        const double eps = std::exp(-a / 2 * h), theta = h * std::sqrt(b - a * a / 4.0), gamma = std::asin(a / (2.0 * std::sqrt(b)));
        o.c1.push_back(2.0 * eps * std::cos(theta));
        o.c2.push_back(-eps * eps);
        o.c3.push_back(2.0 * (eps * std::cos(theta + gamma) - eps * eps * std::cos(2.0 * theta + gamma)) / (3.0 * std::sqrt(b) * std::sqrt(b - a * a / 4.0)) * 1E9);
    }
    return o;
}

struct Tables {
    std::vector<float> ca, cb, pc, wt, gq, sc, ft, g32, sq, sd, ss;
    std::vector<double> c3, shapes;
};

// what finalize builds (engine_finalize.cpp, finalize_coefs / finalize_shapes) for these objects
static Tables host_tables(const std::vector<ObjCoefs> &objs, const std::vector<int> &n_dof, const std::vector<std::vector<double>> &shapes_mm,
                          int m_pad, int frames, bool direct, bool bf16) {
    Tables t;
    std::vector<ModeCoefs> mc;
    for (const ObjCoefs &o : objs) mc.push_back(ModeCoefs{o.c1.data(), o.c2.data(), o.c3.data(), (int)o.c1.size()});
    const size_t nm = objs.size() * (size_t)m_pad;
    build_bank_coefs(mc, m_pad, direct, t.ca, t.cb, t.c3);
    t.gq = build_gq_table(mc, m_pad, frames);
    build_wp_tables(mc, m_pad, t.pc, t.wt);
    if (bf16) wtab_to_split_bf16(t.wt, nm);
    t.sc = build_scan_table(mc, m_pad, frames);
    t.ft = build_f_table(mc, m_pad);
    for (size_t i = 0; i < objs.size(); ++i) {
        if (!n_dof[i]) continue;
        std::vector<double> vm;
        std::vector<float> vg;
        transpose_shapes(shapes_mm[i], objs[i].c3.data(), (int)objs[i].c1.size(), n_dof[i], m_pad, vm, vg);
        t.shapes.insert(t.shapes.end(), vm.begin(), vm.end());
        t.g32.insert(t.g32.end(), vg.begin(), vg.end());
    }
    t.sq.assign(nm, 0.f); t.sd.assign(nm, 0.f); t.ss.assign(nm, 1.f);
    return t;
}

template <class T>
static void same(const char *name, const std::vector<T> &a, const std::vector<T> &b, const char *what) {
    CHECK(a.size() == b.size(), "%s %s: sizes %zu %zu", what, name, a.size(), b.size());
    if (a.size() != b.size()) return;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) { CHECK(false, "%s %s: element %zu differs", what, name, i); return; }
}

static void run_case(const std::vector<int> &n_modes, int m_pad, int frames, bool direct, bool bf16, bool zero_state) {
    char what[128];
    std::snprintf(what, sizeof(what), "m_pad %d frames %d direct %d bf16 %d zero %d", m_pad, frames, (int)direct, (int)bf16, (int)zero_state);
    const int N = (int)n_modes.size(), rate = 44100;
    std::vector<ObjCoefs> oldc, newc;
    std::vector<int> n_dof(N, 0);
    std::vector<std::vector<double>> shapes_mm(N);
    for (int i = 0; i < N; ++i) {
        oldc.push_back(make_coefs(n_modes[i], i, 2700.0, 6.0, 1e-7, rate));
        newc.push_back(make_coefs(n_modes[i], i, 1100.0, 30.0, 4e-7, rate));
        if (i % 2 == 1) {                                      // every other object has shapes of 5 vertices
            n_dof[i] = 15;
            for (int k = 0; k < n_modes[i] * 15; ++k) shapes_mm[i].push_back(std::sin(0.7 * k + i) * 1e-3);
        }
    }
    // the retuned objects: all but object 2, which must keep the old material's tables
    std::vector<ObjCoefs> want_c = newc;
    if (N > 2) want_c[2] = oldc[2];
    Tables got = host_tables(oldc, n_dof, shapes_mm, m_pad, frames, direct, bf16);
    Tables want = host_tables(want_c, n_dof, shapes_mm, m_pad, frames, direct, bf16);
    // a state in the planes; zero_state clears the named objects' columns only
    for (size_t k = 0; k < got.sq.size(); ++k) { got.sq[k] = 0.25f + (float)k; got.sd[k] = -1.5f; got.ss[k] = 2.f; }
    want.sq = got.sq; want.sd = got.sd; want.ss = got.ss;
    std::vector<RetuneObj> recs;
    std::vector<double> coefs;
    long long shape_off = 0;
    for (int i = 0; i < N; ++i) {
        if (!(N > 2 && i == 2)) {
            recs.push_back(RetuneObj{i, n_modes[i], n_dof[i], 0, (long long)coefs.size(), shape_off});
            for (int m = 0; m < n_modes[i]; ++m) { coefs.push_back(newc[i].c1[m]); coefs.push_back(newc[i].c2[m]); coefs.push_back(newc[i].c3[m]); }
            if (zero_state)
                for (int m = 0; m < m_pad; ++m) { const size_t k = (size_t)i * m_pad + m; want.sq[k] = 0.f; want.sd[k] = 0.f; want.ss[k] = 1.f; }
        }
        shape_off += (long long)n_dof[i] * m_pad;
    }
    // the named objects in another order than their ids, as a caller may give them
    if (recs.size() > 1) std::swap(recs[0], recs[recs.size() - 1]);
    RetuneTables t;
    std::memset(&t, 0, sizeof(t));
    t.ca = got.ca.data(); t.cb = got.cb.data(); t.c3 = got.c3.data(); t.pc = got.pc.data(); t.wtab = got.wt.data(); t.gq = got.gq.data();
    t.sc = got.sc.data(); t.ftab = got.ft.data();
    if (zero_state) { t.sq = got.sq.data(); t.sd = got.sd.data(); t.ss = got.ss.data(); }
    t.plane = (long long)N * m_pad; t.m_pad = m_pad; t.frames = frames; t.direct_form = direct; t.w_kind = bf16 ? W_SPLIT_BF16 : W_F32;
    // the grid of retune_tables_kernel: blocks of 256 lanes over the columns, one row of blocks per named object
    for (size_t y = 0; y < recs.size(); ++y)
        for (int bx = 0; bx < (m_pad + 255) / 256; ++bx)
            for (int tid = 0; tid < 256; ++tid) {
                const int m = bx * 256 + tid;
                if (m < m_pad) retune_lane(t, recs[y], coefs.data(), m);
            }
    // ... and of retune_g32_kernel: a grid-stride loop over the elements of each named object
    for (size_t y = 0; y < recs.size(); ++y) {
        const long long n = (long long)recs[y].n_dof * m_pad;
        for (long long e = 0; e < n; ++e) retune_g32_lane(recs[y], coefs.data(), got.shapes.data(), got.g32.data(), m_pad, e);
    }
    same("ca", got.ca, want.ca, what); same("cb", got.cb, want.cb, what); same("c3", got.c3, want.c3, what);
    same("pc", got.pc, want.pc, what); same("wtab", got.wt, want.wt, what); same("gq", got.gq, want.gq, what);
    same("sc", got.sc, want.sc, what); same("ftab", got.ft, want.ft, what); same("g32", got.g32, want.g32, what);
    same("sq", got.sq, want.sq, what); same("sd", got.sd, want.sd, what); same("ss", got.ss, want.ss, what);
    // a table the engine does not have (null) is not touched, and the others come out the same
    Tables got2 = host_tables(oldc, n_dof, shapes_mm, m_pad, frames, direct, bf16);
    RetuneTables t2 = t;
    t2.ca = got2.ca.data(); t2.cb = got2.cb.data(); t2.c3 = got2.c3.data(); t2.gq = nullptr; t2.pc = got2.pc.data(); t2.wtab = got2.wt.data();
    t2.sc = nullptr; t2.ftab = nullptr; t2.sq = t2.sd = t2.ss = nullptr;
    for (size_t y = 0; y < recs.size(); ++y)
        for (int m = 0; m < m_pad; ++m) retune_lane(t2, recs[y], coefs.data(), m);
    same("pc (no sc)", got2.pc, want.pc, what); same("wtab (no sc)", got2.wt, want.wt, what); same("ca (no sc)", got2.ca, want.ca, what);
}

int main() {
    // ragged objects; m_pad as finalize pads it: 64 R waves, and whole 256-column waves where the time-chunked launches exist
    const std::vector<int> n_modes = {1, 63, 64, 65, 200, 1100};
    for (int frames : {27, 513, 864})
        for (int m_pad : {1152, 1280})
            for (int direct = 0; direct < 2; ++direct)
                for (int bf16 = 0; bf16 < 2; ++bf16) {
                    if (bf16 && m_pad % 256) continue;          // the 16-column groups of the split layout: m_pad a multiple of 256 there
                    run_case(n_modes, m_pad, frames, direct != 0, bf16 != 0, (frames + m_pad + direct) % 2 == 0);
                }
    run_case({1}, 64, 27, false, false, true);                  // one object, one mode, one wave
    run_case({65, 1}, 256, 513, false, true, false);
    if (g_fail) { std::printf("retune tables check: %d FAILURES\n", g_fail); return 1; }
    std::printf("retune tables check ok\n");
    return 0;
}
