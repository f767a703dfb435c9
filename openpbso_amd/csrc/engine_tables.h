// What Engine::finalize computes, apart from where it puts it: the choice of modes per lane, the team tables of the three
// kinds of bank launch, the coefficient tables of the block form and the transposed copies of shapes and FFAT maps.  Pure
// functions over std::vector, host only: no HIP call in here (kernels.h is included for the structures and constants the
// kernels share), so tests/cpp/engine_tables_check.cpp runs them without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "mode_tables.h"

namespace pbso {

// ---- shape: R oscillators per lane; an object of n modes needs ceil(n / 64R) waves -----------------------------------
inline int waves_of(int n_modes, int r) { return std::max(1, (n_modes + 64 * r - 1) / (64 * r)); }
inline long long total_waves(const std::vector<int> &n_modes, int r) {
    long long w = 0;
    for (int n : n_modes) w += waves_of(n, r);
    return w;
}
inline std::vector<int> waves_per_object(const std::vector<int> &n_modes, int r) {
    std::vector<int> w(n_modes.size());
    for (size_t i = 0; i < n_modes.size(); ++i) w[i] = waves_of(n_modes[i], r);
    return w;
}
// The policy's modes per lane (pbso_engine_desc::modes_per_lane = 0).
inline int choose_modes_per_lane(const std::vector<int> &n_modes, bool block, int n_cus) {
    if (block) {
        // The block form is paced by the matrix pipe: two waves per SIMD keep it busy (one issues MFMAs while
        // the other steps its coarse recurrence), and a wave holds 32 R operand registers for its W table.
        // The fewest modes per lane that fit the chip at two waves per SIMD; more objects run in rounds.
        for (int r : {1, 2, 4})
            if (total_waves(n_modes, r) <= 8LL * n_cus) return r;
        return 4;
    }
    // the fewest modes per lane whose waves are all resident at once (16 waves per CU is what the
    // LDS tiles allow: 4096 on the chip) -- a second round of workgroups costs more than the
    // deeper per-lane work (768 x 512: 2.83 ms with R = 1 in two rounds, 1.93 ms with R = 2).
    // Engines that cannot be resident at once with R <= 4 minimise rounds x instructions per
    // wave-sample (5 R + 2.2); R = 8 needs more registers than 4 waves per SIMD leave.
    for (int r : {1, 2, 3, 4})
        if (total_waves(n_modes, r) <= 16LL * n_cus) return r;
    int R = 0;
    double best = 0;
    for (int r : {1, 2, 3, 4}) {
        const double cost = (double)((total_waves(n_modes, r) + 16LL * n_cus - 1) / (16LL * n_cus)) * (5.0 * r + 2.2);
        if (R == 0 || cost < best) { R = r; best = cost; }
    }
    return R;
}
// Team size of the engine's own shape.  A full chip (>= 4096 waves) runs whole objects as teams of up to 16 waves.  Below
// that the launch is bound by the per-sample latency of a wave, which is shortest when the
// wave shares its SIMD / CU with as few others as possible (measured: 8 x 4096 modes 425 -> 570 x
// real time with 2-wave teams, 1 x 512 modes 778 -> 822 x with 1-wave teams): spread the waves
// evenly over the 256 CUs.
inline int engine_team_cap(long long waves, int n_cus, int team_max, int team_waves) {
    if (team_waves > 0) return std::min(team_max, team_waves);
    return (int)std::min<long long>(team_max, std::max<long long>(1, (waves + n_cus - 1) / n_cus));
}
// The per-sample bank's workgroup keeps a ring of n_tiles + 1 row-sum tiles per wave (kernels.h, iir_lds_bytes), so its LDS grows
// with the buffer length: the largest team whose request a CU's 160 KB can hold -- 16 waves up to 25 tiles (675 frames), 15 from
// 26, 14 at 32 (864 frames, where 16 waves would ask for 175 888 bytes).  Objects that need more waves are cut into several teams.
constexpr size_t IIR_LDS_LIMIT = 160 * 1024;
inline int iir_team_cap_by_lds(int n_tiles, int team_max) {
    int w = std::max(1, team_max);
    while (w > 1 && iir_lds_bytes(w, n_tiles) > IIR_LDS_LIMIT) --w;
    return w;
}

// ---- team tables -----------------------------------------------------------------------------------------------------
struct SizeClass { int W, first, count; };               // teams of W waves: teams[first, first + count)
struct TeamTable {
    std::vector<TeamDesc> teams;                         // largest class first, ids in list order
    std::vector<SplitObj> split;                         // objects stepped by more than one team
    std::vector<SizeClass> classes;
    int n_part_rows = 0, w_max = 1;                      // partial rows of the split objects; waves of the largest team
};
// Object i of waves[i] waves (R modes per lane) as ceil(waves / cap[i]) teams of nearly equal size, none above team_max.
// The SoA rows stay m_pad wide and a team touches its own columns only.
inline TeamTable build_team_table(const std::vector<int> &waves, int R, const std::vector<int> &cap, int team_max) {
    TeamTable t;
    std::vector<std::vector<TeamDesc>> by_w(team_max + 1);
    for (int i = 0; i < (int)waves.size(); ++i) {
        const int w = waves[i];
        const int parts = (w + cap[i] - 1) / cap[i];
        const int base = w / parts, rem = w % parts;
        int w0 = 0;
        if (parts > 1) {
            SplitObj so = {i, t.n_part_rows, parts, 0};
            t.split.push_back(so);
        }
        for (int pi = 0; pi < parts; ++pi) {
            const int wp = base + (pi < rem ? 1 : 0);
            TeamDesc td = {i, 64 * R * w0, parts > 1 ? t.n_part_rows++ : -1, 0};
            by_w[wp].push_back(td);
            t.w_max = std::max(t.w_max, wp);
            w0 += wp;
        }
    }
    for (int w = team_max; w >= 1; --w) {
        if (by_w[w].empty()) continue;
        SizeClass c;
        c.W = w;
        c.first = (int)t.teams.size();
        c.count = (int)by_w[w].size();
        t.teams.insert(t.teams.end(), by_w[w].begin(), by_w[w].end());
        t.classes.push_back(c);
    }
    for (size_t k = 0; k < t.teams.size(); ++k) t.teams[k].id = (int)k;
    return t;
}
// K5, one shape of the time-chunked launches: whole objects as teams of up to 8 waves (an object that needs more is cut into
// several teams whose partial sums sum_parts adds), and what the policy wants to know about the shape.
struct TcShapeTable {
    TeamTable table;
    long long waves = 0, cover = 0;                      // waves of all teams; columns they cover (padding included)
    int waves_per_cu = 8;                                // of this shape's build, resident at once (registers, LDS)
};
inline TcShapeTable build_tc_shape(const std::vector<int> &n_modes, int R, int team_waves) {
    TcShapeTable s;
    const std::vector<int> waves = waves_per_object(n_modes, R);
    const int tcap_desc = team_waves > 0 ? std::min(MAX_WAVES_PER_BLOCK_TEAM, team_waves) : MAX_WAVES_PER_BLOCK_TEAM;
    std::vector<int> cap(waves.size());
    int wmax_set = 1;
    for (size_t i = 0; i < waves.size(); ++i) {
        const int w = waves[i];
        // One mode per lane: an object that needs several teams anyway gets teams of FOUR waves -- three such workgroups
        // fit a CU's LDS (twelve waves, three per SIMD; one team of eight leaves it at two per SIMD), and these builds are
        // bound by what a wave does between its matrix bursts, not by the matrix pipe (8 x 4096 sustained scraping).
        cap[i] = (R == 1 && w > MAX_WAVES_PER_BLOCK_TEAM && team_waves <= 0) ? 4 : tcap_desc;
        wmax_set = std::max(wmax_set, std::min(w, cap[i]));
        s.waves += w;
        s.cover += (long long)w * 64 * R;
    }
    s.table = build_team_table(waves, R, cap, MAX_WAVES_PER_BLOCK_TEAM);
    // waves of this shape a CU holds at once: two 256-register waves per SIMD for two and four modes per lane; one mode
    // per lane: three per SIMD by its registers, as many whole workgroups as the LDS takes (allocated in 1280-byte granules)
    if (R == 1) {
        const size_t lds = (block_lds_bytes(wmax_set, 1) + 1279) / 1280 * 1280;
        s.waves_per_cu = (int)std::max<size_t>(wmax_set, std::min<size_t>(12, (160 * 1024 / lds) * wmax_set));
    }
    return s;
}
// K1p (kernels_pipe.hip): one team per 64 columns -- the generic table at one mode per lane and one wave per team
inline long long pipe_chunks(const std::vector<int> &n_modes) { return total_waves(n_modes, 1); }
inline TeamTable build_pipe_table(const std::vector<int> &n_modes) {
    return build_team_table(waves_per_object(n_modes, 1), 1, std::vector<int>(n_modes.size(), 1), 1);
}

// ---- coefficient tables: all in fp64, rounded once ---------------------------------------------------------------------
// The arithmetic per mode (Mat2 and the chains of its powers) lives in mode_tables.h, shared with the kernels that rebuild
// the tables on the device (pbso_set_material); here are the builders of whole tables, [n_obj][m_pad] planes with zero padding.
struct ModeCoefs { const double *c1, *c2, *c3; int n_modes; };   // one object (modal_integrator.h:95-99, fp64)

// the oscillator bank's coefficient planes [n_obj][m_pad]
inline void build_bank_coefs(const std::vector<ModeCoefs> &objs, int m_pad, bool direct_form, std::vector<float> &ca, std::vector<float> &cb,
                             std::vector<double> &c3) {
    const size_t nm = objs.size() * (size_t)m_pad;
    ca.assign(nm, 0.f); cb.assign(nm, 0.f); c3.assign(nm, 0.0);
    for (size_t i = 0; i < objs.size(); ++i) {
        const ModeCoefs &o = objs[i];
        for (int m = 0; m < o.n_modes; ++m) {
            const size_t k = i * m_pad + m;
            mode_bank_coefs(o.c1[m], o.c2[m], direct_form, ca[k], cb[k]);
            c3[k] = o.c3[m];
        }
    }
}
// Closed-form qnorm matrices (mode_gq): planes G11, 2 G12, G22.
inline std::vector<float> build_gq_table(const std::vector<ModeCoefs> &objs, int m_pad, int frames) {
    const size_t nm = objs.size() * (size_t)m_pad;
    std::vector<float> gq(3 * nm, 0.f);
    for (size_t i = 0; i < objs.size(); ++i)
        for (int m = 0; m < objs[i].n_modes; ++m) mode_gq(objs[i].c1[m], objs[i].c2[m], frames, gq.data() + i * m_pad + m, nm);
    return gq;
}
// Block form (mode_walk): pc: planes P11 - 1, P12, P21, P22 of P = A^16; wt: [n_obj * m_pad / 2][64], lane = 16 * (2 * mode-of-pair + comp) + (j - 1).
inline void build_wp_tables(const std::vector<ModeCoefs> &objs, int m_pad, std::vector<float> &pc, std::vector<float> &wt) {
    const size_t nm = objs.size() * (size_t)m_pad;
    pc.assign(4 * nm, 0.f);
    wt.assign(nm / 2 * 64, 0.f);
    for (size_t i = 0; i < objs.size(); ++i)
        for (int m = 0; m < objs[i].n_modes; ++m)
            mode_walk(objs[i].c1[m], objs[i].c2[m], 0, i * m_pad + m, nm, W_F32, wt.data(), pc.data(), nullptr);
}
// K5 (mode_walk): A^B (first entry minus one, as P) and A^(B-1) u.  6 planes.
inline std::vector<float> build_scan_table(const std::vector<ModeCoefs> &objs, int m_pad, int frames) {
    const size_t nm = objs.size() * (size_t)m_pad;
    std::vector<float> sc(6 * nm, 0.f);
    for (size_t i = 0; i < objs.size(); ++i)
        for (int m = 0; m < objs[i].n_modes; ++m)
            mode_walk(objs[i].c1[m], objs[i].c2[m], frames, i * m_pad + m, nm, W_NONE, nullptr, nullptr, sc.data());
    return sc;
}
// Forced block path without qnorm rows (mode_ftab): plane 2 i' + c holds component c of A^(15 - i') u, i' = 0..15, per mode.
inline std::vector<float> build_f_table(const std::vector<ModeCoefs> &objs, int m_pad) {
    const size_t nm = objs.size() * (size_t)m_pad;
    std::vector<float> ft((size_t)32 * nm, 0.f);
    for (size_t i = 0; i < objs.size(); ++i)
        for (int m = 0; m < objs[i].n_modes; ++m) mode_ftab(objs[i].c1[m], objs[i].c2[m], i * m_pad + m, nm, ft.data());
    return ft;
}
// Split-bf16 operand table from the f32 W table, in place (layouts: mode_tables.h, wtab_f32_index / wtab_bf16_index).
inline void wtab_to_split_bf16(std::vector<float> &wt, size_t nm) {
    const std::vector<float> wf(wt);
    std::vector<uint32_t> w16(wt.size(), 0u);
    for (size_t col = 0; col < nm / 16 * 16; ++col)                           // flat column index (object * m_pad + column)
        for (int j = 0; j < BLOCK_J; ++j)
            split_bf16_pair(wf[wtab_f32_index(col, 0, j)], wf[wtab_f32_index(col, 1, j)], w16[wtab_bf16_index(col, 0, j)],
                            w16[wtab_bf16_index(col, 1, j)]);
    std::memcpy(wt.data(), w16.data(), wt.size() * sizeof(float));
}

// ---- mode shapes: mode-major (ModeData.h:24) -> vertex-major [dof][m_pad], and g32 = (float)(c3[m] * shape[dof][m]) -----------
inline void transpose_shapes(const std::vector<double> &shapes, const double *c3, int n_modes, int n_dof, int m_pad, std::vector<double> &vm,
                             std::vector<float> &vg) {
    vm.assign((size_t)n_dof * m_pad, 0.0);
    vg.assign((size_t)n_dof * m_pad, 0.f);
    for (int m = 0; m < n_modes; ++m)
        for (int dof = 0; dof < n_dof; ++dof) {
            const double u = shapes[(size_t)m * n_dof + dof];
            vm[(size_t)dof * m_pad + m] = u;
            vg[(size_t)dof * m_pad + m] = mode_g32(c3[m], u);
        }
}

// ---- FFAT maps -------------------------------------------------------------------------------------------------------
// compared field by field, bit for bit
inline bool same_ffat_geometry(const FfatGeom &a, const FfatGeom &b) {
    return a.n_psi == b.n_psi && !std::memcmp(&a.cell_size, &b.cell_size, sizeof(double)) &&
           !std::memcmp(a.center3, b.center3, sizeof(a.center3)) && !std::memcmp(a.low_corners, b.low_corners, sizeof(a.low_corners)) &&
           !std::memcmp(a.center, b.center, sizeof(a.center)) && !std::memcmp(a.bbox_low, b.bbox_low, sizeof(a.bbox_low)) &&
           !std::memcmp(a.bbox_top, b.bbox_top, sizeof(a.bbox_top)) && !std::memcmp(a.n_elements, b.n_elements, sizeof(a.n_elements)) &&
           !std::memcmp(a.strides, b.strides, sizeof(a.strides));
}
// Objects whose valid modes all carry ONE geometry (a map file's header: box, centre, cell size, face layout) -- every scene
// we know of: the maps of an object are made over the same box -- get their maps a second time, transposed, and their listener
// events the kernel that locates a position once per event (kernels_exact.hip, ffat_lookup_shared_kernel).  A single differing
// mode keeps the object on the general kernels.
struct FfatSharedTables {
    std::vector<FfatShared> shared;                      // per object
    std::vector<unsigned char> is_shared;                // per object: its listener events go to ffat_lookup_shared_kernel
    std::vector<double> mode_k, psi_t;
    std::vector<int> mode_valid;
    int n_shared = 0;
};
// geom / goff / psi: the engine's packed maps (goff[i]: first FfatGeom of object i)
inline FfatSharedTables build_ffat_shared(const std::vector<int> &n_modes, const std::vector<FfatGeom> &geom, const std::vector<long long> &goff,
                                          const std::vector<double> &psi, bool want) {
    const int N = (int)n_modes.size();
    FfatSharedTables t;
    t.shared.resize(N);
    std::memset(t.shared.data(), 0, t.shared.size() * sizeof(FfatShared));
    t.mode_k.assign(geom.size(), 0.0);
    t.mode_valid.assign(geom.size(), 0);
    t.is_shared.assign(N, 0);
    for (int i = 0; i < N && want; ++i) {
        const FfatGeom *g = geom.data() + goff[i];
        const int ng = (int)((i + 1 < N ? goff[i + 1] : (long long)geom.size()) - goff[i]);
        const int nm = std::min(n_modes[i], ng);
        int first = -1, n_valid = 0;
        bool same = true;
        for (int m = 0; m < nm && same; ++m) {
            if (!g[m].valid) continue;
            if (first < 0) first = m;
            else same = same_ffat_geometry(g[first], g[m]);
            n_valid += 1;
        }
        if (!same || first < 0 || n_valid < 2) continue;          // (one map: nothing to share)
        const int pitch = (nm + 15) / 16 * 16;
        const size_t n_psi = (size_t)g[first].n_psi;
        t.shared[i].psit_off = (long long)t.psi_t.size();
        t.shared[i].pitch = pitch;
        t.shared[i].first_valid = first;
        t.psi_t.resize(t.psi_t.size() + n_psi * pitch, 0.0);
        double *dst = t.psi_t.data() + t.shared[i].psit_off;
        for (size_t c0 = 0; c0 < n_psi; c0 += 512)          // (blocks of cells: the strided writes of one block stay in cache)
            for (int m = 0; m < nm; ++m) {
                if (!g[m].valid) continue;
                const double *src = psi.data() + g[m].psi_off;
                for (size_t c = c0; c < std::min(n_psi, c0 + 512); ++c) dst[c * pitch + m] = src[c];
            }
        t.is_shared[i] = 1;
        t.n_shared += 1;
    }
    for (size_t j = 0; j < geom.size(); ++j) { t.mode_k[j] = geom[j].k; t.mode_valid[j] = geom[j].valid; }
    return t;
}

}  // namespace pbso
