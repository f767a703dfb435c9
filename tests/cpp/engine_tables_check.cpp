// Pins openpbso_amd/csrc/engine_tables.h and launch_policy.h -- what Engine::finalize computes (team tables, coefficient tables)
// and what a launch decides -- against their rules, written out here once more.  Host compiler only, AddressSanitizer + UBSan
// (make -C openpbso_amd/csrc engine_tables_check); tests/test_engine_tables.py builds and runs it.  Prints "engine tables check ok"
// and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "engine_tables.h"
#include "launch_policy.h"

using namespace pbso;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 40) std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static const int kModes[] = {1, 63, 64, 65, 200, 512, 1100, 2100, 4096};

// ---- team tables ---------------------------------------------------------------------------------------------------------
// the rules of a team table over objects of waves[i] waves, R modes per lane, at most cap[i] waves per team
static void check_table(const TeamTable &t, const std::vector<int> &waves, int R, const std::vector<int> &cap) {
    const int N = (int)waves.size();
    // classes: strictly descending in W, tiling the list; ids equal positions
    int next = 0, prev_w = 1 << 30, w_max = 1;
    for (const SizeClass &c : t.classes) {
        CHECK(c.W < prev_w && c.W >= 1 && c.count > 0 && c.first == next);
        prev_w = c.W;
        next += c.count;
        w_max = std::max(w_max, c.W);
    }
    CHECK(next == (int)t.teams.size());
    CHECK(t.w_max == w_max);
    std::vector<int> team_w(t.teams.size(), 0);
    for (const SizeClass &c : t.classes)
        for (int k = c.first; k < c.first + c.count && k < (int)t.teams.size(); ++k) team_w[k] = c.W;
    for (size_t k = 0; k < t.teams.size(); ++k) CHECK(t.teams[k].id == (int)k);
    // every object's columns [0, 64 R waves) covered exactly once, by teams in ascending col0; no team above its cap
    std::vector<std::vector<int>> of_obj(N);
    for (size_t k = 0; k < t.teams.size(); ++k) {
        CHECK(t.teams[k].obj >= 0 && t.teams[k].obj < N);
        if (t.teams[k].obj >= 0 && t.teams[k].obj < N) of_obj[t.teams[k].obj].push_back((int)k);
    }
    std::vector<int> split_of(N, -1);
    for (size_t s = 0; s < t.split.size(); ++s) {
        CHECK(t.split[s].obj >= 0 && t.split[s].obj < N && split_of[t.split[s].obj] < 0);
        split_of[t.split[s].obj] = (int)s;
    }
    std::vector<int> row_seen(t.n_part_rows, 0);
    for (int i = 0; i < N; ++i) {
        // (teams of one object and one size keep their order in the list; sort by col0 for the cover)
        std::vector<int> ks = of_obj[i];
        std::sort(ks.begin(), ks.end(), [&](int a, int b) { return t.teams[a].col0 < t.teams[b].col0; });
        int col = 0;
        for (int k : ks) {
            CHECK(t.teams[k].col0 == col);
            CHECK(team_w[k] >= 1 && team_w[k] <= cap[i]);
            col += 64 * R * team_w[k];
        }
        CHECK(col == 64 * R * waves[i]);
        // a SplitObj if and only if more than one team; its partial rows consecutive, in column order, counted once
        CHECK((split_of[i] >= 0) == (ks.size() > 1));
        if (ks.size() > 1 && split_of[i] >= 0) {
            const SplitObj &so = t.split[split_of[i]];
            CHECK(so.n_rows == (int)ks.size());
            for (size_t j = 0; j < ks.size(); ++j) {
                const int row = t.teams[ks[j]].part_row;
                CHECK(row == so.first_row + (int)j);
                if (row >= 0 && row < t.n_part_rows) row_seen[row] += 1;
                else CHECK(false);
            }
        } else if (ks.size() == 1) {
            CHECK(t.teams[ks[0]].part_row == -1);
        }
    }
    for (int r : row_seen) CHECK(r == 1);
}

// a team table as the loop finalize kept (three times) before there was one builder: the reference, entry for entry
static TeamTable table_by_hand(const std::vector<int> &waves, int R, const std::vector<int> &cap, int team_max) {
    TeamTable t;
    std::vector<std::vector<TeamDesc>> by_w(team_max + 1);
    for (int i = 0; i < (int)waves.size(); ++i) {
        const int w = waves[i], parts = (w + cap[i] - 1) / cap[i], base = w / parts, rem = w % parts;
        int w0 = 0;
        if (parts > 1) t.split.push_back(SplitObj{i, t.n_part_rows, parts, 0});
        for (int pi = 0; pi < parts; ++pi) {
            const int wp = base + (pi < rem ? 1 : 0);
            by_w[wp].push_back(TeamDesc{i, 64 * R * w0, parts > 1 ? t.n_part_rows++ : -1, 0});
            t.w_max = std::max(t.w_max, wp);
            w0 += wp;
        }
    }
    for (int w = team_max; w >= 1; --w) {
        if (by_w[w].empty()) continue;
        t.classes.push_back(SizeClass{w, (int)t.teams.size(), (int)by_w[w].size()});
        t.teams.insert(t.teams.end(), by_w[w].begin(), by_w[w].end());
    }
    for (size_t k = 0; k < t.teams.size(); ++k) t.teams[k].id = (int)k;
    return t;
}
static void check_same(const TeamTable &a, const TeamTable &b) {
    CHECK(a.n_part_rows == b.n_part_rows && a.w_max == b.w_max);
    CHECK(a.teams.size() == b.teams.size() && (a.teams.empty() || !std::memcmp(a.teams.data(), b.teams.data(), a.teams.size() * sizeof(TeamDesc))));
    CHECK(a.split.size() == b.split.size() && (a.split.empty() || !std::memcmp(a.split.data(), b.split.data(), a.split.size() * sizeof(SplitObj))));
    CHECK(a.classes.size() == b.classes.size() && (a.classes.empty() || !std::memcmp(a.classes.data(), b.classes.data(), a.classes.size() * sizeof(SizeClass))));
}

// the pipeline kernel's table as the loop that built it before there was one builder
static TeamTable pipe_table_by_hand(const std::vector<int> &n_modes) {
    TeamTable t;
    for (int i = 0; i < (int)n_modes.size(); ++i) {
        const int parts = std::max(1, (n_modes[i] + 63) / 64);
        if (parts > 1) t.split.push_back(SplitObj{i, t.n_part_rows, parts, 0});
        for (int c = 0; c < parts; ++c) t.teams.push_back(TeamDesc{i, 64 * c, parts > 1 ? t.n_part_rows++ : -1, (int)t.teams.size()});
    }
    return t;
}

static void team_tables() {
    std::vector<std::vector<int>> scenes;
    scenes.push_back(std::vector<int>(kModes, kModes + 9));                  // all sizes in one scene: several classes, several split objects
    for (int n : kModes) scenes.push_back(std::vector<int>(1, n));
    scenes.push_back(std::vector<int>(300, 512));                            // a scene the policy's own cap spreads over the chip
    scenes.push_back(std::vector<int>{4096, 4096, 64, 4096, 1});
    for (const std::vector<int> &n_modes : scenes) {
        for (int form = 0; form < 2; ++form) {                               // 0: block form, 1: per-sample form
            const int team_max = form == 0 ? MAX_WAVES_PER_BLOCK_TEAM : MAX_WAVES_PER_TEAM;
            const std::vector<int> Rs = form == 0 ? std::vector<int>{1, 2, 4} : std::vector<int>{1, 2, 3, 4, 8};
            for (int R : Rs) {
                const std::vector<int> waves = waves_per_object(n_modes, R);
                for (size_t i = 0; i < n_modes.size(); ++i) CHECK(waves[i] >= 1 && 64 * R * waves[i] >= n_modes[i] && 64 * R * (waves[i] - 1) < std::max(n_modes[i], 1));
                std::vector<int> caps = {1, 2, 4, 8, 16, engine_team_cap(total_waves(n_modes, R), 256, team_max, 0)};
                for (int c : caps) {
                    const int cap = std::min(c, team_max);
                    const std::vector<int> capv(n_modes.size(), cap);
                    const TeamTable t = build_team_table(waves, R, capv, MAX_WAVES_PER_TEAM);
                    check_table(t, waves, R, capv);
                    check_same(t, table_by_hand(waves, R, capv, MAX_WAVES_PER_TEAM));
                }
                CHECK(engine_team_cap(total_waves(n_modes, R), 256, team_max, 3) == 3 && engine_team_cap(1, 256, team_max, 99) == team_max);
            }
        }
        // the shapes of the time-chunked launches: 4-wave teams for one-mode-per-lane objects above 8 waves unless team_waves is set
        for (int R : {1, 2, 4})
            for (int team_waves : {0, 2, 8, 16}) {
                const TcShapeTable s = build_tc_shape(n_modes, R, team_waves);
                const std::vector<int> waves = waves_per_object(n_modes, R);
                std::vector<int> cap(waves.size());
                long long w_all = 0;
                for (size_t i = 0; i < waves.size(); ++i) {
                    cap[i] = team_waves > 0 ? std::min(8, team_waves) : (R == 1 && waves[i] > 8) ? 4 : 8;
                    w_all += waves[i];
                }
                check_table(s.table, waves, R, cap);
                check_same(s.table, table_by_hand(waves, R, cap, MAX_WAVES_PER_BLOCK_TEAM));
                CHECK(s.waves == w_all && s.cover == w_all * 64 * R);
                CHECK(R == 1 ? (s.waves_per_cu >= 1 && s.waves_per_cu <= 12) : s.waves_per_cu == 8);
            }
        // the pipeline kernel's table: the generic builder at R = 1, cap 1 == the loop it replaces, entry for entry
        const TeamTable g = build_team_table(waves_per_object(n_modes, 1), 1, std::vector<int>(n_modes.size(), 1), 1), p = build_pipe_table(n_modes);
        const TeamTable h = pipe_table_by_hand(n_modes);
        CHECK(g.teams.size() == h.teams.size() && g.split.size() == h.split.size() && g.n_part_rows == h.n_part_rows);
        CHECK(p.teams.size() == h.teams.size() && p.split.size() == h.split.size() && p.n_part_rows == h.n_part_rows);
        CHECK(g.classes.size() == 1 && g.classes[0].W == 1 && g.classes[0].first == 0 && g.classes[0].count == (int)g.teams.size());
        if (g.teams.size() == h.teams.size() && p.teams.size() == h.teams.size())
            CHECK(!std::memcmp(g.teams.data(), h.teams.data(), h.teams.size() * sizeof(TeamDesc)) &&
                  !std::memcmp(p.teams.data(), h.teams.data(), h.teams.size() * sizeof(TeamDesc)));
        if (g.split.size() == h.split.size() && p.split.size() == h.split.size() && !h.split.empty())
            CHECK(!std::memcmp(g.split.data(), h.split.data(), h.split.size() * sizeof(SplitObj)) &&
                  !std::memcmp(p.split.data(), h.split.data(), h.split.size() * sizeof(SplitObj)));
        CHECK(pipe_chunks(n_modes) == (long long)h.teams.size());
    }
    // the per-sample bank's team size by LDS: whatever the buffer length, the chosen team's request fits a CU's 160 KB and one more
    // wave would not (or is not allowed); 513 frames keep their 16 waves, 864 frames cannot
    for (int nt = 1; nt <= MAX_TILES; ++nt) {
        const int cap = iir_team_cap_by_lds(nt, MAX_WAVES_PER_TEAM);
        CHECK(cap >= 1 && cap <= MAX_WAVES_PER_TEAM);
        CHECK(iir_lds_bytes(cap, nt) <= 160 * 1024);
        CHECK(cap == MAX_WAVES_PER_TEAM || iir_lds_bytes(cap + 1, nt) > 160 * 1024);
        for (int tw : {0, 1, 3, 16, 99}) {                                   // whatever the caller asks for, and on a full chip
            const int c = engine_team_cap(1 << 20, 256, cap, tw);
            CHECK(c >= 1 && c <= cap && iir_lds_bytes(c, nt) <= 160 * 1024);
        }
        CHECK(iir_team_cap_by_lds(nt, 4) == 4);
    }
    CHECK(MAX_TILES == 32);
    CHECK(iir_team_cap_by_lds(19, MAX_WAVES_PER_TEAM) == 16);
    CHECK(iir_team_cap_by_lds(25, MAX_WAVES_PER_TEAM) == 16 && iir_team_cap_by_lds(26, MAX_WAVES_PER_TEAM) == 15);
    CHECK(iir_team_cap_by_lds(32, MAX_WAVES_PER_TEAM) == 14 && iir_lds_bytes(16, 32) == 175888);
    // the policy's modes per lane at 256 CUs: the fewest whose waves fit (8 per CU in the block form, 16 per sample)
    CHECK(choose_modes_per_lane(std::vector<int>(256, 512), true, 256) == 1);      // 2048 waves
    CHECK(choose_modes_per_lane(std::vector<int>(512, 512), true, 256) == 2);
    CHECK(choose_modes_per_lane(std::vector<int>(1024, 512), true, 256) == 4);
    CHECK(choose_modes_per_lane(std::vector<int>(3000, 512), true, 256) == 4);
    CHECK(choose_modes_per_lane(std::vector<int>(512, 512), false, 256) == 1);     // 4096 waves
    CHECK(choose_modes_per_lane(std::vector<int>(768, 512), false, 256) == 2);
}

// ---- coefficient tables ----------------------------------------------------------------------------------------------------
static int ulps_apart(float a, float b) {
    int32_t ia, ib;
    std::memcpy(&ia, &a, 4);
    std::memcpy(&ib, &b, 4);
    if (ia < 0) ia = (int32_t)0x80000000 - ia;
    if (ib < 0) ib = (int32_t)0x80000000 - ib;
    return ia > ib ? ia - ib : ib - ia;
}
struct M { double a, b, c, d; };
static M mul(const M &x, const M &y) { return M{x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d}; }

static void coefficient_tables() {
    // modes as a synthetic object has them: c1 = 2 eps cos(theta), c2 = -eps^2 (modal_integrator.h:95-96); eps the decay per
    // sample, theta the angle per sample: 100 Hz .. 18 kHz at 44.1 kHz, light and heavy damping
    const double eps[] = {0.99999, 0.9999, 0.9995, 0.999, 0.995, 0.98, 0.9997, 0.99995};
    const double theta[] = {0.014247585730565955, 0.06, 0.14247585730565955, 0.7, 1.4247585730565955, 2.5645654315018719, 0.3, 0.001};
    const int n = 8, m_pad = 256, B = 513;
    std::vector<double> c1(n), c2(n), c3(n, 1.0);
    for (int m = 0; m < n; ++m) { c1[m] = 2.0 * eps[m] * std::cos(theta[m]); c2[m] = -eps[m] * eps[m]; }
    const std::vector<ModeCoefs> objs = {ModeCoefs{c1.data(), c2.data(), c3.data(), n}, ModeCoefs{c1.data() + 3, c2.data() + 3, c3.data(), n - 3}};
    const size_t nm = objs.size() * (size_t)m_pad;
    std::vector<float> pc, wt;
    build_wp_tables(objs, m_pad, pc, wt);
    const std::vector<float> sc = build_scan_table(objs, m_pad, B), ft = build_f_table(objs, m_pad), gq = build_gq_table(objs, m_pad, B);
    CHECK(pc.size() == 4 * nm && wt.size() == nm / 2 * 64 && sc.size() == 6 * nm && ft.size() == 32 * nm && gq.size() == 3 * nm);
    int worst_scan = 0;
    for (size_t o = 0; o < objs.size(); ++o)
        for (int m = 0; m < objs[o].n_modes; ++m) {
            const double e = (1.0 - objs[o].c1[m]) - objs[o].c2[m], eps2 = -objs[o].c2[m];
            const M A = {1.0 - e, eps2, -e, eps2};
            const size_t k = o * m_pad + m;
            // P = A^16 by sixteen applications of the one-step matrix, and row 0 of every power: to the last bit
            M P = {1, 0, 0, 1};
            const float *w = wt.data() + (k / 2) * 64 + 16 * (2 * (k & 1));
            for (int j = 1; j <= 16; ++j) {
                P = mul(A, P);
                CHECK(w[j - 1] == (float)P.a && w[16 + j - 1] == (float)P.b);
            }
            CHECK(pc[k] == (float)(P.a - 1.0) && pc[nm + k] == (float)P.b && pc[2 * nm + k] == (float)P.c && pc[3 * nm + k] == (float)P.d);
            // the scan table's A^513 against (A^16)^32 A: another order of the same product of 513 factors.  Every fp64 product is
            // good to a few 2^-53 of the matrix' norm (<= 2.1: a decaying rotation in the (q, q - q_prev) basis), so the two orders
            // differ by < 1e-12 in every entry, five orders below the spacing of floats there: they round to the same float or, where
            // the value lies next to a rounding boundary, to two neighbours -- at most 1 ulp
            M Q = {1, 0, 0, 1};
            for (int j = 0; j < 32; ++j) Q = mul(P, Q);
            Q = mul(A, Q);
            const double want[4] = {Q.a - 1.0, Q.b, Q.c, Q.d};
            for (int c = 0; c < 4; ++c) {
                const float got = sc[c * nm + k];
                const int u = ulps_apart(got, (float)want[c]);
                worst_scan = std::max(worst_scan, u);
                CHECK(u <= 1);
            }
            // the F table: plane 2 i' + c holds component c of A^(15 - i') u, u = (1, 1)', to the last bit
            double v0 = 1.0, v1 = 1.0;
            for (int d = 0; d < 16; ++d) {
                CHECK(ft[(size_t)(2 * (15 - d)) * nm + k] == (float)v0 && ft[(size_t)(2 * (15 - d) + 1) * nm + k] == (float)v1);
                const double n0 = A.a * v0 + A.b * v1, n1 = A.c * v0 + A.d * v1;
                v0 = n0; v1 = n1;
            }
            // padding columns stay zero
            CHECK(pc[o * m_pad + objs[o].n_modes] == 0.f && sc[o * m_pad + m_pad - 1] == 0.f && ft[o * m_pad + objs[o].n_modes] == 0.f);
            // closed-form qnorm sums: G11 >= 1 (r_0 = e1), all finite
            CHECK(gq[k] >= 1.0f && std::isfinite(gq[k]) && std::isfinite(gq[nm + k]) && gq[2 * nm + k] >= 0.f);
        }
    std::printf("scan table against (A^16)^32 A: at most %d ulp\n", worst_scan);
    // bf16 hi + lo reconstructs x * TRUNC_SPLIT_GAIN to within 2^-16 relative, for every entry of the W table, at the place the
    // split table keeps it: rows 8 G + dd (hi) and 8 G + 4 + dd (lo), lane 16 kq + j, low half a_j, high half b_j
    std::vector<float> w16(wt);
    wtab_to_split_bf16(w16, nm);
    auto bf = [](uint32_t h) { const uint32_t u = h << 16; float f; std::memcpy(&f, &u, 4); return (double)f; };
    for (size_t col = 0; col < nm; ++col)
        for (int j = 0; j < 16; ++j)
            for (int comp = 0; comp < 2; ++comp) {
                const double x = (double)wt[(col / 2) * 64 + 16 * (2 * (col & 1) + comp) + j] * TRUNC_SPLIT_GAIN;
                const size_t G = col / 16, kq = (col % 16) / 4, dd = col % 4;
                uint32_t hi, lo;
                std::memcpy(&hi, &w16[(8 * G + dd) * 64 + 16 * kq + j], 4);
                std::memcpy(&lo, &w16[(8 * G + 4 + dd) * 64 + 16 * kq + j], 4);
                const double got = bf(comp ? hi >> 16 : hi & 0xFFFFu) + bf(comp ? lo >> 16 : lo & 0xFFFFu);
                CHECK(std::fabs(got - x) <= std::ldexp(std::fabs(x), -16));
            }
}

// ---- the launch policy at 256 CUs ------------------------------------------------------------------------------------------------
// an engine of n_obj objects of 512 modes as finalize sets it up (f32 block form, every default), a launch of nb buffers
static bool cut_in_time(int n_obj, int nb, int n_dense_rows, int tc_mode, int *shape = nullptr) {
    const std::vector<int> n_modes(n_obj, 512);
    PolicyScene sc;
    sc.n_obj = n_obj;
    sc.m_pad = 512;
    sc.n_cus = 256;
    const int Rs[3] = {1, 2, 4};
    for (int k = 0; k < 3; ++k) {
        const TcShapeTable s = build_tc_shape(n_modes, Rs[k], 0);
        sc.shape[k] = PolicyShape{s.waves, s.cover, s.waves_per_cu};
    }
    sc.pipe_teams = (int)pipe_chunks(n_modes);
    PolicySettings s;
    std::memset(&s, 0, sizeof(s));
    s.block = true;
    s.tc_ok = tc_mode >= 0;
    s.have_scan = s.tc_ok;
    s.have_ftab = s.ftab_forced = true;
    s.use_split = choose_modes_per_lane(n_modes, true, 256) == 1 && pipe_chunks(n_modes) <= 2 * 256;
    s.device_profiles = s.sync_values = true;
    s.tc_mode = tc_mode;
    const PolicyLaunch l = {nb, n_dense_rows, true};
    int set = -1, cb = 0;
    const bool tc = s.block && !s.split_always && choose_time_chunks(sc, s, l, &set, &cb);
    if (tc) {
        CHECK(set >= 0 && set < 3 && cb >= 1 && cb < nb && (nb + cb - 1) / cb >= 2);
        if (shape) *shape = Rs[set];
        CHECK(bank_kind(sc, s, l, tc) == BankKind::TimeChunked && !split_launch(sc, s, l, tc));
    }
    return tc;
}
static void policy() {
    // tests/test_gpu_time_chunks.py: 1 x 512 x 86 runs time-chunked, the same engine stepping ONE buffer does not, an engine pinned to
    // the walk never does, twelve buffers of sustained scraping are cut too, with one mode per lane
    CHECK(cut_in_time(1, 86, 0, 0));
    CHECK(!cut_in_time(1, 1, 0, 0));
    CHECK(!cut_in_time(1, 86, 0, -1));
    int shape = 0;
    CHECK(cut_in_time(1, 12, 12, 0, &shape) && shape == 1);
    // ... a scene that fills the chip exactly keeps the walk; 1100 / 1536 / 2048 x 512 are cut, 3000 x 512 is not
    CHECK(!cut_in_time(1024, 86, 0, 0));
    CHECK(cut_in_time(1100, 86, 0, 0));
    CHECK(cut_in_time(1536, 86, 0, 0));
    CHECK(cut_in_time(2048, 86, 0, 0));
    CHECK(!cut_in_time(3000, 86, 0, 0));
    // the start gate by policy from 256 buffers on, the value hand-over below; never on the bank's own stream
    PolicySettings s;
    std::memset(&s, 0, sizeof(s));
    s.sync_values = true;
    CHECK(!gate_now(s, PolicyLaunch{128, 0, true}, false, true) && gate_now(s, PolicyLaunch{256, 0, true}, false, true));
    CHECK(!gate_now(s, PolicyLaunch{300, 0, true}, false, false) && !gate_now(s, PolicyLaunch{300, 0, true}, true, true));
    CHECK(value_handover(s, PolicyLaunch{128, 0, true}) && !value_handover(s, PolicyLaunch{256, 0, true}));
    s.stream_sync = 3;
    CHECK(gate_now(s, PolicyLaunch{1, 0, true}, false, true));
}

int main() {
    team_tables();
    coefficient_tables();
    policy();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("engine tables check ok\n");
    return 0;
}
