// The EQ bus's schedule on the host compiler alone (openpbso_amd/csrc/eq_schedule.h; built by `make eq_schedule_check` under
// AddressSanitizer + UBSan and run by tests/test_eq_schedule_abi.py): the spacing rule and the smallest next t_set, the per-step limit,
// the block lists against a per-sample labelling (origins, cut lengths, the pair positions at k = 0, 1, P - 2 and P - 1, the tails),
// and -- by walking the plan sample by sample exactly as the kernels of kernels_eq_schedule.hip do, in fp64 on the host -- the
// values and the history sources against the definition: the same input cut at every t_set with a plain set before each piece.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "eq_schedule.h"

using namespace pbso;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            if (++failures > 20) std::exit(1);                            \
        }                                                                 \
    } while (0)

static const int P = EQ_BLOCK, H = EQ_HIST;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static double urand() { return (double)rnd() / 2147483648.0 - 0.5; }

// ---- the definition: cascades on their own grids, stepped in pieces -------------------------------------------------------------
struct Casc {
    std::vector<double> tab;                             // [S][5][P]
    long long t_set = 0;
    std::vector<double> hist;                            // [S + 1][H]
};

static void block_section(const double *tab, long k0, long n, const double *x, double *y) {
    const double *h = tab, *r = tab + P, *s = tab + 2 * P, *p = tab + 3 * P, *q = tab + 4 * P;
    for (long i = 0; i < n; ++i) {
        const long k = (k0 + i) % P, o = H + i - k;
        double acc = 0.0;
        for (long j = k; j >= 0; --j) acc = std::fma(h[j], x[o + k - j], acc);
        acc = std::fma(r[k], x[o - 1], acc);
        acc = std::fma(s[k], x[o - 2], acc);
        acc = std::fma(q[k], y[o - 2], acc);
        acc = std::fma(p[k], y[o - 1], acc);
        y[H + i] = acc;
    }
}

static void run(Casc &c, int S, const float *u, long n, long long t, std::vector<double> &out) {
    const long k0 = (long)((t - c.t_set) % P);
    std::vector<double> x((size_t)H + n), y((size_t)H + n);
    for (int i = 0; i < H; ++i) x[i] = c.hist[i];
    for (long i = 0; i < n; ++i) x[H + i] = (double)u[i];
    for (int i = 0; i < H; ++i) c.hist[i] = x[n + i];
    for (int s = 0; s < S; ++s) {
        for (int i = 0; i < H; ++i) y[i] = c.hist[(size_t)(s + 1) * H + i];
        block_section(c.tab.data() + (size_t)s * 5 * P, k0, n, x.data(), y.data());
        for (int i = 0; i < H; ++i) c.hist[(size_t)(s + 1) * H + i] = y[n + i];
        x = y;
    }
    out.assign(x.begin() + H, x.end());
}

struct State {                                           // what the stage keeps between steps, and the definition's model alike
    int S = 1, R = 0;
    long long t = 0;
    Casc to, from;
    bool have_from = false;
    bool fading() const { return have_from && t - to.t_set + 1 < R; }
};

static std::vector<double> tables_of(const double *sos, int S) {
    std::vector<double> tab((size_t)S * 5 * P);
    for (int s = 0; s < S; ++s) eq_tables(sos + 5 * s, tab.data() + (size_t)s * 5 * P);
    return tab;
}

static void init(State &m, int S, int R) {
    m.S = S;
    m.R = R;
    m.t = 0;
    std::vector<double> id((size_t)S * 5, 0.0);
    for (int s = 0; s < S; ++s) id[5 * s] = 1.0;
    m.to.tab = tables_of(id.data(), S);
    m.to.t_set = 0;
    m.to.hist.assign((size_t)(S + 1) * H, 0.0);
    m.from = m.to;
    m.have_from = false;
}

// a plain set at m.t, then n samples
static void plain_piece(State &m, const double *sos, const float *u, long n, float *out) {
    if (sos) {
        CHECK(!m.fading());
        m.from = m.to;
        m.to.tab = tables_of(sos, m.S);
        m.to.t_set = m.t;
        m.have_from = true;
    }
    if (n == 0) return;
    const long n_fade = m.fading() ? (long)std::min<long long>(n, m.to.t_set + m.R - 1 - m.t) : 0;
    std::vector<double> yt, yf;
    run(m.to, m.S, u, n, m.t, yt);
    if (n_fade) run(m.from, m.S, u, n_fade, m.t, yf);
    for (long i = 0; i < n; ++i) {
        float v = (float)yt[i];
        if (i < n_fade) {
            const float f = (float)yf[i], w = (float)((double)(m.t + i - m.to.t_set + 1) / (double)m.R), d = v - f, wd = w * d;
            v = f + wd;
        }
        out[i] = v;
    }
    m.t += n;
}

// ---- the plan, walked as the kernels walk it --------------------------------------------------------------------------------------
static int segment_of(const EqPlan &p, int K, int i) {
    int g = 1;
    for (int j = 1; j <= 1 + K; ++j)
        if (p.seg[j].s <= i) g = j;
    return g;
}

static void scheduled_step(State &m, int K, const long long *ts, const double *sos, const float *u, long n, float *out) {
    const int S = m.S, N = (int)(H + n);
    EqPlan p;
    eq_plan(m.t, n, m.R, 0, m.to.t_set, m.from.t_set, m.have_from, K, ts, p);
    std::vector<std::vector<double>> tabs;               // by table id
    tabs.push_back(m.to.tab);
    tabs.push_back(m.from.tab);
    for (int j = 0; j < K; ++j) tabs.push_back(tables_of(sos + (size_t)j * S * 5, S));
    std::vector<double> v[2], f[2], wv(N, NAN), wf(N, NAN);
    for (int a = 0; a < 2; ++a) {
        v[a].assign(N, NAN);
        f[a].assign(N, NAN);
    }
    Casc next_to, next_from;
    next_to.hist.assign((size_t)(S + 1) * H, NAN);
    next_from.hist.assign((size_t)(S + 1) * H, NAN);
    for (int i = 0; i < N; ++i) v[0][i] = i < H ? m.to.hist[i] : (double)u[i - H];
    auto hist_of = [&](int s, const std::vector<double> &vx, const std::vector<double> &fx) {
        for (int k = 0; k < H; ++k) {
            const int i = (int)n + k;
            next_to.hist[(size_t)s * H + k] = vx[i];
            if (p.from_hist) next_from.hist[(size_t)s * H + k] = i < p.vs_last ? vx[i] : fx[i];
        }
    };
    for (int s = 0; s < S; ++s) {
        const std::vector<double> &vx = v[s & 1], &fx = s ? f[s & 1] : v[0];
        std::vector<double> &vy = v[(s + 1) & 1], &fy = f[(s + 1) & 1];
        std::fill(vy.begin(), vy.end(), NAN);
        std::fill(fy.begin(), fy.end(), NAN);
        for (int k = 0; k < H; ++k) {
            vy[k] = m.to.hist[(size_t)(s + 1) * H + k];
            fy[k] = m.from.hist[(size_t)(s + 1) * H + k];
        }
        hist_of(s, vx, fx);
        // forward
        for (int i = H; i < N; ++i) {
            const int g = segment_of(p, K, i);
            const EqSeg &sg = p.seg[g];
            {
                const int o = sg.a + (i - sg.a) / P * P, k = i - o;
                const double *t = tabs[sg.tab].data() + (size_t)s * 5 * P;
                double acc = 0.0;
                for (int j = k; j >= 0; --j) acc = std::fma(t[j], vx[i - j], acc);
                acc = std::fma(t[P + k], vx[o - 1], acc);
                acc = std::fma(t[2 * P + k], vx[o - 2], acc);
                wv[i] = acc;
            }
            if (i < sg.fe) {
                const EqSeg &fr = p.seg[g - 1];
                const int o = fr.a + (i - fr.a) / P * P, k = i - o;
                const double *t = tabs[fr.tab].data() + (size_t)s * 5 * P;
                auto x = [&](int q) { return q < sg.vs ? vx[q] : fx[q]; };
                double acc = 0.0;
                for (int j = k; j >= 0; --j) acc = std::fma(t[j], x(i - j), acc);
                acc = std::fma(t[P + k], x(o - 1), acc);
                acc = std::fma(t[2 * P + k], x(o - 2), acc);
                wf[i] = acc;
            }
        }
        // chain
        double y1 = NAN, y2 = NAN;
        for (int list = 0; list < 2; ++list) {
            const std::vector<EqBlk> &blk = list ? p.fblk : p.vblk;
            const std::vector<double> &w = list ? wf : wv;
            std::vector<double> &yo = list ? fy : vy;
            for (const EqBlk &k : blk) {
                const double *t = tabs[k.tab].data() + (size_t)s * 5 * P;
                auto stored = [&](int q) { return q < k.vs ? vy[q] : fy[q]; };
                if (k.flags & EQ_BLK_RESET) {
                    y1 = stored(k.o - 1);
                    y2 = stored(k.o - 2);
                }
                const int ia = k.o + k.L - 2, ib = ia + 1;
                double na;
                if (k.L == 1) na = y1;
                else if (ia < k.lo) na = stored(ia);
                else {
                    na = std::fma(t[3 * P + k.L - 2], y1, std::fma(t[4 * P + k.L - 2], y2, w[ia]));
                    yo[ia] = na;
                }
                const double nb = std::fma(t[3 * P + k.L - 1], y1, std::fma(t[4 * P + k.L - 1], y2, w[ib]));
                yo[ib] = nb;
                y2 = na;
                y1 = nb;
            }
        }
        // finish
        for (int i = H; i < N; ++i) {
            const int g = segment_of(p, K, i);
            const EqSeg &sg = p.seg[g];
            {
                const int e = g < 1 + K ? p.seg[g + 1].s : N;
                const int o = sg.a + (i - sg.a) / P * P, k = i - o, L = e - o < P ? e - o : P;
                const double *t = tabs[sg.tab].data() + (size_t)s * 5 * P;
                if (k < L - 2) vy[i] = std::fma(t[3 * P + k], vy[o - 1], std::fma(t[4 * P + k], vy[o - 2], wv[i]));
            }
            if (i < sg.fe) {
                const EqSeg &fr = p.seg[g - 1];
                const int o = fr.a + (i - fr.a) / P * P, k = i - o, L = sg.fe - o < P ? sg.fe - o : P;
                const double *t = tabs[fr.tab].data() + (size_t)s * 5 * P;
                if (k < L - 2) {
                    const double a1 = o - 1 < sg.vs ? vy[o - 1] : fy[o - 1], a2 = o - 2 < sg.vs ? vy[o - 2] : fy[o - 2];
                    fy[i] = std::fma(t[3 * P + k], a1, std::fma(t[4 * P + k], a2, wf[i]));
                }
            }
        }
    }
    const std::vector<double> &vy = v[S & 1], &fy = f[S & 1];
    hist_of(S, vy, fy);
    for (int i = H; i < N; ++i) {
        const EqSeg &sg = p.seg[segment_of(p, K, i)];
        float o = (float)vy[i];
        if (i < sg.fe) {
            const float yf = (float)fy[i], w = (float)((double)(sg.d0 + (i - sg.s)) / (double)m.R), d = o - yf, wd = w * d;
            o = yf + wd;
        }
        out[i - H] = o;
    }
    // the stage behind the step, as eq.cpp leaves it
    const long long t_from2 = K >= 2 ? ts[K - 2] : m.to.t_set;
    std::vector<double> tab_from2 = K >= 2 ? tabs[2 + K - 2] : m.to.tab;
    m.to.tab = tabs[2 + K - 1];
    m.to.t_set = ts[K - 1];
    m.to.hist = next_to.hist;
    m.from.tab = tab_from2;
    m.from.t_set = t_from2;
    m.from.hist = next_from.hist;                        // NaN where the plan says it is not needed
    m.have_from = true;
    m.t += n;
}

static bool same(const void *a, const void *b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }

// A run: steps of the given lengths, sets at the given samples; the stage (scheduled steps where sets fall inside) against the model
// (cut at every set).
static void scenario(const char *name, int S, int R, const std::vector<long> &steps, const std::vector<long long> &sets) {
    long total = 0;
    for (long s : steps) total += s;
    std::vector<float> u(total);
    for (float &x : u) x = (float)(urand() * 0.5);
    std::vector<double> sos(sets.size() * S * 5);
    for (size_t i = 0; i < sets.size() * S; ++i) {
        const double a2 = 0.9 * urand() + 0.3, a1 = (1.0 + a2) * 1.8 * urand();
        double *c = sos.data() + 5 * i;
        c[0] = 1.0 + urand();
        c[1] = urand();
        c[2] = urand();
        c[3] = a1;
        c[4] = a2;
        CHECK(eq_refusal(c, 1) == nullptr);
    }
    for (size_t i = 0; i + 1 < sets.size(); ++i) CHECK(sets[i + 1] > sets[i] && eq_spacing_ok(sets[i + 1], sets[i], R));
    // the model
    State ref;
    init(ref, S, R);
    std::vector<float> want(total);
    {
        size_t k = 0;
        long at = 0;
        while (at < total) {
            const double *c = nullptr;
            if (k < sets.size() && sets[k] == at) c = sos.data() + (k++) * S * 5;
            const long end = k < sets.size() && sets[k] < total ? (long)sets[k] : total;
            plain_piece(ref, c, u.data() + at, end - at, want.data() + at);
            at = end;
        }
    }
    // the stage
    State st;
    init(st, S, R);
    std::vector<float> got(total);
    size_t k = 0;
    long at = 0;
    for (long n : steps) {
        int K = 0;
        while (k + K < sets.size() && sets[k + K] < at + n) ++K;
        CHECK(K == eq_sets_in_step(sets.data() + k, (int)(sets.size() - k), at, n));
        if (K) scheduled_step(st, K, sets.data() + k, sos.data() + k * S * 5, u.data() + at, n, got.data() + at);
        else plain_piece(st, nullptr, u.data() + at, n, got.data() + at);
        k += K;
        at += n;
    }
    const bool ok = same(got.data(), want.data(), total * sizeof(float));
    if (!ok) {
        long i = 0;
        while (i < total && same(&got[i], &want[i], sizeof(float))) ++i;
        std::printf("FAIL scenario %s: first difference at sample %ld of %ld\n", name, i, total);
        ++failures;
    }
    // the histories behind the run: To's always, From's while a fade runs
    CHECK(st.t == ref.t && st.to.t_set == ref.to.t_set);
    const bool h_to = same(st.to.hist.data(), ref.to.hist.data(), st.to.hist.size() * sizeof(double));
    CHECK(h_to);
    if (ref.fading()) {
        CHECK(st.fading() && st.from.t_set == ref.from.t_set);
        const bool h_from = same(st.from.hist.data(), ref.from.hist.data(), st.from.hist.size() * sizeof(double));
        CHECK(h_from);
    }
    std::printf("scenario %s S=%d R=%d steps=%zu sets=%zu %s\n", name, S, R, steps.size(), sets.size(), ok && h_to ? "ok" : "FAILED");
}

// the block lists against a per-sample labelling
static void structure(long long t, long n, int R, long long t_to, long long t_from, bool have_from, const std::vector<long long> &ts) {
    const int K = (int)ts.size(), N = (int)(H + n);
    EqPlan p;
    eq_plan(t, n, R, 0, t_to, t_from, have_from, K, ts.data(), p);
    CHECK((int)p.seg.size() == 2 + K);
    // label every sample of the step: the set in force and its block origin
    std::vector<int> set_of(N, -1), origin(N, 0);
    for (int i = H; i < N; ++i) {
        const long long ta = t + (i - H);
        int g = 0;
        long long ts_g = t_to;
        for (int j = 0; j < K; ++j)
            if (ts[j] <= ta) {
                g = 1 + j;
                ts_g = ts[j];
            }
        set_of[i] = g;
        origin[i] = (int)(i - (ta - ts_g) % P);
    }
    // V: the blocks tile [first origin, N) in order; each holds samples of one set and one origin, and ends at a cut or at P
    int at = -1;
    std::vector<char> seen(N, 0);
    for (size_t b = 0; b < p.vblk.size(); ++b) {
        const EqBlk &k = p.vblk[b];
        CHECK(k.L >= 1 && k.L <= P && k.o + k.L <= N && k.o + k.L - 1 >= H && k.o >= 3);
        CHECK(((k.flags & EQ_BLK_RESET) != 0) == (b == 0) && !(k.flags & EQ_BLK_F) && k.lo == H);
        if (b) CHECK(k.o == at);
        at = k.o + k.L;
        for (int i = std::max(k.o, H); i < k.o + k.L; ++i) {
            CHECK(!seen[i] && origin[i] == k.o && p.seg[1 + set_of[i]].tab == k.tab);
            seen[i] = 1;
        }
        // cut exactly where the next set begins, where the step ends, or whole
        const int end = k.o + k.L;
        CHECK(k.L == P || end == N || (end < N && set_of[end] != set_of[end - 1]));
    }
    CHECK(at == N);
    for (int i = H; i < N; ++i) CHECK(seen[i]);
    // the tails: for every set, R - 1 samples of its predecessor on the predecessor's grid (the first: of the cascade fading out)
    std::vector<char> in_tail(N, 0);
    size_t b = 0;
    for (int g = 0; g <= K; ++g) {
        const long long ts_g = g ? ts[g - 1] : t_to, ts_prev = g >= 2 ? ts[g - 2] : g == 1 ? t_to : t_from;
        if (R < 2 || (g == 0 && !have_from)) continue;
        const long long lo = std::max(ts_g, t), hi = std::min<long long>(ts_g + R - 1, t + n);
        if (hi <= lo) continue;
        bool first = true;
        for (long long ta = lo; ta < hi;) {
            CHECK(b < p.fblk.size());
            if (b >= p.fblk.size()) return;
            const EqBlk &k = p.fblk[b++];
            const int i = (int)(H + (ta - t)), o = (int)(i - (ta - ts_prev) % P);
            CHECK(k.o == o && (k.flags & EQ_BLK_F) && ((k.flags & EQ_BLK_RESET) != 0) == first);
            CHECK(k.o + k.L == std::min<long long>(o + P, H + (hi - t)));
            CHECK(k.lo == (int)(H + (lo - t)) && k.vs == (g ? k.lo : 0));
            CHECK(k.tab == (g >= 2 ? 2 + g - 2 : g == 1 ? 0 : 1));
            CHECK(k.o + k.L - 1 >= k.lo);               // the last sample of a tail block is always the tail's own
            for (int q = i; q < k.o + k.L; ++q) in_tail[q] = 1;
            ta = t + (k.o + k.L - H);
            first = false;
        }
    }
    CHECK(b == p.fblk.size());
    for (int i = H; i < N; ++i) {
        const EqSeg &sg = p.seg[1 + set_of[i]];
        CHECK((i < sg.fe) == (in_tail[i] != 0));
        const long long ts_g = set_of[i] ? ts[set_of[i] - 1] : t_to;
        if (i < sg.fe) CHECK(sg.d0 + (i - sg.s) == t + (i - H) - ts_g + 1);
    }
    // From's history: needed exactly while the fade of the last set runs past the step
    const long long ts_last = K ? ts[K - 1] : t_to;
    const bool fading_after = R >= 2 && (K > 0 || have_from) && (t + n) - ts_last + 1 < R;
    CHECK((p.from_hist != 0) == fading_after);
    if (K) CHECK(p.vs_last == (int)(H + (ts_last - t)));
}

int main() {
    // the spacing rule and the smallest next t_set
    CHECK(eq_spacing_ok(5, 5, 0) && eq_spacing_ok(5, 5, 1) && eq_spacing_ok(6, 5, 2) && !eq_spacing_ok(5, 4, 3) && eq_spacing_ok(6, 4, 3));
    CHECK(eq_spacing_ok(63, 0, 64) && !eq_spacing_ok(62, 0, 64) && eq_spacing_ok(1199, 1000, 200) && !eq_spacing_ok(1198, 1000, 200));
    for (int R : {0, 1, 2, 3, 64, 67, 200})
        for (long long t_prev : {0ll, 5ll, 1000ll})
            for (long long t_next : {0ll, 5ll, 1000ll, 1300ll})
                for (int pend = 0; pend < 2; ++pend) {
                    if (!pend && t_prev > t_next) continue;
                    const long long m = eq_next_t_min(t_next, pend != 0, t_prev, R);
                    long long brute = t_next;            // the first t_set >= t_next that passes every rule
                    while (!((!pend || brute > t_prev) && eq_spacing_ok(brute, t_prev, R))) ++brute;
                    CHECK(m == brute);
                }
    // the identity of enable / reset is a predecessor at 0
    CHECK(eq_next_t_min(0, false, 0, 64) == 63 && eq_next_t_min(0, false, 0, 1) == 0 && eq_next_t_min(0, false, 0, 2) == 1);
    // the per-step limit
    {
        std::vector<long long> ts(EQ_MAX_SETS_PER_STEP + 1);
        for (size_t i = 0; i < ts.size(); ++i) ts[i] = 10 + (long long)i;
        CHECK(eq_sets_in_step(ts.data(), (int)ts.size(), 0, 10) == 0 && eq_sets_in_step(ts.data(), (int)ts.size(), 0, 11) == 1);
        CHECK(eq_sets_in_step(ts.data(), (int)ts.size(), 10, 4096) == EQ_MAX_SETS_PER_STEP);
        CHECK(eq_sets_in_step(ts.data(), (int)ts.size(), 10, 4097) > EQ_MAX_SETS_PER_STEP);
        CHECK(EQ_MAX_SETS_PER_STEP == 4096 && EQ_MAX_PENDING == 65536);
    }
    // the pair positions of a block cut at k = 0, 1, P - 2, P - 1 (and whole): set 0 in force since 0, a set at offset k of its block
    for (int k : {0, 1, 2, P - 2, P - 1}) {
        const long long t = 3 * P, ts = 5 * P + k;
        EqPlan p;
        eq_plan(t, 4 * P, 0, 0, 0, 0, false, 1, &ts, p);
        const int cut = (int)(H + (ts - t));
        size_t b = 0;
        while (b < p.vblk.size() && p.vblk[b].o + p.vblk[b].L < cut) ++b;
        CHECK(b + 1 < p.vblk.size() && p.vblk[b].o + p.vblk[b].L == cut && p.vblk[b + 1].o == cut && p.vblk[b + 1].tab == 2);
        CHECK(p.vblk[b].L == (k ? k : P));              // k = 0: the block before is whole, its pair is the origin pair of the new set
        CHECK(p.vblk[b].o == cut - (k ? k : P) && p.vblk[b].tab == 0);
        std::printf("cut at k=%d: block o=%d L=%d pair at %d %d\n", k, p.vblk[b].o, p.vblk[b].L, p.vblk[b].o + p.vblk[b].L - 2,
                    p.vblk[b].o + p.vblk[b].L - 1);
    }
    // structure: every predecessor offset, every R, the hazards
    for (int R : {0, 1, 2, 3, 64, 67, 200}) {
        for (int off = 0; off < P; ++off) structure(1000, 513, R, 1000 - 300 - off, 0, false, {1000 + 100});
        for (int off = 0; off < P; ++off) structure(1000, 513, R, 1000 - 300, 0, false, {1000 + 100 + off, 1000 + 100 + off + std::max(R - 1, 1)});
        structure(1000, 27, R, std::min(998, 1026 - (R - 1) - 3), 100, true, {1000 + 26});    // n < EQ_HIST, a fade into the step
        structure(1000, 27, R, 998, 700, true, {});
        structure(1000, 513, R, 998, 700, true, {1000 + 512});
        structure(1000, 513, R, 400, 100, true, {1000});
        for (int d = -1; d <= 1; ++d) {                  // a tail that ends at, one before and one after the step end
            const long long ts = 1000 + 513 - (R - 1) + d;
            if (R >= 2 && ts >= 1000 && ts < 1513) structure(1000, 513, R, 400, 100, true, {ts});
        }
        if (R <= 2) {
            std::vector<long long> run70;
            for (int d = -1; d <= 1; ++d) {
                run70.clear();
                for (int j = 0; j < 70; ++j) run70.push_back(1000 + 513 - 70 + j + d - (d > 0 ? 1 : 0) * 0);
                while (!run70.empty() && run70.back() >= 1513) run70.pop_back();
                structure(1000, 513, R, 400, 100, true, run70);
            }
        }
    }
    // values and histories
    for (int R : {0, 1, 2, 3, 64, 67, 200}) {
        const long long r1 = std::max(R - 1, 1);
        scenario("one set mid-step", 2, R, {513, 513}, {700});
        scenario("first and last sample", 2, R, {513, 513, 513}, {513, 513 + 512});
        scenario("spacing R-1", 2, R, {300, 1500}, {400, 400 + r1, 400 + 2 * r1, 400 + 3 * r1});
        scenario("27 frames", 2, R, {27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27, 27}, {30, 30 + r1, 30 + 2 * r1 + 5, 30 + 3 * r1 + 40});
        scenario("set then plain steps", 1, R, {100, 27, 27, 300}, {64});
        for (int d = -1; d <= 1; ++d) scenario("tail at the step end", 2, R, {513, 200}, {513 - r1 + d > 0 ? 513 - r1 + d : 1});
        for (int off : {0, 1, 2, 31, 62, 63}) scenario("predecessor offset", 2, R, {1200}, {200, 200 + 3 * P + 200 + off});
        if (R <= 2)
            for (int d = -1; d <= 1; ++d) {
                std::vector<long long> sets;
                for (int j = 0; j < 70; ++j) sets.push_back(513 - 70 + j + d);
                scenario("70 one-sample sets at a step end", 2, R, {513, 513, 100}, sets);
            }
        // random
        for (int rep = 0; rep < 6; ++rep) {
            std::vector<long> steps;
            std::vector<long long> sets;
            long total = 0;
            for (int i = 0; i < 5; ++i) {
                steps.push_back(rep % 2 ? 27 * (1 + rnd() % 4) : 1 + rnd() % 700);
                total += steps.back();
            }
            long long ts = rnd() % 100;
            while (ts < total) {
                sets.push_back(ts);
                ts += r1 + (rnd() % 3 == 0 ? 0 : rnd() % 200);
            }
            scenario("random", 1 + rep % 3, R, steps, sets);
        }
    }
    if (failures) {
        std::printf("eq_schedule_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("eq_schedule_check: all ok\n");
    return 0;
}
