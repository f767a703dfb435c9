/* The master bus of include/openpbso_amd.h, literally: v [C][HL + n] holds v_c(t0 - HL) .. v_c(t0 + n - 1), HL = 2 L + H (the
 * history, zero before t = 0, in front of the step with the gain applied); w the L taps.  Writes y [C][n], g [n], and counts the
 * samples whose chain ended above 1.f.  Compile with -ffp-contract=off.
 *
 * Two entries with one signature.  master_ref_literal takes the sliding minimum a(t) by the header's double loop, O(N W);
 * master_ref takes it in O(N) by block prefix and suffix minima (van Herk / Gil-Werman).  fminf over values in [0, 1] without a
 * NaN is exact and does not depend on the order, so the two give the same bits: tests/test_master_model.py holds them to that.
 * Everything behind the minimum (the one fmaf chain, the fminf with r(t - L), the clamp) is the same literal code in both. */
#include <math.h>
#include <stdlib.h>

/* a(e) = min r[e - (W - 1) .. e] for e >= W - 1, the header's loop */
static void minimum_literal(const float *r, long N, long W, float *a) {
    for (long e = W - 1; e < N; ++e) {
        float m = 1.f;
        for (long j = 0; j < W; ++j) m = fminf(m, r[e - j]);
        a[e] = m;
    }
}

/* the same in O(N): with the axis cut into blocks of W, p(e) = min r[block start .. e] and s(e) = min r[e .. block end]; a window
 * of W samples that ends at e lies in at most two neighbouring blocks and is s(e - W + 1) joined with p(e) */
static void minimum_linear(const float *r, long N, long W, float *a) {
    float *p = malloc(sizeof(float) * N), *s = malloc(sizeof(float) * N);
    for (long e = 0; e < N; ++e) p[e] = e % W == 0 ? fminf(1.f, r[e]) : fminf(p[e - 1], r[e]);
    for (long e = N - 1; e >= 0; --e) s[e] = e == N - 1 || (e + 1) % W == 0 ? fminf(1.f, r[e]) : fminf(s[e + 1], r[e]);
    for (long e = W - 1; e < N; ++e) a[e] = fminf(s[e - W + 1], p[e]);
    free(p);
    free(s);
}

static void master(const float *v, int C, long n, int L, int H, float T, const float *w, float *y, float *g, long *n_acc_above_one,
                   void (*minimum)(const float *, long, long, float *)) {
    const long HL = 2L * L + H, N = HL + n;
    float *r = malloc(sizeof(float) * N), *a = malloc(sizeof(float) * N);
    *n_acc_above_one = 0;
    for (long e = 0; e < N; ++e) {
        float pk = 0.f;
        for (int c = 0; c < C; ++c) pk = fmaxf(pk, fabsf(v[c * N + e]));
        r[e] = pk > T ? T / pk : 1.f;
    }
    minimum(r, N, (long)L + H + 1, a);                   /* (g reads a(t - k), k < L, t >= t0: index HL - (L - 1) = L + H + 1 on) */
    for (long q = 0; q < n; ++q) {
        const long e = HL + q;
        float acc = 0.f;
        for (int k = L - 1; k >= 0; --k) acc = fmaf(w[k], a[e - k], acc);
        if (acc > 1.f) ++*n_acc_above_one;
        g[q] = fminf(acc, r[e - L]);
        for (int c = 0; c < C; ++c) y[c * n + q] = fminf(fmaxf(v[c * N + e - L] * g[q], -T), T);
    }
    free(r);
    free(a);
}

void master_ref(const float *v, int C, long n, int L, int H, float T, const float *w, float *y, float *g, long *n_acc_above_one) {
    master(v, C, n, L, H, T, w, y, g, n_acc_above_one, minimum_linear);
}

void master_ref_literal(const float *v, int C, long n, int L, int H, float T, const float *w, float *y, float *g,
                        long *n_acc_above_one) {
    master(v, C, n, L, H, T, w, y, g, n_acc_above_one, minimum_literal);
}
