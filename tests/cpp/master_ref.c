/* The master bus of include/openpbso_amd.h, literally: v [C][HL + n] holds v_c(t0 - HL) .. v_c(t0 + n - 1), HL = 2 L + H (the
 * history, zero before t = 0, in front of the step with the gain applied); w the L taps.  Writes y [C][n], g [n], and counts the
 * samples whose chain ended above 1.f.  Compile with -ffp-contract=off. */
#include <math.h>
#include <stdlib.h>

void master_ref(const float *v, int C, long n, int L, int H, float T, const float *w, float *y, float *g, long *n_acc_above_one) {
    const long HL = 2L * L + H, N = HL + n;
    float *r = malloc(sizeof(float) * N), *a = malloc(sizeof(float) * N);
    *n_acc_above_one = 0;
    for (long e = 0; e < N; ++e) {
        float pk = 0.f;
        for (int c = 0; c < C; ++c) pk = fmaxf(pk, fabsf(v[c * N + e]));
        r[e] = pk > T ? T / pk : 1.f;
    }
    for (long e = L + H; e < N; ++e) {                   /* (g reads a(t - k), k < L, t >= t0: index HL - (L - 1) = L + H + 1 on) */
        float m = 1.f;
        for (long j = 0; j <= L + H; ++j) m = fminf(m, r[e - j]);
        a[e] = m;
    }
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
