/* The scene filter mix's order of arithmetic (include/openpbso_amd.h "scene filter mix") as plain C: the reference of the tests.
 * Compiled by tests/scene_fir_model.py with -ffp-contract=off: every fmaf below is one, nothing else is fused.
 * x[N][L] holds the samples base .. base + L - 1 (absolute); anything outside is silence. */
#include <math.h>
#include <stddef.h>

static float chain(const float *x, int N, long L, long base, const float *h, const int *D, int K, int c, long t) {
    float sum = 0.f;
    for (int g = 0; g < N; g += 32) {
        float acc = 0.f;
        for (int o = g; o < N && o < g + 32; ++o)
            for (int k = K - 1; k >= 0; --k) {
                const long i = t - D[o] - k - base;
                acc = fmaf(h[((size_t)c * N + o) * K + k], i >= 0 && i < L ? x[(size_t)o * L + i] : 0.f, acc);
            }
        sum = sum + acc;
    }
    return sum;
}

/* out[c][j] for the absolute samples ts[j]; h_from NULL: no filters were in force before t_set (no fade) */
void scene_fir_ref(const float *x, int N, long L, long base, const float *h_to, const int *d_to, const float *h_from, const int *d_from,
                   int C, int K, long t_set, int R, const long *ts, int nt, float *out) {
    for (int c = 0; c < C; ++c)
        for (int j = 0; j < nt; ++j) {
            const long t = ts[j];
            const float yto = chain(x, N, L, base, h_to, d_to, K, c, t);
            if (h_from && t - t_set + 1 < R) {
                const float yfrom = chain(x, N, L, base, h_from, d_from, K, c, t);
                const float w = (float)((double)(t - t_set + 1) / (double)R);
                const float d = yto - yfrom;
                const float wd = w * d;
                out[(size_t)c * nt + j] = yfrom + wd;
            } else
                out[(size_t)c * nt + j] = yto;
        }
}
