/* The scene reverb's order of arithmetic (include/openpbso_amd.h "scene reverb") as plain C: the reference of the tests.
 * Compiled by tests/scene_reverb_model.py with -ffp-contract=off: every fmaf below is one, nothing else is fused.
 * u[n_in][L] holds the samples base .. base + L - 1 (absolute); anything outside is silence. */
#include <math.h>
#include <stddef.h>

#define S 2048 /* PBSO_SCENE_REVERB_SEGMENT */

static float y_of(const float *u, int n_in, long L, long base, const float *r, int K, int c, long t) {
    float y = 0.f;
    for (int i = 0; i < n_in; ++i)
        for (long j = 0; j * S < K; ++j) {
            float acc = 0.f;
            for (long k = ((j + 1) * S < K ? (j + 1) * S : K) - 1; k >= j * S; --k) {
                const long q = t - k - base;
                acc = fmaf(r[((size_t)c * n_in + i) * K + k], q >= 0 && q < L ? u[(size_t)i * L + q] : 0.f, acc);
            }
            y = y + acc;
        }
    return y;
}

/* out[c][j] for the absolute samples ts[j]; r_to NULL: nothing set yet (0.f); r_from NULL: no taps were in force before t_set (no
 * fade); add NULL or [n_out][nt], the samples of d_add at ts */
void scene_reverb_ref(const float *u, int n_in, long L, long base, const float *r_to, const float *r_from, int n_out, int K, long t_set,
                      int R, const long *ts, int nt, const float *add, float *out) {
    for (int c = 0; c < n_out; ++c)
        for (int j = 0; j < nt; ++j) {
            const long t = ts[j];
            float y = r_to ? y_of(u, n_in, L, base, r_to, K, c, t) : 0.f;
            if (r_to && r_from && t - t_set + 1 < R) {
                const float yfrom = y_of(u, n_in, L, base, r_from, K, c, t);
                const float w = (float)((double)(t - t_set + 1) / (double)R);
                const float d = y - yfrom;
                const float wd = w * d;
                y = yfrom + wd;
            }
            if (add) y = add[(size_t)c * nt + j] + y;
            out[(size_t)c * nt + j] = y;
        }
}
