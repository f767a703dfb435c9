/* The scene mix's order of arithmetic (include/openpbso_amd.h "scene mix") as plain C: the reference of the tests.
 * Compiled by tests/scene_mix_model.py with -ffp-contract=off: every operation below rounds once, nothing is fused.
 * x[N][L] holds the samples base .. base + L - 1 (absolute); anything outside is silence.
 * p[C][N][2] are the (gain, delay) records as the engine keeps them, slope = (to - from) / R rounded once at the set call. */
#include <math.h>
#include <stddef.h>

typedef struct { double from, to; long long t_set; double slope; } scene_param;

static double ramp(const scene_param *p, long long t, int R) {
    const long long k = t - p->t_set + 1;
    if (R == 0 || k >= R) return p->to;
    const double rise = p->slope * (double)k;
    return p->from + rise;
}

static float at(const float *x, long long L, long long base, long long i) {
    i -= base;
    return i >= 0 && i < L ? x[i] : 0.f;
}

/* out[c][j] for the absolute samples ts[j] */
void scene_mix_ref(const float *x, int N, long long L, long long base, const scene_param *p, int C, int R, const long long *ts, int nt,
                   float *out) {
    for (int c = 0; c < C; ++c)
        for (int j = 0; j < nt; ++j) {
            const long long t = ts[j];
            float sum = 0.f;
            for (int g0 = 0; g0 < N; g0 += 32) {
                float acc = 0.f;
                for (int o = g0; o < N && o < g0 + 32; ++o) {
                    const scene_param *q = p + ((size_t)c * N + o) * 2;
                    const float *xo = x + (size_t)o * L;
                    const float g = (float)ramp(q, t, R);
                    const double d = ramp(q + 1, t, R);
                    const double fl = floor(d), fr = d - fl;
                    const long long off = (long long)fl + (fr != 0.0 ? 1 : 0);
                    const float f = fr != 0.0 ? (float)(1.0 - fr) : 0.f;
                    const float x0 = at(xo, L, base, t - off);
                    float v = x0;
                    if (f != 0.f) {
                        const float dx = at(xo, L, base, t - off + 1) - x0;
                        const float fdx = f * dx;
                        v = x0 + fdx;
                    }
                    const float gv = g * v;
                    acc = acc + gv;
                }
                sum = sum + acc;
            }
            out[(size_t)c * nt + j] = sum;
        }
}
