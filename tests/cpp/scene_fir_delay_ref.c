/* The delayed signal of the scene filter mix's delay stage (include/openpbso_amd.h "scene filter mix", the delay stage) as plain
 * C: z of one step, the reference of the tests.  Compiled by tests/scene_fir_delay_model.py with -ffp-contract=off: every
 * operation below rounds once, nothing is fused.
 * xx[N][Hx + n] = the x history ++ the step's rows: xx[o][Hx + j] = x_o(t0 + j), Hx = max_delay + 1 (silence where t0 + j < 0).
 * p[N] are the delay records in force in this step, slope = (to - from) / R rounded once when the set took effect. */
#include <math.h>
#include <stddef.h>

typedef struct { double from, to; long long t_set; double slope; } scene_param;

/* z[o][j] = z_o(t0 + j) for j < n */
void scene_fir_delay_ref(const float *xx, int N, long long Hx, long long n, const scene_param *p, int R, long long t0, float *z) {
    for (int o = 0; o < N; ++o) {
        const float *x = xx + (size_t)o * (Hx + n) + Hx;                   /* x[j] = x_o(t0 + j), j >= -Hx */
        for (long long j = 0; j < n; ++j) {
            const long long k = t0 + j - p[o].t_set + 1;
            double d = p[o].to;
            if (R != 0 && k < R) {
                const double rise = p[o].slope * (double)k;
                d = p[o].from + rise;
            }
            const double fl = floor(d), fr = d - fl;
            const long long i0 = j - (long long)fl - (fr != 0.0 ? 1 : 0);
            const float f = fr != 0.0 ? (float)(1.0 - fr) : 0.f;
            float v = x[i0];
            if (f != 0.f) {
                const float dx = x[i0 + 1] - x[i0];
                const float fdx = f * dx;
                v = x[i0] + fdx;
            }
            z[(size_t)o * n + j] = v;
        }
    }
}
