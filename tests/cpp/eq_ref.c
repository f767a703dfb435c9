/* The EQ bus of include/openpbso_amd.h, literally.  One section at a time: x and y are rows of P + 2 + n doubles that hold the
 * P + 2 samples before the step (zero before t = 0) in front of the step's n; index P + 2 + i is sample t + i, and k0 = (t - t_set)
 * mod P says where sample t lies in its block.  eq_ref_block fills y[P + 2 ..] by the stated fma chains from tab [5][P] = h r s p q;
 * eq_ref_serial is the plain recurrence in its literal order, from and to the state st = x1 x2 y1 y2; eq_ref_tables builds the five
 * tables with it.  Compile with -ffp-contract=off: only the fma() calls fuse. */
#include <math.h>

void eq_ref_serial(const double *c, long n, const double *x, double *st, double *y) {
    double x1 = st[0], x2 = st[1], y1 = st[2], y2 = st[3];
    for (long i = 0; i < n; ++i) {
        const double v = x[i], o = c[0] * v + c[1] * x1 + c[2] * x2 - c[3] * y1 - c[4] * y2;
        x2 = x1; x1 = v; y2 = y1; y1 = o;
        y[i] = o;
    }
    st[0] = x1; st[1] = x2; st[2] = y1; st[3] = y2;
}

void eq_ref_tables(const double *c, int P, double *tab) {
    for (int m = 0; m < 5; ++m) {
        double in[64] = {0}, st[4] = {0, 0, 0, 0};
        if (m == 0) in[0] = 1.0; else st[m - 1] = 1.0;   /* h: an impulse; r s p q: unit x(-1), x(-2), y(-1), y(-2) */
        eq_ref_serial(c, P, in, st, tab + m * P);
    }
}

void eq_ref_block(const double *tab, int P, long k0, long n, const double *x, double *y) {
    const double *h = tab, *r = tab + P, *s = tab + 2 * P, *p = tab + 3 * P, *q = tab + 4 * P;
    for (long i = 0; i < n; ++i) {
        const long k = (k0 + i) % P, o = P + 2 + i - k;   /* the block's origin T0 as an index */
        double acc = 0.0;
        for (long j = k; j >= 0; --j) acc = fma(h[j], x[o + k - j], acc);
        acc = fma(r[k], x[o - 1], acc);
        acc = fma(s[k], x[o - 2], acc);
        acc = fma(q[k], y[o - 2], acc);
        acc = fma(p[k], y[o - 1], acc);
        y[P + 2 + i] = acc;
    }
}
