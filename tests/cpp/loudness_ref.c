/* The loudness bus of include/openpbso_amd.h, literally.  The K-weighted signal is the EQ bus's block form: x and y are rows of
 * P + 2 + n doubles that hold the P + 2 samples before the step (zero before t = 0) in front of the step's n, index P + 2 + i is
 * sample t + i, and k0 = t mod P says where sample t lies in its block (t_set = 0).  loud_ref_tables builds the five tables of a
 * section by the recurrence in its literal order; loud_ref_serial is that plain recurrence; loud_ref_block fills y[P + 2 ..] by
 * the stated fma chains.  loud_ref_energy walks the 64 accumulators of an open sub-block over a step and does the tree where a
 * sub-block ends; loud_ref_peak does the fmaf chains of the true peak and the two running maxima.  Compile with
 * -ffp-contract=off: only the fma() and fmaf() calls fuse. */
#include <math.h>

void loud_ref_serial(const double *c, long n, const double *x, double *st, double *y) {
    double x1 = st[0], x2 = st[1], y1 = st[2], y2 = st[3];
    for (long i = 0; i < n; ++i) {
        const double v = x[i], o = c[0] * v + c[1] * x1 + c[2] * x2 - c[3] * y1 - c[4] * y2;
        x2 = x1; x1 = v; y2 = y1; y1 = o;
        y[i] = o;
    }
    st[0] = x1; st[1] = x2; st[2] = y1; st[3] = y2;
}

void loud_ref_tables(const double *c, int P, double *tab) {
    for (int m = 0; m < 5; ++m) {
        double in[64] = {0}, st[4] = {0, 0, 0, 0};
        if (m == 0) in[0] = 1.0; else st[m - 1] = 1.0;   /* h: an impulse; r s p q: unit x(-1), x(-2), y(-1), y(-2) */
        loud_ref_serial(c, P, in, st, tab + m * P);
    }
}

void loud_ref_block(const double *tab, int P, long k0, long n, const double *x, double *y) {
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

/* z[n]: the step's weighted samples, the first of them k0 samples into its sub-block of hs; acc[64] the open sub-block's
 * accumulators, carried in and out.  Writes the energies of the sub-blocks that end inside the step and returns their number. */
long loud_ref_energy(const double *z, long n, long k0, long hs, double *acc, double *energy) {
    long done = 0, k = k0;
    for (long i = 0; i < n; ++i) {
        const long l = k % 64;
        acc[l] = fma(z[i], z[i], acc[l]);
        if (++k == hs) {
            for (int s = 32; s >= 1; s /= 2)
                for (int m = 0; m < s; ++m) acc[m] = acc[m] + acc[m + s];
            energy[done++] = acc[0];
            for (int m = 0; m < 64; ++m) acc[m] = 0.0;
            k = 0;
        }
    }
    return done;
}

/* u: 11 samples of history in front of the step's n; h [O][12]; run[2] the open sub-block's maxima (true peak, sample peak),
 * carried in and out.  Writes tp / sp of the sub-blocks that end inside the step and returns their number. */
long loud_ref_peak(const float *u, long n, long k0, long hs, const float *h, int O, float *run, float *tp, float *sp) {
    long done = 0, k = k0;
    for (long i = 0; i < n; ++i) {
        const float *w = u + 11 + i;
        for (int phi = 0; phi < O; ++phi) {
            float acc = 0.f;
            for (int j = 11; j >= 0; --j) acc = fmaf(h[phi * 12 + j], w[-j], acc);
            if (fabsf(acc) > run[0]) run[0] = fabsf(acc);
        }
        if (fabsf(w[0]) > run[1]) run[1] = fabsf(w[0]);
        if (++k == hs) {
            tp[done] = run[0];
            sp[done++] = run[1];
            run[0] = run[1] = 0.f;
            k = 0;
        }
    }
    return done;
}
