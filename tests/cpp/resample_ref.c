/* The resampler bus of include/openpbso_amd.h, literally: u [C][T - 1 + n] holds u_c(t0 - (T - 1)) .. u_c(t0 + n - 1) (the history,
 * zero before t = 0, in front of the step); h the phase table [L][T].  Output j < n_out of the call is output m_lo + j: it reads
 * at i = floor(m M / L) with phase (m M) mod L, and i - t0 and the phase are taken here from the absolute m and t0 with a 128-bit
 * product, NOT from p0 as the engine takes them.  Writes y [C][n_out].  Compile with -ffp-contract=off. */
#include <math.h>

void resample_ref(const float *u, int C, long n, long t0, long m_lo, long n_out, int L, int M, int T, const float *h, float *y) {
    const long N = T - 1 + n;
    for (long j = 0; j < n_out; ++j) {
        const unsigned __int128 pos = (unsigned __int128)(unsigned long)(m_lo + j) * (unsigned)M;
        const long i = (long)(pos / (unsigned)L) - t0;   /* local: 0 <= i < n */
        const int phi = (int)(pos % (unsigned)L);
        for (int c = 0; c < C; ++c) {
            const float *e = u + c * N + (T - 1) + i;    /* u_c(i) */
            float acc = 0.f;
            for (int k = T - 1; k >= 0; --k) acc = fmaf(h[(long)phi * T + k], e[-k], acc);
            y[c * n_out + j] = acc;
        }
    }
}
