// The EQ bus's schedule (include/openpbso_amd.h "The EQ bus's SCHEDULE"; eq_schedule.h has the plan): a step with coefficient sets
// that take effect inside it, in a number of launches that does not depend on how many they are.  The arithmetic of every sample
// is that of kernels_eq.hip, word for word; what differs is where a sample finds its block origin, its tables and its neighbours.
//
// Every signal has two extended rows of EQ_HIST + n doubles (eq_schedule.h): V, the timeline in force, and F, the tails of the sets
// that fade out.  Per section, three kernels as in kernels_eq.hip:
//
//   forward   one thread per sample: it finds its segment in the plan by a search, derives its origin, its k and its tables, and
//             runs the chain over h, r, s from a window of x staged in LDS ([first - P - 1, first + 255], of V and of F); inside a
//             fade it runs the predecessor's chain as well.  It also copies the output signal's histories in front of its rows and
//             writes the input signal's next histories.
//   chain     one wave per channel walks the block list of V and then that of the tails, 64 blocks at a time from LDS.  A block cut
//             short at length L ends in samples L - 2 and L - 1, which are fma(p[k], y(o-1), fma(q[k], y(o-2), W)) as ever.
//   finish    one thread per sample: q and p on the other samples of every block, of V and of the tails.
//
// The tables of the step's sets are built on the device from their coefficients, by the recurrence of eq_block.h in its literal
// order.  Built with -ffp-contract=off and without any fast-math or denormal flag.
#include <hip/hip_runtime.h>

#include "eq_schedule.h"
#include "kernels.h"

namespace pbso {

namespace {
constexpr int P = EQ_BLOCK, H = EQ_HIST;
constexpr int TPB = 256;
constexpr int WIN = TPB + P + 1;                         // indices first - P - 1 .. first + 255

// what every kernel of a step is told
struct EqStep {
    const EqSeg *seg;                                    // 2 + K records
    int K;
    int N;                                               // H + n
    int C, S;
    int R;
    const double *tab2;                                  // the stage's two slots [2][C][S][5][P]
    const double *pool;                                  // the step's sets [K][C][S][5][P]
};

__device__ __forceinline__ const double *table_of(const EqStep &q, int id, int c, int s) {
    const size_t tw = (size_t)q.C * q.S * EQ_TABLES * P;
    const double *base = id < 2 ? q.tab2 + (size_t)id * tw : q.pool + (size_t)(id - 2) * tw;
    return base + ((size_t)c * q.S + s) * EQ_TABLES * P;
}

// the record index (1 + g) of the segment that holds row index i >= H: the last one with s <= i
__device__ __forceinline__ int segment_of(const EqStep &q, int i) {
    int lo = 1, hi = 1 + q.K;                            // (records 1 .. 1 + K; an empty segment 0 shares s with segment 1)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (q.seg[mid].s <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
}  // namespace

// pool [K][C][S][5][P] from sos [K][C][S][5]: one thread per table
__global__ __launch_bounds__(256) void eq_sched_tables_kernel(const double *__restrict__ sos, long long n_sections, double *__restrict__ pool) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_sections * EQ_TABLES) return;
    const long long sec = u / EQ_TABLES;
    const int which = (int)(u % EQ_TABLES);
    double c[5];
    for (int k = 0; k < 5; ++k) c[k] = sos[sec * 5 + k];
    double v = which == 0 ? 1.0 : 0.0, x1 = which == 1 ? 1.0 : 0.0, x2 = which == 2 ? 1.0 : 0.0, y1 = which == 3 ? 1.0 : 0.0,
           y2 = which == 4 ? 1.0 : 0.0;
    double *out = pool + (sec * EQ_TABLES + which) * P;
    for (int k = 0; k < P; ++k) {
        const double o = c[0] * v + c[1] * x1 + c[2] * x2 - c[3] * y1 - c[4] * y2;    // eq_step, in its order
        x2 = x1;
        x1 = v;
        y2 = y1;
        y1 = o;
        out[k] = o;
        v = 0.0;
    }
}

// signal 0: x [C][N] = hist ++ (double)in
__global__ __launch_bounds__(256) void eq_sched_input_kernel(const float *__restrict__ in, int n, const double *__restrict__ hist,
                                                             long long hist_stride, double *__restrict__ x) {
    const int c = blockIdx.y;
    const long long N = (long long)H + n, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    x[c * N + i] = i < H ? hist[c * hist_stride + i] : (double)in[(long long)c * n + (i - H)];
}

// Section s: W of V and of the tails from the rows vx, fx of signal s (fx == vx for signal 0).  Workgroup 0 also puts the
// histories of signal s + 1 in front of vy and fy, and writes the next histories of signal s.
__global__ __launch_bounds__(TPB) void eq_sched_forward_kernel(EqStep q, int s, const double *__restrict__ vx, const double *__restrict__ fx,
                                                               double *__restrict__ wv, double *__restrict__ wf, double *__restrict__ vy,
                                                               double *__restrict__ fy, const double *__restrict__ hist_to,
                                                               const double *__restrict__ hist_from, double *__restrict__ next_to,
                                                               double *__restrict__ next_from, int from_hist, int vs_last) {
    __shared__ double win_v[WIN], win_f[WIN];
    const int c = blockIdx.y, N = q.N, n = N - H;
    const size_t row = (size_t)c * N;
    const long long first = (long long)H + (long long)blockIdx.x * TPB, base = first - P - 1;      // base >= 1
    for (int l = threadIdx.x; l < WIN; l += TPB) {
        const long long i = base + l;
        win_v[l] = i < N ? vx[row + i] : 0.0;
        win_f[l] = i < N ? fx[row + i] : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x < H) {
        const int u = threadIdx.x;
        const size_t hx = ((size_t)c * (q.S + 1) + s) * H + u, hy = hx + H;
        vy[row + u] = hist_to[hy];
        fy[row + u] = hist_from[hy];
        const int i = n + u;
        next_to[hx] = vx[row + i];
        if (from_hist) next_from[hx] = i < vs_last ? vx[row + i] : fx[row + i];
    }
    __syncthreads();
    const long long i = first + threadIdx.x;
    if (i >= N) return;
    const int g = segment_of(q, (int)i);
    const EqSeg sg = q.seg[g];
    {
        const int o = sg.a + ((int)i - sg.a) / P * P, k = (int)i - o;
        const double *__restrict__ t = table_of(q, sg.tab, c, s);
        double acc = 0.0;
        for (int j = k; j >= 0; --j) acc = fma(t[j], win_v[(int)(i - j - base)], acc);
        acc = fma(t[P + k], win_v[(int)(o - 1 - base)], acc);
        acc = fma(t[2 * P + k], win_v[(int)(o - 2 - base)], acc);
        wv[row + i] = acc;
    }
    if (i < sg.fe) {
        const EqSeg fr = q.seg[g - 1];
        const int o = fr.a + ((int)i - fr.a) / P * P, k = (int)i - o, vs = sg.vs;
        const double *__restrict__ t = table_of(q, fr.tab, c, s);
        auto x = [&](int p) { return p < vs ? win_v[(int)(p - base)] : win_f[(int)(p - base)]; };
        double acc = 0.0;
        for (int j = k; j >= 0; --j) acc = fma(t[j], x((int)i - j), acc);
        acc = fma(t[P + k], x(o - 1), acc);
        acc = fma(t[2 * P + k], x(o - 2), acc);
        wf[row + i] = acc;
    }
}

// Section s: the last two samples of every block of the two lists, one wave per channel.  Lane b of a batch fetches block b's
// partial sums, table words and stored values; all lanes walk the batch from LDS alike; lane b keeps block b's pair and stores it.
__global__ __launch_bounds__(64) void eq_sched_chain_kernel(EqStep q, int s, const EqBlk *__restrict__ vblk, int n_vblk,
                                                            const EqBlk *__restrict__ fblk, int n_fblk, const double *__restrict__ wv,
                                                            const double *__restrict__ wf, double *vy, double *fy) {
    __shared__ double s_wa[64], s_wb[64], s_pa[64], s_pb[64], s_qa[64], s_qb[64], s_r1[64], s_r2[64];
    __shared__ int s_mode[64];                           // bits 0 .. 1: sample L - 2 is computed (0), y(o - 1) (1) or stored (2); bit 2: reset
    const int c = blockIdx.x, lane = threadIdx.x;
    const size_t row = (size_t)c * q.N;
    double *vyc = vy + row, *fyc = fy + row;
    double y1 = 0.0, y2 = 0.0;
    for (int list = 0; list < 2; ++list) {
        const EqBlk *__restrict__ blk = list ? fblk : vblk;
        const int nb = list ? n_fblk : n_vblk;
        const double *__restrict__ w = (list ? wf : wv) + row;
        double *yo = list ? fyc : vyc;
        for (int b0 = 0; b0 < nb; b0 += 64) {
            const int b = b0 + lane;
            double wa = 0.0, wb = 0.0, pa = 0.0, pb = 0.0, qa = 0.0, qb = 0.0, r1 = 0.0, r2 = 0.0;
            int mode = 0, ia = 0, ib = 0;
            if (b < nb) {
                const EqBlk k = blk[b];
                const double *__restrict__ t = table_of(q, k.tab, c, s);
                auto stored = [&](int p) { return p < k.vs ? vyc[p] : fyc[p]; };
                ia = k.o + k.L - 2;
                ib = ia + 1;
                pb = t[3 * P + k.L - 1];
                qb = t[4 * P + k.L - 1];
                wb = w[ib];
                if (k.L == 1) mode = 1;
                else if (ia < k.lo) {
                    mode = 2;
                    wa = stored(ia);
                } else {
                    pa = t[3 * P + k.L - 2];
                    qa = t[4 * P + k.L - 2];
                    wa = w[ia];
                }
                if (k.flags & EQ_BLK_RESET) {
                    mode |= 4;
                    r1 = stored(k.o - 1);
                    r2 = stored(k.o - 2);
                }
            }
            __syncthreads();
            s_wa[lane] = wa;
            s_wb[lane] = wb;
            s_pa[lane] = pa;
            s_pb[lane] = pb;
            s_qa[lane] = qa;
            s_qb[lane] = qb;
            s_r1[lane] = r1;
            s_r2[lane] = r2;
            s_mode[lane] = mode;
            __syncthreads();
            const int cnt = nb - b0 < 64 ? nb - b0 : 64;
            double ra = 0.0, rb = 0.0;
            for (int i = 0; i < cnt; ++i) {
                const int m = s_mode[i];
                if (m & 4) {
                    y1 = s_r1[i];
                    y2 = s_r2[i];
                }
                double na = fma(s_pa[i], y1, fma(s_qa[i], y2, s_wa[i]));
                if ((m & 3) == 1) na = y1;
                if ((m & 3) == 2) na = s_wa[i];
                const double nbv = fma(s_pb[i], y1, fma(s_qb[i], y2, s_wb[i]));
                y2 = na;
                y1 = nbv;
                if (i == lane) {
                    ra = na;
                    rb = nbv;
                }
            }
            if (b < nb) {
                if ((mode & 3) == 0) yo[ia] = ra;
                yo[ib] = rb;
            }
        }
        // the tails read what the chain of V has stored
        __threadfence_block();
        __syncthreads();
    }
}

// Section s: the samples of every block that are not its last two, of V and of the tails
__global__ __launch_bounds__(TPB) void eq_sched_finish_kernel(EqStep q, int s, const double *__restrict__ wv, const double *__restrict__ wf,
                                                              double *vy, double *fy) {
    const int c = blockIdx.y, N = q.N;
    const size_t row = (size_t)c * N;
    const long long i = (long long)H + (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= N) return;
    const int g = segment_of(q, (int)i);
    const EqSeg sg = q.seg[g];
    double *vyc = vy + row, *fyc = fy + row;
    {
        const int e = g < 1 + q.K ? q.seg[g + 1].s : N;
        const int o = sg.a + ((int)i - sg.a) / P * P, k = (int)i - o, L = e - o < P ? e - o : P;
        if (k < L - 2) {
            const double *__restrict__ t = table_of(q, sg.tab, c, s);
            vyc[i] = fma(t[3 * P + k], vyc[o - 1], fma(t[4 * P + k], vyc[o - 2], wv[row + i]));
        }
    }
    if (i < sg.fe) {
        const EqSeg fr = q.seg[g - 1];
        const int o = fr.a + ((int)i - fr.a) / P * P, k = (int)i - o, L = sg.fe - o < P ? sg.fe - o : P, vs = sg.vs;
        if (k < L - 2) {
            const double *__restrict__ t = table_of(q, fr.tab, c, s);
            const double a1 = o - 1 < vs ? vyc[o - 1] : fyc[o - 1], a2 = o - 2 < vs ? vyc[o - 2] : fyc[o - 2];
            fyc[i] = fma(t[3 * P + k], a1, fma(t[4 * P + k], a2, wf[row + i]));
        }
    }
}

// out[c][i] = (float)V; inside a fade yf + w (yt - yf) with yf = (float)F, w = (float)((double)d / (double)R); workgroup 0 also writes
// the next histories of signal S
__global__ __launch_bounds__(256) void eq_sched_output_kernel(EqStep q, const double *__restrict__ vy, const double *__restrict__ fy,
                                                              double *__restrict__ next_to, double *__restrict__ next_from, int from_hist,
                                                              int vs_last, float *__restrict__ out) {
    const int c = blockIdx.y, N = q.N, n = N - H;
    const size_t row = (size_t)c * N;
    if (blockIdx.x == 0 && threadIdx.x < H) {
        const int u = threadIdx.x, i = n + u;
        const size_t hx = ((size_t)c * (q.S + 1) + q.S) * H + u;
        next_to[hx] = vy[row + i];
        if (from_hist) next_from[hx] = i < vs_last ? vy[row + i] : fy[row + i];
    }
    const long long i = (long long)H + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const EqSeg sg = q.seg[segment_of(q, (int)i)];
    float v = (float)vy[row + i];
    if (i < sg.fe) {
        const float yf = (float)fy[row + i];
        const float w = (float)((double)(sg.d0 + (i - sg.s)) / (double)q.R);
        const float d = v - yf;
        const float wd = w * d;
        v = yf + wd;
    }
    out[(size_t)c * n + (i - H)] = v;
}

size_t eq_sched_work_doubles(int C, long long n) { return (size_t)6 * C * (size_t)(H + n); }

int launch_eq_sched_tables(const double *sos, long long n_sections, double *pool, hipStream_t stream) {
    if (!sos || !pool || n_sections <= 0) return (int)hipErrorInvalidValue;
    const long long threads = n_sections * EQ_TABLES;
    hipLaunchKernelGGL(eq_sched_tables_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, sos, n_sections, pool);
    return (int)hipGetLastError();
}

int launch_eq_scheduled(const float *in, int C, int S, long long n, int R, const void *seg, int K, const void *vblk, int n_vblk, const void *fblk,
                        int n_fblk, const double *tab2, const double *pool, const double *hist_to, const double *hist_from, double *next_to,
                        double *next_from, int from_hist, int vs_last, double *work, float *out, hipStream_t stream) {
    if (!in || !seg || !vblk || !tab2 || !pool || !hist_to || !hist_from || !next_to || !next_from || !work || !out || C < 1 ||
        C > SCENE_MAX_CHANNELS || S < 1 || S > EQ_MAX_SECTIONS || !eq_plan_fits(n) || K < 1 || n_vblk < 1 || n_fblk < 0 || (n_fblk && !fblk))
        return (int)hipErrorInvalidValue;
    const long long N = H + n;
    const size_t rows = (size_t)C * N;
    double *v[2] = {work, work + rows}, *f[2] = {work + 2 * rows, work + 3 * rows}, *wv = work + 4 * rows, *wf = work + 5 * rows;
    const EqStep q = {(const EqSeg *)seg, K, (int)N, C, S, R, tab2, pool};
    const long long hist_stride = (long long)(S + 1) * H;
    hipLaunchKernelGGL(eq_sched_input_kernel, dim3((unsigned)((N + 255) / 256), C), dim3(256), 0, stream, in, (int)n, hist_to, hist_stride, v[0]);
    const dim3 grid((unsigned)((n + TPB - 1) / TPB), C);
    for (int s = 0; s < S; ++s) {
        const double *vx = v[s & 1], *fx = s ? f[s & 1] : v[0];
        double *vy = v[(s + 1) & 1], *fy = f[(s + 1) & 1];
        hipLaunchKernelGGL(eq_sched_forward_kernel, grid, dim3(TPB), 0, stream, q, s, vx, fx, wv, wf, vy, fy, hist_to, hist_from, next_to, next_from,
                           from_hist, vs_last);
        hipLaunchKernelGGL(eq_sched_chain_kernel, dim3(C), dim3(64), 0, stream, q, s, (const EqBlk *)vblk, n_vblk, (const EqBlk *)fblk, n_fblk,
                           (const double *)wv, (const double *)wf, vy, fy);
        hipLaunchKernelGGL(eq_sched_finish_kernel, grid, dim3(TPB), 0, stream, q, s, (const double *)wv, (const double *)wf, vy, fy);
    }
    hipLaunchKernelGGL(eq_sched_output_kernel, grid, dim3(256), 0, stream, q, (const double *)v[S & 1], (const double *)f[S & 1], next_to, next_from,
                       from_hist, vs_last, out);
    return (int)hipGetLastError();
}

}  // namespace pbso
