// The coefficient tables of one mode: every table the bank kernels read is a pure fp64 chain of + and x from the three doubles
// (c1, c2, c3) of modal_integrator.h:95-99, rounded once.  One copy of that arithmetic for the host and the device: the vector
// builders of engine_tables.h (finalize) call these functions mode by mode, and retune_tables_kernel / retune_g32_kernel
// (kernels_retune.hip, pbso_set_material) call them lane by lane -- compiled without FMA contraction on both sides, so a table
// rebuilt on the device equals the one finalize uploaded bit for bit.  No math library call in here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kernels.h"

// empty under the host compiler
#if defined(__HIPCC__)
#define PBSO_HD __host__ __device__
#else
#define PBSO_HD
#endif

namespace pbso {

// Per mode the one-sample matrix in the basis x = (q, q - q_prev) is A = [[1 - e, eps^2], [-e, eps^2]] (e = 1 - c1 - c2 =
// |1 - z|^2, eps^2 = -c2; well conditioned at low frequency).
struct Mat2 {
    double m00, m01, m10, m11;
    PBSO_HD static Mat2 identity() { return {1, 0, 0, 1}; }
    PBSO_HD static Mat2 step_of(double c1, double c2) {
        const double eps2 = -c2, e = (1.0 - c1) - c2;
        return {1.0 - e, eps2, -e, eps2};
    }
    PBSO_HD Mat2 times(const Mat2 &p) const {            // this . p
        return {m00 * p.m00 + m01 * p.m10, m00 * p.m01 + m01 * p.m11, m10 * p.m00 + m11 * p.m10, m10 * p.m01 + m11 * p.m11};
    }
    PBSO_HD void apply(double &v0, double &v1) const {   // v = this . v
        const double n0 = m00 * v0 + m01 * v1, n1 = m10 * v0 + m11 * v1;
        v0 = n0; v1 = n1;
    }
    PBSO_HD void apply_row(double &r0, double &r1) const {   // r = r . this
        const double n0 = r0 * m00 + r1 * m10, n1 = r0 * m01 + r1 * m11;
        r0 = n0; r1 = n1;
    }
};

// the oscillator bank's two coefficient words, per recurrence form
PBSO_HD inline void mode_bank_coefs(double c1, double c2, bool direct_form, float &ca, float &cb) {
    if (!direct_form) {
        ca = (float)(-c2);                     // eps^2
        cb = -(float)((1.0 - c1) - c2);        // -e, e = |1 - z|^2 = 1 - c1 - c2 (stored negated:
                                               //  d = eps^2 d + (-e) q is then a plain v_fmac)
    } else {
        ca = (float)c1;
        cb = (float)c2;
    }
}

// Closed-form qnorm matrices (getQBufferNorm, modal_solver.h:270-273): G = sum_{k=0}^{B-1} (A^k)' e1 e1' A^k (the direct-form
// kernel forms the difference itself).  Row r_k = e1' A^k: r_{k+1} = r_k A.  gq[0], gq[plane], gq[2 plane]: G11, 2 G12, G22.
PBSO_HD inline void mode_gq(double c1, double c2, int frames, float *gq, size_t plane) {
    const Mat2 a = Mat2::step_of(c1, c2);
    double r0 = 1.0, r1 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    for (int k = 0; k < frames; ++k) {
        s11 += r0 * r0; s12 += r0 * r1; s22 += r1 * r1;
        a.apply_row(r0, r1);
    }
    gq[0] = (float)s11;
    gq[plane] = (float)(2.0 * s12);
    gq[2 * plane] = (float)s22;
}

// hi = bf16(x) round-to-nearest-even, lo = bf16(x - hi)
PBSO_HD inline uint32_t bf16_rne(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if ((u & 0x7F800000u) == 0x7F800000u) return u >> 16;                 // inf / nan
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
PBSO_HD inline void bf16_split(double x, uint32_t &hi, uint32_t &lo) {
    const float xf = (float)x;
    hi = bf16_rne(xf);
    const uint32_t hb = hi << 16;
    float hf;
    __builtin_memcpy(&hf, &hb, 4);
    lo = bf16_rne(xf - hf);
}
// one dword pair of the split-bf16 operand table from the f32 weights (a_j, b_j) of one mode: low half a, high half b
PBSO_HD inline void split_bf16_pair(float a, float b, uint32_t &hi, uint32_t &lo) {
    uint32_t ah, al, bh, bl;
    bf16_split((double)a * TRUNC_SPLIT_GAIN, ah, al);
    bf16_split((double)b * TRUNC_SPLIT_GAIN, bh, bl);
    hi = ah | (bh << 16);
    lo = al | (bl << 16);
}
// Where the weights of flat column k (object * m_pad + column) and block sample j = 0..15 live.
// f32 table [n_obj * m_pad / 2][64]: lane = 16 * (2 * mode-of-pair + comp) + j.
PBSO_HD inline size_t wtab_f32_index(size_t k, int comp, int j) { return (k / 2) * 64 + 16 * (2 * (k & 1) + comp) + j; }
// split-bf16 table: per group of 16 columns 8 rows of 64 dwords, rows 0..3 the hi parts, 4..7 the lo parts; lane l = 16 kq + j,
// dword dd <-> column 16 G + 4 kq + dd: low half a_j, high half b_j (the k order of v_mfma_f32_16x16x32_bf16: k = 8 kq + 2 dd + comp)
PBSO_HD inline size_t wtab_bf16_index(size_t k, int lo, int j) {
    const size_t G = k / 16, kq = (k % 16) / 4, dd = k % 4;
    return (8 * G + 4 * lo + dd) * 64 + 16 * kq + j;
}

enum { W_NONE = 0, W_F32 = 1, W_SPLIT_BF16 = 2 };
// ONE walk p = A^j, j = 1 .. max(16, frames), for the three tables that are powers of A:
//   wt (w_kind): row 0 of A^j, j = 1..16, the block form's output weights (a_j, b_j), in the f32 or the split-bf16 layout;
//   pc: P = A^16 advances the state by one block; planes P11 - 1, P12, P21, P22 (q' = q + (P11 - 1) q + P12 d keeps the small
//       angle of low modes);
//   sc (K5): a whole buffer as one step of the state -- A^B (first entry minus one, as P) and A^(B-1) u, u = (1, 1)': what a
//       force sample at the buffer's first sample leaves at its end.  6 planes.
// A null table is not written (and frames is ignored without sc).  k: the flat column.
PBSO_HD inline void mode_walk(double c1, double c2, int frames, size_t k, size_t plane, int w_kind, float *wt, float *pc, float *sc) {
    const Mat2 a = Mat2::step_of(c1, c2);
    Mat2 p = Mat2::identity();                                         // A^j
    const int last = (sc && frames > BLOCK_J) ? frames : BLOCK_J;
    uint32_t *w16 = reinterpret_cast<uint32_t *>(wt);
    for (int j = 1; j <= last; ++j) {
        if (sc && j == frames) {                                       // A^(B-1) u
            sc[4 * plane + k] = (float)(p.m00 + p.m01);
            sc[5 * plane + k] = (float)(p.m10 + p.m11);
        }
        p = a.times(p);
        if (j <= BLOCK_J) {
            if (w_kind == W_F32) {
                wt[wtab_f32_index(k, 0, j - 1)] = (float)p.m00;
                wt[wtab_f32_index(k, 1, j - 1)] = (float)p.m01;
            } else if (w_kind == W_SPLIT_BF16) {
                uint32_t hi, lo;
                split_bf16_pair((float)p.m00, (float)p.m01, hi, lo);
                w16[wtab_bf16_index(k, 0, j - 1)] = hi;
                w16[wtab_bf16_index(k, 1, j - 1)] = lo;
            }
            if (j == BLOCK_J && pc) {
                pc[k] = (float)(p.m00 - 1.0);
                pc[plane + k] = (float)p.m01;
                pc[2 * plane + k] = (float)p.m10;
                pc[3 * plane + k] = (float)p.m11;
            }
        }
        if (sc && j == frames) {
            sc[k] = (float)(p.m00 - 1.0);
            sc[plane + k] = (float)p.m01;
            sc[2 * plane + k] = (float)p.m10;
            sc[3 * plane + k] = (float)p.m11;
        }
    }
}

// Forced block path without qnorm rows (kernels_block.hip, FT): a force sample f enters the state as f u, u = (1, 1)'
// (d += f, q += d), so the samples 16 n + i, i = 1..16, of a dense profile move the next block-start state by
// sum_i A^(16 - i) u f_i.  Plane 2 i' + c holds component c of A^(15 - i') u, i' = 0..15.
PBSO_HD inline void mode_ftab(double c1, double c2, size_t k, size_t plane, float *ft) {
    const Mat2 a = Mat2::step_of(c1, c2);
    double v0 = 1.0, v1 = 1.0;                              // A^delta u, delta = 0, 1, ...
    for (int delta = 0; delta < BLOCK_J; ++delta) {
        const int ip = BLOCK_J - 1 - delta;                // in-block sample index (0-based) this power belongs to
        ft[(size_t)(2 * ip) * plane + k] = (float)v0;
        ft[(size_t)(2 * ip + 1) * plane + k] = (float)v1;
        a.apply(v0, v1);
    }
}

// the spatial vector of a plain vertex hit, per (dof, mode)
PBSO_HD inline float mode_g32(double c3, double shape) { return (float)(c3 * shape); }

// ---- pbso_set_material: what one lane of retune_tables_kernel does ---------------------------------------------------------
// The tables of ONE engine as finalize allocated them: a null pointer is a table this engine does not have.
struct RetuneTables {
    float *ca, *cb;                                      // [n_obj][m_pad]
    double *c3;
    float *pc, *wtab, *gq, *sc, *ftab;
    float *sq, *sd, *ss;                                 // the state planes, keep_state == 0 only: q = d = 0, scale 1
    long long plane;                                     // n_obj * m_pad
    int m_pad, frames, direct_form, w_kind;
};
// one named object of a call: coefs[coef_off + 3 m ..] = (c1, c2, c3) of mode m < n_modes; its shapes (n_dof rows of m_pad) and
// g32 rows start at element shape_off
struct RetuneObj {
    int obj, n_modes, n_dof, pad;
    long long coef_off, shape_off;
};
// Column m (0 <= m < m_pad, padding columns included: zero coefficients, as finalize leaves them) of object o.
PBSO_HD inline void retune_lane(const RetuneTables &t, const RetuneObj &o, const double *coefs, int m) {
    const size_t k = (size_t)o.obj * t.m_pad + m, plane = (size_t)t.plane;
    if (t.sq) { t.sq[k] = 0.f; t.sd[k] = 0.f; t.ss[k] = 1.f; }
    if (m < o.n_modes) {
        const double c1 = coefs[o.coef_off + 3 * (long long)m], c2 = coefs[o.coef_off + 3 * (long long)m + 1];
        mode_bank_coefs(c1, c2, t.direct_form != 0, t.ca[k], t.cb[k]);
        t.c3[k] = coefs[o.coef_off + 3 * (long long)m + 2];
        if (t.gq) mode_gq(c1, c2, t.frames, t.gq + k, plane);
        if (t.pc) mode_walk(c1, c2, t.frames, k, plane, t.w_kind, t.wtab, t.pc, t.sc);
        if (t.ftab) mode_ftab(c1, c2, k, plane, t.ftab);
        return;
    }
    t.ca[k] = 0.f; t.cb[k] = 0.f; t.c3[k] = 0.0;
    if (t.gq) for (int i = 0; i < 3; ++i) t.gq[i * plane + k] = 0.f;
    if (t.pc) {
        for (int i = 0; i < 4; ++i) t.pc[i * plane + k] = 0.f;
        uint32_t *w16 = reinterpret_cast<uint32_t *>(t.wtab);
        for (int j = 0; j < BLOCK_J; ++j) {
            if (t.w_kind == W_F32) { t.wtab[wtab_f32_index(k, 0, j)] = 0.f; t.wtab[wtab_f32_index(k, 1, j)] = 0.f; }
            else if (t.w_kind == W_SPLIT_BF16) { w16[wtab_bf16_index(k, 0, j)] = 0u; w16[wtab_bf16_index(k, 1, j)] = 0u; }
        }
        if (t.sc) for (int i = 0; i < 6; ++i) t.sc[i * plane + k] = 0.f;
    }
    if (t.ftab) for (int i = 0; i < 2 * BLOCK_J; ++i) t.ftab[i * plane + k] = 0.f;
}
// element e of the named object's g32 rows: consecutive e on consecutive modes
PBSO_HD inline void retune_g32_lane(const RetuneObj &o, const double *coefs, const double *shapes, float *g32, int m_pad, long long e) {
    const int m = (int)(e % m_pad);
    g32[o.shape_off + e] = m < o.n_modes ? mode_g32(coefs[o.coef_off + 3 * (long long)m + 2], shapes[o.shape_off + e]) : 0.f;
}

// kernels_retune.hip: retune_lane for every (named object, column); retune_g32_lane for every element of the named objects' rows
// (max_elems: the largest n_dof * m_pad among them)
int launch_retune_tables(const RetuneTables &t, const RetuneObj *objs, int n_objs, const double *coefs, hipStream_t stream);
int launch_retune_g32(const RetuneObj *objs, int n_objs, const double *coefs, const double *shapes, float *g32, int m_pad, long long max_elems,
                      hipStream_t stream);

}  // namespace pbso
