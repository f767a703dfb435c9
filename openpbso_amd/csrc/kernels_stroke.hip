// Stroke scripts on the device (pbso_enqueue_strokes): one wave per StrokeRec -- one eligible object of a launch -- expands the
// object's entries into the tables the preparation kernels and the oscillator bank read (kernels.h, StrokeTables).
//
// What the wave reproduces is ModalSolver::step's bookkeeping (modal_solver.h:184-240) for an object under sustained contact:
//   * at most one message is dequeued per buffer (:184), so entry k lands in buffer b_k = max(stamp_k - buffers_done, b_{k-1} + 1)
//     = k + max_{j <= k}(stamp_j - buffers_done - j, 0): a prefix maximum over the entries, one scan per 64 entries;
//   * a sustained force's data is replaced by every message (:197-200), so a buffer's data row is that of the last entry with
//     b_k <= b (the force's own row in front of the first entry), and every buffer in contact gets a dense profile row (:222-240);
//   * the entry with sustainedForceEnd clears the list before the profile is added (:201-204): its buffer is force-free.
// The projection itself stays with modal_project_kernel (fp64, the reference's operation order): this kernel writes its events.
// Plain C++ stores only; grid = records, block = one wave, LDS = b_k of the object's entries.
#include "kernels.h"
#include "../../include/openpbso_amd.h"

namespace pbso {

// inclusive prefix maximum over the wave's 64 lanes
__device__ __forceinline__ int wave_prefix_max(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, up);
    }
    return v;
}

__global__ __launch_bounds__(64) void stroke_expand_kernel(const StrokeTables t) {
    extern __shared__ int bk[];                          // [n_ent] buffer of entry k
    const StrokeRec r = t.recs[blockIdx.x];
    const int lane = threadIdx.x;
    const int nb = t.nb;

    // ---- entries: their buffers, their projection events (or cleared data rows)
    int carry = 0;                                       // max_{j < chunk}(stamp_j - buffers_done - j, 0)
    int n_face = 0;                                      // FACE entries in front of this chunk
    for (int k0 = 0; k0 < r.n_ent; k0 += 64) {
        const int k = k0 + lane;
        const bool have = k < r.n_ent;
        int v = 0;
        int fl = 0;
        if (have) {
            const int64_t rel = t.stamps[r.e0 + k] - t.buffers_done;
            v = (int)min(max(rel, (int64_t)-(1 << 30)), (int64_t)(1 << 30)) - k;
            fl = t.flags ? t.flags[r.e0 + k] : 0;
        }
        v = max(wave_prefix_max(have ? v : -(1 << 30) - k, lane), carry);
        carry = __shfl(v, 63, 64);
        const bool face = have && !(fl & STROKE_ZERO);
        const unsigned long long fmask = __ballot(face);
        if (have) {
            const int b = min(v + k, nb);                // (the planner only hands over entries that land inside the launch)
            bk[k] = b;
            const int slot = r.slot0 + k;
            if (face) {
                const int e = r.proj0 + n_face + __popcll(fmask & ((1ull << lane) - 1ull));
                const size_t i3 = 3 * (size_t)(r.e0 + k);
                ProjectEvent ev;
                ev.obj = r.obj;
                ev.kind = PBSO_DATA_FACE;
                ev.slot = slot;
                for (int j = 0; j < 3; ++j) {
                    ev.vids[j] = t.vids[i3 + j];
                    ev.coords[j] = t.coords[i3 + j];
                    ev.vn[j] = t.vn[i3 + j];
                }
                t.proj[t.proj_base + e] = ev;
            }
        }
        n_face += __popcll(fmask);
        // setZero(N) entries (the dummy start / stop messages): the data row is cleared, by the whole wave
        unsigned long long zmask = __ballot(have && (fl & STROKE_ZERO));
        while (zmask) {
            const int l = __ffsll((long long)zmask) - 1;
            zmask &= zmask - 1;
            double *row = t.slots + (size_t)(r.slot0 + k0 + l) * t.m_pad;
            for (int m = lane; m < t.m_pad; m += 64) row[m] = 0.0;
        }
    }
    __syncthreads();

    // ---- buffers: the dense rows
    const int last_fl = (r.n_ent > 0 && t.flags) ? t.flags[r.e0 + r.n_ent - 1] : 0;
    const int first_dense = r.sustained0 ? 0 : (r.n_ent > 0 ? bk[0] : nb);
    const int end_dense = (last_fl & STROKE_END) ? bk[r.n_ent - 1] : nb;
    for (int b = first_dense + lane; b < end_dense; b += 64) {
        // the last entry with b_k <= b
        int lo = 0, hi = r.n_ent;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bk[mid] <= b) lo = mid + 1; else hi = mid;
        }
        const int slot = lo > 0 ? r.slot0 + lo - 1 : r.carry_slot;
        const int i = b - first_dense;
        if (i >= r.n_dense) continue;                    // (never: the planner counted the same rows)
        const int row = r.row0 + i;
        const int frow = t.frow_base + row, prow = t.prow_base + row, entry = t.entry_base + row;
        BufDesc d = {frow, prow, t.tile_mask, 0.f, XFER_KEEP, 0u, {0, 0}};
        t.desc[(size_t)r.obj * nb + b] = d;
        t.slot_idx[t.sidx_base + row] = slot;
        t.row_ptr[frow + 1] = t.sidx_base + row + 1;
        t.row_obj[frow] = r.obj;
        t.prow_obj[prow] = r.obj;
        ProfRow pr = {prow, entry, entry + 1};
        t.prof_rows[t.prof_row_base + row] = pr;
        const int fl0 = i == 0 ? r.flags0 : 0;
        ProfEntry e;
        e.kind = PBSO_AUTOREGRESSIVE_FORCE;
        e.state = r.ar_state;
        e.flags = fl0;
        e.count = t.ar_uses ? t.use_base + row : 0;
        e.center = 0;
        e.width_samples = 0;
        e.a0 = (fl0 & 2) ? r.arprm[0] : 0.0;
        e.a1 = (fl0 & 2) ? r.arprm[1] : 0.0;
        e.sigma = (fl0 & 2) ? r.arprm[2] : 0.0;
        e.mu = (fl0 & 2) ? r.arprm[3] : 0.0;
        t.prof_entries[entry] = e;
        if (t.ar_uses) {
            ArUse u;
            u.entry = entry;
            u.stream = r.stream;
            u.u = i;
            u.epoch_u = r.flags0 ? 0 : -1;
            u.param_entry = r.flags0 ? t.entry_base + r.row0 : -1;
            u.last = i == r.n_dense - 1 ? 1 : 0;
            u.pad[0] = u.pad[1] = 0;
            t.ar_uses[t.use_base + row] = u;
        }
    }
}

int launch_stroke_expand(const StrokeTables &t, int n_recs, hipStream_t stream) {
    if (n_recs <= 0) return 0;
    if (t.nb > STROKE_MAX_BUFFERS) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(stroke_expand_kernel, dim3((unsigned)n_recs), dim3(64), sizeof(int) * (size_t)t.nb, stream, t);
    return (int)hipGetLastError();
}

}  // namespace pbso
