// What the engine's sides of the scene buses (scene_mix.cpp, scene_fir.cpp, scene_reverb.cpp, master.cpp) have in common, and
// nothing of what is particular to one: device and pinned memory that frees itself, the exact-size grow, the double-buffered
// history, the ring of pinned uploads, the growable staging of a step's scheduled sets, the engine-owned output, and
// (bus_clock.h, free of HIP) the step clock, the cross-fade clock and the ramp.  Included by those four files only; a bus knows
// this header and none of the other buses.
//
// A bus's struct is freed behind a synchronisation of the stream (its *_release), or before anything was launched on its
// memory (a failed enable, where the struct leaves its scope).
#pragma once

#include <algorithm>
#include <memory>

#include "bus_clock.h"
#include "engine.h"

namespace pbso {

// device memory of E, owned: `cap` elements (grow() and HistPair allocate at least one; alloc(0) leaves p null, which is freed as nothing)
template <typename E>
struct DevMem {
    E *p = nullptr;
    size_t cap = 0;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { if (p) (void)hipFree(p); }
    operator E *() const { return p; }
    hipError_t alloc(size_t n) {                         // once, n elements
        const hipError_t e = hipMalloc((void **)&p, n * sizeof(E));
        if (e != hipSuccess) p = nullptr;
        else cap = n;
        return e;
    }
};

// at least n elements in b, exactly n when it has to be allocated; the old block may still be read by a call in flight on the
// stream, so it is freed behind a synchronisation
template <typename E>
hipError_t grow(DevMem<E> &b, size_t n, hipStream_t s) {
    if (b.p && n <= b.cap) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    e = hipMalloc((void **)&b.p, std::max<size_t>(n, 1) * sizeof(E));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return e;
    }
    b.cap = n;
    return hipSuccess;
}
// inside a member of Engine, around a call that may grow: out of memory and any other failure end it with the messages given
// (both are passed because the buses word them differently and the texts are kept: "scene_mix: cannot allocate the output" /
//  "scene_mix: output" against the master bus's "master: output: cannot allocate" / "master: output")
#define GROWTRY(expr, nomem_msg, hip_msg)                                                                                 \
    do {                                                                                                                  \
        hipError_t _e = (expr);                                                                                           \
        if (_e != hipSuccess) return _e == hipErrorOutOfMemory ? fail(PBSO_ERR_NOMEM, nomem_msg) : hip_fail(_e, hip_msg); \
    } while (0)

// the samples before the next step, double-buffered: a call reads cur() and writes next(), then flips
struct HistPair {
    DevMem<float> h[2];
    int at = 0;
    hipError_t create(size_t floats, hipStream_t s) {                     // both silent, on the stream
        for (DevMem<float> &b : h) {
            hipError_t e = b.alloc(std::max<size_t>(floats, 1));
            if (e == hipSuccess) e = hipMemsetAsync(b.p, 0, b.cap * sizeof(float), s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    hipError_t reset(hipStream_t s) {                                     // back to silence
        for (DevMem<float> &b : h) {
            hipError_t e = hipMemsetAsync(b.p, 0, b.cap * sizeof(float), s);
            if (e != hipSuccess) return e;
        }
        at = 0;
        return hipSuccess;
    }
    const float *cur() const { return h[at].p; }
    float *next() const { return h[at ^ 1].p; }
    void flip() { at ^= 1; }
};

// Pinned staging of uploads in a ring: a caller that sets new values every step waits for nothing as long as it is less than
// UP_SLOTS steps ahead of the device.  A slot is rewritten only once the copy that last read it is done.
struct UploadRing {
    static constexpr int UP_SLOTS = 3;
    enum Created { OK, NO_MEMORY, NO_EVENT };
    char *block[UP_SLOTS] = {};
    hipEvent_t ev[UP_SLOTS] = {};                        // the upload from that slot has left it
    bool used[UP_SLOTS] = {};
    int slot = 0;
    UploadRing() = default;
    UploadRing(const UploadRing &) = delete;
    UploadRing &operator=(const UploadRing &) = delete;
    ~UploadRing() {
        for (int i = 0; i < UP_SLOTS; ++i) {
            if (block[i]) (void)hipHostFree(block[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
    Created create(size_t bytes) {
        for (int i = 0; i < UP_SLOTS; ++i) {
            if (hipHostMalloc((void **)&block[i], bytes, hipHostMallocDefault) != hipSuccess) { block[i] = nullptr; return NO_MEMORY; }
            if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { ev[i] = nullptr; return NO_EVENT; }
        }
        return OK;
    }
    // the next slot's block, once its last copy has left it
    hipError_t acquire(char *&b) {
        b = block[slot];
        return used[slot] ? hipEventSynchronize(ev[slot]) : hipSuccess;
    }
    // the copies from the acquired block are on the stream
    hipError_t record(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev[slot], s);
        if (e != hipSuccess) return e;
        used[slot] = true;
        slot = (slot + 1) % UP_SLOTS;
        return hipSuccess;
    }
};

// Pinned staging of one step's scheduled sets (the scene mix's and the filter mix's schedules), in a ring as UploadRing, but each
// slot grows to what a step needs.  A slot is rewritten (or freed for a larger one) only once the copy that last read it is done.
struct StagingRing {
    static constexpr int SLOTS = UploadRing::UP_SLOTS;
    char *block[SLOTS] = {};
    size_t cap[SLOTS] = {};
    hipEvent_t ev[SLOTS] = {};
    bool used[SLOTS] = {};
    int slot = 0;
    StagingRing() = default;
    StagingRing(const StagingRing &) = delete;
    StagingRing &operator=(const StagingRing &) = delete;
    ~StagingRing() {
        for (int i = 0; i < SLOTS; ++i) {
            if (block[i]) (void)hipHostFree(block[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
    // the next slot's block, at least `bytes` long, once its last copy has left it
    hipError_t acquire(size_t bytes, char *&b) {
        hipError_t e = hipSuccess;
        if (!ev[slot] && (e = hipEventCreateWithFlags(&ev[slot], hipEventDisableTiming)) != hipSuccess) { ev[slot] = nullptr; return e; }
        if (used[slot] && (e = hipEventSynchronize(ev[slot])) != hipSuccess) return e;
        used[slot] = false;
        if (cap[slot] < bytes) {
            if (block[slot]) (void)hipHostFree(block[slot]);
            block[slot] = nullptr;
            cap[slot] = 0;
            if ((e = hipHostMalloc((void **)&block[slot], bytes, hipHostMallocDefault)) != hipSuccess) { block[slot] = nullptr; return e; }
            cap[slot] = bytes;
        }
        b = block[slot];
        return hipSuccess;
    }
    hipError_t record(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev[slot], s);
        if (e != hipSuccess) return e;
        used[slot] = true;
        slot = (slot + 1) % SLOTS;
        return hipSuccess;
    }
};

// where a call writes: the caller's d_out, or (d_out NULL) a buffer the engine owns and read_*() copies from
struct BusOut {
    DevMem<float> own;
    const float *last = nullptr;                         // where the last call wrote, n_channels x last_nb x B floats
    int last_nb = 0;
    // out = d_out, or the engine-owned buffer grown to n floats
    hipError_t resolve(void *d_out, size_t n, hipStream_t s, float *&out) {
        out = (float *)d_out;
        if (out) return hipSuccess;
        const hipError_t e = grow(own, n, s);
        out = own;
        return e;
    }
    void wrote(const float *out, int nb) { last = out; last_nb = nb; }
};

inline int Engine::read_bus(const BusOut *o, int n_channels, const BusWords &w, float *out, size_t n) {
    const std::string name = std::string("read_") + w.name;
    if (!o || !o->last) return fail(PBSO_ERR_STATE, name + ": no " + w.result + " yet");
    if (!out) return fail(PBSO_ERR_INVALID, name + ": host_out is NULL");
    const size_t total = (size_t)n_channels * o->last_nb * B_;
    if (n != total) return fail(PBSO_ERR_INVALID, name + " size mismatch (n = " + w.channels + " * n_buffers * frames_per_buffer)");
    { int src = sync(); if (src != PBSO_OK) return src; }
    HIPTRY(hipMemcpy(out, o->last, total * sizeof(float), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

}  // namespace pbso
