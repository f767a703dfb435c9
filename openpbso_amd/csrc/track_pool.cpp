// Tracks: immutable mono f32 signals in device memory that PBSO_TRACK_FORCE messages play (include/openpbso_amd.h,
// pbso_track_create).  One pool of samples and one table of (offset, length) pairs per engine; K2 (kernels_exact.hip, track_add)
// reads both.  Tracks are never freed or moved apart: a new one goes behind the last, so kernels in flight -- which read only
// tracks that existed when their launch was planned -- are not disturbed by the upload.  Only when the pool or the table has to
// GROW does the call wait for the engine (Engine::sync: the submitting thread first, then every stream), copy, and free the
// old block; the launch arguments recorded for the submitting thread hold the pool's address by value.
#include <cmath>
#include <cstring>
#include <vector>

#include "engine.h"

namespace pbso {

struct TrackPool {
    float *d_pool = nullptr;
    long long *d_tab = nullptr;
    size_t pool_cap = 0, tab_cap = 0;                    // in samples / in tracks
    std::vector<long long> tab;                          // host copy of the table: (offset, length) per track
    int64_t samples = 0;
    std::vector<std::vector<float>> host;                // engines with host profiles (device_profiles < 0): the samples once more
};

void Engine::track_release() {
    if (!tracks_) return;
    if (tracks_->d_pool) (void)hipFree(tracks_->d_pool);
    if (tracks_->d_tab) (void)hipFree(tracks_->d_tab);
    delete tracks_;
    tracks_ = nullptr;
}

int64_t Engine::track_length(int track) const {
    if (!tracks_ || track < 0 || (size_t)track >= tracks_->tab.size() / 2) return -1;
    return tracks_->tab[2 * (size_t)track + 1];
}
const float *Engine::track_device_pool() const { return tracks_ ? tracks_->d_pool : nullptr; }
const long long *Engine::track_device_table() const { return tracks_ ? tracks_->d_tab : nullptr; }
const float *Engine::track_host_samples(int track) const {
    if (!tracks_ || track < 0 || (size_t)track >= tracks_->host.size()) return nullptr;
    return tracks_->host[(size_t)track].data();
}

void Engine::track_stats(int64_t out[4]) const {
    out[0] = tracks_ ? (int64_t)(tracks_->tab.size() / 2) : 0;
    out[1] = tracks_ ? tracks_->samples : 0;
    out[2] = track_msgs_.load();
    out[3] = track_rows_.load();
}

int Engine::track_create(const float *samples, int64_t n, int *track_id) {
    if (!samples || n < 1 || !track_id) return fail(PBSO_ERR_INVALID, "track_create: samples, n >= 1 and track_id are required");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(samples[i])) return fail(PBSO_ERR_INVALID, "track_create: every sample must be finite");
    if (hipSetDevice(desc_.device) != hipSuccess) return hip_fail(hipGetLastError(), "hipSetDevice");
    if (!tracks_) tracks_ = new TrackPool();
    TrackPool &t = *tracks_;
    const size_t n_tracks = t.tab.size() / 2;
    const size_t need_pool = (size_t)t.samples + (size_t)n, need_tab = n_tracks + 1;
    if (need_pool > t.pool_cap || need_tab > t.tab_cap) {
        // launches in flight (and the calls the submitting thread has not made yet) hold the old addresses
        if (finalized_) { int src = sync(); if (src != PBSO_OK) return src; }
        if (need_pool > t.pool_cap) {
            const size_t ncap = std::max(need_pool + need_pool / 4, t.pool_cap + t.pool_cap / 2);
            float *np = nullptr;
            hipError_t e = hipMalloc((void **)&np, ncap * sizeof(float));
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(track pool)");
            if (t.d_pool && t.samples) {
                e = hipMemcpy(np, t.d_pool, (size_t)t.samples * sizeof(float), hipMemcpyDeviceToDevice);
                if (e != hipSuccess) { (void)hipFree(np); return hip_fail(e, "hipMemcpy(track pool)"); }
            }
            if (t.d_pool) (void)hipFree(t.d_pool);
            t.d_pool = np;
            t.pool_cap = ncap;
        }
        if (need_tab > t.tab_cap) {
            const size_t ncap = std::max<size_t>(need_tab + need_tab / 4 + 15, t.tab_cap + t.tab_cap / 2);
            long long *nt = nullptr;
            hipError_t e = hipMalloc((void **)&nt, ncap * 2 * sizeof(long long));
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(track table)");
            if (!t.tab.empty()) {
                e = hipMemcpy(nt, t.tab.data(), t.tab.size() * sizeof(long long), hipMemcpyHostToDevice);
                if (e != hipSuccess) { (void)hipFree(nt); return hip_fail(e, "hipMemcpy(track table)"); }
            }
            if (t.d_tab) (void)hipFree(t.d_tab);
            t.d_tab = nt;
            t.tab_cap = ncap;
        }
    }
    // the samples are in device memory when the call returns (a blocking copy): the caller's array is free again
    hipError_t e = hipMemcpy(t.d_pool + t.samples, samples, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(track samples)");
    const long long rec[2] = {(long long)t.samples, (long long)n};
    e = hipMemcpy(t.d_tab + 2 * n_tracks, rec, sizeof(rec), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(track table entry)");
    t.tab.push_back(rec[0]);
    t.tab.push_back(rec[1]);
    t.samples += n;
    if (desc_.device_profiles < 0) t.host.emplace_back(samples, samples + n);
    *track_id = (int)n_tracks;
    return PBSO_OK;
}

}  // namespace pbso
