// Device group: one engine per GPU, objects sharded over the ranks, RCCL only to gather the finished audio
// (include/openpbso_amd.h "device group").  Objects never interact (modal_solver.h:100-126), so
// stepping needs no exchange; this file is host-side plumbing over the C ABI of the single engine plus three collectives.
// librccl is loaded at run time (dlopen) when a group of more than one rank is created -- or when a test asks for the
// communicator of a one-rank group (PBSO_GROUP_RCCL_ALWAYS) --: an engine alone does not need it, and this file does not
// need RCCL's headers to build (the dozen declarations it uses are below).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/openpbso_amd.h"
#include "kernels.h"

namespace pbso {
// capi.cpp: pbso_set_material's validation alone (nothing changes)
int material_check(pbso_engine *e, int n, const int *object_ids, const pbso_material *materials);
}  // namespace pbso

namespace {

// ---- the part of RCCL's C API this file calls (rccl/rccl.h; the values are NCCL's ABI)
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[PBSO_GROUP_ID_BYTES]; } ncclUniqueId;
// (fixed underlying type: the library returns codes this file does not name -- values outside a plain enum's range would be
//  undefined behaviour)
enum ncclResult_t : int { ncclSuccess = 0 };
enum ncclDataType_t : int { ncclFloat = 7 };
enum ncclRedOp_t : int { ncclSum = 0 };
static_assert(sizeof(ncclUniqueId) == 128, "NCCL_UNIQUE_ID_BYTES");

struct Rccl {
    void *lib = nullptr;
    bool ok = false;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int *) = nullptr;
    int version = 0;
    std::string err;
    bool load() {
        if (lib) return ok;                              // (a library that lacks a symbol stays unusable: no second try through null pointers)
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("librccl not found: ") + dlerror(); return false; }
        bool all = true;
        auto sym = [&](auto &fp, const char *n) {
            fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(lib, n));
            if (!fp) { all = false; err = std::string("librccl lacks ") + n; }
        };
        sym(GetUniqueId, "ncclGetUniqueId"); sym(CommInitRank, "ncclCommInitRank"); sym(CommInitAll, "ncclCommInitAll");
        sym(CommDestroy, "ncclCommDestroy"); sym(AllGather, "ncclAllGather"); sym(AllReduce, "ncclAllReduce");
        sym(Send, "ncclSend"); sym(Recv, "ncclRecv"); sym(GroupStart, "ncclGroupStart"); sym(GroupEnd, "ncclGroupEnd");
        sym(GetErrorString, "ncclGetErrorString"); sym(GetVersion, "ncclGetVersion");
        // the declarations above are NCCL 2's ABI (ncclFloat = 7, a 128-byte id, ncclSum = 0: unchanged since 2.0): refuse anything else
        if (all && (GetVersion(&version) != ncclSuccess || version < 2000)) {
            all = false;
            err = "librccl reports version " + std::to_string(version) + ": not the NCCL 2 ABI this file declares";
        }
        ok = all;
        return ok;
    }
};
Rccl g_rccl;

struct Rank {
    int rank = 0, device = 0;
    pbso_engine *eng = nullptr;
    hipStream_t stream = nullptr, coll = nullptr;        // the engine's launch stream; the collective's stream
    ncclComm_t comm = nullptr;
    float *target[2] = {nullptr, nullptr};               // gather targets [rows_total][row] (ALL / ROOT on rank 0) or the rank's own rows
    float *mix[2] = {nullptr, nullptr};                  // [row]
    float *scratch = nullptr;                            // RCCL_ALWAYS, one rank: where the send to itself lands; LOOPBACK: [world][row] mix rows + the sum's partial rows
    size_t target_floats = 0, mix_floats = 0, scratch_floats = 0;
    float *scene[2] = {nullptr, nullptr};                // PBSO_GATHER_SCENE: [C][row]
    float *scene_scratch = nullptr;                      // ... LOOPBACK: [world][C * row] the ranks' mixes + the sum's partial rows + the result
    size_t scene_floats = 0, scene_scratch_floats = 0;
    hipEvent_t ev_step[2] = {nullptr, nullptr}, ev_coll[2] = {nullptr, nullptr};
    int n_local = 0, next_local = 0;
};

}  // namespace

struct pbso_group {
    pbso_engine_desc edesc;
    std::vector<Rank> ranks;                             // the LOCAL ranks
    int world = 0, first = 0;
    std::vector<int> cuts;                               // world + 1 cut points: rank r owns global ids [cuts[r], cuts[r + 1])
    int n_objects = 0, cmax = 0;
    bool planned = false, finalized = false;
    int slot = 0, last_nb = 0, last_mode = 0, last_slot = -1;
    bool stepped = false;
    int transport = PBSO_GROUP_RCCL;
    int scene_c = 0, scene_max_delay = 0;                // the scene mixer (pbso_group_scene_mix_enable)
    bool scene_on = false, scene_mixed = false;          // ... and whether the last step has had its PBSO_GATHER_SCENE
    int fir_c = 0, fir_k = 0, fir_max_onset = 0;         // the scene filter mix (pbso_group_scene_fir_enable)
    int fir_max_delay = 0;                               // ... its delay stage (pbso_group_scene_fir_delay_enable)
    bool fir_delay_on = false;
    int fir_bank_f = 0;                                  // ... its bank (pbso_group_scene_fir_bank_create): F, and A = max |tap|
    double fir_bank_a = 0.0;
    bool fir_on = false, fir_mixed = false;              // ... and whether the last step has had its PBSO_GATHER_FIR
    bool use_rccl = false;                               // a communicator exists: the collectives go through librccl
    bool loopback() const { return transport == PBSO_GROUP_LOOPBACK; }
    std::string err;
    int frames = PBSO_FRAMES_PER_BUFFER;
};

namespace {

int gfail(pbso_group *g, int code, const std::string &m) {
    if (g) g->err = m;
    return code;
}
#define GHIP(g, expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return gfail(g, PBSO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define GNCCL(g, expr)                                                                            \
    do {                                                                                          \
        ncclResult_t _r = (expr);                                                                 \
        if (_r != ncclSuccess) return gfail(g, PBSO_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(_r)); \
    } while (0)
// ... between ncclGroupStart and ncclGroupEnd: the group is closed before the error is returned (an open group would swallow
// every later call of this thread)
#define GNCCL_OPEN(g, expr)                                                                       \
    do {                                                                                          \
        ncclResult_t _r = (expr);                                                                 \
        if (_r != ncclSuccess) {                                                                  \
            (void)g_rccl.GroupEnd();                                                              \
            return gfail(g, PBSO_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(_r)); \
        }                                                                                         \
    } while (0)
#define GHIP_OPEN(g, expr)                                                                        \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            (void)g_rccl.GroupEnd();                                                              \
            return gfail(g, PBSO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
        }                                                                                         \
    } while (0)
#define GENG(g, rk, expr)                                                                         \
    do {                                                                                          \
        int _c = (expr);                                                                          \
        if (_c < 0) return gfail(g, _c, std::string("rank ") + std::to_string((rk).rank) + ": " + pbso_last_error((rk).eng)); \
    } while (0)

// loopback all-reduce: [world mix rows | partial rows of the sum | the result row]
float *loop_mix_out(const pbso_group *g, const Rank &rk, size_t row) {
    return rk.scratch + (size_t)(g->world + pbso::mix_objects_groups(g->world)) * row;
}

// loopback all-reduce of the scene mix: [world scene mixes | partial rows of the sum | the result], each C * row floats
float *scene_loop_out(const pbso_group *g, const Rank &rk, size_t count) {
    return rk.scene_scratch + (size_t)(g->world + pbso::mix_objects_groups(g->world)) * count;
}

Rank *local_rank(pbso_group *g, int rank) {
    const int i = rank - g->first;
    return i >= 0 && i < (int)g->ranks.size() ? &g->ranks[i] : nullptr;
}

int ensure_buffers(pbso_group *g, Rank &rk, int nb, int mode) {
    const size_t row = (size_t)nb * g->frames;
    const bool full = mode == PBSO_GATHER_ALL || (mode == PBSO_GATHER_ROOT && rk.rank == 0);
    const size_t want = row * (size_t)(full ? g->world * g->cmax : std::max(1, g->cmax));
    GHIP(g, hipSetDevice(rk.device));
    if (want > rk.target_floats) {
        GHIP(g, hipStreamSynchronize(rk.stream));
        GHIP(g, hipStreamSynchronize(rk.coll));
        for (int s = 0; s < 2; ++s) {
            if (rk.target[s]) GHIP(g, hipFree(rk.target[s]));
            GHIP(g, hipMalloc(&rk.target[s], want * sizeof(float)));
            GHIP(g, hipMemsetAsync(rk.target[s], 0, want * sizeof(float), rk.stream));     // (padding rows of ragged shards stay silent)
        }
        rk.target_floats = want;
    }
    if (row > rk.mix_floats) {
        GHIP(g, hipStreamSynchronize(rk.coll));
        for (int s = 0; s < 2; ++s) {
            if (rk.mix[s]) GHIP(g, hipFree(rk.mix[s]));
            GHIP(g, hipMalloc(&rk.mix[s], row * sizeof(float)));
        }
        rk.mix_floats = row;
    }
    size_t want_scratch = 0;
    if (g->loopback()) want_scratch = row * (size_t)(g->world + pbso::mix_objects_groups(g->world) + 1);
    else if (g->use_rccl && g->world == 1) want_scratch = row * (size_t)std::max(1, g->cmax);
    if (want_scratch > rk.scratch_floats) {
        GHIP(g, hipStreamSynchronize(rk.coll));
        if (rk.scratch) GHIP(g, hipFree(rk.scratch));
        GHIP(g, hipMalloc(&rk.scratch, want_scratch * sizeof(float)));
        rk.scratch_floats = want_scratch;
    }
    return PBSO_OK;
}

// the scene mix's buffers of every local rank: count = C * row floats (a block that grows is freed once nothing reads it: the
// loopback ranks' collectives read each other's)
int ensure_scene_buffers(pbso_group *g, size_t count) {
    const size_t want_scratch = g->loopback() ? count * (size_t)(g->world + pbso::mix_objects_groups(g->world) + 1) : 0;
    bool grow = false;
    for (Rank &rk : g->ranks) grow = grow || count > rk.scene_floats || want_scratch > rk.scene_scratch_floats;
    if (!grow) return PBSO_OK;
    for (Rank &rk : g->ranks) {
        GHIP(g, hipSetDevice(rk.device));
        GHIP(g, hipStreamSynchronize(rk.stream));
        GHIP(g, hipStreamSynchronize(rk.coll));
    }
    for (Rank &rk : g->ranks) {
        GHIP(g, hipSetDevice(rk.device));
        if (count > rk.scene_floats) {
            for (float *&p : rk.scene) {
                if (p) GHIP(g, hipFree(p));
                p = nullptr;
                GHIP(g, hipMalloc(&p, count * sizeof(float)));
            }
            rk.scene_floats = count;
        }
        if (want_scratch > rk.scene_scratch_floats) {
            if (rk.scene_scratch) GHIP(g, hipFree(rk.scene_scratch));
            rk.scene_scratch = nullptr;
            GHIP(g, hipMalloc(&rk.scene_scratch, want_scratch * sizeof(float)));
            rk.scene_scratch_floats = want_scratch;
        }
    }
    return PBSO_OK;
}

}  // namespace

extern "C" {

int pbso_group_unique_id(void *out) {
    if (!out) return PBSO_ERR_INVALID;
    if (!g_rccl.load()) return PBSO_ERR_HIP;
    static_assert(sizeof(ncclUniqueId) == PBSO_GROUP_ID_BYTES, "PBSO_GROUP_ID_BYTES");
    ncclUniqueId id;
    if (g_rccl.GetUniqueId(&id) != ncclSuccess) return PBSO_ERR_HIP;
    std::memcpy(out, &id, sizeof(id));
    return PBSO_OK;
}

const char *pbso_group_last_error(const pbso_group *g) { return g ? g->err.c_str() : "null group"; }

int pbso_group_create(const pbso_group_desc *d, pbso_group **out) {
    if (!d || !out) return PBSO_ERR_INVALID;
    *out = nullptr;
    pbso_group *g = nullptr;
    try {
        g = new pbso_group();
        *out = g;                                        // (kept alive on failure so that the caller can read the error text)
        if (d->abi_version != PBSO_ABI_VERSION) return gfail(g, PBSO_ERR_INVALID, "abi_version mismatch");
        if (d->n_devices < 1 || !d->devices) return gfail(g, PBSO_ERR_INVALID, "a group needs at least one device");
        g->world = d->world_size > 0 ? d->world_size : d->n_devices;
        g->first = d->first_rank;
        if (g->first < 0 || g->first + d->n_devices > g->world) return gfail(g, PBSO_ERR_INVALID, "first_rank + n_devices exceeds world_size");
        g->transport = d->transport;
        if (g->transport != PBSO_GROUP_RCCL && g->transport != PBSO_GROUP_RCCL_ALWAYS && g->transport != PBSO_GROUP_LOOPBACK)
            return gfail(g, PBSO_ERR_INVALID, "transport");
        if (g->loopback()) {
            // every rank of the job in this process, any of them on any device (the same one, typically): the collectives are
            // device copies -- what the group does AROUND them (shards, padding, slices, the two targets, the events) is the product's
            if (g->world != d->n_devices || g->first != 0) return gfail(g, PBSO_ERR_INVALID, "the loopback transport holds every rank of the job in one process");
        } else {
            if (g->world > d->n_devices && !d->unique_id) return gfail(g, PBSO_ERR_INVALID, "a job of several processes needs the shared unique_id");
            for (int i = 0; i < d->n_devices; ++i)
                for (int j = 0; j < i; ++j)
                    if (d->devices[i] == d->devices[j]) return gfail(g, PBSO_ERR_INVALID, "a device appears twice (one rank per GPU)");
        }
        g->edesc = d->engine;
        g->edesc.abi_version = PBSO_ABI_VERSION;
        g->edesc.submit_thread = 0;          // (the group puts its collectives on the ranks' streams right behind a step: no deferred launches)
        g->frames = d->engine.frames_per_buffer > 0 ? d->engine.frames_per_buffer : PBSO_FRAMES_PER_BUFFER;
        int ndev = 0;
        GHIP(g, hipGetDeviceCount(&ndev));
        if (ndev <= 0) return gfail(g, PBSO_ERR_HIP, "no HIP device: this engine has no CPU fallback");
        g->ranks.resize(d->n_devices);
        for (int i = 0; i < d->n_devices; ++i) {
            Rank &rk = g->ranks[i];
            rk.rank = g->first + i;
            rk.device = d->devices[i];
            if (rk.device < 0 || rk.device >= ndev) return gfail(g, PBSO_ERR_INVALID, "device ordinal out of range");
            GHIP(g, hipSetDevice(rk.device));
            GHIP(g, hipStreamCreateWithFlags(&rk.stream, hipStreamNonBlocking));
            GHIP(g, hipStreamCreateWithFlags(&rk.coll, hipStreamNonBlocking));
            for (int s = 0; s < 2; ++s) {
                GHIP(g, hipEventCreateWithFlags(&rk.ev_step[s], hipEventDisableTiming));
                GHIP(g, hipEventCreateWithFlags(&rk.ev_coll[s], hipEventDisableTiming));
            }
            pbso_engine_desc ed = g->edesc;
            ed.device = rk.device;
            ed.stream = rk.stream;
            int rc = pbso_engine_create(&ed, &rk.eng);
            if (rc != PBSO_OK) return gfail(g, rc, std::string("engine on device ") + std::to_string(rk.device) + ": " + (rk.eng ? pbso_last_error(rk.eng) : "create failed"));
        }
        g->use_rccl = !g->loopback() && (g->world > 1 || g->transport == PBSO_GROUP_RCCL_ALWAYS);
        if (g->use_rccl) {
            if (!g_rccl.load()) return gfail(g, PBSO_ERR_HIP, g_rccl.err);
            if (g->world == 1) {
                // (tests: a communicator of one rank, created the way a rank of a larger job creates its own)
                ncclUniqueId id;
                if (d->unique_id) std::memcpy(&id, d->unique_id, sizeof(id));
                else GNCCL(g, g_rccl.GetUniqueId(&id));
                GHIP(g, hipSetDevice(g->ranks[0].device));
                GNCCL(g, g_rccl.CommInitRank(&g->ranks[0].comm, 1, id, 0));
            } else if (g->world == d->n_devices) {
                std::vector<ncclComm_t> comms(d->n_devices);
                GNCCL(g, g_rccl.CommInitAll(comms.data(), d->n_devices, d->devices));
                for (int i = 0; i < d->n_devices; ++i) g->ranks[i].comm = comms[i];
            } else {
                ncclUniqueId id;
                std::memcpy(&id, d->unique_id, sizeof(id));
                GNCCL(g, g_rccl.GroupStart());
                for (Rank &rk : g->ranks) {
                    GHIP_OPEN(g, hipSetDevice(rk.device));
                    GNCCL_OPEN(g, g_rccl.CommInitRank(&rk.comm, g->world, id, rk.rank));
                }
                GNCCL(g, g_rccl.GroupEnd());
            }
        }
        return PBSO_OK;
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
}

void pbso_group_destroy(pbso_group *g) {
    if (!g) return;
    for (Rank &rk : g->ranks) {
        (void)hipSetDevice(rk.device);
        if (rk.stream) (void)hipStreamSynchronize(rk.stream);
        if (rk.coll) (void)hipStreamSynchronize(rk.coll);
        if (rk.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(rk.comm);
        if (rk.eng) pbso_engine_destroy(rk.eng);
        for (int s = 0; s < 2; ++s) {
            if (rk.target[s]) (void)hipFree(rk.target[s]);
            if (rk.mix[s]) (void)hipFree(rk.mix[s]);
            if (rk.scene[s]) (void)hipFree(rk.scene[s]);
            if (s == 0 && rk.scene_scratch) (void)hipFree(rk.scene_scratch);
            if (s == 0 && rk.scratch) (void)hipFree(rk.scratch);
            if (rk.ev_step[s]) (void)hipEventDestroy(rk.ev_step[s]);
            if (rk.ev_coll[s]) (void)hipEventDestroy(rk.ev_coll[s]);
        }
        if (rk.coll) (void)hipStreamDestroy(rk.coll);
        if (rk.stream) (void)hipStreamDestroy(rk.stream);
    }
    delete g;
}

// shards balanced by the sum of modes: the cut points are the object boundaries nearest to the ideal prefix sums
// k / world of the total (the same rule as openpbso_amd/distributed.py shard_by_modes: every rank computes the same cuts)
int pbso_shard_by_modes(const int *modes, int n, int world, int *cuts) {
    if (n < 0 || world < 1 || !cuts || (n > 0 && !modes)) return PBSO_ERR_INVALID;
    std::vector<long long> prefix(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (modes[i] < 0) return PBSO_ERR_INVALID;
        prefix[i + 1] = prefix[i] + modes[i];
    }
    const long long total = prefix[n];
    cuts[0] = 0;
    for (int k = 1; k < world; ++k) {
        int c;
        if (total == 0) {
            const int base = n / world, rem = n % world;
            c = k * base + std::min(k, rem);
        } else {
            const double target = (double)total * k / world;
            c = (int)(std::lower_bound(prefix.begin() + cuts[k - 1], prefix.end(), target,
                                       [](long long p, double t) { return (double)p < t; }) - prefix.begin());
            c = std::min(c, n);
            if (c > cuts[k - 1] && target - (double)prefix[c - 1] < (double)prefix[c] - target) c -= 1;
        }
        cuts[k] = std::max(c, cuts[k - 1]);
    }
    cuts[world] = n;
    return PBSO_OK;
}

int pbso_group_plan(pbso_group *g, const int *modes, int n) {
    if (!g || n < 0 || (n > 0 && !modes)) return gfail(g, PBSO_ERR_INVALID, "plan arguments");
    if (g->planned) return gfail(g, PBSO_ERR_STATE, "plan called twice");
    g->cuts.assign((size_t)g->world + 1, 0);
    if (pbso_shard_by_modes(modes, n, g->world, g->cuts.data()) != PBSO_OK) return gfail(g, PBSO_ERR_INVALID, "negative mode count");
    g->n_objects = n;
    g->cmax = 0;
    for (int r = 0; r < g->world; ++r) g->cmax = std::max(g->cmax, g->cuts[r + 1] - g->cuts[r]);
    for (Rank &rk : g->ranks) rk.n_local = g->cuts[rk.rank + 1] - g->cuts[rk.rank];
    g->planned = true;
    return PBSO_OK;
}

int pbso_group_rank_span(pbso_group *g, int rank, int *lo, int *hi) {
    if (!g || !g->planned || rank < 0 || rank >= g->world) return gfail(g, PBSO_ERR_INVALID, "rank_span arguments (plan first)");
    if (lo) *lo = g->cuts[rank];
    if (hi) *hi = g->cuts[rank + 1];
    return PBSO_OK;
}

int pbso_group_owner(pbso_group *g, int id, int *rank, int *local_id) {
    if (!g || !g->planned || id < 0 || id >= g->n_objects) return gfail(g, PBSO_ERR_INVALID, "owner arguments (plan first)");
    const int r = (int)(std::upper_bound(g->cuts.begin(), g->cuts.end(), id) - g->cuts.begin()) - 1;
    if (rank) *rank = r;
    if (local_id) *local_id = id - g->cuts[r];
    return PBSO_OK;
}

int pbso_group_add_object(pbso_group *g, int id, const pbso_object_desc *d) {
    if (!g || !d) return PBSO_ERR_INVALID;
    int r = 0, l = 0;
    int rc = pbso_group_owner(g, id, &r, &l);
    if (rc != PBSO_OK) return rc;
    Rank *rk = local_rank(g, r);
    if (!rk) return PBSO_OK;                              // another process builds it
    if (l != rk->next_local) return gfail(g, PBSO_ERR_STATE, "objects of a rank are added in ascending id order");
    int got = -1;
    GENG(g, *rk, pbso_add_object(rk->eng, d, &got));
    if (got != l) return gfail(g, PBSO_ERR_STATE, "engine numbered the object differently");
    rk->next_local += 1;
    return PBSO_OK;
}

int pbso_group_finalize(pbso_group *g) {
    if (!g || !g->planned) return gfail(g, PBSO_ERR_STATE, "finalize before plan");
    for (Rank &rk : g->ranks) {
        if (rk.next_local != rk.n_local) return gfail(g, PBSO_ERR_STATE, "rank " + std::to_string(rk.rank) + " is missing objects");
        if (rk.n_local > 0) GENG(g, rk, pbso_finalize(rk.eng));
    }
    g->finalized = true;
    return PBSO_OK;
}

pbso_engine *pbso_group_engine(pbso_group *g, int rank) {
    Rank *rk = g ? local_rank(g, rank) : nullptr;
    return rk ? rk->eng : nullptr;
}

int pbso_group_enqueue_force(pbso_group *g, int id, const pbso_force_msg *m, int64_t not_before) {
    int r = 0, l = 0;
    int rc = pbso_group_owner(g, id, &r, &l);
    if (rc != PBSO_OK) return rc;
    Rank *rk = local_rank(g, r);
    if (!rk) return 1;
    int took = pbso_enqueue_force(rk->eng, l, m, not_before);
    if (took < 0) return gfail(g, took, pbso_last_error(rk->eng));
    return took;
}

int pbso_group_set_material(pbso_group *g, int n, const int *ids, const pbso_material *mats, int keep_state) {
    if (!g || !g->finalized) return gfail(g, PBSO_ERR_STATE, "set_material before finalize");
    if (n < 0 || (n > 0 && (!ids || !mats))) return gfail(g, PBSO_ERR_INVALID, "set_material arguments");
    // every rank's share, in call order; then all of them checked before the first one is taken
    std::vector<std::vector<int>> lid(g->ranks.size());
    std::vector<std::vector<pbso_material>> lmat(g->ranks.size());
    std::vector<unsigned char> named(g->n_objects, 0);
    for (int i = 0; i < n; ++i) {
        int r = 0, l = 0;
        int rc = pbso_group_owner(g, ids[i], &r, &l);
        if (rc != PBSO_OK) return gfail(g, PBSO_ERR_INVALID, "set_material: object id out of range");
        if (named[ids[i]]) return gfail(g, PBSO_ERR_INVALID, "set_material: an object id is named twice");
        named[ids[i]] = 1;
        if (!local_rank(g, r)) continue;                  // its owner does it
        lid[r - g->first].push_back(l);
        lmat[r - g->first].push_back(mats[i]);
    }
    for (size_t k = 0; k < g->ranks.size(); ++k)
        if (!lid[k].empty()) GENG(g, g->ranks[k], pbso::material_check(g->ranks[k].eng, (int)lid[k].size(), lid[k].data(), lmat[k].data()));
    for (size_t k = 0; k < g->ranks.size(); ++k)
        if (!lid[k].empty()) GENG(g, g->ranks[k], pbso_set_material(g->ranks[k].eng, (int)lid[k].size(), lid[k].data(), lmat[k].data(), keep_state));
    return PBSO_OK;
}

int pbso_group_step(pbso_group *g, int nb) {
    if (!g || !g->finalized) return gfail(g, PBSO_ERR_STATE, "step before finalize");
    if (nb <= 0) return gfail(g, PBSO_ERR_INVALID, "n_buffers must be > 0");
    const int slot = g->slot;
    const size_t row = (size_t)nb * g->frames;
    for (Rank &rk : g->ranks) {
        // (the target doubles as the all-gather's receive buffer: sized for that from the start, so the engine's slice never moves)
        int rc = ensure_buffers(g, rk, nb, PBSO_GATHER_ALL);
        if (rc != PBSO_OK) return rc;
        GHIP(g, hipSetDevice(rk.device));
        // the collective that last read this target is done (loopback: the OTHER ranks' copies read this rank's slice)
        if (g->loopback()) for (Rank &other : g->ranks) GHIP(g, hipStreamWaitEvent(rk.stream, other.ev_coll[slot], 0));
        else GHIP(g, hipStreamWaitEvent(rk.stream, rk.ev_coll[slot], 0));
        float *mine = rk.target[slot] + (size_t)rk.rank * g->cmax * row;
        // Ragged shards: the rows behind this rank's objects are shipped to every rank with the all-gather and must be SILENT.
        // The row layout depends on n_buffers, so a step shorter than an earlier one would find old samples there: zeroed
        // every step (a few rows), on the stream the step runs on.
        if (rk.n_local < g->cmax)
            GHIP(g, hipMemsetAsync(mine + (size_t)rk.n_local * row, 0, (size_t)(g->cmax - rk.n_local) * row * sizeof(float), rk.stream));
        if (rk.n_local > 0) GENG(g, rk, pbso_step_into(rk.eng, nb, mine));
        GHIP(g, hipEventRecord(rk.ev_step[slot], rk.stream));       // (an empty rank too: its silent rows are ordered before the collective)
    }
    g->last_slot = slot;
    g->last_nb = nb;
    g->last_mode = 0;
    g->slot ^= 1;
    g->stepped = true;
    g->scene_mixed = false;
    g->fir_mixed = false;
    return PBSO_OK;
}

int pbso_group_scene_mix_enable(pbso_group *g, int n_channels, int max_delay, int ramp_samples) {
    if (!g || !g->finalized) return gfail(g, PBSO_ERR_STATE, "scene_mix_enable before finalize");
    if (n_channels < 1 || n_channels > pbso::SCENE_MAX_CHANNELS || max_delay < 0 || max_delay > (1 << 20) || ramp_samples < 0 ||
        ramp_samples > (1 << 20))
        return gfail(g, PBSO_ERR_INVALID, "scene_mix_enable: n_channels 1 .. 8, max_delay and ramp_samples 0 .. 1 << 20");
    for (Rank &rk : g->ranks)                            // (an empty rank has no engine to mix: it contributes silence)
        if (rk.n_local > 0) GENG(g, rk, pbso_scene_mix_enable(rk.eng, n_channels, max_delay, ramp_samples));
    g->scene_on = true;
    g->scene_c = n_channels;
    g->scene_max_delay = max_delay;
    g->scene_mixed = true;                               // (armed for the next step, as every engine is)
    return PBSO_OK;
}

int pbso_group_scene_mix_set(pbso_group *g, const float *gain, const float *delay) {
    if (!g || !g->scene_on) return gfail(g, PBSO_ERR_STATE, "scene_mix_set: the group's scene mixer is not enabled");
    if (!gain) return gfail(g, PBSO_ERR_INVALID, "scene_mix_set: gain is NULL");
    const size_t n = (size_t)g->n_objects, cn = (size_t)g->scene_c * n;
    // checked for the whole job first: no rank takes a set that another one refuses
    for (size_t i = 0; i < cn; ++i) {
        if (!std::isfinite(gain[i])) return gfail(g, PBSO_ERR_INVALID, "scene_mix_set: a gain is not finite");
        if (delay && !(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)g->scene_max_delay))
            return gfail(g, PBSO_ERR_INVALID, "scene_mix_set: a delay is not finite or outside [0, max_delay]");
    }
    try {
        std::vector<float> gs, ds;
        for (Rank &rk : g->ranks) {
            if (rk.n_local == 0) continue;
            const size_t lo = (size_t)g->cuts[rk.rank], nl = (size_t)rk.n_local;
            gs.resize((size_t)g->scene_c * nl);
            ds.resize(delay ? gs.size() : 0);
            for (int c = 0; c < g->scene_c; ++c)
                for (size_t l = 0; l < nl; ++l) {
                    gs[c * nl + l] = gain[c * n + lo + l];
                    if (delay) ds[c * nl + l] = delay[c * n + lo + l];
                }
            GENG(g, rk, pbso_scene_mix_set(rk.eng, gs.data(), delay ? ds.data() : nullptr));
        }
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
    return PBSO_OK;
}

// the scene mix's schedule: every rank takes the slice of its own objects of every set, [n_sets][C][n_local].  The values are
// checked for the whole job first; the times are checked by the engines, which are mixed in lockstep and so hold one clock and one
// pending list: the first rank's refusal is every rank's, and no rank has taken anything by then.
static int group_scene_mix_schedule(pbso_group *g, const char *call, int n_sets, const int64_t *t_set, const float *gain, const float *delay) {
    const std::string name(call);
    if (!g || !g->scene_on) return gfail(g, PBSO_ERR_STATE, name + ": the group's scene mixer is not enabled");
    if (n_sets < 0) return gfail(g, PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set) return gfail(g, PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!gain) return gfail(g, PBSO_ERR_INVALID, name + ": gain is NULL");
    const size_t n = (size_t)g->n_objects, cn = (size_t)g->scene_c * n;
    for (size_t i = 0; i < (size_t)n_sets * cn; ++i) {
        if (!std::isfinite(gain[i])) return gfail(g, PBSO_ERR_INVALID, name + ": a gain is not finite");
        if (delay && !(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)g->scene_max_delay))
            return gfail(g, PBSO_ERR_INVALID, name + ": a delay is not finite or outside [0, max_delay]");
    }
    try {
        std::vector<float> gs, ds;
        for (Rank &rk : g->ranks) {
            if (rk.n_local == 0) continue;
            const size_t lo = (size_t)g->cuts[rk.rank], nl = (size_t)rk.n_local, cl = (size_t)g->scene_c * nl;
            gs.resize((size_t)n_sets * cl);
            ds.resize(delay ? gs.size() : 0);
            for (size_t k = 0; k < (size_t)n_sets; ++k)
                for (size_t c = 0; c < (size_t)g->scene_c; ++c)
                    for (size_t l = 0; l < nl; ++l) {
                        gs[k * cl + c * nl + l] = gain[k * cn + c * n + lo + l];
                        if (delay) ds[k * cl + c * nl + l] = delay[k * cn + c * n + lo + l];
                    }
            GENG(g, rk, pbso_scene_mix_schedule(rk.eng, n_sets, t_set, gs.data(), delay ? ds.data() : nullptr));
        }
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
    return PBSO_OK;
}

int pbso_group_scene_mix_set_at(pbso_group *g, int64_t t_set, const float *gain, const float *delay) {
    return group_scene_mix_schedule(g, "scene_mix_set_at", 1, &t_set, gain, delay);
}

int pbso_group_scene_mix_schedule(pbso_group *g, int n_sets, const int64_t *t_set, const float *gain, const float *delay) {
    return group_scene_mix_schedule(g, "scene_mix_schedule", n_sets, t_set, gain, delay);
}

int pbso_group_scene_mix_clear_schedule(pbso_group *g) {
    if (!g || !g->scene_on) return gfail(g, PBSO_ERR_STATE, "scene_mix_clear_schedule: the group's scene mixer is not enabled");
    for (Rank &rk : g->ranks)
        if (rk.n_local > 0) GENG(g, rk, pbso_scene_mix_clear_schedule(rk.eng));
    return PBSO_OK;
}

int pbso_group_scene_fir_enable(pbso_group *g, int n_channels, int n_taps, int max_onset, int xfade_samples) {
    if (!g || !g->finalized) return gfail(g, PBSO_ERR_STATE, "scene_fir_enable before finalize");
    if (n_channels < 1 || n_channels > pbso::SCENE_MAX_CHANNELS || n_taps < 1 || n_taps > pbso::SCENE_FIR_MAX_TAPS || max_onset < 0 ||
        max_onset > (1 << 20) || xfade_samples < 0 || xfade_samples > (1 << 20))
        return gfail(g, PBSO_ERR_INVALID, "scene_fir_enable: n_channels 1 .. 8, n_taps 1 .. 1024, max_onset and xfade_samples 0 .. 1 << 20");
    for (Rank &rk : g->ranks)                            // (an empty rank has no engine to mix: it contributes silence)
        if (rk.n_local > 0) GENG(g, rk, pbso_scene_fir_enable(rk.eng, n_channels, n_taps, max_onset, xfade_samples));
    g->fir_on = true;
    g->fir_c = n_channels;
    g->fir_k = n_taps;
    g->fir_max_onset = max_onset;
    g->fir_delay_on = false;                             // (a new enable drops the delay stage and the bank with everything else)
    g->fir_bank_f = 0;
    g->fir_mixed = true;                                 // (armed for the next step, as every engine is)
    return PBSO_OK;
}

int pbso_group_scene_fir_set(pbso_group *g, const float *taps, const int *onset) {
    if (!g || !g->fir_on) return gfail(g, PBSO_ERR_STATE, "scene_fir_set: the group's scene filter mix is not enabled");
    if (!taps) return gfail(g, PBSO_ERR_INVALID, "scene_fir_set: taps is NULL");
    const size_t n = (size_t)g->n_objects, K = (size_t)g->fir_k;
    // checked for the whole job first: no rank takes a set that another one refuses
    for (size_t i = 0; i < (size_t)g->fir_c * n * K; ++i)
        if (!std::isfinite(taps[i])) return gfail(g, PBSO_ERR_INVALID, "scene_fir_set: a tap is not finite");
    if (onset)
        for (size_t o = 0; o < n; ++o)
            if (onset[o] < 0 || onset[o] > g->fir_max_onset) return gfail(g, PBSO_ERR_INVALID, "scene_fir_set: an onset is outside [0, max_onset]");
    try {
        std::vector<float> ts;
        for (Rank &rk : g->ranks) {
            if (rk.n_local == 0) continue;
            const size_t lo = (size_t)g->cuts[rk.rank], nl = (size_t)rk.n_local;
            ts.resize((size_t)g->fir_c * nl * K);
            for (int c = 0; c < g->fir_c; ++c)
                std::copy(taps + (c * n + lo) * K, taps + (c * n + lo + nl) * K, ts.begin() + c * nl * K);
            GENG(g, rk, pbso_scene_fir_set(rk.eng, ts.data(), onset ? onset + lo : nullptr));
        }
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
    return PBSO_OK;
}

int pbso_group_scene_fir_delay_enable(pbso_group *g, int max_delay, int ramp_samples) {
    if (!g || !g->fir_on) return gfail(g, PBSO_ERR_STATE, "scene_fir_delay_enable: the group's scene filter mix is not enabled");
    if (max_delay < 0 || max_delay > (1 << 20) || ramp_samples < 0 || ramp_samples > (1 << 20))
        return gfail(g, PBSO_ERR_INVALID, "scene_fir_delay_enable: max_delay and ramp_samples 0 .. 1 << 20");
    for (Rank &rk : g->ranks)
        if (rk.n_local > 0) GENG(g, rk, pbso_scene_fir_delay_enable(rk.eng, max_delay, ramp_samples));
    g->fir_delay_on = true;
    g->fir_max_delay = max_delay;
    return PBSO_OK;
}

int pbso_group_scene_fir_set_delay(pbso_group *g, const float *delay) {
    if (!g || !g->fir_on || !g->fir_delay_on) return gfail(g, PBSO_ERR_STATE, "scene_fir_set_delay: the group's delay stage is not enabled");
    if (!delay) return gfail(g, PBSO_ERR_INVALID, "scene_fir_set_delay: delay is NULL");
    // checked for the whole job first: no rank takes a set that another one refuses
    for (size_t o = 0; o < (size_t)g->n_objects; ++o)
        if (!(std::isfinite(delay[o]) && delay[o] >= 0.f && delay[o] <= (float)g->fir_max_delay))
            return gfail(g, PBSO_ERR_INVALID, "scene_fir_set_delay: a delay is not finite or outside [0, max_delay]");
    for (Rank &rk : g->ranks)
        if (rk.n_local > 0) GENG(g, rk, pbso_scene_fir_set_delay(rk.eng, delay + g->cuts[rk.rank]));
    return PBSO_OK;
}

// the filter mix's schedule: every rank takes the slice of its own objects of every set.  The values are checked for the whole
// job first; the times are checked by the engines, which are mixed in lockstep and so hold one clock and one pending list: the
// first rank's refusal is every rank's, and no rank has taken anything by then.
static int group_scene_fir_schedule(pbso_group *g, const char *call, int n_sets, const int64_t *t_set, const float *taps, const int *onset) {
    const std::string name(call);
    if (!g || !g->fir_on) return gfail(g, PBSO_ERR_STATE, name + ": the group's scene filter mix is not enabled");
    if (n_sets < 0) return gfail(g, PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set) return gfail(g, PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!taps) return gfail(g, PBSO_ERR_INVALID, name + ": taps is NULL");
    const size_t n = (size_t)g->n_objects, K = (size_t)g->fir_k, C = (size_t)g->fir_c;
    for (size_t i = 0; i < (size_t)n_sets * C * n * K; ++i)
        if (!std::isfinite(taps[i])) return gfail(g, PBSO_ERR_INVALID, name + ": a tap is not finite");
    if (onset)
        for (size_t i = 0; i < (size_t)n_sets * n; ++i)
            if (onset[i] < 0 || onset[i] > g->fir_max_onset) return gfail(g, PBSO_ERR_INVALID, name + ": an onset is outside [0, max_onset]");
    try {
        std::vector<float> ts;
        std::vector<int> os;
        for (Rank &rk : g->ranks) {
            if (rk.n_local == 0) continue;
            const size_t lo = (size_t)g->cuts[rk.rank], nl = (size_t)rk.n_local;
            ts.resize((size_t)n_sets * C * nl * K);
            os.resize(onset ? (size_t)n_sets * nl : 0);
            for (size_t k = 0; k < (size_t)n_sets; ++k) {
                for (size_t c = 0; c < C; ++c)
                    std::copy(taps + ((k * C + c) * n + lo) * K, taps + ((k * C + c) * n + lo + nl) * K, ts.begin() + (k * C + c) * nl * K);
                if (onset) std::copy(onset + k * n + lo, onset + k * n + lo + nl, os.begin() + k * nl);
            }
            GENG(g, rk, pbso_scene_fir_schedule(rk.eng, n_sets, t_set, ts.data(), onset ? os.data() : nullptr));
        }
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
    return PBSO_OK;
}

static int group_scene_fir_delay_schedule(pbso_group *g, const char *call, int n_sets, const int64_t *t_set, const float *delay) {
    const std::string name(call);
    if (!g || !g->fir_on || !g->fir_delay_on) return gfail(g, PBSO_ERR_STATE, name + ": the group's delay stage is not enabled");
    if (n_sets < 0) return gfail(g, PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!t_set) return gfail(g, PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!delay) return gfail(g, PBSO_ERR_INVALID, name + ": delay is NULL");
    const size_t n = (size_t)g->n_objects;
    for (size_t i = 0; i < (size_t)n_sets * n; ++i)
        if (!(std::isfinite(delay[i]) && delay[i] >= 0.f && delay[i] <= (float)g->fir_max_delay))
            return gfail(g, PBSO_ERR_INVALID, name + ": a delay is not finite or outside [0, max_delay]");
    try {
        std::vector<float> ds;
        for (Rank &rk : g->ranks) {
            if (rk.n_local == 0) continue;
            const size_t lo = (size_t)g->cuts[rk.rank], nl = (size_t)rk.n_local;
            ds.resize((size_t)n_sets * nl);
            for (size_t k = 0; k < (size_t)n_sets; ++k) std::copy(delay + k * n + lo, delay + k * n + lo + nl, ds.begin() + k * nl);
            GENG(g, rk, pbso_scene_fir_delay_schedule(rk.eng, n_sets, t_set, ds.data()));
        }
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
    return PBSO_OK;
}

int pbso_group_scene_fir_set_at(pbso_group *g, int64_t t_set, const float *taps, const int *onset) {
    return group_scene_fir_schedule(g, "scene_fir_set_at", 1, &t_set, taps, onset);
}

int pbso_group_scene_fir_schedule(pbso_group *g, int n_sets, const int64_t *t_set, const float *taps, const int *onset) {
    return group_scene_fir_schedule(g, "scene_fir_schedule", n_sets, t_set, taps, onset);
}

int pbso_group_scene_fir_set_delay_at(pbso_group *g, int64_t t_set, const float *delay) {
    return group_scene_fir_delay_schedule(g, "scene_fir_set_delay_at", 1, &t_set, delay);
}

int pbso_group_scene_fir_delay_schedule(pbso_group *g, int n_sets, const int64_t *t_set, const float *delay) {
    return group_scene_fir_delay_schedule(g, "scene_fir_delay_schedule", n_sets, t_set, delay);
}

int pbso_group_scene_fir_clear_schedule(pbso_group *g) {
    if (!g || !g->fir_on) return gfail(g, PBSO_ERR_STATE, "scene_fir_clear_schedule: the group's scene filter mix is not enabled");
    for (Rank &rk : g->ranks)
        if (rk.n_local > 0) GENG(g, rk, pbso_scene_fir_clear_schedule(rk.eng));
    return PBSO_OK;
}

// the filter mix's bank: the whole bank on every rank (any object may use any filter)
int pbso_group_scene_fir_bank_create(pbso_group *g, int n_filters, const float *taps) {
    if (!g || !g->fir_on) return gfail(g, PBSO_ERR_STATE, "scene_fir_bank_create: the group's scene filter mix is not enabled");
    if (n_filters < 1 || n_filters > pbso::SCENE_FIR_BANK_MAX_FILTERS) return gfail(g, PBSO_ERR_INVALID, "scene_fir_bank_create: n_filters must be 1 .. 1 << 20");
    if (!taps) return gfail(g, PBSO_ERR_INVALID, "scene_fir_bank_create: taps is NULL");
    double A = 0.0;
    for (size_t i = 0; i < (size_t)n_filters * g->fir_c * g->fir_k; ++i) {
        if (!std::isfinite(taps[i])) return gfail(g, PBSO_ERR_INVALID, "scene_fir_bank_create: a tap is not finite");
        A = std::max(A, (double)std::fabs(taps[i]));
    }
    // rank by rank, as every enable of the group: should a rank fail, the ranks before it hold the new bank and the others the old
    // one or none, so the group counts itself as without a bank (bank sets are refused) until a create succeeds on every rank
    const int had = g->fir_bank_f;
    g->fir_bank_f = 0;
    bool first = true;
    for (Rank &rk : g->ranks)
        if (rk.n_local > 0) {
            const int rc = pbso_scene_fir_bank_create(rk.eng, n_filters, taps);
            // (a refusal by the first rank -- bank sets pending -- is every rank's, and nothing has changed: the old bank stands)
            if (rc < 0 && first) g->fir_bank_f = had;
            GENG(g, rk, rc);
            first = false;
        }
    g->fir_bank_f = n_filters;
    g->fir_bank_a = A;
    return PBSO_OK;
}

// bank sets: every rank takes the pairs and onsets of its own objects, a contiguous slice of every set (the arrays are object-major).
// The values are checked for the whole job first; the times and the state by the engines, which hold one clock and one pending
// list: the first rank's refusal is every rank's, and no rank has taken anything by then.  `plain`: the set that waits for the next mix.
static int group_scene_fir_bank_sets(pbso_group *g, const char *call, int n_sets, const int64_t *t_set, bool plain, int J, const int *index,
                                     const float *weight, const int *onset) {
    const std::string name(call);
    if (!g || !g->fir_on) return gfail(g, PBSO_ERR_STATE, name + ": the group's scene filter mix is not enabled");
    if (g->fir_bank_f == 0) return gfail(g, PBSO_ERR_STATE, name + ": no bank (pbso_group_scene_fir_bank_create)");
    if (n_sets < 0) return gfail(g, PBSO_ERR_INVALID, name + ": n_sets is negative");
    if (n_sets == 0) return PBSO_OK;
    if (!plain && !t_set) return gfail(g, PBSO_ERR_INVALID, name + ": t_set is NULL");
    if (!index) return gfail(g, PBSO_ERR_INVALID, name + ": index is NULL");
    if (!weight) return gfail(g, PBSO_ERR_INVALID, name + ": weight is NULL");
    if (J < 1 || J > pbso::SCENE_FIR_BANK_MAX_J) return gfail(g, PBSO_ERR_INVALID, name + ": J must be 1 .. 8");
    const size_t n = (size_t)g->n_objects, nj = (size_t)J;
    for (size_t r = 0; r < (size_t)n_sets * n; ++r) {
        double sum = 0.0;
        for (size_t j = 0; j < nj; ++j) {
            if (index[r * nj + j] < 0 || index[r * nj + j] >= g->fir_bank_f) return gfail(g, PBSO_ERR_INVALID, name + ": an index is outside [0, n_filters)");
            if (!std::isfinite(weight[r * nj + j])) return gfail(g, PBSO_ERR_INVALID, name + ": a weight is not finite");
            sum += std::fabs((double)weight[r * nj + j]);
        }
        if (!(sum * g->fir_bank_a <= (double)FLT_MAX))
            return gfail(g, PBSO_ERR_INVALID, name + ": an object's sum of |weight| times the bank's largest |tap| exceeds FLT_MAX");
    }
    if (onset)
        for (size_t i = 0; i < (size_t)n_sets * n; ++i)
            if (onset[i] < 0 || onset[i] > g->fir_max_onset) return gfail(g, PBSO_ERR_INVALID, name + ": an onset is outside [0, max_onset]");
    try {
        std::vector<int> is, os;
        std::vector<float> ws;
        for (Rank &rk : g->ranks) {
            if (rk.n_local == 0) continue;
            const size_t lo = (size_t)g->cuts[rk.rank], nl = (size_t)rk.n_local;
            is.resize((size_t)n_sets * nl * nj);
            ws.resize((size_t)n_sets * nl * nj);
            os.resize(onset ? (size_t)n_sets * nl : 0);
            for (size_t k = 0; k < (size_t)n_sets; ++k) {
                std::copy(index + (k * n + lo) * nj, index + (k * n + lo + nl) * nj, is.begin() + k * nl * nj);
                std::copy(weight + (k * n + lo) * nj, weight + (k * n + lo + nl) * nj, ws.begin() + k * nl * nj);
                if (onset) std::copy(onset + k * n + lo, onset + k * n + lo + nl, os.begin() + k * nl);
            }
            const int *op = onset ? os.data() : nullptr;
            GENG(g, rk, plain ? pbso_scene_fir_set_bank(rk.eng, J, is.data(), ws.data(), op)
                              : pbso_scene_fir_bank_schedule(rk.eng, n_sets, t_set, J, is.data(), ws.data(), op));
        }
    } catch (const std::exception &ex) {
        return gfail(g, PBSO_ERR_NOMEM, ex.what());
    }
    return PBSO_OK;
}

int pbso_group_scene_fir_set_bank(pbso_group *g, int J, const int *index, const float *weight, const int *onset) {
    return group_scene_fir_bank_sets(g, "scene_fir_set_bank", 1, nullptr, true, J, index, weight, onset);
}

int pbso_group_scene_fir_set_bank_at(pbso_group *g, int64_t t_set, int J, const int *index, const float *weight, const int *onset) {
    return group_scene_fir_bank_sets(g, "scene_fir_set_bank_at", 1, &t_set, false, J, index, weight, onset);
}

int pbso_group_scene_fir_bank_schedule(pbso_group *g, int n_sets, const int64_t *t_set, int J, const int *index, const float *weight,
                                       const int *onset) {
    return group_scene_fir_bank_sets(g, "scene_fir_bank_schedule", n_sets, t_set, false, J, index, weight, onset);
}

// point-to-point transfers in pieces of at most 256 MB: a 1.8 GB ncclSend / ncclRecv pair of a rank to itself (1024 objects x ten seconds
// of audio) came back WRONG on RCCL 2.26.6 while 0.45 GB was right (profiles/r05 bench_1rank.err); sender and receiver cut alike
static constexpr size_t P2P_MAX = (size_t)64 << 20;      // floats

int pbso_group_gather(pbso_group *g, int mode) {
    if (!g || !g->stepped) return gfail(g, PBSO_ERR_STATE, "gather before step");
    if (mode != PBSO_GATHER_ALL && mode != PBSO_GATHER_ROOT && mode != PBSO_GATHER_MIX && mode != PBSO_GATHER_SCENE && mode != PBSO_GATHER_FIR)
        return gfail(g, PBSO_ERR_INVALID, "gather mode");
    const int slot = g->last_slot;
    const size_t row = (size_t)g->last_nb * g->frames, blk = (size_t)g->cmax * row;
    // PBSO_GATHER_SCENE and PBSO_GATHER_FIR share their buffers and their all-reduce: floats of one rank's mix
    const bool fir = mode == PBSO_GATHER_FIR, scene_like = fir || mode == PBSO_GATHER_SCENE;
    const size_t scount = (size_t)(fir ? g->fir_c : g->scene_c) * row;
    if (scene_like) {
        if (fir) {
            if (!g->fir_on) return gfail(g, PBSO_ERR_STATE, "filter gather: the group's scene filter mix is not enabled");
            if (g->fir_mixed) return gfail(g, PBSO_ERR_STATE, "filter gather: this step is mixed already (or was taken before the mixer was enabled)");
        } else {
            if (!g->scene_on) return gfail(g, PBSO_ERR_STATE, "scene gather: the group's scene mixer is not enabled");
            if (g->scene_mixed) return gfail(g, PBSO_ERR_STATE, "scene gather: this step is mixed already (or was taken before the mixer was enabled)");
        }
        int rc = ensure_scene_buffers(g, scount);
        if (rc != PBSO_OK) return rc;
        for (Rank &rk : g->ranks) {
            GHIP(g, hipSetDevice(rk.device));
            // (the collective that last read this slot's mix is done)
            if (g->loopback()) for (Rank &other : g->ranks) GHIP(g, hipStreamWaitEvent(rk.stream, other.ev_coll[slot], 0));
            else GHIP(g, hipStreamWaitEvent(rk.stream, rk.ev_coll[slot], 0));
            if (rk.n_local > 0) GENG(g, rk, fir ? pbso_scene_fir(rk.eng, rk.scene[slot]) : pbso_scene_mix(rk.eng, rk.scene[slot]));
            else GHIP(g, hipMemsetAsync(rk.scene[slot], 0, scount * sizeof(float), rk.stream));
            GHIP(g, hipEventRecord(rk.ev_step[slot], rk.stream));
        }
        (fir ? g->fir_mixed : g->scene_mixed) = true;
    }
    if (mode == PBSO_GATHER_MIX) {
        for (Rank &rk : g->ranks) {
            GHIP(g, hipSetDevice(rk.device));
            // (a second collective on the same step: the first one's reads of the mix row are done)
            if (g->loopback()) for (Rank &other : g->ranks) GHIP(g, hipStreamWaitEvent(rk.stream, other.ev_coll[slot], 0));
            else GHIP(g, hipStreamWaitEvent(rk.stream, rk.ev_coll[slot], 0));
            if (rk.n_local > 0) GENG(g, rk, pbso_mix_objects(rk.eng, rk.mix[slot]));
            else GHIP(g, hipMemsetAsync(rk.mix[slot], 0, row * sizeof(float), rk.stream));
            GHIP(g, hipEventRecord(rk.ev_step[slot], rk.stream));
        }
    }
    for (Rank &rk : g->ranks) {
        GHIP(g, hipSetDevice(rk.device));
        // (loopback: a rank's copies read the other ranks' slices)
        if (g->loopback()) for (Rank &other : g->ranks) GHIP(g, hipStreamWaitEvent(rk.coll, other.ev_step[slot], 0));
        else GHIP(g, hipStreamWaitEvent(rk.coll, rk.ev_step[slot], 0));
    }
    if (g->use_rccl) {
        GNCCL(g, g_rccl.GroupStart());
        for (Rank &rk : g->ranks) {
            float *base = rk.target[slot], *mine = base + (size_t)rk.rank * blk;
            if (mode == PBSO_GATHER_ALL) {
                GNCCL_OPEN(g, g_rccl.AllGather(mine, base, blk, ncclFloat, rk.comm, rk.coll));          // in place: sendbuff == recvbuff + rank * count
            } else if (mode == PBSO_GATHER_MIX) {
                GNCCL_OPEN(g, g_rccl.AllReduce(rk.mix[slot], rk.mix[slot], row, ncclFloat, ncclSum, rk.comm, rk.coll));
            } else if (scene_like) {
                GNCCL_OPEN(g, g_rccl.AllReduce(rk.scene[slot], rk.scene[slot], scount, ncclFloat, ncclSum, rk.comm, rk.coll));
            } else if (g->world == 1) {
                // (PBSO_GROUP_RCCL_ALWAYS: the root's receive and a rank's send, both on the one rank there is -- the rows land in
                //  the scratch rows, which is what pbso_group_result_device_ptr then hands out)
                for (size_t o = 0; o < blk; o += P2P_MAX) {
                    const size_t n = std::min(P2P_MAX, blk - o);
                    GNCCL_OPEN(g, g_rccl.Send(mine + o, n, ncclFloat, 0, rk.comm, rk.coll));
                    GNCCL_OPEN(g, g_rccl.Recv(rk.scratch + o, n, ncclFloat, 0, rk.comm, rk.coll));
                }
            } else if (rk.rank == 0) {
                for (int r = 1; r < g->world; ++r)
                    for (size_t o = 0; o < blk; o += P2P_MAX)
                        GNCCL_OPEN(g, g_rccl.Recv(base + (size_t)r * blk + o, std::min(P2P_MAX, blk - o), ncclFloat, r, rk.comm, rk.coll));
            } else {
                for (size_t o = 0; o < blk; o += P2P_MAX)
                    GNCCL_OPEN(g, g_rccl.Send(mine + o, std::min(P2P_MAX, blk - o), ncclFloat, 0, rk.comm, rk.coll));
            }
        }
        GNCCL(g, g_rccl.GroupEnd());
    } else if (g->loopback()) {
        for (Rank &rk : g->ranks) {
            GHIP(g, hipSetDevice(rk.device));
            if (mode == PBSO_GATHER_ALL || (mode == PBSO_GATHER_ROOT && rk.rank == 0)) {
                for (Rank &src : g->ranks) {
                    if (src.rank == rk.rank) continue;
                    GHIP(g, hipMemcpyAsync(rk.target[slot] + (size_t)src.rank * blk, src.target[slot] + (size_t)src.rank * blk, blk * sizeof(float),
                                           hipMemcpyDeviceToDevice, rk.coll));
                }
            } else if (mode == PBSO_GATHER_MIX) {
                // all-reduce: every rank collects the ranks' mixed rows and adds them in rank order (the object sum's kernels)
                float *rows = rk.scratch, *parts = rk.scratch + (size_t)g->world * row;
                for (Rank &src : g->ranks)
                    GHIP(g, hipMemcpyAsync(rows + (size_t)src.rank * row, src.mix[slot], row * sizeof(float), hipMemcpyDeviceToDevice, rk.coll));
                // (into a row of its own: the other ranks' copies still read this rank's mix row)
                int lrc = pbso::launch_mix_objects(rows, g->world, (long long)row, (long long)row, parts, loop_mix_out(g, rk, row), rk.coll);
                if (lrc != 0) return gfail(g, PBSO_ERR_HIP, "loopback all-reduce: launch_mix_objects");
            } else if (scene_like) {
                // the same for the ranks' C channels, as one row of C * row floats per rank: summed in rank order
                float *rows = rk.scene_scratch, *parts = rk.scene_scratch + (size_t)g->world * scount;
                for (Rank &src : g->ranks)
                    GHIP(g, hipMemcpyAsync(rows + (size_t)src.rank * scount, src.scene[slot], scount * sizeof(float), hipMemcpyDeviceToDevice, rk.coll));
                int lrc = pbso::launch_mix_objects(rows, g->world, (long long)scount, (long long)scount, parts, scene_loop_out(g, rk, scount), rk.coll);
                if (lrc != 0) return gfail(g, PBSO_ERR_HIP, "loopback all-reduce: launch_mix_objects");
            }
        }
    }
    for (Rank &rk : g->ranks) {
        GHIP(g, hipSetDevice(rk.device));
        GHIP(g, hipEventRecord(rk.ev_coll[slot], rk.coll));
    }
    g->last_mode = mode;
    return PBSO_OK;
}

int pbso_group_sync(pbso_group *g) {
    if (!g) return PBSO_ERR_INVALID;
    for (Rank &rk : g->ranks) {
        GHIP(g, hipSetDevice(rk.device));
        if (rk.eng && rk.n_local > 0) GENG(g, rk, pbso_sync(rk.eng));
        GHIP(g, hipStreamSynchronize(rk.stream));
        GHIP(g, hipStreamSynchronize(rk.coll));
    }
    return PBSO_OK;
}

void *pbso_group_result_device_ptr(pbso_group *g, int rank, size_t *rows, size_t *row_floats) {
    Rank *rk = g ? local_rank(g, rank) : nullptr;
    if (!rk || g->last_slot < 0) return nullptr;
    const size_t row = (size_t)g->last_nb * g->frames;
    if (row_floats) *row_floats = row;
    if (g->last_mode == PBSO_GATHER_MIX) {
        if (rows) *rows = 1;
        return g->loopback() ? loop_mix_out(g, *rk, row) : rk->mix[g->last_slot];
    }
    if (g->last_mode == PBSO_GATHER_SCENE || g->last_mode == PBSO_GATHER_FIR) {
        const size_t c = (size_t)(g->last_mode == PBSO_GATHER_FIR ? g->fir_c : g->scene_c);
        if (rows) *rows = c;
        return g->loopback() ? scene_loop_out(g, *rk, c * row) : rk->scene[g->last_slot];
    }
    const bool full = g->last_mode == PBSO_GATHER_ALL || (g->last_mode == PBSO_GATHER_ROOT && rk->rank == 0);
    if (rows) *rows = full ? (size_t)g->world * g->cmax : (size_t)g->cmax;
    // (a one-rank communicator made for tests: the rows this rank sent to itself through ncclSend / ncclRecv)
    if (g->last_mode == PBSO_GATHER_ROOT && g->use_rccl && g->world == 1) return rk->scratch;
    return full ? rk->target[g->last_slot] : rk->target[g->last_slot] + (size_t)rk->rank * g->cmax * row;
}

int pbso_group_read_result(pbso_group *g, int rank, float *out, size_t n) {
    size_t rows = 0, row = 0;
    void *p = pbso_group_result_device_ptr(g, rank, &rows, &row);
    if (!p || !out) return gfail(g, PBSO_ERR_STATE, "no result on that rank");
    if (n != rows * row) return gfail(g, PBSO_ERR_INVALID, "read_result size mismatch");
    int rc = pbso_group_sync(g);
    if (rc != PBSO_OK) return rc;
    Rank *rk = local_rank(g, rank);
    GHIP(g, hipSetDevice(rk->device));
    GHIP(g, hipMemcpy(out, p, n * sizeof(float), hipMemcpyDeviceToHost));
    return PBSO_OK;
}

}  // extern "C"
