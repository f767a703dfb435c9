/*
 * openpbso_amd.h -- C ABI of the MI355X-native modal sound engine.
 *
 * Drop-in boundary for the per-audio-sample hot path of jhwang7628/openpbso.
 * The reference has no FFI of its own: the boundary it sits behind is the
 * public interface of the header-only template ModalSolver<double,513>
 * (modal_solver.h:100-179) plus its message structs.  Every entry point below
 * names the reference interface it replaces (file:line, relative to the
 * reference root).  One engine batches MANY independent ModalSolver instances
 * ("objects") on one GPU; object i behaves like its own ModalSolver<double>.
 *
 * Conventions
 *  - every function returns an int status (PBSO_OK == 0, errors < 0); the
 *    bool-returning queue operations of the reference return 1 (true) /
 *    0 (false) / <0 (error).  No exceptions cross this boundary.
 *  - plain pointers and sizes only; `void *` device pointers are HIP device
 *    addresses, `void *stream` is a hipStream_t.
 *  - one caller thread per engine (the facade keeps the reference's
 *    single-producer/single-consumer discipline).
 *  - time is counted in audio buffers of `frames_per_buffer` samples; buffer 0
 *    is the first buffer the first pbso_step() produces.  `not_before` stamps
 *    let a batch caller say at which buffer a message becomes visible to the
 *    simulation thread's try_dequeue (the GUI thread's wall-clock in the
 *    reference).  not_before = 0 means "already there".  Stamped calls other than force
 *    messages (AR parameters, listener position, use-transfer flag) of one object form a FIFO in
 *    stamp order: an AR-parameter message that finds the 1-slot queue full waits there -- the
 *    NoFail spin of modal_solver.h:382-393 -- and so do the calls stamped behind it.
 *  - the HIP path is the only path: there is no CPU fallback.
 */
#ifndef OPENPBSO_AMD_H
#define OPENPBSO_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBSO_ABI_VERSION 6
#define PBSO_SAMPLE_RATE 44100          /* config.h:13 */
#define PBSO_FRAMES_PER_BUFFER 513      /* config.h:14 */

enum pbso_status {
    PBSO_OK = 0,
    PBSO_ERR_INVALID = -1,      /* bad argument (the reference would assert) */
    PBSO_ERR_HIP = -2,          /* a HIP runtime call failed; see pbso_last_error */
    PBSO_ERR_STATE = -3,        /* call not valid in the engine's current state */
    PBSO_ERR_IO = -4,           /* file missing / unreadable / malformed */
    PBSO_ERR_MISSING_MAP = -5,  /* std::map::at would throw (modal_solver.h:296,312) */
    PBSO_ERR_ASSERT = -6,       /* a live reference assert would fire (e.g. modal_solver.h:223) */
    PBSO_ERR_NOMEM = -7
};

/* forces.h:12-16 */
enum pbso_force_type {
    PBSO_POINT_FORCE = 0,
    PBSO_GAUSSIAN_FORCE = 1,
    PBSO_AUTOREGRESSIVE_FORCE = 2,
    PBSO_TRACK_FORCE = 3      /* not in the reference: plays a caller-supplied signal, see pbso_enqueue_track_force */
};

/* how the spatial (modal) part of a force message is given */
enum pbso_force_data_kind {
    PBSO_DATA_EXPLICIT = 0,   /* data[n_data] doubles: ForceMessage::data as the GUI built it */
    PBSO_DATA_VERTEX = 1,     /* GetModalForceVertex on the device (tools/real_time_modal_sound.cpp:268-280) */
    PBSO_DATA_FACE = 2,       /* GetModalForceFace on the device   (tools/real_time_modal_sound.cpp:236-252) */
    PBSO_DATA_ZERO = 3        /* setZero(N): the dummy start/stop messages (tools/...:754-776) */
};

enum pbso_recurrence_form {
    PBSO_FORM_BLOCK = 0,      /* default: block state-space form.  Between forces a mode is autonomous, so the 16
                                 samples after a state x = (q, q-q_prev) are e1' A^j x and the state 16 samples on
                                 is A^16 x: the sum over modes becomes a [16 x 2M].[2M x 16 blocks] product on the
                                 f32 matrix pipe (exact f32 FMA chains), the state advances 33 times per buffer
                                 instead of 513.  Buffers with a dense force profile (Gaussian / AR) step every
                                 sample as PBSO_FORM_VELOCITY does.  Needs frames_per_buffer = 513 (else the
                                 engine runs PBSO_FORM_VELOCITY); qnorm is evaluated in closed form.            */
    PBSO_FORM_VELOCITY = 1,   /* per-sample recurrence, state (q, q-q_prev), coefficients (eps^2, 1-c1-c2): fp32-safe */
    PBSO_FORM_DIRECT = 2,     /* per-sample, the reference's literal q = c1 q1 + c2 q2 + c3 Q in fp32 */
    PBSO_FORM_BLOCK_BF16 = 3  /* the block form with the OUTPUT projection (which has no feedback) evaluated as a
                                 split-bf16 product: every f32 operand x = hi + lo (two bf16, 16 significant bits),
                                 W.X ~ Whi.Xhi + Whi.Xlo + Wlo.Xhi on v_mfma_f32_16x16x32_bf16 (16x the f32 MFMA rate,
                                 f32 accumulation).  The state recurrence stays exact f32.  Error 1.5e-5 ... 3e-5 of
                                 the peak (PBSO_FORM_BLOCK: 7e-6; stated tolerance 5e-4).                               */
};

enum pbso_qnorm_mode {
    PBSO_QNORM_OFF = 0,       /* getQBufferNorm never consumed: skip the 5th FMA */
    PBSO_QNORM_ALL = 1,       /* per-sample accumulation, one row per (object, buffer): modal_solver.h:262-273 */
    PBSO_QNORM_CLOSED = 2     /* same rows; in buffers that are force-free after their first sample the sum
                                 of q^2 is the quadratic form x0' G x0 of the state after sample 0 (G per mode,
                                 fp64 on the host) -- exact in exact arithmetic; other buffers as mode 1 */
};

typedef struct pbso_engine pbso_engine;

typedef struct pbso_engine_desc {
    int abi_version;          /* PBSO_ABI_VERSION */
    int device;               /* HIP device ordinal */
    int frames_per_buffer;    /* 0 -> 513 (ModalSolver's BUF_SIZE template argument).  Any multiple of 27 up to 864; at a length
                               * other than 513 both block forms silently run as PBSO_FORM_VELOCITY (pbso_engine_info says so),
                               * time_chunks, PBSO_BANK_PIPE and the multi-listener mix do not apply, and from 702 frames on a
                               * team of the per-sample kernel holds fewer than 16 waves (its LDS).  Tested against the oracle
                               * at 27, 54, 270, 513, 540 and 864 frames. */
    int sample_rate;          /* 0 -> 44100.  Any positive rate whose Nyquist frequency lies above the objects' modes; tested
                               * against the oracle at 22050, 44100, 48000 and 96000 Hz. */
    int recurrence_form;      /* enum pbso_recurrence_form */
    int qnorm_mode;           /* enum pbso_qnorm_mode */
    int modes_per_lane;       /* 0 = auto; 1, 2, 3, 4 or 8 oscillators per lane (block form: 1, 2 or 4) */
    void *stream;             /* hipStream_t to launch on; NULL -> engine-owned non-blocking stream (the
                               * legacy null stream cannot be selected: order other work on it with
                               * pbso_sync).  A second, engine-owned high-priority stream prepares the
                               * next launch (projection, FFAT lookup, force profiles).                */
    /* ---- ABI 4: which kernels run and how.  Per ENGINE (two engines of one process may differ); 0 is the engine's
     * own policy in every field, so a zeroed descriptor is the product's default.  None of them changes what is
     * computed beyond the stated tolerance; tests and A/B runs use them to pin one path.                           */
    int bank_kernel;          /* enum pbso_bank_kernel */
    int time_chunks;          /* K5, launches cut along the time axis (a scan of the buffer-start states makes the buffers of a
                               * launch independent): 0 = when the scene leaves SIMDs idle, < 0 = never, n > 0 = always, n buffers
                               * per chunk */
    int direct_hits;          /* < 0: plain vertex hits go through the fp64 projection / combine kernels instead of the bank's f32 table */
    int forced_block;         /* < 0: dense-profile buffers are stepped per sample (no block form for them) */
    int dense_launches;       /* launches that are mostly dense-profile buffers: 0 policy, 1 block kernel, 2 per-sample kernel */
    int device_profiles;      /* < 0: force time profiles (forces.h:81-137) on the host in fp64, uploaded */
    int profile_kernel;       /* K2: 0 row-parallel, 1 chain kernel (parallel AR scan), 2 chain kernel with the reference's serial AR loop */
    int profile_margin_pct;   /* K2 row-parallel: candidate range in percent of the expected need (0 -> 100; tests: < 100 forces the shortfall path) */
    int profile_priority;     /* K2 chain kernel's wave priority: 0 auto, 1..4 -> s_setprio 0..3 */
    int team_waves;           /* > 0: waves per team (workgroup) of the oscillator bank; 0 = policy */
    int pipe_consumers;       /* pipeline kernel: 0 policy, 1..3 consumer waves per team, 4 = the five-role team of mostly-dense launches */
    long long pipe_max_teams; /* pipeline kernel eligibility: at most this many 64-mode teams (0 -> 2 per CU) */
    int chunk_buffers;        /* a step longer than this is cut into several launches (0 -> 128).  A launch's fixed costs (ramp, write drain,
                               * hand-over between the streams: ~35 us) are per launch: throughput callers that step many seconds per call
                               * set it to their step */
    int plan_threads;         /* host planner threads (0 -> 1: the caller's thread) */
    int plan_pin;             /* != 0: pin the helper threads into the caller's core complex */
    int timing_every;         /* HIP-event pairs around every n-th launch (0 -> 1; < 0: none) */
    int warm_copies;          /* < 0: pbso_finalize does not warm the runtime's copy queues */
    int stream_sync;          /* how the engine's two streams order their launches.  0 policy: events, and -- where the device supports
                               * hipStreamWaitValue64 -- a START GATE in front of the preparation kernels of launches of >= 256 buffers:
                               * they wait for a value the previous launch's bank kernel stores when it starts, so the preparation
                               * never runs two launches ahead (a long scan that does trails its bank and collides with the next
                               * bank's start); since round 6 also the hand-over of launches of fewer than 256 buffers to the bank's stream
                               * through a value in signal memory instead of an event (half the latency: 1.5 - 6 % per step of 86 buffers).
                               * 1 events only.  2 the hand-over through a value for every launch.  3 the gate for every launch (costs 0.5 - 1.5 %
                               * per step of 86 buffers).  2 and 3 fail at creation where the device lacks the interface.  4 (round 5): the gate
                               * for every launch as a wait of the SUBMITTING thread on a word of pinned host memory the previous bank's first
                               * workgroup writes (hipStreamWaitValue64 runs as a waiting kernel on this stack); costs the host one launch of
                               * run-ahead; fails at creation without pinned host memory.
                               * Round 6: the DEVICE form of the gate is a kernel that spins on a memory word until another kernel
                               * has started; where something serialises kernel dispatches -- a profiler collecting counters
                               * (rocprofv3 --pmc: five of five passes ended at their time limit with the gate, none without),
                               * AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING -- the waiting kernel can be dispatched first and never ends.  Under 0
                               * (policy) the engine looks for such an environment at creation and then orders its launches by events only
                               * (pbso_engine_info::start_gate says what it chose); 2 and 3 are the caller's explicit choice */
    int latency_path;         /* < 0: never prepare a launch on the bank's own stream (0: a step of at most four buffers submitted
                               * while the device is idle does -- nothing to overlap with, one stream hand-over less) */
    /* ---- ABI 5 */
    int time_chunk_shape;     /* modes per lane of the teams of a time-chunked launch: 0 policy, 1 / 2 / 4 (A/B runs) */
    int scan_kernel;          /* K5's scan of chunk-start states: 0 policy (cut along the time axis itself -- one wave per chunk, the chunks' affine
                               * maps composed in LDS -- for launches of 2 .. 8 chunks of more than one buffer whose whole scan is a few hundred
                               * waves: it shortens a lone scan, not a throughput-bound one), 1 always the serial scan, 2 the segmented one
                               * wherever the launch has 2 .. 8 chunks */
    /* ---- ABI 6 */
    int fuse_short_launches;  /* < 0: never.  0 (policy): a launch in which every AutoregressiveForce adds its samples once -- any launch of
                               * one buffer: the real-time step -- evaluates variates, zero-state uses and profile rows in ONE kernel instead
                               * of three, and in a launch of one buffer the combine kernel takes the rows of explicit data and the
                               * projections that outlive the buffer itself instead of a scatter and a projection launch in front of it:
                               * a sustained-contact buffer is three kernels (profiles, combine, oscillator bank) instead of seven.  The same
                               * values in the same order: bit-identical to the separate launches */
    int submit_thread;        /* > 0: a second host thread makes the HIP calls of a launch (uploads, kernel launches, event records) while
                               * pbso_step returns and the caller's thread plans the next one -- for scenes whose step is set by the HOST
                               * (64 x 256 with a listener move per buffer: 0.045 ms of planning + 0.043 ms of calls against a 0.057 ms
                               * bank).  What changes for the caller: when pbso_step returns, its launches are not necessarily in their
                               * streams yet.  Every entry point that reads results or uses the engine's streams waits for that thread first;
                               * a caller that puts work of its OWN on the engine's stream behind a step calls pbso_flush in between; an
                               * error of a recorded call surfaces at the next entry point that waits.  0 (default): every call is made by
                               * pbso_step itself.  Not with stream_sync = 4; engines of a device group never use it */
} pbso_engine_desc;

enum pbso_bank_kernel {
    PBSO_BANK_AUTO = 0,       /* per launch: the block kernel K1b (chunked along time when the scene is small, K5), the pipeline
                                 kernel K1p for small scenes whose launches are mostly dense-profile buffers */
    PBSO_BANK_BLOCK = 1,      /* K1b always (never the pipeline kernel) */
    PBSO_BANK_PIPE = 2        /* K1p whenever the engine is eligible for it (f32 block form, one mode per lane, few teams) */
};

/* --- lifetime ------------------------------------------------------------- */
int pbso_engine_create(const pbso_engine_desc *desc, pbso_engine **out);
void pbso_engine_destroy(pbso_engine *e);
const char *pbso_last_error(const pbso_engine *e);
const char *pbso_status_string(int status);
int pbso_abi_version(void);

/* --- BuildSolver (tools/real_time_modal_sound.cpp:309-345) ------------------
 * new ModalSolver<double>(n_modes) + ModalIntegrator<double>::Build(density,
 * omega_squared, alpha, beta, 1/44100, n_modes) (modal_integrator.h:47-101).
 * mode_shapes (optional) is ModeData::_modes, mode-major [>=n_modes][n_dof]
 * doubles (ModeData.h:24), needed only for PBSO_DATA_VERTEX/FACE messages.   */
typedef struct pbso_object_desc {
    int n_modes;                    /* N_modesAudible */
    int n_omega;                    /* entries in omega_squared (>= n_modes; the reference asserts) */
    const double *omega_squared;    /* ModeData::_omegaSquared */
    double density, alpha, beta;    /* ModalMaterial */
    int n_dof;                      /* 3 * |V|, 0 if no mode shapes */
    const double *mode_shapes;      /* [n_modes][n_dof] or NULL */
} pbso_object_desc;
int pbso_add_object(pbso_engine *e, const pbso_object_desc *d, int *object_id);

/* the reference's file conventions (tools/...:480-501, 316-329): reads
 * <modes_path> (ModeData.h:61-83), <material_path> (ModalMaterial.h:35-55),
 * optional <ffat_dir>/freq_threshold.txt and <ffat_dir>/ *.fatcube
 * (ffat_map_serialize.h:166-279).  ffat_dir may be NULL.                      */
int pbso_add_object_from_files(pbso_engine *e, const char *modes_path,
                               const char *material_path, const char *ffat_dir,
                               int *object_id, int *n_modes_audible);

/* FFAT_Map<double,3> runtime fields (ffat_solver.h:171-180, 281-293) as the
 * .fatcube loader fills them (ffat_map_serialize.h:166-254).                  */
typedef struct pbso_ffat_map {
    int mode_id;
    double k;
    double center3[3];
    double cell_size;
    double low_corners[6][3];
    int n_elements[6][2];
    int strides[6];
    double center[3];
    double bbox_low[3];
    double bbox_top[3];
    int n_psi;
    const double *psi;
} pbso_ffat_map;
/* ModalSolver::readFFATMaps (modal_solver.h:278-284), maps already parsed */
int pbso_object_set_ffat_maps(pbso_engine *e, int object_id, const pbso_ffat_map *maps, int n_maps);
/* ModalSolver::readFFATMaps from a directory of .fatcube files */
int pbso_object_read_ffat_maps(pbso_engine *e, int object_id, const char *dir);
/* parse one .fatcube byte string (ffat_map.proto:8-51). psi is malloc'ed:
 * release with pbso_ffat_map_free.                                            */
int pbso_fatcube_parse(const unsigned char *bytes, size_t n, pbso_ffat_map *out);
void pbso_ffat_map_free(pbso_ffat_map *m);

/* --- loaders, usable without an engine -------------- */
/* ModeData<double>::read (ModeData.h:61-83).  *omega_squared [n_modes] and
 * *modes [n_modes][n_dof] are malloc'ed: release with pbso_free.              */
int pbso_modes_read(const char *path, int *n_dof, int *n_modes, double **omega_squared, double **modes);
/* ModeData<double>::numModesAudible (ModeData.h:120-148) */
int pbso_num_modes_audible(const double *omega_squared, int n_modes, double density, double audible_freq);
/* ModalMaterial<double>::Read (ModalMaterial.h:35-55): out = density,
 * youngsModulus, poissonRatio, alpha, beta                                    */
int pbso_material_read(const char *path, double out[5]);
/* <name>.tet.obj as the tool reads it (tools/real_time_modal_sound.cpp:508-509): igl::read_triangle_mesh
 * (only `v` / `f` records; 1-based, negative and a/b/c indices; polygons become triangle fans) and
 * igl::per_vertex_normals with libigl's default (area) weighting, each row normalised -- the tool normalises
 * VN.row(vid) again at the hit (:607).  libigl is an un-vendored submodule of the reference: the weighting is
 * its documented default, not pinned by code in the reference tree.  vertices [n_vertices][3], faces
 * [n_faces][3] (0-based), vertex_normals [n_vertices][3] are malloc'ed: release with pbso_free.             */
int pbso_obj_read(const char *path, int *n_vertices, int *n_faces, double **vertices, int **faces,
                  double **vertex_normals);
void pbso_free(void *p);

/* uploads all objects to HBM; no pbso_add_object afterwards */
int pbso_finalize(pbso_engine *e);

/* --- messages (modal_solver.h:27-98, forces.h:50-55) ---------------------- */
typedef struct pbso_force_msg {
    int force_type;                 /* ForceMessage::forceType; selects the Force subclass */
    double gaussian_width_us;       /* GaussianForce(width), forces.h:42-46 */
    int sustained_force_start;      /* ForceMessage::sustainedForceStart */
    int sustained_force_end;        /* ForceMessage::sustainedForceEnd */
    int clear_all_forces;           /* ForceMessage::clearAllForces */
    int data_kind;                  /* enum pbso_force_data_kind */
    const double *data;             /* PBSO_DATA_EXPLICIT: ForceMessage::data */
    int n_data;
    int vids[3];                    /* VERTEX: vids[0]; FACE: the three vertex ids */
    double coords[3];               /* FACE: barycentric coordinates */
    double vn[3];                   /* hit normal (ONE normal for all three vertices, tools/...:241) */
} pbso_force_msg;

/* ModalSolver::enqueueForceMessage (modal_solver.h:329-333): 1 = enqueued,
 * 0 = the 1023-slot queue is full.                                            */
int pbso_enqueue_force(pbso_engine *e, int object_id, const pbso_force_msg *m, int64_t not_before);
/* The same for a pre-scheduled force script (the throughput harness drives the
 * engine from a script instead of a GUI thread): n messages, message i for object_ids[i] with
 * stamp not_before[i], enqueued in order.  accepted[i] (may be NULL) receives each call's
 * result; returns the number enqueued, or a negative pbso_status on the first hard error.     */
int pbso_enqueue_force_batch(pbso_engine *e, int n, const int *object_ids, const pbso_force_msg *msgs,
                             const int64_t *not_before, unsigned char *accepted);
/* A step's worth of PLAIN VERTEX HITS -- what the tool does on a mouse click: GetModalForceVertex with a fresh
 * PointForce, then enqueueForceMessage (tools/real_time_modal_sound.cpp:268-295, 594-622) -- as parallel arrays,
 * object by object (object_ids ascending, not_before ascending within an object): hit i strikes vertex vids[i] of
 * object object_ids[i] along vn[3 i .. 3 i + 2] at buffer stamp not_before[i].  Semantically n calls of
 * pbso_enqueue_force in that order, except that nothing is copied: the arrays are BORROWED until the next pbso_step
 * returns.  That step consumes them -- the hits of an idle object with an empty queue go straight into the step's
 * descriptors (no queue round trip), the others, and the hits stamped beyond the step, enter the object's queue as if
 * enqueued one by one (a full queue, 1023 slots, rejects a hit exactly as enqueueForceMessage returns false for it,
 * modal_solver.h:329-333: the hit is dropped and counted in pbso_engine_info::total_dropped_hits).  One script may be
 * pending at a time; any other enqueue call for the engine first moves a pending script into the queues (order is kept).
 * Returns n, or PBSO_ERR_INVALID (ids / vertex ids out of range, object order) / PBSO_ERR_STATE (a script is pending). */
int pbso_enqueue_vertex_hits(pbso_engine *e, int n, const int *object_ids, const int *vids, const double *vn,
                             const int64_t *not_before);
/* A step's worth of CONTACT STROKES -- what the tool does while the mouse is dragged over the surface: a dummy message with
 * sustainedForceStart (tools/real_time_modal_sound.cpp:754-776), one GetModalForceFace message per frame that replaces the
 * spatial vector of the one live force (:1127-1160, modal_solver.h:190-204), a stop message -- as parallel arrays, object by
 * object.  Entry i is exactly pbso_enqueue_force(e, object_ids[i], &m, not_before[i]) with m.force_type = force_type,
 * m.data_kind = PBSO_DATA_FACE (vids / coords / vn from entry i of the arrays) or, with PBSO_STROKE_ZERO, PBSO_DATA_ZERO
 * (setZero(N): the dummy start / stop messages; the entry's vids / coords / vn are ignored), and the two sustained flags from
 * PBSO_STROKE_START / PBSO_STROKE_END; the entries are enqueued in array order.  flags == NULL: all 0.
 * Everything else as pbso_enqueue_vertex_hits: object ids ascending, stamps ascending within an object, the arrays BORROWED
 * until the next pbso_step returns, one script pending per engine (a vertex-hit script counts), any other enqueue call first
 * moves a pending script into the queues with order kept, a full queue rejects an entry (counted in total_dropped_hits).
 * That step takes the entries of an ELIGIBLE object straight into its descriptors: one record per object from the host, the
 * per-buffer tables from a kernel on the device (kernels_stroke.hip).  Eligible: force_type autoregressive, a launch of at
 * least two buffers (a one-buffer launch keeps the host path), nothing in the object's queue, no stamped call due inside the
 * launch, listeners not enabled, and either no live force -- then the entries open with PBSO_STROKE_START -- or exactly the one
 * sustained autoregressive force; an entry with PBSO_STROKE_END is the last one of the launch.  Every other object, and the
 * entries that fall beyond the launch, go through the queue: the result is the same either way, pbso_stroke_stats says which
 * way was taken.  Engines with time_chunks forced on take the fast path too.
 * force_type: PBSO_POINT_FORCE or PBSO_AUTOREGRESSIVE_FORCE (a Gaussian needs a width per message: pbso_enqueue_force).
 * Returns n, or PBSO_ERR_INVALID (ids / vertex ids out of range, object order, force_type) / PBSO_ERR_STATE. */
#define PBSO_STROKE_START 1u
#define PBSO_STROKE_END 2u
#define PBSO_STROKE_ZERO 4u
int pbso_enqueue_strokes(pbso_engine *e, int n, const int *object_ids, const int *vids /* [n][3] */,
                         const double *coords /* [n][3] */, const double *vn /* [n][3] */, const int64_t *not_before,
                         const unsigned char *flags /* [n] or NULL */, int force_type);
/* totals since the engine was created: out[0] stroke entries taken straight into descriptors, out[1] entries that went through
 * the queue, out[2] entries dropped (full queue), out[3] launches that ran the stroke kernel */
int pbso_stroke_stats(pbso_engine *e, int64_t out[4]);
/* --- force tracks: contacts driven by caller-supplied force signals ----------------------------------------------------------
 * A TRACK is an immutable mono f32 signal in device memory, owned by the engine.  A TRACK FORCE is a fourth Force subclass in
 * the sense of forces.h:18-23: a message of type PBSO_TRACK_FORCE carries a PLAY RECORD saying which part of which track it
 * plays, at what rate and gain, and at which sample of its first buffer it starts.  Everything else about the message -- its
 * spatial vector, the sustained flags, clear_all_forces, the 1023-slot queue, not_before -- is what it is for the other three
 * types, and ModalSolver::step's bookkeeping (modal_solver.h:184-240) applies unchanged, including that a buffer's force is
 * (sum of data) x (sum of profiles).
 * Semantics (fp64, no fused multiply-add, this order).  s[0 .. L-1] the track; S(j) = s[j] for 0 <= j < L and 0 otherwise, or
 * with loop s[j mod L].  For p >= 0, i = floor(p), f = p - i:  x(p) = S(i) + f * (S(i + 1) - S(i)).  Output sample k = 0, 1, ... of
 * the force is gain * x(first + rate * (double)k) -- from the 64-bit index k, never an accumulated position, so a row does not
 * depend on how a run is cut into steps.  The force lasts N output samples: n_samples if > 0 (positions past the track read
 * zeros); else without loop the number of k with first + rate * k < L; with loop for ever.  Add(buf), once per buffer from the
 * buffer that dequeued the message on: exhausted (k0 >= N) -> false; else buf[i] += v_k for i = o .. frames - 1 while k < N, with
 * o = start_sample in the first buffer and 0 afterwards.  Like a GaussianForce it returns true in the buffer that holds its
 * last sample and is erased by the Add of the buffer after; under sustained contact an exhausted track adds nothing and stays.
 * A one-sample track is a hit at sample start_sample of its buffer: the reference admits a force at sample 0 only.
 * Out of scope: track forces in pbso_enqueue_strokes (a sustained track scene is planned per (object, buffer) on the host like
 * any message feed); a cheap descriptor for "one sample at offset s" (such a hit is a dense profile row and runs the
 * dense-profile path, slower than the impulse path); independent signals at several contact points of ONE object in one
 * buffer (they multiply as (sum data)(sum profiles), the reference's step(): add the object twice and mix, the bank is
 * linear); interpolation better than linear, tracks in fp64, freeing a track. */
typedef struct pbso_track_play {
    int track;            /* id from pbso_track_create */
    int loop;             /* != 0: read positions wrap around the track's length */
    int start_sample;     /* in-buffer index of output sample 0, in the buffer that dequeues the message: 0 .. frames - 1 */
    int reserved;         /* 0 */
    int64_t n_samples;    /* output samples the force lasts; 0 = until the read position leaves the track (with loop: for ever) */
    double first;         /* read position of output sample 0, in track samples; >= 0, may be fractional */
    double rate;          /* track samples per output sample; finite, > 0 */
    double gain;          /* finite */
} pbso_track_play;
/* Copies n >= 1 finite samples into the engine's track pool before it returns; ids count from 0; tracks live until the engine
 * is destroyed.  Any time after pbso_engine_create, before or after pbso_finalize.  NOT a hot-loop call: when the pool has to
 * grow while launches are in flight, the call waits for them (and for the submitting thread).  PBSO_ERR_INVALID: n < 1, a
 * sample that is not finite. */
int pbso_track_create(pbso_engine *e, const float *samples, int64_t n, int *track_id);
/* pbso_enqueue_force for a message with m->force_type == PBSO_TRACK_FORCE and its play record, validated here
 * (PBSO_ERR_INVALID, pbso_last_error names the field).  1 = enqueued, 0 = the queue is full.  pbso_enqueue_force / _batch
 * reject PBSO_TRACK_FORCE: a track force without a play record means nothing. */
int pbso_enqueue_track_force(pbso_engine *e, int object_id, const pbso_force_msg *m, const pbso_track_play *play,
                             int64_t not_before);
/* totals since the engine was created: out[0] tracks created, out[1] samples held, out[2] track-force messages dequeued by
 * step, out[3] profile rows that contained at least one track entry */
int pbso_track_stats(pbso_engine *e, int64_t out[4]);
/* ModalSolver::enqueueArprmMessageNoFail (modal_solver.h:382-393); 1-slot queue: a message that finds the slot taken waits in
 * the engine and enters when step() has taken the one before it (the reference's caller spins on try_enqueue meanwhile) */
int pbso_enqueue_arprm(pbso_engine *e, int object_id, const double a[2], double sigma,
                       double mu, int64_t not_before);
/* ABI 6.  1 while the object's AR-parameter slot holds a message that step() has not taken yet (or one is waiting for it): what
 * ModalSolver::enqueueArprmMessage's try_enqueue would find full (modal_solver.h:378-381); 0 when a try_enqueue would succeed.  A
 * caller that wants the reference's bounded spin (enqueueArprmMessageNoFail with maxIte >= 0) polls this between attempts. */
int pbso_arprm_pending(pbso_engine *e, int object_id);
/* ModalSolver::computeTransfer(pos) (modal_solver.h:286-300): FFAT lookup for
 * every mode on the device, result offered to the 1-slot transfer queue.
 * 1 = enqueued, 0 = no maps / queue still full.                               */
int pbso_compute_transfer(pbso_engine *e, int object_id, const double pos[3], int64_t not_before);
/* A listener PATH, the twin of pbso_enqueue_force_batch for ModalSolver::computeTransfer(pos) (modal_solver.h:286-300; the
 * tool calls it from its camera callback, tools/real_time_modal_sound.cpp:844, 1172): n positions, position i for object
 * object_ids[i] at stamp not_before[i], issued in order -- semantically n calls of pbso_compute_transfer, one entry into the
 * library.  accepted[i] (may be NULL) receives each call's result; returns the number accepted, or a negative pbso_status on
 * the first hard error (bad id, PBSO_ERR_MISSING_MAP).  The arrays are read before the call returns.                        */
int pbso_compute_transfer_path(pbso_engine *e, int n, const int *object_ids, const double *pos, const int64_t *not_before,
                               unsigned char *accepted);
/* ModalSolver::computeTransfer(pos, T *trans) (modal_solver.h:302-315), batched over n_pos listener
 * positions.  Like the reference it writes _ffat_maps->size() (= pbso_object_n_maps) entries per position:
 * out[n_pos][out_cols] doubles, columns [0, n_maps) of every row are written, the others left alone;
 * out_cols < n_maps is PBSO_ERR_INVALID.  1 = done, 0 = the object has no maps.                         */
int pbso_compute_transfer_batch(pbso_engine *e, int object_id, const double *pos, int n_pos, double *out, int out_cols);
/* Multi-listener output (the reference evaluates the transfer for many positions, modal_solver.h:302-315,
 * tools/...:916-927, but mixes one listener): after pbso_listeners_enable(obj) every pbso_step keeps the block-start
 * states of that object (block forms only), and pbso_mix_listeners returns the LAST step's audio of the object as heard
 * at each of n_listeners positions -- out[n_listeners][n_buffers * 513] floats, host memory -- i.e. what n_listeners
 * ModalSolvers fed the same forces and computeTransfer(pos_l) would emit.  The per-sample dot q . transfer_l becomes an
 * [L x 16 samples x 2M] . [2M x 16 blocks] contraction on the f32 matrix pipe.  PBSO_ERR_STATE if the last step holds a
 * buffer of the object with a dense force profile (Gaussian / AR: stepped per sample, no block states).            */
int pbso_listeners_enable(pbso_engine *e, int object_id);
int pbso_mix_listeners(pbso_engine *e, int object_id, const double *pos, int n_listeners, float *out, size_t n_out);
/* _ffat_maps->size() of an object (modal_solver.h:312); 0 while readFFATMaps has not been called */
int pbso_object_n_maps(pbso_engine *e, int object_id);
/* ModalSolver::setUseTransfer (modal_solver.h:148-152) */
int pbso_set_use_transfer(pbso_engine *e, int object_id, int use, int64_t not_before);
/* ModalSolver::getLatestTransfer (modal_solver.h:145-147): n_modes doubles */
int pbso_get_latest_transfer(pbso_engine *e, int object_id, double *out);

/* --- ModalSolver::step (modal_solver.h:181-276) for every object, n_buffers
 * times, one launch.  Asynchronous on the engine's stream.                    */
int pbso_step(pbso_engine *e, int n_buffers);
/* same, audio written to a caller-owned device buffer [n_objects][n_buffers*B] fp32 */
int pbso_step_into(pbso_engine *e, int n_buffers, void *d_audio);
/* ABI 6, engines with submit_thread > 0: returns when every launch of the pbso_step calls so far is in its stream (NOT when the device is
 * done: that is pbso_sync) -- from then on work of the caller on the engine's stream is ordered behind them.  A no-op otherwise. */
int pbso_flush(pbso_engine *e);
/* ... and delivered to the HOST, where the reference's consumer lives (the PortAudio callback takes SoundMessages from a host
 * queue, modal_solver.h:79-82, 346-363; tools/real_time_modal_sound.cpp:192-212): host_out[n_objects][n_buffers * B] fp32.
 * host_out from pbso_host_alloc (or any pinned, device-mapped host memory): the oscillator bank writes its samples straight
 * into it over PCIe -- no copy pass; the step then runs at the link's rate.  Pageable memory: the bank writes device memory
 * and a copy follows on its own stream (two device buffers in turn).  Asynchronous either way: pbso_host_wait blocks until the
 * LAST pbso_step_to_host's samples are in host_out; a caller that alternates two host buffers consumes step k while step
 * k + 1 runs.                                                                                                              */
int pbso_step_to_host(pbso_engine *e, int n_buffers, float *host_out, size_t n_floats);
int pbso_host_wait(pbso_engine *e);
int pbso_host_alloc(size_t bytes, void **out);      /* pinned host memory (hipHostMalloc) for callers that do not link HIP */
void pbso_host_free(void *p);
int pbso_sync(pbso_engine *e);

/* results of the LAST step.  audio is the reference's SoundMessage::data
 * (pressure units; PaModalCallback divides by 1e10, tools/...:207-210), fp32,
 * [n_objects][n_buffers * frames_per_buffer].  emitted[obj][buf] is 0 where
 * the reference's step() returned early without a buffer (clearAllForces,
 * modal_solver.h:186-189); those samples are 0.                               */
int pbso_read_audio(pbso_engine *e, float *host_out, size_t n_floats);
/* the rows of some objects only: host_out[n_rows][n_buffers * frames_per_buffer] */
int pbso_read_audio_rows(pbso_engine *e, const int *object_ids, int n_rows, float *host_out);
int pbso_read_emitted(pbso_engine *e, unsigned char *host_out, size_t n);
/* getQBufferNorm (modal_solver.h:153-159) for (object, buffer) of the last step */
int pbso_read_qnorm(pbso_engine *e, int object_id, int buffer, float *host_out, int n);
/* integrator state after the last step: q_{k-1}, q_{k-2} (modal_integrator.h:24) */
int pbso_read_state(pbso_engine *e, int object_id, double *q1, double *q2, int n);
/* the counterpart (checkpoint / resume: the reference has none; its integrator state is the ring
 * _q[3] of modal_integrator.h:24,29): sets q_{k-1}, q_{k-2} of the first n modes of an object (rounded once to
 * fp32; modes beyond n keep their state).  Force lists, queues and the transfer in effect are not part of it:
 * a resumed run re-sends its pending messages.  Waits for the launches in flight.                              */
int pbso_write_state(pbso_engine *e, int object_id, const double *q1, const double *q2, int n);

/* --- retune: a new material for objects of a finalized engine ------------------------------------------------------------------
 * ModalSolver::setIntegrator (modal_solver.h:142-144) swaps the integrator of a live solver; the tool rebuilds its solver when a
 * new model is loaded (tools/real_time_modal_sound.cpp:446-455).  pbso_set_material gives objects object_ids[0 .. n-1] the
 * materials materials[0 .. n-1]: the host evaluates c1, c2, c3 of every mode (modal_integrator.h:63-99, the code pbso_add_object
 * runs), uploads 24 bytes per mode, and kernels rebuild every coefficient table of the named objects on the device, bit for bit
 * as pbso_finalize would have built them for that material (kernels_retune.hip; the tables are fp64 chains of + and x).
 * WHEN.  After pbso_finalize, between steps.  It takes effect at the first sample of the next step, for every sample of that
 *   step on.  Nothing of an earlier step changes.
 * WHAT DOES NOT CHANGE.  The mode count of an object stays as given to pbso_add_object (the reference's numModesAudible is not
 *   re-applied for the new density).  FFAT maps and their k, listener paths, transfer rows, tracks and queued messages are
 *   untouched: the maps were computed for the material they were loaded with, and stay that material's.
 * FORCES.  A force's modal vector g = (float)(c3 . S) is formed per launch from the force's data and the c3 table, and the
 *   vertex-hit rows (float)(c3 . shape) are rebuilt with the tables: a force alive across the call goes on with the new c3, and
 *   so does a message enqueued before the call for a stamp after it.  Nothing computed from c3 is kept from enqueue time.
 * KEEP_STATE.  keep_state != 0: the state pbso_read_state returns is the same immediately before and after the call; the
 *   displacement carries on under the new coefficients (a material slider).  keep_state == 0: q_{k-1} = q_{k-2} = 0 for the
 *   named objects -- the reference's setIntegrator with a freshly built integrator, whose state lives in the integrator.
 * ALL OR NOTHING.  Everything is validated before the device is touched; on any error nothing has changed.  PBSO_ERR_STATE
 *   before pbso_finalize (or after a step that failed half-way).  PBSO_ERR_INVALID: n < 0, a NULL array with n > 0, an id out of
 *   range, an id named twice, a value that is not finite, density <= 0, or any mode whose new c1, c2 or c3 is not finite (an
 *   over-damped mode) -- stricter than pbso_add_object, on purpose, for a live engine.  n == 0 is accepted.
 * COST.  A control operation, not a hot-loop call: it first drains the engine -- the submitting thread's queue, every stream,
 *   the launch in flight --, runs the rebuild on the engine's stream and returns when the tables are in place: it costs a
 *   device synchronisation.  After pbso_listeners_enable, pbso_mix_listeners of a retuned object needs a step after the call. */
typedef struct pbso_material { double density, alpha, beta; } pbso_material;      /* 24 bytes */
int pbso_set_material(pbso_engine *e, int n, const int *object_ids, const pbso_material *materials, int keep_state);
/* the material in force: the one given to pbso_add_object, or the last accepted pbso_set_material */
int pbso_get_material(pbso_engine *e, int object_id, pbso_material *out);
/* totals since the engine was created: out[0] pbso_set_material calls accepted, out[1] objects retuned, out[2] modes rebuilt
 * (padding columns not counted), out[3] g32 elements rebuilt (dof x padded modes of the retuned objects that have shapes) */
int pbso_material_stats(pbso_engine *e, int64_t out[4]);
void *pbso_audio_device_ptr(pbso_engine *e);

/* Sum over the engine's objects of the LAST step's audio, on the device, in object order (deterministic):
 * d_out[n_buffers * frames_per_buffer] fp32 (a device pointer).  What a consumer of ONE mixed stream plays when the
 * scene's objects sound together (the reference mixes nothing: one ModalSolver, one PortAudio stream,
 * tools/real_time_modal_sound.cpp:192-212); also the per-rank half of PBSO_GATHER_MIX below.  Asynchronous on the engine's stream. */
int pbso_mix_objects(pbso_engine *e, void *d_out);

/* Scene mix: the step's audio placed in C output channels (1 <= C <= 8) -- a stereo or multichannel stream -- on the device.
 * Every (channel, object) pair has a gain and a fractional delay in samples (the FFAT transfer gives a magnitude but no time of
 * flight; the caller owns the geometry and computes both):
 *     out_c(t) = sum_o g_co(t) * x_o(t - d_co(t)),  summed in object order as the object mix above (groups of 32, then the groups)
 * t counts mixed samples from the enable (or the last reset), 64-bit; x_o(i) is object o's audio at absolute sample i across
 * steps, 0 for i < 0; a fractional read position i0 + f is x(i0) + f (x(i0 + 1) - x(i0)), a fraction of exactly 0 reads x(i0).
 * A set call takes effect at t_set = the first sample of the next mixed step and ramps each parameter over R = ramp_samples:
 * p(t) = p_from + (p_to - p_from) (t - t_set + 1) / R until t = t_set + R - 1, p_to from then on (at once for R = 0); a set
 * during a ramp starts from the current value p(t_set - 1); the first set after enable / reset takes effect without a ramp;
 * until then every gain and delay is 0 (silence).
 * Order of arithmetic: the values set are f32, kept as fp64; with k = t - t_set + 1 a ramp is evaluated as p(t) = from + slope * k in
 * fp64, two rounded operations, slope = (to - from) / R rounded once at the set call (0 for R = 0), and p(t) = to for k >= R.  The gain
 * is g = (float)p_gain(t).  The delay d = p_delay(t) splits the read position in fp64: fr = d - floor(d), i0 = t - floor(d) - (fr != 0),
 * f = (float)(1.0 - fr) for fr != 0, else 0.  Then five f32 operations, each rounded, none fused: v = x(i0) + f * (x(i0 + 1) - x(i0))
 * (v = x(i0) itself when f == 0.f), acc = acc + g * v.  Per channel and per group of 32 consecutive objects acc starts from 0.f and
 * takes the objects in ascending order; the groups' results are then added in group order starting from 0.f.  Subnormals are kept.
 * tests/cpp/scene_mix_ref.c states this as plain C, and the device's output equals it bit for bit.  So the output is
 * bit-reproducible and depends on the rows, the values set and the absolute samples at
 * which they took effect only -- not on how the samples are cut into steps.  The last max_delay + 1 samples of every object
 * are kept on the device, so delays reach back across steps; hence, while the mixer is enabled, every step (pbso_step /
 * pbso_step_into) is mixed exactly once: a mix after a step that was not mixed, a second mix of the same step, or a mix after a
 * step delivered to host memory (the rows are not on the device) is PBSO_ERR_STATE.  The reset clears the history to silence,
 * restarts t at 0, keeps the gains and delays last set (ramps finished) and arms the mixer for the next step.              */
int pbso_scene_mix_enable(pbso_engine *e, int n_channels, int max_delay, int ramp_samples);  /* after finalize; max_delay, ramp <= 1 << 20 */
int pbso_scene_mix_set(pbso_engine *e, const float *gain, const float *delay);  /* [C][n_objects] each; delay NULL = unchanged */
int pbso_scene_mix(pbso_engine *e, void *d_out);           /* the last step, async on the engine's stream: d_out [C][n_buffers * B] f32, or NULL = engine-owned */
int pbso_read_scene_mix(pbso_engine *e, float *host_out, size_t n);   /* the last mix, synchronously; n = C * n_buffers * B */
int pbso_scene_mix_reset(pbso_engine *e);
/* The scene mix's SCHEDULE: sets that take effect at absolute samples the caller gives, any number of them inside one step, so
 * that a source that moves along a path does not cut the run at every change point.
 * EFFECT.  A scheduled set does to every parameter exactly what pbso_scene_mix_set does, with t_set given by the caller instead
 *   of "the first sample of the next mixed step": p_from = the value at t_set - 1 of the record in force at t_set - 1 (a set
 *   during a running ramp starts from the current value), slope = (p_to - p_from) / R divided once, R the ramp_samples of the
 *   enable.  The first set after enable / reset takes effect without a ramp, whichever call made it.  delay == NULL leaves the
 *   delay records untouched.  At sample t the record in force is that of the latest set with t_set <= t, and the per-sample
 *   arithmetic above is applied to it, word for word: the output still depends on the rows, the values set and the absolute
 *   samples at which they took effect only, not on how the samples are cut into steps -- a schedule mixed in one step equals, bit
 *   for bit, the same rows cut at every t_set with pbso_scene_mix_set before each piece.
 * VALIDATION, ALL OR NOTHING.  t_set must be >= the next mixed sample (out[0] of pbso_scene_mix_info) and strictly greater than
 *   the last pending scheduled set's, and the values are validated as pbso_scene_mix_set validates them; otherwise
 *   PBSO_ERR_INVALID.  pbso_scene_mix_schedule validates all of its sets before it takes any: a refused call changes nothing.
 *   PBSO_ERR_STATE before the enable.  n_sets == 0 is accepted.
 * LIFETIME.  A set scheduled beyond the next step stays pending until the step that contains it.  At most 65 536 sets may take
 *   effect inside one mixed step: with more, pbso_scene_mix returns PBSO_ERR_INVALID and nothing has changed (step in shorter
 *   pieces, or clear the schedule).  If the device memory for a step's records (n_sets_in_step + 1 blocks of C * n_objects * 64
 *   bytes) cannot be allocated, pbso_scene_mix returns PBSO_ERR_NOMEM and nothing has changed.
 * WITH pbso_scene_mix_set.  While scheduled sets are pending pbso_scene_mix_set returns PBSO_ERR_STATE; with none pending it
 *   behaves exactly as without a schedule.  After a drained schedule it continues from the value the schedule left, mid-ramp
 *   included: as if every scheduled set had been a plain set between two steps cut at its sample.  (It then waits for the mix
 *   that took the last scheduled sets, not for more.)
 * pbso_scene_mix_clear_schedule drops the sets not yet in force.  pbso_scene_mix_reset and a new pbso_scene_mix_enable drop them
 *   too; the reset keeps the targets last IN FORCE.
 * pbso_scene_mix_info: out[0] = t of the next mixed sample, out[1] = scheduled sets still pending (t_set >= out[0]), out[2] = mixes
 *   done, out[3] = sets accepted (plain and scheduled, each set of a pbso_scene_mix_schedule call counted); out[2] and out[3]
 *   count from the enable.                                                                                                      */
int pbso_scene_mix_set_at(pbso_engine *e, int64_t t_set, const float *gain, const float *delay);   /* one scheduled set; [C][n_objects] each */
int pbso_scene_mix_schedule(pbso_engine *e, int n_sets, const int64_t *t_set,
                            const float *gain  /* [n_sets][C][n_objects] */,
                            const float *delay /* [n_sets][C][n_objects], or NULL = unchanged by all of them */);
int pbso_scene_mix_clear_schedule(pbso_engine *e);      /* drops the sets not yet in force */
int pbso_scene_mix_info(pbso_engine *e, int64_t out[4]);

/* Scene filter mix: a second, independent mixer beside the scene mix -- a K-tap FIR per (channel, object) instead of one gain and
 * delay: a head-related impulse response per ear, an air-absorption filter, a handful of early reflections.
 *     y_c(t; h, D) = sum_o sum_{k = 0 .. K-1} h_co[k] * x_o(t - D_o - k)
 *     out_c(t)     = Yfrom_c(t) + w(t) * (Yto_c(t) - Yfrom_c(t))
 * x_o(i) is object o's audio at absolute sample i across steps, 0 for i < 0; t counts mixed samples from the enable (or the
 * last reset), 64-bit.  h_co are K f32 taps per (channel, object); D_o is an integer onset per OBJECT, shared by the channels
 * (interaural delays live in the taps, the onset carries the time of flight).  A set call takes effect at t_set = the first
 * sample of the next mixed step and cross-fades from the filters and onsets in force (from) to the new ones (to) over
 * R = xfade_samples: w(t) = (float)((double)(t - t_set + 1) / (double)R) while t - t_set + 1 < R, 1 from then on (at once for
 * R = 0); once w = 1 only Yto is computed and out = Yto exactly.  The first set after enable / reset takes effect without a
 * fade; until then the output is silence.  A set that follows another with no mix in between replaces it.  A set while a fade is
 * still running -- the next mixed sample t has t - t_set + 1 < R -- is PBSO_ERR_STATE (the faded-through filter of two onsets is
 * not one filter); callers whose steps are at least R samples long never meet this.
 * Order of arithmetic: per channel and per group of 32 consecutive objects acc = 0.f; objects ascending, taps k = K-1 down to 0,
 * each acc = fmaf(h[k], x(t - D - k), acc); the groups' results then added in group order starting from 0.f (the order of
 * pbso_mix_objects and pbso_scene_mix).  Yfrom and Yto are each such a full sum; the blend is three separately rounded f32
 * operations.  Neither the taps nor a group's objects are split over accumulators summed afterwards, so the output is
 * bit-reproducible and depends on the rows, the sets and the absolute samples at which they took effect only -- not on how the
 * samples are cut into steps.  Subnormals are kept.
 * The last max_onset + K - 1 samples of every object are kept on the device; hence, while this mixer is enabled, every step is
 * mixed by it exactly once, with the scene mix's error returns: a mix after a step that was not mixed, a second mix of the same
 * step, or a mix after a step delivered to host memory is PBSO_ERR_STATE.  The reset clears the history and the filters, restarts
 * t at 0 and arms the mixer for the next step.  The two mixers do not know of each other; both may be enabled.             */
int pbso_scene_fir_enable(pbso_engine *e, int n_channels, int n_taps, int max_onset, int xfade_samples);  /* after finalize; C 1 .. 8, K 1 .. 1024, max_onset, xfade <= 1 << 20 */
int pbso_scene_fir_set(pbso_engine *e, const float *taps, const int *onset);  /* taps [C][n_objects][K] (finite); onset [n_objects] in [0, max_onset], NULL = unchanged (0 at first) */
int pbso_scene_fir(pbso_engine *e, void *d_out);           /* the last step, async on the engine's stream: d_out [C][n_buffers * B] f32, or NULL = engine-owned */
int pbso_read_scene_fir(pbso_engine *e, float *host_out, size_t n);   /* the last mix, synchronously; n = C * n_buffers * B */
int pbso_scene_fir_reset(pbso_engine *e);
/* out[0] = t of the next mixed sample, out[1] = the first t at which the running fade is over (= out[0] when none runs),
 * out[2] = mixes done, out[3] = set calls accepted */
int pbso_scene_fir_info(pbso_engine *e, int64_t out[4]);
/* The delay stage of the scene filter mix: a ramped fractional delay per OBJECT in front of the filters -- a moving source heard
 * through head-related filters; its changing time of flight is a Doppler shift instead of a cross-fade between two onsets.
 *     y_c(t; h, D) = sum_o sum_k h_co[k] * z_o(t - D_o - k)
 * is the text above with z_o in place of x_o: the chain order, the groups of 32 and the cross-fade's blend are the same, both
 * filter sets of a cross-fade read the same z, and the integer onset stays and adds to the delay.  z_o(tau) is 0 for tau < 0.
 * The delay d_o is an f32 value kept as fp64 and ramped over R_d = ramp_samples by exactly the scene mix's rule and order of
 * arithmetic (p(t) = from + slope * (t - t_set + 1) in fp64, slope divided once when the set takes effect, p(t) = to from
 * t_set + R_d - 1 on): a set takes effect at t_set = the first sample of the next mixed step; a set during a ramp starts from
 * p(t_set - 1); the first set after the delay stage is enabled or the mixer reset takes effect without a ramp; until then every
 * delay is 0.  A set that follows another with no mix in between replaces it.  For tau >= 0, with the record in force at tau:
 *     d  = p_o(tau)                                                        (fp64)
 *     fr = d - floor(d);   i0 = tau - (long)floor(d) - (fr != 0);   f = fr != 0 ? (float)(1.0 - fr) : 0.f
 *     z_o(tau) = f == 0.f ? x_o(i0) : x_o(i0) + f * (x_o(i0 + 1) - x_o(i0))     three rounded f32 operations, none fused
 * -- the scene mix's read, word for word; i0 + 1 <= tau always: nothing reads the future.  Past values stay fixed: z_o(tau) is defined by the record in force at
 * tau, never by a later one extrapolated backwards.  The device therefore keeps two histories per object, the last max_delay + 1
 * samples of x (what z of the next step reads) and the last max_onset + K - 1 samples of z (what the filters' window of the next
 * step reads); z itself is computed on the way into the filters and never stored as rows.  So the output stays bit-reproducible
 * and depends on the rows, the sets and the absolute samples at which they took effect only, not on the cut into steps;
 * tests/cpp/scene_fir_delay_ref.c states z as plain C.
 * pbso_scene_fir_delay_enable needs pbso_scene_fir_enable first and a mixer that has mixed nothing since its enable or its last
 * reset (else PBSO_ERR_STATE); a new pbso_scene_fir_enable drops the delay stage with everything else; pbso_scene_fir_reset
 * clears both histories and keeps the delays last set, their ramps finished.  A delay set is independent of the filter sets'
 * cross-fade: it is accepted while a fade runs.  A mixer without the delay stage behaves, and is launched, as before.        */
int pbso_scene_fir_delay_enable(pbso_engine *e, int max_delay, int ramp_samples);   /* both 0 .. 1 << 20 */
int pbso_scene_fir_set_delay(pbso_engine *e, const float *delay);   /* [n_objects], finite, 0 <= d <= max_delay; PBSO_ERR_STATE without the enable */
/* out[0] = max_delay, out[1] = ramp_samples, out[2] = the first t at which every delay ramp is over (= the next mixed t when none
 * runs), out[3] = delay sets accepted */
int pbso_scene_fir_delay_info(pbso_engine *e, int64_t out[4]);
/* The scene filter mix's SCHEDULE: filter sets and delay sets that take effect at absolute samples the caller gives, any number of
 * them inside one step, so that a source that moves past a listener -- new head-related filters and a new time of flight all the
 * time -- does not cut the run at every change point.  The two kinds of set are scheduled independently of each other.
 * EFFECT.  A scheduled set does exactly what pbso_scene_fir_set / pbso_scene_fir_set_delay does, with t_set given by the caller
 *   instead of "the first sample of the next mixed step".  A filter set fades in from the set in force at t_set - 1 over the
 *   xfade_samples R of the enable, by the w(t) above; onset == NULL keeps the onsets of the set before it (0 at first).  A delay set
 *   ramps every delay from p(t_set - 1) of the record in force at t_set - 1 (a set during a running ramp starts from the current
 *   value), slope = (p_to - p_from) / ramp_samples divided once; z(tau) uses the record in force at tau.  The first set of a kind
 *   after enable / reset takes effect without a fade or ramp, whichever call made it.  The output still depends on the rows, the
 *   sets and the absolute samples at which they took effect only: a schedule mixed in one step equals, bit for bit, the same rows
 *   cut at every t_set with pbso_scene_fir_set / pbso_scene_fir_set_delay before each piece.
 * VALIDATION, ALL OR NOTHING.  t_set must be >= the next mixed sample (out[0] of pbso_scene_fir_schedule_info) and strictly greater
 *   than the last pending set's of its kind (a plain set still waiting for the next mix counts as pending at the next mixed sample).
 *   No filter set while a fade runs: against its predecessor, pending or in force, a filter set needs t_set - t_prev + 1 >= R
 *   whenever there is a predecessor and R >= 2 (out[3] is the smallest t_set that passes); delay sets may follow each other at any
 *   spacing.  Taps, onsets and delays are validated as the plain calls validate them.  Otherwise PBSO_ERR_INVALID.  The *_schedule
 *   calls validate all of their sets before they take any: a refused call changes nothing.  PBSO_ERR_STATE before the enable, and
 *   for a delay set before pbso_scene_fir_delay_enable.  n_sets == 0 is accepted.
 * LIFETIME.  A set scheduled beyond the next step stays pending until the step that contains it.  At most 4096 filter sets and
 *   65 536 delay sets may take effect inside one mixed step: with more, pbso_scene_fir returns PBSO_ERR_INVALID and nothing has
 *   changed (step in shorter pieces, or clear the schedule).  If the device memory for a step's sets -- a pool of S + 2 padded
 *   filter sets of C * n_objects * LP floats, LP = (K + 22) / 8 * 8 + 16, and K_d + 1 blocks of n_objects * 32 bytes of delay
 *   records -- cannot be allocated, pbso_scene_fir returns PBSO_ERR_NOMEM and nothing has changed.  A step without a scheduled
 *   set inside it is launched exactly as without a schedule.
 * WITH pbso_scene_fir_set / pbso_scene_fir_set_delay.  While scheduled sets of its kind are pending the plain set returns
 *   PBSO_ERR_STATE; with none pending it behaves exactly as without a schedule.  After a drained schedule it continues from what
 *   the schedule left, mid-fade (refused until the fade is over, as ever) or mid-ramp included: as if every scheduled set had been
 *   a plain set between two steps cut at its sample.  (A plain delay set then waits for the mix that took the last scheduled delay
 *   sets, not for more.)
 * pbso_scene_fir_clear_schedule drops the pending filter AND delay sets not yet in force.  pbso_scene_fir_reset and a new
 *   pbso_scene_fir_enable drop them too; the reset keeps the delays last IN FORCE, ramps finished.
 * pbso_scene_fir_schedule_info: out[0] = t of the next mixed sample, out[1] = scheduled filter sets pending, out[2] = scheduled delay
 *   sets pending, out[3] = the smallest t_set the next scheduled filter set may have.  pbso_scene_fir_info out[3] and
 *   pbso_scene_fir_delay_info out[3] count every set of a *_schedule call.                                                    */
int pbso_scene_fir_set_at(pbso_engine *e, int64_t t_set, const float *taps /* [C][n_objects][K] */, const int *onset /* [n_objects] or NULL = unchanged */);
int pbso_scene_fir_schedule(pbso_engine *e, int n_sets, const int64_t *t_set,
                            const float *taps /* [n_sets][C][n_objects][K] */,
                            const int *onset  /* [n_sets][n_objects], or NULL = unchanged by all of them */);
int pbso_scene_fir_set_delay_at(pbso_engine *e, int64_t t_set, const float *delay /* [n_objects] */);
int pbso_scene_fir_delay_schedule(pbso_engine *e, int n_sets, const int64_t *t_set, const float *delay /* [n_sets][n_objects] */);
int pbso_scene_fir_clear_schedule(pbso_engine *e);      /* drops the pending filter AND delay sets not yet in force */
int pbso_scene_fir_schedule_info(pbso_engine *e, int64_t out[4]);
/* The scene filter mix's BANK: the filters of a moving source come from a fixed measured table -- a head-related impulse response per
 * direction, a handful of air-absorption filters, a set of wall reflections -- and what changes with time is which entries an
 * object uses and with what weights.  The table is uploaded once and stays on the device; a set is then a few indices and weights
 * per object instead of C * n_objects * K taps.
 * A bank is F filters of [C][K] f32 taps, C and K those of the enabled mixer.  A bank set names, per object o, J entries
 *   (index[o][j], weight[o][j]), 1 <= J <= 8, and optionally an onset per object as ever.  The taps it stands for are one chain per
 *   (channel c, object o, tap k):
 *       acc = 0.f;  for j = 0 .. J-1 ascending:  acc = fmaf(weight[o][j], bank[index[o][j]][c][k], acc);   h_co[k] = acc
 *   (tests/cpp/scene_fir_bank_ref.c states it as plain C).  From there on a bank set IS the plain or scheduled set with those taps:
 *   the same t_set rules and cross-fade, the same spacing rule t_set - t_prev + 1 >= R, onset == NULL meaning the onsets of the set
 *   before it, the same counts in pbso_scene_fir_info and pbso_scene_fir_schedule_info, the same caps of 4096 filter sets per step
 *   and of the pool.  The mixer's output is bit for bit what pbso_scene_fir_set / _set_at / _schedule gives for taps computed by
 *   that chain on the host; J = 1 with weight 1.f is the bank's filter itself.  The same index may occur twice for one object;
 *   weights may be 0 or negative.  The chain is evaluated on the device, straight into the padded reversed rows the filters read.
 * Bank sets and taps sets are one ordered kind: they share the pending list and the spacing rule, a step may hold both, either may
 *   follow the other, and pbso_scene_fir_set_bank -- a bank set waiting for the next mix -- follows the rules of pbso_scene_fir_set
 *   (it replaces a plain set still waiting, of either form, and is replaced by one).
 * VALIDATION, ALL OR NOTHING, before anything is taken.  Every index in [0, F), every weight finite, and per object
 *   sum_j |weight[o][j]| * A <= FLT_MAX in fp64, A = max |bank tap| computed once at creation: every partial sum of the chain and
 *   every resulting tap stay finite, without the taps being built on the host.  J outside 1 .. 8, a NULL index or weight, and what
 *   the taps calls refuse (onset range, times) are PBSO_ERR_INVALID; a call before the enable or without a bank is PBSO_ERR_STATE.
 * LIFETIME of the bank.  pbso_scene_fir_bank_create needs pbso_scene_fir_enable first; the taps must be finite, 1 <= F <= 1 << 20
 *   (and n_objects * LP / 4 below 1 << 31).  If the bank cannot be allocated it returns PBSO_ERR_NOMEM and the mixer is as it was.
 *   A second create replaces the bank; it is PBSO_ERR_STATE while bank sets are pending (scheduled, or waiting for the next mix).
 *   Sets already taken by a mix are materialised taps and are not affected.  pbso_scene_fir_reset keeps the bank (and drops the
 *   scheduled sets, bank sets among them, as ever).  A new pbso_scene_fir_enable drops the bank with everything else.
 * pbso_scene_fir_bank_info: out[0] = F (0: no bank), out[1] = the largest J (8), out[2] = bank sets accepted since the enable
 *   (they count in pbso_scene_fir_info out[3] as well), out[3] = device bytes of the bank.                                      */
int pbso_scene_fir_bank_create(pbso_engine *e, int n_filters, const float *taps /* [F][C][K] */);
int pbso_scene_fir_bank_info(pbso_engine *e, int64_t out[4]);
int pbso_scene_fir_set_bank(pbso_engine *e, int J, const int *index /* [n_objects][J] */, const float *weight /* [n_objects][J] */,
                            const int *onset /* [n_objects] or NULL = unchanged */);
int pbso_scene_fir_set_bank_at(pbso_engine *e, int64_t t_set, int J, const int *index, const float *weight, const int *onset);
int pbso_scene_fir_bank_schedule(pbso_engine *e, int n_sets, const int64_t *t_set, int J,
                                 const int *index    /* [n_sets][n_objects][J] */,
                                 const float *weight /* [n_sets][n_objects][J] */,
                                 const int *onset    /* [n_sets][n_objects], or NULL = unchanged by all of them */);

/* Scene reverb: a bus effect behind the mixers -- n_in device-resident signals (a send bus: what pbso_mix_objects, pbso_scene_mix
 * or pbso_scene_fir just wrote, or some of their channels) convolved with a long impulse response per (output channel, input),
 * a room's tail of seconds, in the direct form and with the input's history kept across steps.
 * u_i(t) is input channel i (0 <= i < n_in <= 8) at absolute sample t, 0 for t < 0; t counts processed samples from the enable (or
 * the last reset), 64-bit; r_ci[k] are K f32 taps per (output channel c, input i), 0 <= c < n_out <= 8, 1 <= K <= 1 << 17.  The
 * taps are cut into segments of S = PBSO_SCENE_REVERB_SEGMENT = 2048 taps -- S is part of the definition --, J = ceil(K / S)
 * of them, the last one may be shorter.
 * Order of arithmetic:
 *     p_cij(t) : acc = 0.f;  for k = min(K, (j+1) S) - 1 down to j S :  acc = fmaf(r_ci[k], u_i(t - k), acc)
 *     Y_c(t)   : y = 0.f;    for i ascending, for j ascending :          y = y + p_cij(t)
 *     out_c(t) = Yfrom_c(t) + w(t) * (Yto_c(t) - Yfrom_c(t))             (three separately rounded operations)
 *     out_c(t) = add_c(t) + out_c(t)                                     (only when d_add is given; one more rounded add)
 * The cross-fade follows the rules of the scene filter mix: a set takes effect at t_set = the first sample of the next processed
 * step; w(t) = (float)((double)(t - t_set + 1) / (double)R) while t - t_set + 1 < R, R = xfade_samples; after that only Yto is
 * computed and out = Yto exactly.  The first set after enable / reset takes effect without a fade; until then the output is
 * silence (0.f), or add + 0.f when d_add is given.  A set with no step between it and the previous set replaces it.  A set while a
 * fade is still running is PBSO_ERR_STATE.
 * Subnormals are kept.  Nothing else is split over accumulators: the output is bit-reproducible and depends on the input samples,
 * the sets and the absolute samples at which the sets took effect only -- not on how the samples are cut into steps.  Inputs must
 * be finite: a non-finite input sample leaves the outputs within K + 15 samples after it unspecified (the kernel multiplies zero
 * pad taps around every segment with the samples next to its window, and 0 * infinity is NaN).
 * pbso_scene_reverb processes n = the last step's n_buffers * 513 samples: d_in [n_in][n] f32 on the device, required; d_add
 * [n_out][n] f32 or NULL, may be the same pointer as d_out (the wet signal added into a dry mix); d_out [n_out][n] f32, or NULL
 * for an engine-owned buffer, must not overlap d_in.  Asynchronous on the engine's stream: whatever produces d_in must be on that
 * stream or complete.  The last K - 1 samples of every input channel are kept on the device, double-buffered; hence, while the
 * reverb is enabled, every step is processed exactly once: a second call for the same step, a call after a step that was skipped
 * or a call before any step is PBSO_ERR_STATE.  A step delivered to host memory is not an error here: the input is the caller's
 * buffer.  The reset clears the history and the taps, restarts t at 0 and arms the reverb for the next step.  The reverb knows
 * nothing of the two mixers; all three may be enabled.  A device group has no reverb: the wet signal of an all-reduced bus is not
 * the bitwise sum of per-rank wet signals.                                                                                    */
#define PBSO_SCENE_REVERB_SEGMENT 2048
int pbso_scene_reverb_enable(pbso_engine *e, int n_in, int n_out, int n_taps, int xfade_samples);   /* after finalize; n_in, n_out 1 .. 8, K 1 .. 1 << 17, xfade <= 1 << 20 */
int pbso_scene_reverb_set(pbso_engine *e, const float *taps);            /* [n_out][n_in][K], finite */
int pbso_scene_reverb(pbso_engine *e, const void *d_in, const void *d_add, void *d_out);
int pbso_read_scene_reverb(pbso_engine *e, float *host_out, size_t n);   /* the last output, synchronously; n = n_out * n_buffers * B */
int pbso_scene_reverb_reset(pbso_engine *e);
/* out[0] = t of the next processed sample, out[1] = the first t at which the running fade is over (= out[0] when none runs),
 * out[2] = steps processed, out[3] = set calls accepted */
int pbso_scene_reverb_info(pbso_engine *e, int64_t out[4]);

/* Master bus: the end of the output chain -- a ramped master gain, a linked look-ahead peak limiter with a hard ceiling, meters per
 * buffer and 16-bit PCM, on a device buffer [C][n] (what the mixers and the reverb write).  The limiter has no recursion: a sliding
 * minimum followed by a FIR smoothing of the gain, so it is parallel, bit-reproducible and independent of how the samples are cut
 * into steps.
 * Parameters at enable: C channels, 1 .. 8; ceiling T, f32, finite, 0 < T <= 1; look-ahead L, 1 .. 4096; hold H, 0 .. 65536; gain
 * ramp R <= 1 << 20.  t counts processed samples from the enable (or the last reset), 64-bit; u_c(t) is input channel c, 0 for
 * t < 0, and must be finite: a non-finite input sample leaves the output unspecified.
 * Order of arithmetic:
 *     p(t)    master gain: the scene mix's ramp rule for one parameter (fp64 from + slope * k, slope divided once at the set call),
 *             initial value 1; a set takes effect at t_set = the first sample of the next processed step and ramps from the value
 *             in force at t_set - 1 over R samples (at once for R = 0)
 *     v_c(t)  = (float)p(t) * u_c(t)                                   one rounded f32 multiplication; 0 for t < 0
 *     pk(t)   = max over c of fabsf(v_c(t))
 *     r(t)    = pk(t) > T ? T / pk(t) : 1.f                            IEEE f32 division, correctly rounded; 1.f for t < 0
 *     a(t)    = min over j = 0 .. L + H of r(t - j)
 *     g(t)    : acc = 0.f; for k = L-1 down to 0: acc = fmaf(w[k], a(t - k), acc);   g = fminf(acc, r(t - L))
 *     y_c(t)  = fminf(fmaxf(v_c(t - L) * g(t), -T), T)                 one rounded multiplication, then the clamp
 * The output is the input delayed by L samples.
 * Smoothing window: L f32 taps, computed once on the host at enable.  In fp64, h_k = 1 - cos(2 pi (k+1) / (L+1)); the sum of the
 * h_k is taken in ascending k; w[k] = (float)(h_k / sum), so w[0] = 1 for L = 1.  pbso_master_window reads the taps back.
 * Why it holds: the window of every a(t - k), k = 0 .. L-1, contains sample t - L, so g(t) <= r(t - L) up to the rounding of the
 * chain, and fminf(acc, r(t - L)) makes that exact.  The f32 taps sum to 1 only up to rounding.  Where the chain over them ends
 * at or above 1.f (L = 1, 64, 65, 128, 4096 and about half of all L; acc reaches 1.0000001) the fminf gives g = 1.f exactly over
 * unlimited stretches and the output is the delayed input bit for bit; where it ends below (L = 12 is the first) such stretches
 * pass at a gain just below 1 (at worst 2.3e-6 below, over all L) and count as limited in the meters.  The final clamp covers
 * v * fl(T / |v|), which can exceed T by an ulp.  Hence |y_c(t)| <= T for every sample, exactly.
 * Subnormals are kept.  The device keeps the last 2 L + H samples of every v_c, double-buffered as the reverb's history: all that
 * r, a and g need.  The output depends only on the input samples, the sets and the absolute samples at which the sets took effect.
 * pbso_master processes n = the last step's n_buffers * 513 samples: d_in [C][n] f32 on the device, required; d_out [C][n] f32, or
 * NULL for an engine-owned buffer; d_out == d_in is allowed (d_in is read completely before anything is written).  Asynchronous
 * on the engine's stream.  While enabled, every step is processed exactly once: a second call for the same step, a call after a
 * step that was skipped or a call before any step is PBSO_ERR_STATE.  A step delivered to host memory is not an error here: the
 * input is the caller's buffer.  The reset clears the history, restarts t at 0, keeps the gain last set with its ramp finished
 * and arms the stage for the next step.  The stage knows nothing of the mixers or the reverb.  A device group has none.
 * Meters: one record per (buffer b of the call, channel c), [n_buffers][C].  min_gain and n_limited are identical for all c.  */
typedef struct pbso_master_meter {
    float in_peak;       /* max |v_c| over the buffer's 513 input samples */
    float out_peak;      /* max |y_c| over its 513 output samples */
    float min_gain;      /* min g(t) over them */
    int32_t n_limited;   /* count of g(t) < 1.f */
    double sumsq;        /* sum of (double)y * (double)y: each product exact in fp64, the order of the sum is free */
} pbso_master_meter;     /* 24 bytes */
int pbso_master_enable(pbso_engine *e, int n_channels, float ceiling, int lookahead, int hold, int ramp_samples);   /* after finalize */
int pbso_master_set_gain(pbso_engine *e, float gain);                       /* finite */
int pbso_master(pbso_engine *e, const void *d_in, void *d_out);             /* n = last step's n_buffers * 513; [C][n] f32; d_out NULL = engine-owned; d_out == d_in allowed */
int pbso_read_master(pbso_engine *e, float *host_out, size_t n);            /* planar [C][n], synchronous; n = C * n_buffers * 513 */
int pbso_read_master_pcm16(pbso_engine *e, int16_t *host_out, size_t n);    /* interleaved [n][C]: (int16_t)lrintf(y * 32767.f), converted on the device; n as above */
int pbso_read_master_meters(pbso_engine *e, pbso_master_meter *out, size_t n_records);   /* [n_buffers][C] */
int pbso_master_window(pbso_engine *e, float *out, size_t n);               /* the L taps in force; n = L */
int pbso_master_reset(pbso_engine *e);
/* out[0] = t of the next processed sample, out[1] = the first t at which the gain ramp is over (= out[0] when none runs),
 * out[2] = steps processed, out[3] = sets accepted */
int pbso_master_info(pbso_engine *e, int64_t out[4]);

/* Resampler bus: the output rate -- a rational polyphase sample-rate converter on a device buffer [C][n] (what the mixers, the
 * reverb and the master bus write), so that a scene computed at 44100 Hz leaves the device at 48000 or 96000 Hz.  A plain FIR per
 * output sample: parallel, bit-reproducible and independent of how the samples are cut into steps.
 * Parameters at enable: C channels, 1 .. 8; rate_out; T taps per output sample, 1 .. 256; the Kaiser beta, finite, 0 <= beta <= 20;
 * cutoff, finite, 0 < cutoff <= 1 (a fraction of the lower of the two Nyquist frequencies).  rate_in is the engine's sample_rate.
 * L = rate_out / gcd(rate_in, rate_out), M = rate_in / gcd(rate_in, rate_out); both must be <= 4096 and L * T <= 1 << 18, else
 * PBSO_ERR_INVALID.
 * Prototype: N = L * T taps, computed once on the host in fp64 at enable and rounded to f32 once.  With c = (N - 1) / 2, x = j - c
 * and fc = cutoff * 0.5 / max(L, M),
 *     g[j] = L * 2 fc * sinc(2 fc x) * I0(beta * sqrt(1 - (2 x / (N - 1))^2)) / I0(beta)
 * sinc(a) = sin(pi a) / (pi a), 1 at a = 0; the window is 1 for N = 1; I0 is the power series sum of ((x / 2)^k / k!)^2, summed in
 * ascending k until a term is below 1e-17 of the sum.  The phase table is h[phi][k] = (float)g[k * L + phi], [L][T];
 * pbso_resample_taps reads it back.
 * Clock: t counts input samples and m output samples, both 64-bit and from the enable (or the last reset); u_c(t) is input channel
 * c, 0 for t < 0.  Output m reads at i = floor(m * M / L) with phase phi = (m * M) mod L.  A call that processes the input samples
 * [t, t + n) produces exactly the outputs m with t <= i < t + n: m from ceil(t * L / M) to ceil((t + n) * L / M) - 1.  Their number
 * differs from call to call and is at most ceil(n * L / M) (pbso_resample_max_out): for 160 / 147 and n = 513 it is 559, then 558.
 * Order of arithmetic:
 *     acc = 0.f; for k = T-1 down to 0: acc = fmaf(h[phi][k], u_c(i - k), acc);   y_c(m) = acc
 * one f32 fmaf chain, nothing split over accumulators.  Subnormals are kept.  The output is the input delayed by (N - 1) / (2 L)
 * input samples, which is (N - 1) / (2 M) output samples.
 * State: the device keeps the last T - 1 input samples of every channel, double-buffered as the master bus's history.  Between
 * calls the host keeps only p0 = m_lo * M - t * L, which lies in [0, M), and counters: output j of a call has position p0 + j * M,
 * so that i - t = position div L and phi = position mod L.  The device never multiplies an absolute index; the output depends only
 * on the input samples, not on how they were cut into steps.
 * pbso_resample processes n = the last step's n_buffers * frames_per_buffer samples: d_in [C][n] f32 on the device, required; d_out
 * [C][out_stride] f32 with out_stride >= ceil(n * L / M), must not overlap d_in, or NULL for an engine-owned buffer whose stride is
 * n_out (out_stride is not read then).  *n_out (may be NULL) receives the number of outputs per channel; the words of a row behind
 * them are not written.  Asynchronous on the engine's stream.  While enabled, every step is processed exactly once: a second call
 * for the same step, a call after a step that was skipped or a call before any step is PBSO_ERR_STATE.  A step delivered to host
 * memory is not an error here: the input is the caller's buffer.  A refused call changes nothing.  The reset makes the history
 * silent, sets t = m = p0 = 0 and arms the stage for the next step.  The stage knows nothing of the other buses.  A device group
 * has none.
 * Meters of the last call: one record per channel.  Resampling reconstructs the signal between the input samples, where it can be
 * larger than at any of them: behind a limiter the output can overshoot the limiter's ceiling (by a few tenths of a dB on dense
 * material, by more on a clipped square).  out_peak and n_over make that visible; a caller that must not exceed full scale gives
 * the master bus a ceiling with headroom (0.9 is a common choice) rather than 1.  The PCM conversion saturates.
 * PCM: (int16_t)lrintf(fminf(fmaxf(y, -1.f), 1.f) * 32767.f), interleaved [n_out][C], converted on the device.                  */
typedef struct pbso_resample_meter {
    float out_peak;      /* max |y_c| over the call's outputs (0 when it had none) */
    int32_t n_over;      /* count of |y_c| > 1.f */
} pbso_resample_meter;   /* 8 bytes */
int pbso_resample_enable(pbso_engine *e, int n_channels, int rate_out, int taps, double beta, double cutoff);   /* after finalize */
int pbso_resample(pbso_engine *e, const void *d_in, void *d_out, int64_t out_stride, int64_t *n_out);
int pbso_resample_max_out(pbso_engine *e, int n_buffers, int64_t *out);     /* ceil(n L / M), n = n_buffers * frames_per_buffer */
int pbso_read_resample(pbso_engine *e, float *host_out, size_t n);          /* planar [C][n_out] of the last call, synchronous; n = C * n_out */
int pbso_read_resample_pcm16(pbso_engine *e, int16_t *host_out, size_t n);  /* interleaved [n_out][C]; n as above */
int pbso_read_resample_meters(pbso_engine *e, pbso_resample_meter *out, size_t n_channels);   /* [C] */
int pbso_resample_taps(pbso_engine *e, float *out, size_t n);               /* the phase table [L][T]; n = L * T */
int pbso_resample_reset(pbso_engine *e);
/* out[0] = t, out[1] = m, out[2] = steps processed, out[3] = L, out[4] = M, out[5] = T, out[6] = N - 1 (the numerator of the delay:
 * over 2 L in input samples, over 2 M in output samples), out[7] = n_out of the last call */
int pbso_resample_info(pbso_engine *e, int64_t out[8]);

/* EQ bus: biquad cascades -- S second-order IIR sections in cascade on every channel of a device buffer [C][n] (what the mixers,
 * the reverb and the master bus read and write): a high-pass in front of the limiter, a shelf on the reverb send, peaking bands on
 * the master.  The recurrence is evaluated in block form, so that a step of any length is parallel work, bit-reproducible and
 * independent of how the samples are cut into steps.
 * Why fp64 inside: an f32 biquad, serial or in block form, is 1e-4 to 2e-3 of peak away from the fp64 recurrence for sections at
 * 20 .. 100 Hz (coefficient rounding at a1 near -2).  So inputs and outputs are f32 and everything between is fp64: tables, states
 * and the signals between sections; the result is rounded to f32 once at the end.
 * Stage: C channels, 1 .. 8; S sections per channel, 1 .. 8, in cascade.  Section (c, s) has five fp64 coefficients b0 b1 b2 a1 a2
 * (a0 = 1).  Signal 0 of channel c is (double)u_c(t); signal s + 1 is the output of section s.  All signals are 0 for t < 0.
 * t counts processed samples from the enable or the last reset, 64-bit.
 * Block form: P = PBSO_EQ_BLOCK is part of the definition.  A coefficient set in force since absolute sample t_set has its block
 * origins at T0 = t_set + g * P.  For a section with input x and output y, five tables of P doubles are built on the host at the set
 * call by running the recurrence  o = b0 v + b1 x1 + b2 x2 - a1 y1 - a2 y2  in fp64, in this literal order of operations (no fused
 * multiply-add), over P samples: h, the response to a unit impulse from zero state; r, s, p, q, the response with zero input to unit
 * x(T0-1), x(T0-2), y(T0-1), y(T0-2) respectively.  Order of arithmetic, with fma the fp64 fused multiply-add:
 *     y(T0+k): acc = 0.0; for j = k down to 0: acc = fma(h[j], x(T0+k-j), acc);
 *              acc = fma(r[k], x(T0-1), acc); acc = fma(s[k], x(T0-2), acc);
 *              acc = fma(q[k], y(T0-2), acc); acc = fma(p[k], y(T0-1), acc)
 * one fp64 chain per sample, nothing split over accumulators; the only serial dependence across blocks is two fma per block and
 * section.  out_c(t) = (float)signal S.  Subnormals are kept.  A non-finite input leaves every later output of that channel
 * unspecified.  Against the serial fp64 recurrence the block form stays within 1e-9 of peak (DESIGN.md has the table).
 * Sets and the cross-fade: enable and reset install the identity cascade (b0 = 1, the rest 0, t_set = 0), under which the output is
 * the input bit for bit.  A set (pbso_eq_set: sos [C][S][5]) takes effect at t_set = the first sample of the next processed step.
 * With xfade_samples R > 0 the old cascade (From) keeps running on its own grid through t_set + R - 2 and the new one (To) starts
 * at t_set on a grid of its own; for t < t_set To takes every signal's values from From (the direct-form-I state, so nothing
 * jumps).  While t - t_set + 1 < R:  out = yf + w * (yt - yf)  with yf = (float)From, yt = (float)To and
 * w = (float)((double)(t - t_set + 1) / (double)R), three separately rounded f32 operations; after that only To.  R = 0: To at
 * once.  The first set after enable or reset fades from the identity like any other.  A set with no step since the previous set
 * replaces it.  A set while a fade runs is PBSO_ERR_STATE.  Validation happens before anything changes: all values finite, every
 * section stable (|a2| < 1 and |a1| < 1 + a2), else PBSO_ERR_INVALID and the stage stays as it was.
 * State: for each cascade (at most two), channel and signal, the device keeps the last P + 2 fp64 samples, double-buffered as the
 * master bus's history.  A step may end inside a block; the next step finishes that block from the same origin, so each sample is
 * computed by the formula above whatever the cut.
 * pbso_eq processes n = the last step's n_buffers * frames_per_buffer samples: d_in [C][n] f32 on the device, required; d_out [C][n]
 * or NULL for an engine-owned buffer; d_out == d_in is allowed (the input is read before anything is written), any other overlap is
 * PBSO_ERR_INVALID.  Asynchronous on the engine's stream.  While enabled, every step is processed exactly once: a second call for the
 * same step, a call after a step that was skipped or a call before any step is PBSO_ERR_STATE.  A refused call changes nothing.  The
 * stage knows nothing of the other buses.  A device group has none.
 * pbso_eq_tables reads back the tables in force, [C][S][5][P] in the order h r s p q: To's, once its set has taken effect.
 * pbso_eq_design needs no engine: the Audio-EQ-Cookbook forms, computed in fp64 exactly as written here.  With
 *     w0 = 2 pi f0 / rate, cs = cos(w0), sn = sin(w0), alpha = sn / (2 Q), A = pow(10, gain_db / 40), g = 2 sqrt(A) alpha
 *   low-pass    b1 = 1 - cs, b0 = b2 = b1 / 2;            a0 = 1 + alpha, a1 = -2 cs, a2 = 1 - alpha
 *   high-pass   b1 = -(1 + cs), b0 = b2 = (1 + cs) / 2;   a0, a1, a2 as the low-pass
 *   peaking     b0 = 1 + alpha A, b1 = -2 cs, b2 = 1 - alpha A;   a0 = 1 + alpha / A, a1 = -2 cs, a2 = 1 - alpha / A
 *   low shelf   b0 = A ((A+1) - (A-1) cs + g), b1 = 2 A ((A-1) - (A+1) cs), b2 = A ((A+1) - (A-1) cs - g);
 *               a0 = (A+1) + (A-1) cs + g, a1 = -2 ((A-1) + (A+1) cs), a2 = (A+1) + (A-1) cs - g
 *   high shelf  b0 = A ((A+1) + (A-1) cs + g), b1 = -2 A ((A-1) + (A+1) cs), b2 = A ((A+1) + (A-1) cs - g);
 *               a0 = (A+1) - (A-1) cs + g, a1 = 2 ((A-1) - (A+1) cs), a2 = (A+1) - (A-1) cs - g
 * out = b0/a0 b1/a0 b2/a0 a1/a0 a2/a0.  rate > 0, 0 < f0 < rate / 2, Q > 0, |gain_db| <= 120, all finite, else PBSO_ERR_INVALID;
 * gain_db is read by the peaking and shelf forms only.                                                                             */
#define PBSO_EQ_BLOCK 64
enum pbso_eq_kind {
    PBSO_EQ_LOWPASS = 0,
    PBSO_EQ_HIGHPASS = 1,
    PBSO_EQ_PEAK = 2,
    PBSO_EQ_LOWSHELF = 3,
    PBSO_EQ_HIGHSHELF = 4
};
int pbso_eq_enable(pbso_engine *e, int n_channels, int n_sections, int xfade_samples);   /* after finalize; xfade_samples 0 .. 1 << 20 */
int pbso_eq_set(pbso_engine *e, const double *sos);                          /* [C][S][5] = b0 b1 b2 a1 a2 */
int pbso_eq(pbso_engine *e, const void *d_in, void *d_out);                  /* n = last step's n_buffers * 513; [C][n] f32; d_out NULL = engine-owned; d_out == d_in allowed */
int pbso_read_eq(pbso_engine *e, float *host_out, size_t n);                 /* planar [C][n], synchronous; n = C * n_buffers * 513 */
int pbso_eq_tables(pbso_engine *e, double *out, size_t n);                   /* [C][S][5][P]; n = C * S * 5 * PBSO_EQ_BLOCK */
int pbso_eq_reset(pbso_engine *e);
/* out[0] = t of the next processed sample, out[1] = the first t at which the running fade is over (= out[0] when none runs),
 * out[2] = steps processed, out[3] = sets accepted */
int pbso_eq_info(pbso_engine *e, int64_t out[4]);
int pbso_eq_design(int kind, double rate, double f0, double q, double gain_db, double out[5]);
/* The EQ bus's SCHEDULE: coefficient sets that take effect at absolute samples the caller gives, any number of them inside one step,
 * so that a swept filter -- a high-pass that opens, a shelf that follows the reverb send, a band that follows a retune -- does not
 * cut the run, and every stage in front of the EQ with it, at every change point.
 * EFFECT.  A scheduled set does exactly what pbso_eq_set does, with t_set given by the caller instead of "the first sample of the
 *   next processed step": the new cascade's block origins are t_set + g * P; for t < t_set every one of its signals is the value of
 *   the cascade in force at t; From keeps running on its own grid through t_set + R - 2; the fade is the three f32 operations stated
 *   above.  The output still depends on the input, the sets and the absolute samples at which they took effect only: a schedule
 *   processed in one step equals, bit for bit, the same input cut at every t_set with pbso_eq_set before each piece, however the
 *   samples are cut into steps.
 * VALIDATION, ALL OR NOTHING.  t_set must be >= the next processed sample (out[0] of pbso_eq_schedule_info) and strictly greater
 *   than the last pending set's (a plain set still waiting for the next step counts as pending at the next processed sample).  No
 *   set while a fade runs: against its predecessor, pending or in force, a set needs t_set - t_prev + 1 >= R whenever R >= 2 (out[2]
 *   is the smallest t_set that passes); the identity installed by enable or reset is a predecessor with t_set = 0, since the first
 *   set fades from the identity like any other.  Coefficients are validated as pbso_eq_set validates them.  Otherwise
 *   PBSO_ERR_INVALID.  pbso_eq_schedule validates all of its sets before it takes any: a refused call changes nothing.
 *   PBSO_ERR_STATE before the enable.  n_sets == 0 is accepted.
 * LIFETIME.  A set scheduled beyond the next step stays pending until the step that contains it.  At most 65 536 sets may be pending
 *   (more: PBSO_ERR_INVALID).  At most 4096 sets may take effect inside one processed step: with more, pbso_eq returns
 *   PBSO_ERR_INVALID and nothing has changed (step in shorter pieces, or clear the schedule).  If the device memory for a step's
 *   tables (n_sets_in_step * C * S * 5 * P doubles) or work rows cannot be allocated, pbso_eq returns PBSO_ERR_NOMEM and nothing has
 *   changed.  The pending list holds coefficients; a step builds the tables of the sets it takes on the device, by the recurrence
 *   above in its literal order.  A step in which no scheduled set takes effect is launched exactly as without a schedule, even when a
 *   fade that a scheduled set started in an earlier step is still running; a step with sets inside it takes a number of launches
 *   that does not depend on how many they are.
 * WITH pbso_eq_set.  While scheduled sets are pending pbso_eq_set returns PBSO_ERR_STATE; with none pending it behaves exactly as
 *   without a schedule.  After a drained schedule it continues from what the schedule left, mid-fade included (refused until the
 *   fade is over, as ever): as if every scheduled set had been a plain set between two steps cut at its sample.
 * pbso_eq_clear_schedule drops the sets not yet in force.  pbso_eq_reset and a new pbso_eq_enable drop them too.
 * pbso_eq_schedule_info: out[0] = t of the next processed sample, out[1] = scheduled sets pending, out[2] = the smallest t_set the
 *   next scheduled set may have, out[3] = the number of sets that took effect inside the last processed step (a plain set that the
 *   step took counts as one).  pbso_eq_info out[3] counts every set of a pbso_eq_schedule call; out[1] stays the first t at which the
 *   running fade is over.  pbso_eq_tables returns the tables of the last set that has taken effect.                              */
int pbso_eq_set_at(pbso_engine *e, int64_t t_set, const double *sos /* [C][S][5] */);
int pbso_eq_schedule(pbso_engine *e, int n_sets, const int64_t *t_set, const double *sos /* [n_sets][C][S][5] */);
int pbso_eq_clear_schedule(pbso_engine *e);             /* drops the sets not yet in force */
int pbso_eq_schedule_info(pbso_engine *e, int64_t out[4]);

/* Loudness bus: programme loudness and true peak -- ITU-R BS.1770-4 K-weighted energies and the gating of EBU Tech 3341
 * (momentary, short-term, integrated) on a device buffer [C][n] (what the mixers, the reverb, the EQ and the master bus write), so
 * that a render can be brought to a delivery target (-23 LUFS for EBU R128, -14 or -16 for streaming) without bringing the audio to
 * the host.  The stage reads its input and writes no audio.  Every record is bit-reproducible and independent of how the samples
 * are cut into steps.
 * Clock and hop: t counts processed samples from the enable or the last reset, 64-bit; u_c(t) is input channel c, 0 for t < 0.  The
 * hop is Hs = rate / 10 samples (100 ms), rate the engine's sample_rate, which must be a multiple of 10 with Hs >= 256, else
 * PBSO_ERR_INVALID.  Sub-block j covers t in [j Hs, (j + 1) Hs).
 * K-weighting: two sections.  pbso_loudness_design(rate, out[2][5]) computes them in fp64 exactly as written here and needs no
 * engine (rate finite and above twice the shelf's f0, else PBSO_ERR_INVALID).
 *   stage 1, the shelf: f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196,
 *     K = tan(pi f0 / rate), Vh = pow(10, G / 20), Vb = pow(Vh, 0.4996667741545416), a0 = 1 + K/Q + K K,
 *     b0 = (Vh + Vb K/Q + K K) / a0, b1 = 2 (K K - Vh) / a0, b2 = (Vh - Vb K/Q + K K) / a0,
 *     a1 = 2 (K K - 1) / a0, a2 = (1 - K/Q + K K) / a0
 *   stage 2, the high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 as above,
 *     b = 1, -2, 1 (not normalised, as the standard has it), a1 = 2 (K K - 1) / a0, a2 = (1 - K/Q + K K) / a0
 * At 48000 Hz this is the standard's table to 9e-16.  The weighted signal z_c(t) is signal 2 of the EQ bus's block form with these
 * two sections on every channel: P = PBSO_EQ_BLOCK, the tables built as the EQ bus builds them, t_set = 0, installed at enable and
 * never changed, kept in fp64 and not rounded to f32; the state is the EQ's P + 2 fp64 samples per signal.
 * Energy of a sub-block, in a prescribed order: with k = t - j Hs and l = k mod 64 there are 64 accumulators per channel, which
 * start at 0.0;  acc_l = fma(z, z, acc_l)  in ascending k; when the sub-block is complete, for s = 32, 16, 8, 4, 2, 1 and every
 * l < s:  acc_l = acc_l + acc_{l+s};  E_c(j) = acc_0.  The device keeps the 64 accumulators per channel across steps.
 * True peak (with true_peak != 0 at enable; without it both peaks of every record are 0): the oversampling factor is O = 4 for a
 * rate below 80 000 Hz and 2 from there up, with T = 12 taps per phase.  The phase table h[O][12] f32 follows the resampler bus's
 * prototype rule (g[j], h[phi][k] = (float)g[k L + phi]) with L = O, M = 1, beta = 8.0, cutoff = 1.0; it is built once on the host
 * at enable, and pbso_loudness_taps reads it back.  For every t and phi:
 *     acc = 0.f; for k = 11 down to 0: acc = fmaf(h[phi][k], u_c(t - k), acc)
 * TP_c(j) is the maximum of fabsf(acc) over the sub-block's t and all phi, SP_c(j) the maximum of fabsf(u_c(t)).  The device keeps
 * the last 11 input samples per channel and the running maxima of an open sub-block.  Subnormals are kept.  A non-finite input
 * leaves later records unspecified.
 * Log: each complete sub-block appends one record per channel to a device-resident log [max_blocks][C] of pbso_loudness_block;
 * record j is sub-block j.  A step whose records would not fit is refused with PBSO_ERR_STATE before anything changes.
 * Report: host fp64 over the log, reachable without an engine through pbso_loudness_report_from_blocks(blocks [n_blocks][C],
 * n_blocks, C, weight, hop, out).  For gating block i >= 3:  ms_c = (((E_c(i-3) + E_c(i-2)) + E_c(i-1)) + E_c(i)) / (4 Hs);
 * w_i is the sum over ascending c of G_c ms_c;  l_i = -0.691 + 10 log10(w_i), -infinity for w_i = 0.  The gates:
 * A = {i : l_i > -70};  Gamma = -0.691 + 10 log10(mean of w over A, ascending i) - 10 (relative_threshold);
 * integrated = -0.691 + 10 log10(mean of w over {i in A : l_i > Gamma}), n_gated the size of that set.  Momentary is l of the last
 * gating block; short-term is the same over the last 30 sub-blocks, summed left-associated in ascending order and divided by 30 Hs;
 * max_momentary and max_short_term are their maxima over the log; true_peak and sample_peak are the maxima of the records' (linear,
 * over all channels).  Whatever has too few blocks, or an empty gate, is -HUGE_VAL.  The channel weights G_c are doubles, finite
 * and >= 0, given at enable; NULL means all 1.
 * pbso_loudness processes n = the last step's n_buffers * frames_per_buffer samples: d_in [C][n] f32 on the device, required and
 * read only.  Asynchronous on the engine's stream.  While enabled, every step is processed exactly once: a second call for the same
 * step, a call after a step that was skipped or a call before any step is PBSO_ERR_STATE.  A refused call changes nothing.  The
 * reset empties the log, silences every state, sets t = 0 and arms the stage for the next step.  pbso_read_loudness_blocks copies
 * records [first, first + n) of the log, [n][C], synchronous; a range beyond the logged blocks is PBSO_ERR_INVALID.  The stage knows
 * nothing of the other buses.  A device group has none.                                                                          */
typedef struct pbso_loudness_block {
    double energy;       /* E_c(j) */
    float true_peak;     /* TP_c(j), linear */
    float sample_peak;   /* SP_c(j), linear */
} pbso_loudness_block;   /* 16 bytes */
typedef struct pbso_loudness_summary {
    double integrated, momentary, short_term;   /* LUFS */
    double max_momentary, max_short_term;       /* LUFS */
    double relative_threshold;                  /* Gamma, LUFS */
    double true_peak, sample_peak;              /* linear; 20 log10 of them is dBTP / dBFS */
    int64_t n_blocks, n_gated;
} pbso_loudness_summary; /* 80 bytes */
int pbso_loudness_enable(pbso_engine *e, int n_channels, const double *weight, int max_blocks, int true_peak);   /* after finalize; n_channels 1 .. 8; weight [C] or NULL; max_blocks 1 .. 1 << 22 */
int pbso_loudness(pbso_engine *e, const void *d_in);                         /* n = last step's n_buffers * frames_per_buffer; [C][n] f32, read only */
int pbso_read_loudness_blocks(pbso_engine *e, int64_t first, int64_t n, pbso_loudness_block *out);   /* [n][C], synchronous */
int pbso_loudness_report(pbso_engine *e, pbso_loudness_summary *out);          /* over the whole log, synchronous */
int pbso_loudness_taps(pbso_engine *e, float *out, size_t n);                /* the phase table [O][12]; n = O * 12 */
int pbso_loudness_reset(pbso_engine *e);
/* out[0] = t of the next processed sample, out[1] = blocks logged, out[2] = steps processed, out[3] = max_blocks */
int pbso_loudness_info(pbso_engine *e, int64_t out[4]);
int pbso_loudness_design(double rate, double out[2][5]);
int pbso_loudness_report_from_blocks(const pbso_loudness_block *blocks, int64_t n_blocks, int n_channels, const double *weight, int hop,
                                     pbso_loudness_summary *out);

/* --- device group ("create/destroy engine (sample rate, buffer size 513, device list)", 8(e)) -------------
 * Objects are independent -- every ModalSolver owns its integrator state, force list and maps, modal_solver.h:100-126 -- so
 * a job of many objects shards over the GPUs of a node with no exchange while stepping: each RANK (one GPU, one engine) owns a
 * contiguous block of objects, balanced by the sum of modes.  RCCL over xGMI is used only to gather finished audio buffers,
 * called from here (C++), not from a Python launcher: one process may drive several GPUs (devices[]), or one process per GPU
 * joins a job of world_size ranks through a shared unique id (ncclCommInitRank).  librccl is loaded when the first group
 * with more than one rank is created; an engine alone never needs it.                                                    */
typedef struct pbso_group pbso_group;
enum pbso_gather_mode {
    PBSO_GATHER_ALL = 1,      /* every rank receives every object's buffers: ncclAllGather, in place (each engine writes its buffers
                                 straight into its slice of the gather target) */
    PBSO_GATHER_ROOT = 2,     /* only rank 0 receives them: ncclSend / ncclRecv */
    PBSO_GATHER_MIX = 3,      /* the consumer wants ONE mixed stream: every rank sums its objects' buffers on the device
                                 (pbso_mix_objects) and the ranks all-reduce n_buffers * 513 floats */
    PBSO_GATHER_SCENE = 4,    /* the scene mix: every rank mixes its own objects into C channels (the scene mix above; an empty rank
                                 contributes silence) and the ranks all-reduce C * n_buffers * 513 floats.  While the group's mixer is
                                 enabled, every group step is gathered this way exactly once (a second time: PBSO_ERR_STATE); the
                                 other modes can still be gathered for that step */
    PBSO_GATHER_FIR = 5       /* the scene filter mix, as PBSO_GATHER_SCENE: every rank filters its own objects (an empty rank contributes
                                 silence), the ranks all-reduce C * n_buffers * 513 floats; once per step while the group's filter mix is
                                 enabled */
};
#define PBSO_GROUP_ID_BYTES 128
enum pbso_group_transport {
    PBSO_GROUP_RCCL = 0,        /* the product: RCCL whenever the job has more than one rank (a one-rank group has nothing to exchange) */
    PBSO_GROUP_RCCL_ALWAYS = 1, /* tests: a one-rank group builds its communicator too (ncclCommInitRank) and issues every collective --
                                   the in-place ncclAllGather, ncclAllReduce, and for GATHER_ROOT an ncclSend / ncclRecv pair to itself
                                   whose received rows are the result -- so the RCCL code runs on a one-GPU box */
    PBSO_GROUP_LOOPBACK = 2     /* tests: ALL ranks of the job in this process, several of them on one device (devices[] may repeat); the
                                   collectives are plain device copies.  Everything the group does around them -- shards, padding of
                                   ragged shards, slice offsets, the two gather targets and their events, ROOT / MIX -- is the product's */
};
typedef struct pbso_group_desc {
    int abi_version;          /* PBSO_ABI_VERSION */
    const int *devices;       /* HIP ordinals THIS process drives: one rank (engine) each */
    int n_devices;
    int world_size;           /* ranks of the whole job; 0 -> n_devices (a single process) */
    int first_rank;           /* rank of devices[0]; this process owns ranks first_rank .. first_rank + n_devices - 1 */
    const void *unique_id;    /* world_size > n_devices: the PBSO_GROUP_ID_BYTES bytes pbso_group_unique_id() gave ONE process,
                                 handed to all of them by the launcher (a file, an environment variable, a store) */
    pbso_engine_desc engine;  /* settings of every engine; `device` and `stream` are the group's */
    /* ---- ABI 5 */
    int transport;            /* enum pbso_group_transport; 0 = the product's */
} pbso_group_desc;
int pbso_group_unique_id(void *out_bytes);
int pbso_group_create(const pbso_group_desc *d, pbso_group **out);
void pbso_group_destroy(pbso_group *g);
const char *pbso_group_last_error(const pbso_group *g);
/* the job: mode counts of ALL its objects, the same list in every process.  Computes the shards -- contiguous blocks whose cut
 * points are the object boundaries nearest to the ideal prefix sums of the mode counts.                                    */
int pbso_group_plan(pbso_group *g, const int *modes_per_object, int n_objects);
/* the rule by itself (no group, no GPU): cuts[world_size + 1], rank r owns ids [cuts[r], cuts[r + 1]) */
int pbso_shard_by_modes(const int *modes_per_object, int n_objects, int world_size, int *cuts);
int pbso_group_rank_span(pbso_group *g, int rank, int *lo, int *hi);          /* global ids [lo, hi) of a rank */
int pbso_group_owner(pbso_group *g, int global_id, int *rank, int *local_id);
/* BuildSolver for object global_id (pbso_add_object on its owner), in ascending id order; ids of ranks in OTHER processes are
 * accepted and ignored, so every process may run the same loop over the job's objects.                                    */
int pbso_group_add_object(pbso_group *g, int global_id, const pbso_object_desc *d);
int pbso_group_finalize(pbso_group *g);
pbso_engine *pbso_group_engine(pbso_group *g, int rank);                      /* NULL for a rank of another process */
/* pbso_enqueue_force on the object's owner (1 / 0 / < 0); an object of another process: 1, nothing done (its owner does it) */
int pbso_group_enqueue_force(pbso_group *g, int global_id, const pbso_force_msg *m, int64_t not_before);
/* pbso_set_material on the owners of global_ids[0 .. n-1].  Everything is validated on every local rank before any rank takes its
 * share: all or nothing within the ranks of this process.  Ids of ranks in other processes are checked for range and duplicates
 * and otherwise ignored (their owner does it).  After pbso_group_finalize. */
int pbso_group_set_material(pbso_group *g, int n, const int *global_ids, const pbso_material *materials, int keep_state);
/* ModalSolver::step n_buffers times on every local rank; each engine writes into its slice of the group's gather target
 * (two targets used in turn: the gather of step k runs beside the oscillator bank of step k + 1)                          */
int pbso_group_step(pbso_group *g, int n_buffers);
/* the collective for the LAST step, asynchronous (its own stream per rank, ordered behind the step); enum pbso_gather_mode  */
int pbso_group_gather(pbso_group *g, int mode);
int pbso_group_sync(pbso_group *g);
/* the scene mixer on every local rank; gain / delay [C][n_objects of the whole job] by global id (each rank takes the slice of
 * its own objects).  After pbso_group_finalize; the arguments as for a single engine.                                       */
int pbso_group_scene_mix_enable(pbso_group *g, int n_channels, int max_delay, int ramp_samples);
int pbso_group_scene_mix_set(pbso_group *g, const float *gain, const float *delay);
/* ... and its schedule on every local rank: gain / delay [n_sets][C][n_objects of the whole job] by global id, each rank taking
 * its slice of every set.  The values are checked for the whole job before any rank takes a set; the times are checked by the
 * ranks' engines, which are mixed in lockstep and hold one clock (pbso_scene_mix_info of any pbso_group_engine has the counts). */
int pbso_group_scene_mix_set_at(pbso_group *g, int64_t t_set, const float *gain, const float *delay);
int pbso_group_scene_mix_schedule(pbso_group *g, int n_sets, const int64_t *t_set, const float *gain, const float *delay);
int pbso_group_scene_mix_clear_schedule(pbso_group *g);
/* the scene filter mix on every local rank; taps [C][n_objects of the whole job][K] and onset [n_objects of the whole job] by
 * global id.  After pbso_group_finalize; the arguments as for a single engine.                                              */
int pbso_group_scene_fir_enable(pbso_group *g, int n_channels, int n_taps, int max_onset, int xfade_samples);
int pbso_group_scene_fir_set(pbso_group *g, const float *taps, const int *onset);
/* ... and its delay stage on every local rank; delay [n_objects of the whole job] by global object id, sliced per rank.  Checked
 * for the whole job before any rank takes it.  The enable goes rank by rank, as every enable of the group does: should a rank fail
 * (PBSO_ERR_NOMEM), the ranks before it have the stage and the group does not count it as enabled; pbso_group_scene_fir_enable
 * again, which drops the stage on every rank, puts the group back in one state. */
int pbso_group_scene_fir_delay_enable(pbso_group *g, int max_delay, int ramp_samples);
int pbso_group_scene_fir_set_delay(pbso_group *g, const float *delay);
/* ... and the filter mix's schedule on every local rank: taps [n_sets][C][n_objects of the whole job][K], onset and delay
 * [n_sets][n_objects of the whole job] by global id, each rank taking its slice of every set.  The values are checked for the
 * whole job before any rank takes a set; the times are checked by the ranks' engines, which are mixed in lockstep and hold one
 * clock (pbso_scene_fir_schedule_info of any pbso_group_engine has the counts).                                              */
int pbso_group_scene_fir_set_at(pbso_group *g, int64_t t_set, const float *taps, const int *onset);
int pbso_group_scene_fir_schedule(pbso_group *g, int n_sets, const int64_t *t_set, const float *taps, const int *onset);
int pbso_group_scene_fir_set_delay_at(pbso_group *g, int64_t t_set, const float *delay);
int pbso_group_scene_fir_delay_schedule(pbso_group *g, int n_sets, const int64_t *t_set, const float *delay);
int pbso_group_scene_fir_clear_schedule(pbso_group *g);
/* ... and the filter mix's bank: the whole bank on every local rank, rank by rank, as every enable of the group: should a rank
 * after the first fail (PBSO_ERR_NOMEM), the ranks before it hold the new bank and the group counts itself as without a bank -- bank
 * sets are PBSO_ERR_STATE -- until a pbso_group_scene_fir_bank_create succeeds on every rank.  index, weight
 * [n_sets][n_objects of the whole job][J] and onset [n_sets][n_objects of the whole job] by global id: object-major, so every rank
 * takes a contiguous slice (pbso_group_rank_span) of every set.  The values are checked for the whole job before any rank takes a
 * set, the times and the state by the ranks' engines.                                                                          */
int pbso_group_scene_fir_bank_create(pbso_group *g, int n_filters, const float *taps);
int pbso_group_scene_fir_set_bank(pbso_group *g, int J, const int *index, const float *weight, const int *onset);
int pbso_group_scene_fir_set_bank_at(pbso_group *g, int64_t t_set, int J, const int *index, const float *weight, const int *onset);
int pbso_group_scene_fir_bank_schedule(pbso_group *g, int n_sets, const int64_t *t_set, int J, const int *index, const float *weight,
                                       const int *onset);
/* the last gather's result on a local rank, a device pointer: ALL -> [world_size * rows_per_rank][n_buffers * 513] (rank r's
 * objects from row r * rows_per_rank; shards smaller than the largest are padded with silent rows), ROOT -> the same on rank 0
 * and the rank's own rows elsewhere, MIX -> [n_buffers * 513], SCENE and FIR -> [C][n_buffers * 513].  rows / row_floats (may be NULL)
 * receive the shape.                                                                                                        */
void *pbso_group_result_device_ptr(pbso_group *g, int rank, size_t *rows, size_t *row_floats);
int pbso_group_read_result(pbso_group *g, int rank, float *host_out, size_t n_floats);   /* that buffer, synchronously */

/* PaModalCallback body (tools/real_time_modal_sound.cpp:207-210): mono sound
 * -> interleaved stereo float32 scaled by 1e-10.                              */
void pbso_pa_convert(const float *sound, unsigned long frames, float *out_stereo);

/* --- introspection -------------------------------------------------------- */
typedef struct pbso_engine_info {
    int n_objects;
    int frames_per_buffer;
    int modes_padded;         /* oscillators per object after padding */
    int modes_per_lane;
    int waves_per_object;     /* largest team (workgroup) in waves */
    int lds_bytes_per_workgroup;
    int64_t buffers_done;
    double last_step_kernel_ms;       /* HIP-event time of the oscillator-bank kernel, last step */
    double last_step_device_ms;       /* HIP-event time of the whole device pipeline, last step */
    double last_step_host_plan_ms;    /* host bookkeeping (modal_solver.h:184-256) */
    int64_t last_step_forced_rows;
    int64_t last_step_transfer_rows;
    /* running totals since engine creation (HIP events on the engine's stream,
     * one pair per pbso_step around the oscillator-bank kernel / the pipeline) */
    double total_kernel_ms;
    double total_device_ms;
    double total_host_plan_ms;
    int64_t total_steps;
    int n_teams;              /* workgroups of the oscillator bank per launch (objects with more than
                               * 16 waves of modes are stepped by several) */
    int recurrence_form;      /* the form that runs (PBSO_FORM_BLOCK falls back to VELOCITY when
                               * frames_per_buffer != 513) */
    int64_t total_block_launches;     /* oscillator-bank launches on the block kernel (K1b) ...            */
    int64_t total_sample_launches;    /* ... and on the per-sample kernel (K1): every launch of the per-sample
                                       * forms, and launches of the block form in which more than half of the
                                       * (object, buffer) pairs carry a dense force profile (sustained contact) */
    int64_t total_timed_launches;     /* launches whose HIP-event times are in total_kernel_ms / total_device_ms: all of
                                       * them, or every n-th with pbso_engine_desc::timing_every = n (an event pair costs
                                       * the stream ~8 us per launch)                                                 */
    int64_t total_split_launches;     /* of the block launches, those on the pipeline kernel of small scenes (K1p, kernels_pipe.hip:
                                       * a producer wave and two consumer waves per 64 modes)                               */
    int64_t total_time_chunk_launches;/* of the block launches, those cut along the time axis (K5, kernels_scan.hip: a scan of the
                                       * buffer-start states, then the block kernel over (team, chunk of buffers) workgroups) */
    int64_t total_dropped_hits;       /* hits of pbso_enqueue_vertex_hits scripts that found their object's 1023-slot queue full:
                                       * rejected, as enqueueForceMessage would have been (modal_solver.h:329-333)              */
    int64_t total_one_stream_launches;/* launches whose preparation ran on the bank's own stream (the latency path: a short step
                                       * submitted while the device was idle -- the real-time facade's pattern)                   */
    /* ---- ABI 5 */
    int64_t total_dense_increment_launches; /* of the time-chunked launches, those with dense-profile buffers (Gaussian / AR: forces.h:92-128):
                                       * dense_increment_kernel evaluated what each leaves in the state, all of them at once      */
    int64_t total_segmented_scans;    /* ... whose scan of chunk-start states ran cut along the time axis (one wave per chunk)             */
    int last_time_chunk_shape;        /* the last time-chunked launch: modes per lane of its teams (0: none yet), ...              */
    int last_time_chunk_buffers;      /* ... buffers per chunk, ...                                                               */
    int last_time_chunk_teams;        /* ... and teams per chunk (its census has teams x chunks rows, chunk-major)                */
    /* ---- ABI 6 */
    int start_gate;                   /* the start gate of long launches (pbso_engine_desc::stream_sync): 0 none (asked for, or no interface),
                                       * 1 a device-side wait (hipStreamWaitValue64), 2 the submitting thread waits on pinned host memory,
                                       * -1 none because the environment serialises kernel dispatches (a waiting kernel would never end)   */
    int64_t total_gate_timeouts;      /* host-side gate only: waits that gave up after 2 s (the launch then went ungated)                 */
    double total_host_submit_ms;      /* the caller's thread in pbso_step behind the planner: packing the plan, the upload and launch calls -- or, with
                                       * submit_thread, recording them (the wait for a free plan set is not in it)                        */
    int64_t total_ffat_shared_events; /* listener events located once per EVENT (objects whose modes share one map geometry, round 6) ...   */
    int64_t total_ffat_general_events;/* ... and those evaluated per (event, mode)                                                          */
} pbso_engine_info;
int pbso_get_info(pbso_engine *e, pbso_engine_info *out);
/* diagnostics (engine created with env PBSO_CENSUS=1): for every object's
 * workgroup of the last oscillator-bank launch: start, end (100 MHz ticks),
 * HW_REG_HW_ID, HW_REG_XCC_ID, shader-clock count at start and end.
 * out[n_teams][12]; words 6..9 (block form): shader cycles of wave 0 spent in the buffer head, the MFMA pipeline, the barrier, the combine.
 * A launch on the kernel of under-filled engines (total_split_launches) has one row per team of 64 modes -- n may then be that
 * count x 12 --: words 0..2 the producer's cycles (head | stepping | wait at the barrier), 3 its HW_ID | XCC_ID << 32, 6..8
 * consumer 0's (head + taps + qnorm chains | projection | wait), 9, 10 the consumers' HW_ID words, 11 qnorm chain groups stepped
 * in unit-force form.                                                                                                            */
int pbso_read_census(pbso_engine *e, unsigned long long *out, size_t n);

#ifdef __cplusplus
}
#endif
#endif
