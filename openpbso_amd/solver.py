"""Host-side mirror of the reference's ModalSolver interface over the C ABI.

`Engine` batches many objects (one reference ModalSolver<double> each) on one
GPU; `ModalSolver` is the one-object facade with the reference's method names
(modal_solver.h:100-179) so that tests read like code written against the
reference.  All numerics happen in libopenpbso_amd.so (HIP); nothing here
computes audio.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import capi

POINT_FORCE = capi.POINT_FORCE
GAUSSIAN_FORCE = capi.GAUSSIAN_FORCE
AUTOREGRESSIVE_FORCE = capi.AUTOREGRESSIVE_FORCE
TRACK_FORCE = capi.TRACK_FORCE


class PbsoError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"[{status}] {text}")
        self.status = status


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# numpy view of capi.ForceMsg (same layout: checked at import)
FORCE_MSG_DTYPE = np.dtype([("force_type", np.int32), ("gaussian_width_us", np.float64),
                            ("sustained_force_start", np.int32), ("sustained_force_end", np.int32),
                            ("clear_all_forces", np.int32), ("data_kind", np.int32), ("data", np.uintp),
                            ("n_data", np.int32), ("vids", np.int32, 3), ("coords", np.float64, 3),
                            ("vn", np.float64, 3)], align=True)
assert FORCE_MSG_DTYPE.itemsize == C.sizeof(capi.ForceMsg) and all(
    FORCE_MSG_DTYPE.fields[n][1] == getattr(capi.ForceMsg, n).offset for n, _ in capi.ForceMsg._fields_)


class ForceMessage:
    """ForceMessage<double> (modal_solver.h:27-77).

    The modal `data` is either given explicitly (as the GUI thread built it), or
    as a vertex / face hit to be projected onto the mode shapes on the device
    (GetModalForceVertex / GetModalForceFace, tools/real_time_modal_sound.cpp:236-295).
    """

    def __init__(self, data=None, forceType=POINT_FORCE, gaussianWidth=0.0, sustainedForceStart=False,
                 sustainedForceEnd=False, clearAllForces=False, vid=None, vids=None, coords=None, vn=None):
        self.data = None if data is None else np.ascontiguousarray(data, dtype=np.float64)
        self.forceType = forceType
        self.gaussianWidth = float(gaussianWidth)
        self.sustainedForceStart = sustainedForceStart
        self.sustainedForceEnd = sustainedForceEnd
        self.clearAllForces = clearAllForces
        self.vid, self.vids, self.coords, self.vn = vid, vids, coords, vn

    def to_c(self):
        m = capi.ForceMsg()
        m.force_type = int(self.forceType)
        m.gaussian_width_us = self.gaussianWidth
        m.sustained_force_start = int(bool(self.sustainedForceStart))
        m.sustained_force_end = int(bool(self.sustainedForceEnd))
        m.clear_all_forces = int(bool(self.clearAllForces))
        if self.data is not None:
            m.data_kind = capi.DATA_EXPLICIT
            m.data = _dp(self.data)
            m.n_data = self.data.size
        elif self.vid is not None:
            m.data_kind = capi.DATA_VERTEX
            m.vids[0] = int(self.vid)
            for j in range(3):
                m.vn[j] = float(self.vn[j])
        elif self.vids is not None:
            m.data_kind = capi.DATA_FACE
            for j in range(3):
                m.vids[j] = int(self.vids[j])
                m.coords[j] = float(self.coords[j])
                m.vn[j] = float(self.vn[j])
        else:
            m.data_kind = capi.DATA_ZERO
        return m


def material_array(ids, density, alpha, beta):
    """an array of capi.Material, one per id; scalars broadcast over the ids"""
    n = np.atleast_1d(ids).size
    d, a, b = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (density, alpha, beta))
    mats = (capi.Material * max(n, 1))()
    for i in range(n):
        mats[i].density, mats[i].alpha, mats[i].beta = float(d[i]), float(a[i]), float(b[i])
    return mats


def _select_from_env():
    """Test / A-B convenience of THIS wrapper (the library reads no such variables): the kernel- and path-selection fields of
    pbso_engine_desc (ABI 4) from the environment, so that a whole pytest / bench run can pin one path.
    PBSO_ENGINE_OPTS="field=value,..." names descriptor fields directly; the older switches map onto them."""
    env = os.environ
    sel = {}
    split = env.get("PBSO_SPLIT")
    if split == "0":                                  # the block kernel K1b for every launch, walked buffer by buffer
        sel.update(bank_kernel=capi.BANK_BLOCK, time_chunks=-1)
    elif split == "2":                                # the pipeline kernel K1p for every launch
        sel.update(bank_kernel=capi.BANK_PIPE)
    if "PBSO_TIME_CHUNKS" in env:
        sel["time_chunks"] = int(env["PBSO_TIME_CHUNKS"])
    if "PBSO_TC_SHAPE" in env:
        sel["time_chunk_shape"] = int(env["PBSO_TC_SHAPE"])
    if env.get("PBSO_DIRECT_HITS") == "0":
        sel["direct_hits"] = -1
    if env.get("PBSO_FORCED_BLOCK") == "0":
        sel["forced_block"] = -1
    if "PBSO_DENSE_LAUNCHES" in env:
        sel["dense_launches"] = {"block": 1, "sample": 2}[env["PBSO_DENSE_LAUNCHES"]]
    if env.get("PBSO_DEVICE_PROFILES") == "0":
        sel["device_profiles"] = -1
    if env.get("PBSO_AR_SERIAL") == "1":
        sel["profile_kernel"] = 2
    elif env.get("PBSO_K2_ROWS") == "0":
        sel["profile_kernel"] = 1
    for name, field in (("PBSO_K2_MARGIN_PCT", "profile_margin_pct"), ("PBSO_TEAM_WAVES", "team_waves"),
                        ("PBSO_PIPE_CONSUMERS", "pipe_consumers"), ("PBSO_SPLIT_MAX_CHUNKS", "pipe_max_teams"),
                        ("PBSO_CHUNK_BUFFERS", "chunk_buffers"), ("PBSO_PLAN_THREADS", "plan_threads"),
                        ("PBSO_PLAN_PIN", "plan_pin")):
        if name in env:
            sel[field] = int(env[name])
    if "PBSO_K2_PRIO" in env:
        sel["profile_priority"] = int(env["PBSO_K2_PRIO"]) + 1
    if "PBSO_TIMING_EVERY" in env:
        n = int(env["PBSO_TIMING_EVERY"])
        sel["timing_every"] = n if n > 0 else -1
    if env.get("PBSO_WARM_COPIES") == "0":
        sel["warm_copies"] = -1
    for item in filter(None, env.get("PBSO_ENGINE_OPTS", "").split(",")):
        k, v = item.split("=")
        sel[k.strip()] = int(v)
    return sel


SELECT_FIELDS = ("bank_kernel", "time_chunks", "direct_hits", "forced_block", "dense_launches", "device_profiles",
                 "profile_kernel", "profile_margin_pct", "profile_priority", "team_waves", "pipe_consumers",
                 "pipe_max_teams", "chunk_buffers", "plan_threads", "plan_pin", "timing_every", "warm_copies", "stream_sync", "latency_path",
                 "time_chunk_shape", "scan_kernel", "fuse_short_launches", "submit_thread")


def fill_engine_desc(d, device, form, qnorm, modes_per_lane, stream, frames_per_buffer, select, sample_rate=0):
    """a capi.EngineDesc from the wrapper's arguments; returns the kernel / path selection that went into it"""
    d.abi_version = capi.ABI_VERSION
    d.device = device
    d.frames_per_buffer = frames_per_buffer
    d.sample_rate = sample_rate
    d.recurrence_form = form
    d.qnorm_mode = qnorm
    d.modes_per_lane = modes_per_lane
    d.stream = stream
    sel = _select_from_env()
    sel.update(select)
    for k, v in sel.items():
        if k not in SELECT_FIELDS:
            raise TypeError(f"unknown engine option {k!r}")
        setattr(d, k, int(v))
    return sel


def default_form():
    return {"block": capi.FORM_BLOCK, "velocity": capi.FORM_VELOCITY, "direct": capi.FORM_DIRECT,
            "block_bf16": capi.FORM_BLOCK_BF16}[os.environ.get("PBSO_FORM", "block")]


class Engine:
    @classmethod
    def from_handle(cls, handle, n_modes, qnorm, frames_per_buffer=0, sample_rate=0):
        """a view of an engine somebody else owns (a device group's rank): same methods, close() leaves it alone"""
        self = cls.__new__(cls)
        self._l = capi.lib()
        self._h = C.c_void_p(handle)
        self._owned = False
        self.n_modes = list(n_modes)
        self.B = frames_per_buffer or 513
        self.sample_rate = sample_rate or 44100
        self.qnorm_mode = qnorm
        self._last_nb = 0
        self._borrowed = None
        self.select = {}
        return self

    def __init__(self, device=0, form=None, qnorm=capi.QNORM_ALL, modes_per_lane=0,
                 stream=None, frames_per_buffer=0, sample_rate=0, **select):
        """frames_per_buffer (a multiple of 27, at most 864) / sample_rate: 0 = the reference's 513 / 44100.
        select: the ABI-4 fields of pbso_engine_desc that pick kernels and paths for THIS engine (bank_kernel,
        time_chunks, direct_hits, ...; include/openpbso_amd.h).  0 / absent = the engine's policy."""
        if form is None:
            # the C ABI's default (a zeroed pbso_engine_desc): the block form with the exact f32 projection.
            # PBSO_FORM=block|block_bf16|velocity|direct lets a whole test / bench run pick the oscillator-bank kernel
            form = default_form()
        self.form = form
        self._l = capi.lib()
        d = capi.EngineDesc()
        self.select = fill_engine_desc(d, device, form, qnorm, modes_per_lane, stream, frames_per_buffer, select, sample_rate)
        self._owned = True
        h = C.c_void_p()
        rc = self._l.pbso_engine_create(C.byref(d), C.byref(h))
        self._h = h
        if rc != capi.OK:
            text = self._l.pbso_last_error(h).decode() if h else "engine_create failed"
            if h:
                self._l.pbso_engine_destroy(h)
            self._h = None
            raise PbsoError(rc, text)
        self.n_modes = []
        self.B = frames_per_buffer or 513
        self.sample_rate = sample_rate or 44100
        self.qnorm_mode = qnorm
        self._last_nb = 0
        self._borrowed = None

    # -- plumbing -----------------------------------------------------------
    def _chk(self, rc):
        if rc < 0:
            raise PbsoError(rc, self._l.pbso_last_error(self._h).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._l.pbso_engine_destroy(self._h)
            self._h = None
            for p in getattr(self, "_pinned", []):
                self._l.pbso_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- BuildSolver ----------------------------------------------------------
    def add_object(self, omega_squared, density, alpha, beta, n_modes=None, mode_shapes=None):
        om = np.ascontiguousarray(omega_squared, dtype=np.float64)
        d = capi.ObjectDesc()
        d.n_modes = om.size if n_modes is None else int(n_modes)
        d.n_omega = om.size
        d.omega_squared = _dp(om)
        d.density, d.alpha, d.beta = float(density), float(alpha), float(beta)
        if mode_shapes is not None:
            ms = np.ascontiguousarray(mode_shapes, dtype=np.float64)
            assert ms.ndim == 2 and ms.shape[0] >= d.n_modes
            ms = np.ascontiguousarray(ms[: d.n_modes])
            d.n_dof = ms.shape[1]
            d.mode_shapes = _dp(ms)
        oid = C.c_int(-1)
        self._chk(self._l.pbso_add_object(self._h, C.byref(d), C.byref(oid)))
        self.n_modes.append(d.n_modes)
        return oid.value

    def add_object_from_files(self, modes_path, material_path, ffat_dir=None):
        oid, naud = C.c_int(-1), C.c_int(0)
        self._chk(self._l.pbso_add_object_from_files(
            self._h, modes_path.encode(), material_path.encode(),
            None if ffat_dir is None else ffat_dir.encode(), C.byref(oid), C.byref(naud)))
        self.n_modes.append(naud.value)
        return oid.value, naud.value

    def set_ffat_maps(self, obj, maps):
        """maps: list of dicts with the FFAT_Map<double,3> runtime fields."""
        arr = (capi.FfatMap * len(maps))()
        keep = []
        for i, m in enumerate(maps):
            a = arr[i]
            a.mode_id = int(m["mode_id"])
            a.k = float(m["k"])
            a.cell_size = float(m["cell_size"])
            for j in range(3):
                a.center3[j] = float(m["center3"][j])
                a.center[j] = float(m["center"][j])
                a.bbox_low[j] = float(m["bbox_low"][j])
                a.bbox_top[j] = float(m["bbox_top"][j])
            for f in range(6):
                for j in range(3):
                    a.low_corners[f][j] = float(m["low_corners"][f][j])
                a.n_elements[f][0] = int(m["n_elements"][f][0])
                a.n_elements[f][1] = int(m["n_elements"][f][1])
                a.strides[f] = int(m["strides"][f])
            psi = np.ascontiguousarray(m["psi"], dtype=np.float64)
            keep.append(psi)
            a.n_psi = psi.size
            a.psi = _dp(psi)
        self._chk(self._l.pbso_object_set_ffat_maps(self._h, obj, arr, len(maps)))

    def read_ffat_maps(self, obj, directory):
        self._chk(self._l.pbso_object_read_ffat_maps(self._h, obj, directory.encode()))

    def finalize(self):
        self._chk(self._l.pbso_finalize(self._h))

    # -- messages -------------------------------------------------------------
    def enqueue_force(self, obj, msg, not_before=0):
        return bool(self._chk(self._l.pbso_enqueue_force(self._h, obj, C.byref(msg.to_c()), not_before)))

    @staticmethod
    def hit_messages(objs, vids, vns, not_before, coords=None, force_type=capi.POINT_FORCE):
        """(object ids, pbso_force_msg array, stamps) ready for enqueue_force_batch.  Vertex hits
        (GetModalForceVertex): vids [n]; face hits (GetModalForceFace): vids [n][3] and barycentric
        coords [n][3]; vns [n][3]; objs / not_before int arrays [n]."""
        objs = np.ascontiguousarray(objs, dtype=np.int32)
        stamps = np.ascontiguousarray(not_before, dtype=np.int64)
        n = objs.size
        msgs = np.zeros(n, dtype=FORCE_MSG_DTYPE)
        msgs["force_type"] = force_type
        if coords is None:
            msgs["data_kind"] = capi.DATA_VERTEX
            msgs["vids"][:, 0] = vids
        else:
            msgs["data_kind"] = capi.DATA_FACE
            msgs["vids"] = np.asarray(vids).reshape(n, 3)
            msgs["coords"] = np.asarray(coords, dtype=np.float64).reshape(n, 3)
        msgs["vn"] = np.asarray(vns, dtype=np.float64).reshape(n, 3)
        return objs, msgs, stamps

    def enqueue_force_batch(self, objs, msgs, not_before):
        """pbso_enqueue_force_batch: one call for a whole step of the force script; returns the
        number of messages the queues took."""
        return self._chk(self._l.pbso_enqueue_force_batch(
            self._h, objs.size, objs.ctypes.data_as(C.POINTER(C.c_int)), msgs.ctypes.data_as(C.POINTER(capi.ForceMsg)),
            not_before.ctypes.data_as(C.POINTER(C.c_int64)), None))

    def enqueue_vertex_hits(self, objs, vids, vns, not_before):
        """pbso_enqueue_vertex_hits: a step's plain PointForce vertex hits as parallel arrays, object by object (ids ascending,
        stamps ascending within an object).  The arrays are borrowed by the engine until the next step() returns: they are kept
        alive here; do not modify them in between.  Arrays of the right dtype and layout are passed through without a copy."""
        o = np.ascontiguousarray(objs, dtype=np.int32)
        v = np.ascontiguousarray(vids, dtype=np.int32)
        n = np.ascontiguousarray(vns, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(not_before, dtype=np.int64)
        assert o.size == v.size == t.size == n.shape[0]
        rc = self._chk(self._l.pbso_enqueue_vertex_hits(
            self._h, o.size, o.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_int)), _dp(n),
            t.ctypes.data_as(C.POINTER(C.c_int64))))
        # (only a script the engine TOOK is held here: a refused call -- a script already pending, bad ids -- leaves the
        #  arrays of the pending one, which the engine still points at, alive)
        self._borrowed = (o, v, n, t)
        return rc

    @staticmethod
    def prepare_vertex_hits(objs, vids, vns, not_before):
        """the arguments of enqueue_vertex_hits converted once (a caller that replays pre-built scripts step after step: the
        conversions cost more than the call for a small step); hand the result to enqueue_prepared_vertex_hits"""
        o = np.ascontiguousarray(objs, dtype=np.int32)
        v = np.ascontiguousarray(vids, dtype=np.int32)
        n = np.ascontiguousarray(vns, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(not_before, dtype=np.int64)
        assert o.size == v.size == t.size == n.shape[0]
        return (o.size, o.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_int)), _dp(n),
                t.ctypes.data_as(C.POINTER(C.c_int64)), (o, v, n, t))

    def enqueue_prepared_vertex_hits(self, prepared):
        rc = self._chk(self._l.pbso_enqueue_vertex_hits(self._h, *prepared[:5]))
        self._borrowed = prepared[5]
        return rc

    @staticmethod
    def prepare_strokes(objs, vids, coords, vns, not_before, flags=None, force_type=capi.AUTOREGRESSIVE_FORCE):
        """the arguments of pbso_enqueue_strokes converted once: objs / not_before [n], vids / coords / vns [n][3], flags [n] of
        capi.STROKE_START | STROKE_END | STROKE_ZERO (None: all 0); hand the result to enqueue_prepared_strokes"""
        o = np.ascontiguousarray(objs, dtype=np.int32)
        v = np.ascontiguousarray(vids, dtype=np.int32).reshape(-1, 3)
        c = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1, 3)
        n = np.ascontiguousarray(vns, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(not_before, dtype=np.int64)
        f = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert o.size == t.size == v.shape[0] == c.shape[0] == n.shape[0] and (f is None or f.size == o.size)
        return (o.size, o.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_int)), _dp(c), _dp(n),
                t.ctypes.data_as(C.POINTER(C.c_int64)), None if f is None else f.ctypes.data_as(C.POINTER(C.c_ubyte)), int(force_type),
                (o, v, c, n, t, f))

    def enqueue_prepared_strokes(self, prepared):
        rc = self._chk(self._l.pbso_enqueue_strokes(self._h, *prepared[:8]))
        self._borrowed = prepared[8]                    # (only a script the engine TOOK: the arrays stay alive until the step)
        return rc

    def enqueue_strokes(self, objs, vids, coords, vns, not_before, flags=None, force_type=capi.AUTOREGRESSIVE_FORCE):
        """pbso_enqueue_strokes: a step's contact-stroke entries as parallel arrays, object by object (ids ascending, stamps
        ascending within an object); borrowed by the engine until the next step() returns (kept alive here)"""
        return self.enqueue_prepared_strokes(self.prepare_strokes(objs, vids, coords, vns, not_before, flags, force_type))

    def stroke_stats(self):
        """pbso_stroke_stats: totals of stroke entries by the way they took, and launches that ran the stroke kernel"""
        out = (C.c_int64 * 4)()
        self._chk(self._l.pbso_stroke_stats(self._h, out))
        return dict(direct=out[0], queued=out[1], dropped=out[2], kernel_launches=out[3])

    # -- force tracks -----------------------------------------------------------
    def create_track(self, samples):
        """pbso_track_create: copy a mono f32 signal into the engine's track pool; returns its id (not a hot-loop call)"""
        a = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        tid = C.c_int(-1)
        self._chk(self._l.pbso_track_create(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.size, C.byref(tid)))
        return tid.value

    def enqueue_track_force(self, obj, msg, track, first=0.0, rate=1.0, gain=1.0, n_samples=0, start_sample=0, loop=False,
                            not_before=0):
        """pbso_enqueue_track_force: `msg` (its spatial vector and flags; its forceType is set to TRACK_FORCE) plays output
        samples gain * x(first + rate * k) of `track` from in-buffer sample `start_sample` of the buffer that dequeues it"""
        m = msg.to_c()
        m.force_type = capi.TRACK_FORCE
        p = capi.TrackPlay(int(track), int(bool(loop)), int(start_sample), 0, int(n_samples), float(first), float(rate), float(gain))
        return bool(self._chk(self._l.pbso_enqueue_track_force(self._h, obj, C.byref(m), C.byref(p), not_before)))

    def track_stats(self):
        """pbso_track_stats: tracks created, samples held, track-force messages dequeued, profile rows with a track entry"""
        out = (C.c_int64 * 4)()
        self._chk(self._l.pbso_track_stats(self._h, out))
        return tuple(out)

    def enqueue_arprm(self, obj, a, sigma, mu, not_before=0):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return bool(self._chk(self._l.pbso_enqueue_arprm(self._h, obj, _dp(a), sigma, mu, not_before)))

    def arprm_pending(self, obj):
        """pbso_arprm_pending: True while the object's AR-parameter slot is taken (a try_enqueue would fail, modal_solver.h:378-381)"""
        return bool(self._chk(self._l.pbso_arprm_pending(self._h, obj)))

    def compute_transfer(self, obj, pos, not_before=0):
        p = np.ascontiguousarray(pos, dtype=np.float64)
        return bool(self._chk(self._l.pbso_compute_transfer(self._h, obj, _dp(p), not_before)))

    def compute_transfer_path(self, objs, pos, not_before):
        """pbso_compute_transfer_path: n computeTransfer(pos) calls in one; returns the accepted flags [n]"""
        o = np.ascontiguousarray(objs, dtype=np.int32)
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(not_before, dtype=np.int64)
        assert o.size == t.size == p.shape[0]
        acc = np.zeros(o.size, dtype=np.uint8)
        self._chk(self._l.pbso_compute_transfer_path(self._h, o.size, o.ctypes.data_as(C.POINTER(C.c_int)), _dp(p),
                                                     t.ctypes.data_as(C.POINTER(C.c_int64)), acc.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return acc.astype(bool)

    def listeners_enable(self, obj):
        """from the next step on, keep this object's block-start states for mix_listeners"""
        self._chk(self._l.pbso_listeners_enable(self._h, obj))

    def mix_listeners(self, obj, pos):
        """the last step's audio of `obj` at every listener position: [n_listeners][n_buffers * 513] float32"""
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        out = np.empty((p.shape[0], self._last_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_mix_listeners(self._h, obj, _dp(p), p.shape[0], out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def n_maps(self, obj):
        """_ffat_maps->size() (0 before readFFATMaps)"""
        return self._chk(self._l.pbso_object_n_maps(self._h, obj))

    def compute_transfer_batch(self, obj, pos, n_cols=None, out=None):
        """computeTransfer(pos, T*) for many positions: [n_pos][n_cols]; columns beyond the object's map count stay 0.
        out: a C-contiguous float64 array [n_pos][n_cols] to fill (a caller that asks every frame keeps one: a fresh
        84 MB array costs more in page faults than the lookups and the copy together)"""
        p = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        if n_cols is None:
            n_cols = self.n_maps(obj) if out is None else out.shape[1]
        if out is None:
            out = np.zeros((p.shape[0], n_cols))
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (p.shape[0], n_cols)
        rc = self._chk(self._l.pbso_compute_transfer_batch(self._h, obj, _dp(p), p.shape[0], _dp(out), n_cols))
        return bool(rc), out

    def set_use_transfer(self, obj, use, not_before=0):
        self._chk(self._l.pbso_set_use_transfer(self._h, obj, int(use), not_before))

    def latest_transfer(self, obj):
        out = np.empty(max(self.n_modes[obj], 1))
        self._chk(self._l.pbso_get_latest_transfer(self._h, obj, _dp(out)))
        return out[: self.n_modes[obj]]

    # -- stepping -------------------------------------------------------------
    def step(self, n_buffers=1, into=None):
        if into is None:
            self._chk(self._l.pbso_step(self._h, n_buffers))
        else:
            self._chk(self._l.pbso_step_into(self._h, n_buffers, C.c_void_p(into)))
        self._last_nb = n_buffers
        self._borrowed = None                           # (a hit script is consumed by the step that follows it)

    def sync(self):
        self._chk(self._l.pbso_sync(self._h))

    def flush(self):
        """pbso_flush: with submit_thread, until the recorded launches of the steps so far are in their streams (not a device sync)"""
        self._chk(self._l.pbso_flush(self._h))

    def host_buffer(self, n_buffers):
        """a pinned numpy array [n_objects][n_buffers * 513] float32 for step_to_host (freed with the engine)"""
        n = len(self.n_modes) * n_buffers * self.B
        p = C.c_void_p()
        rc = self._l.pbso_host_alloc(n * 4, C.byref(p))
        if rc != capi.OK:
            raise PbsoError(rc, "pbso_host_alloc failed")
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,))
        return arr.reshape(len(self.n_modes), n_buffers * self.B)

    def step_to_host(self, n_buffers, out):
        """pbso_step_to_host: the step's audio of all objects into `out` (a host_buffer), asynchronously"""
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == len(self.n_modes) * n_buffers * self.B
        self._chk(self._l.pbso_step_to_host(self._h, n_buffers, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        self._last_nb = n_buffers
        self._borrowed = None

    def host_wait(self):
        self._chk(self._l.pbso_host_wait(self._h))

    def audio(self):
        n = len(self.n_modes) * self._last_nb * self.B
        out = np.empty(n, dtype=np.float32)
        self._chk(self._l.pbso_read_audio(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out.reshape(len(self.n_modes), self._last_nb * self.B)

    def audio_rows(self, rows):
        """the last step's audio of some objects only: [len(rows)][n_buffers * 513] float32"""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.empty((r.size, self._last_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_read_audio_rows(self._h, r.ctypes.data_as(C.POINTER(C.c_int)), r.size, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def emitted(self):
        n = len(self.n_modes) * self._last_nb
        out = np.empty(n, dtype=np.uint8)
        self._chk(self._l.pbso_read_emitted(self._h, out.ctypes.data_as(C.POINTER(C.c_ubyte)), n))
        return out.reshape(len(self.n_modes), self._last_nb).astype(bool)

    def qnorm(self, obj, buffer):
        n = self.n_modes[obj]
        out = np.empty(max(n, 1), dtype=np.float32)
        self._chk(self._l.pbso_read_qnorm(self._h, obj, buffer, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out[:n]

    def state(self, obj):
        n = self.n_modes[obj]
        q1, q2 = np.empty(max(n, 1)), np.empty(max(n, 1))
        self._chk(self._l.pbso_read_state(self._h, obj, _dp(q1), _dp(q2), n))
        return q1[:n], q2[:n]

    def set_state(self, obj, q1, q2):
        """pbso_write_state: restore (q_{k-1}, q_{k-2}) as state() returned them"""
        a = np.ascontiguousarray(q1, dtype=np.float64)
        b = np.ascontiguousarray(q2, dtype=np.float64)
        assert a.size == b.size
        self._chk(self._l.pbso_write_state(self._h, obj, _dp(a), _dp(b), a.size))

    def set_material(self, ids, density, alpha, beta, keep_state=True):
        """pbso_set_material: a new material for the objects `ids` of a finalized engine, in force from the next step's first
        sample; scalars broadcast over the ids.  keep_state: the state carries on (True) or is zeroed (False)."""
        mats = material_array(ids, density, alpha, beta)
        oid = np.ascontiguousarray(np.atleast_1d(ids), dtype=np.int32)
        self._chk(self._l.pbso_set_material(self._h, oid.size, oid.ctypes.data_as(C.POINTER(C.c_int)), mats, int(bool(keep_state))))

    def material(self, obj):
        """pbso_get_material: (density, alpha, beta) in force for an object"""
        m = capi.Material()
        self._chk(self._l.pbso_get_material(self._h, int(obj), C.byref(m)))
        return m.density, m.alpha, m.beta

    def material_stats(self):
        """pbso_material_stats: calls accepted, objects retuned, modes rebuilt, g32 elements rebuilt"""
        out = (C.c_int64 * 4)()
        self._chk(self._l.pbso_material_stats(self._h, out))
        return tuple(int(v) for v in out)

    def census(self, n_teams=None):
        """per-workgroup (start, end [100 MHz ticks], HW_ID, XCC_ID, clock start/end, block form: cycles in head / pipeline / barrier / combine) of the last launch (PBSO_CENSUS=1).
        n_teams: the number of rows to read when the launch ran on the kernel of under-filled scenes (one team per 64 modes)."""
        n = (self.info()["n_teams"] if n_teams is None else n_teams) * 12
        out = np.empty(n, dtype=np.uint64)
        self._chk(self._l.pbso_read_census(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out.reshape(-1, 12)

    def audio_device_ptr(self):
        return self._l.pbso_audio_device_ptr(self._h)

    def mix_objects(self, d_out):
        """pbso_mix_objects: the last step's audio summed over the objects, into the device buffer d_out [n_buffers * 513] f32"""
        self._chk(self._l.pbso_mix_objects(self._h, C.c_void_p(d_out)))

    # -- scene mix: C channels, a ramped gain and a fractional delay (samples) per (channel, object) -------------------------
    def scene_mix_enable(self, n_channels, max_delay, ramp_samples=0):
        """pbso_scene_mix_enable: from the next step on, every step is mixed exactly once (scene_mix)"""
        self._chk(self._l.pbso_scene_mix_enable(self._h, n_channels, max_delay, ramp_samples))
        self._scene_c, self._scene_nb = n_channels, 0

    def scene_mix_set(self, gain, delay=None):
        """pbso_scene_mix_set: gain / delay [n_channels][n_objects]; delay None keeps the delays"""
        fp = C.POINTER(C.c_float)
        g = np.ascontiguousarray(gain, dtype=np.float32)
        d = None if delay is None else np.ascontiguousarray(delay, dtype=np.float32)
        assert g.size == self._scene_c * len(self.n_modes) and (d is None or d.size == g.size)
        self._chk(self._l.pbso_scene_mix_set(self._h, g.ctypes.data_as(fp), None if d is None else d.ctypes.data_as(fp)))

    def scene_mix(self, d_out=None):
        """pbso_scene_mix: the last step into the device buffer d_out [n_channels][n_buffers * 513] f32 (None: the engine's own)"""
        self._chk(self._l.pbso_scene_mix(self._h, None if d_out is None else C.c_void_p(d_out)))
        self._scene_nb = self._last_nb

    def read_scene_mix(self):
        """the last scene mix: [n_channels][n_buffers * 513] float32 (synchronous)"""
        out = np.empty((self._scene_c, self._scene_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_read_scene_mix(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def scene_mix_reset(self):
        self._chk(self._l.pbso_scene_mix_reset(self._h))

    def scene_mix_set_at(self, t_set, gain, delay=None):
        """pbso_scene_mix_set_at: as scene_mix_set, taking effect at the absolute sample t_set (inside a step or not)"""
        fp = C.POINTER(C.c_float)
        g = np.ascontiguousarray(gain, dtype=np.float32)
        d = None if delay is None else np.ascontiguousarray(delay, dtype=np.float32)
        c = getattr(self, "_scene_c", 0)                             # (not enabled yet: the call itself says so)
        assert not c or (g.size == c * len(self.n_modes) and (d is None or d.size == g.size))
        self._chk(self._l.pbso_scene_mix_set_at(self._h, int(t_set), g.ctypes.data_as(fp), None if d is None else d.ctypes.data_as(fp)))

    def scene_mix_schedule(self, t_set, gain, delay=None):
        """pbso_scene_mix_schedule: t_set [n_sets] ascending absolute samples, gain / delay [n_sets][n_channels][n_objects]; delay
        None keeps the delays in all of them.  All or nothing."""
        fp = C.POINTER(C.c_float)
        t = np.ascontiguousarray(t_set, dtype=np.int64)
        g = np.ascontiguousarray(gain, dtype=np.float32)
        d = None if delay is None else np.ascontiguousarray(delay, dtype=np.float32)
        c = getattr(self, "_scene_c", 0)
        assert not c or (g.size == t.size * c * len(self.n_modes) and (d is None or d.size == g.size))
        self._chk(self._l.pbso_scene_mix_schedule(self._h, t.size, t.ctypes.data_as(C.POINTER(C.c_int64)), g.ctypes.data_as(fp),
                                                  None if d is None else d.ctypes.data_as(fp)))

    def scene_mix_clear_schedule(self):
        """pbso_scene_mix_clear_schedule: drops the scheduled sets not yet in force"""
        self._chk(self._l.pbso_scene_mix_clear_schedule(self._h))

    def scene_mix_info(self):
        """pbso_scene_mix_info: t of the next mixed sample, scheduled sets still pending, mixes, sets accepted"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_scene_mix_info(self._h, v))
        return {"t": v[0], "pending": v[1], "mixes": v[2], "sets": v[3]}

    # -- scene filter mix: C channels, K taps per (channel, object) behind an integer onset (samples) per object ---------------
    def scene_fir_enable(self, n_channels, n_taps, max_onset, xfade_samples=0):
        """pbso_scene_fir_enable: from the next step on, every step is mixed exactly once (scene_fir)"""
        self._chk(self._l.pbso_scene_fir_enable(self._h, n_channels, n_taps, max_onset, xfade_samples))
        self._fir_c, self._fir_k, self._fir_nb = n_channels, n_taps, 0

    def scene_fir_set(self, taps, onset=None):
        """pbso_scene_fir_set: taps [n_channels][n_objects][n_taps], onset [n_objects] ints; onset None keeps the onsets"""
        h = np.ascontiguousarray(taps, dtype=np.float32)
        d = None if onset is None else np.ascontiguousarray(onset, dtype=np.int32)
        assert h.size == self._fir_c * len(self.n_modes) * self._fir_k and (d is None or d.size == len(self.n_modes))
        self._chk(self._l.pbso_scene_fir_set(self._h, h.ctypes.data_as(C.POINTER(C.c_float)),
                                             None if d is None else d.ctypes.data_as(C.POINTER(C.c_int))))

    def scene_fir(self, d_out=None):
        """pbso_scene_fir: the last step into the device buffer d_out [n_channels][n_buffers * 513] f32 (None: the engine's own)"""
        self._chk(self._l.pbso_scene_fir(self._h, None if d_out is None else C.c_void_p(d_out)))
        self._fir_nb = self._last_nb

    def read_scene_fir(self):
        """the last scene filter mix: [n_channels][n_buffers * 513] float32 (synchronous)"""
        out = np.empty((self._fir_c, self._fir_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_read_scene_fir(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def scene_fir_reset(self):
        self._chk(self._l.pbso_scene_fir_reset(self._h))

    def scene_fir_info(self):
        """pbso_scene_fir_info: t of the next mixed sample, the first t at which the running fade is over, mixes, sets"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_scene_fir_info(self._h, v))
        return {"t": v[0], "fade_end": v[1], "mixes": v[2], "sets": v[3]}

    def scene_fir_delay_enable(self, max_delay, ramp_samples=0):
        """pbso_scene_fir_delay_enable: a ramped fractional delay per object in front of the filters (before the first mix)"""
        self._chk(self._l.pbso_scene_fir_delay_enable(self._h, max_delay, ramp_samples))

    def scene_fir_set_delay(self, delay):
        """pbso_scene_fir_set_delay: delay [n_objects] in samples, 0 <= d <= max_delay"""
        d = np.ascontiguousarray(delay, dtype=np.float32)
        assert d.size == len(self.n_modes)
        self._chk(self._l.pbso_scene_fir_set_delay(self._h, d.ctypes.data_as(C.POINTER(C.c_float))))

    def scene_fir_delay_info(self):
        """pbso_scene_fir_delay_info: max_delay, ramp_samples, the first t at which every delay ramp is over, delay sets"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_scene_fir_delay_info(self._h, v))
        return {"max_delay": v[0], "ramp_samples": v[1], "ramp_end": v[2], "sets": v[3]}

    # ... and the schedule of both kinds of set: sets that take effect at absolute samples, any number of them inside one step
    def scene_fir_set_at(self, t_set, taps, onset=None):
        """pbso_scene_fir_set_at: as scene_fir_set, taking effect at the absolute sample t_set (inside a step or not)"""
        h = np.ascontiguousarray(taps, dtype=np.float32)
        d = None if onset is None else np.ascontiguousarray(onset, dtype=np.int32)
        c = getattr(self, "_fir_c", 0)                               # (not enabled yet: the call itself says so)
        assert not c or (h.size == c * len(self.n_modes) * self._fir_k and (d is None or d.size == len(self.n_modes)))
        self._chk(self._l.pbso_scene_fir_set_at(self._h, int(t_set), h.ctypes.data_as(C.POINTER(C.c_float)),
                                                None if d is None else d.ctypes.data_as(C.POINTER(C.c_int))))

    def scene_fir_schedule(self, t_set, taps, onset=None):
        """pbso_scene_fir_schedule: t_set [n_sets] ascending absolute samples, taps [n_sets][n_channels][n_objects][n_taps], onset
        [n_sets][n_objects] ints; onset None keeps the onsets in all of them.  All or nothing."""
        t = np.ascontiguousarray(t_set, dtype=np.int64)
        h = np.ascontiguousarray(taps, dtype=np.float32)
        d = None if onset is None else np.ascontiguousarray(onset, dtype=np.int32)
        c = getattr(self, "_fir_c", 0)
        assert not c or (h.size == t.size * c * len(self.n_modes) * self._fir_k and (d is None or d.size == t.size * len(self.n_modes)))
        self._chk(self._l.pbso_scene_fir_schedule(self._h, t.size, t.ctypes.data_as(C.POINTER(C.c_int64)), h.ctypes.data_as(C.POINTER(C.c_float)),
                                                  None if d is None else d.ctypes.data_as(C.POINTER(C.c_int))))

    def scene_fir_set_delay_at(self, t_set, delay):
        """pbso_scene_fir_set_delay_at: as scene_fir_set_delay, taking effect at the absolute sample t_set"""
        d = np.ascontiguousarray(delay, dtype=np.float32)
        assert d.size == len(self.n_modes)
        self._chk(self._l.pbso_scene_fir_set_delay_at(self._h, int(t_set), d.ctypes.data_as(C.POINTER(C.c_float))))

    def scene_fir_delay_schedule(self, t_set, delay):
        """pbso_scene_fir_delay_schedule: t_set [n_sets] ascending absolute samples, delay [n_sets][n_objects].  All or nothing."""
        t = np.ascontiguousarray(t_set, dtype=np.int64)
        d = np.ascontiguousarray(delay, dtype=np.float32)
        assert d.size == t.size * len(self.n_modes)
        self._chk(self._l.pbso_scene_fir_delay_schedule(self._h, t.size, t.ctypes.data_as(C.POINTER(C.c_int64)),
                                                        d.ctypes.data_as(C.POINTER(C.c_float))))

    def scene_fir_clear_schedule(self):
        """pbso_scene_fir_clear_schedule: drops the scheduled filter and delay sets not yet in force"""
        self._chk(self._l.pbso_scene_fir_clear_schedule(self._h))

    def scene_fir_schedule_info(self):
        """pbso_scene_fir_schedule_info: t of the next mixed sample, filter sets pending, delay sets pending, the smallest t_set the
        next scheduled filter set may have"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_scene_fir_schedule_info(self._h, v))
        return {"t": v[0], "pending": v[1], "pending_delay": v[2], "next_t_min": v[3]}

    # ... and the bank: the filters stay on the device, a set is J (index, weight) pairs per object
    def scene_fir_bank_create(self, taps):
        """pbso_scene_fir_bank_create: taps [n_filters][n_channels][n_taps], finite; a second create replaces the bank"""
        h = np.ascontiguousarray(taps, dtype=np.float32)
        assert h.ndim == 3
        self._chk(self._l.pbso_scene_fir_bank_create(self._h, h.shape[0], h.ctypes.data_as(C.POINTER(C.c_float))))

    def scene_fir_bank_info(self):
        """pbso_scene_fir_bank_info: filters in the bank (0: none), the largest J, bank sets accepted, device bytes of the bank"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_scene_fir_bank_info(self._h, v))
        return {"n_filters": v[0], "max_j": v[1], "sets": v[2], "bytes": v[3]}

    @staticmethod
    def _bank_pairs(index, weight, onset, lead):
        """index / weight [*lead][n_objects][J] -> (J, the three arrays as the C ABI takes them)"""
        i = np.ascontiguousarray(index, dtype=np.int32)
        w = np.ascontiguousarray(weight, dtype=np.float32)
        d = None if onset is None else np.ascontiguousarray(onset, dtype=np.int32)
        assert i.ndim == lead + 2 and w.shape == i.shape and (d is None or d.shape == i.shape[:-1])
        return (i.shape[-1], i.ctypes.data_as(C.POINTER(C.c_int)), w.ctypes.data_as(C.POINTER(C.c_float)),
                None if d is None else d.ctypes.data_as(C.POINTER(C.c_int))), (i, w, d)

    def scene_fir_set_bank(self, index, weight, onset=None):
        """pbso_scene_fir_set_bank: index, weight [n_objects][J] into the bank, onset [n_objects] ints; as scene_fir_set with the
        taps acc = fmaf(weight[o][j], bank[index[o][j]][c][k], acc), j ascending"""
        args, _keep = self._bank_pairs(index, weight, onset, 0)
        self._chk(self._l.pbso_scene_fir_set_bank(self._h, *args))

    def scene_fir_set_bank_at(self, t_set, index, weight, onset=None):
        """pbso_scene_fir_set_bank_at: as scene_fir_set_bank, taking effect at the absolute sample t_set"""
        args, _keep = self._bank_pairs(index, weight, onset, 0)
        self._chk(self._l.pbso_scene_fir_set_bank_at(self._h, int(t_set), *args))

    def scene_fir_bank_schedule(self, t_set, index, weight, onset=None):
        """pbso_scene_fir_bank_schedule: t_set [n_sets] ascending absolute samples, index and weight [n_sets][n_objects][J], onset
        [n_sets][n_objects] ints or None.  All or nothing."""
        t = np.ascontiguousarray(t_set, dtype=np.int64)
        args, keep = self._bank_pairs(index, weight, onset, 1)
        assert keep[0].shape[0] == t.size
        self._chk(self._l.pbso_scene_fir_bank_schedule(self._h, t.size, t.ctypes.data_as(C.POINTER(C.c_int64)), *args))

    # -- scene reverb: n_in device-resident bus signals through K taps per (output channel, input), history kept across steps ----
    def scene_reverb_enable(self, n_in, n_out, n_taps, xfade_samples=0):
        """pbso_scene_reverb_enable: from the next step on, every step is processed exactly once (scene_reverb)"""
        self._chk(self._l.pbso_scene_reverb_enable(self._h, n_in, n_out, n_taps, xfade_samples))
        self._rev_shape, self._rev_nb = (n_out, n_in, n_taps), 0

    def scene_reverb_set(self, taps):
        """pbso_scene_reverb_set: taps [n_out][n_in][n_taps], finite"""
        h = np.ascontiguousarray(taps, dtype=np.float32)
        assert h.size == int(np.prod(self._rev_shape))
        self._chk(self._l.pbso_scene_reverb_set(self._h, h.ctypes.data_as(C.POINTER(C.c_float))))

    def scene_reverb(self, d_in, d_add=None, d_out=None):
        """pbso_scene_reverb: the device buffer d_in [n_in][n_buffers * 513] f32 of the last step convolved into d_out
        [n_out][n_buffers * 513] (None: the engine's own), on top of d_add (None: nothing; may be d_out).  Device pointers as integers."""
        vp = lambda p: None if p is None else C.c_void_p(p)
        self._chk(self._l.pbso_scene_reverb(self._h, vp(d_in), vp(d_add), vp(d_out)))
        self._rev_nb = self._last_nb

    def read_scene_reverb(self):
        """the last scene reverb output: [n_out][n_buffers * 513] float32 (synchronous)"""
        out = np.empty((self._rev_shape[0], self._rev_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_read_scene_reverb(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def scene_reverb_reset(self):
        self._chk(self._l.pbso_scene_reverb_reset(self._h))

    def scene_reverb_info(self):
        """pbso_scene_reverb_info: t of the next processed sample, the first t at which the running fade is over, calls, sets"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_scene_reverb_info(self._h, v))
        return {"t": v[0], "fade_end": v[1], "calls": v[2], "sets": v[3]}

    # -- master bus: gain, look-ahead limiter, meters and 16-bit PCM on a device buffer [C][n], history kept across steps ----------
    def master_enable(self, n_channels, ceiling, lookahead=64, hold=0, ramp_samples=0):
        """pbso_master_enable: from the next step on, every step is processed exactly once (master)"""
        self._chk(self._l.pbso_master_enable(self._h, n_channels, ceiling, lookahead, hold, ramp_samples))
        self._master_shape, self._master_nb = (n_channels, lookahead), 0

    def master_set_gain(self, gain):
        """pbso_master_set_gain: takes effect at the first sample of the next processed step, ramped over ramp_samples"""
        self._chk(self._l.pbso_master_set_gain(self._h, gain))

    def master(self, d_in, d_out=None):
        """pbso_master: the device buffer d_in [C][n_buffers * 513] f32 of the last step through the gain and the limiter into
        d_out (None: the engine's own; may be d_in), delayed by the look-ahead.  Device pointers as integers."""
        vp = lambda p: None if p is None else C.c_void_p(p)
        self._chk(self._l.pbso_master(self._h, vp(d_in), vp(d_out)))
        self._master_nb = self._last_nb

    def read_master(self):
        """the last master output: [C][n_buffers * 513] float32 (synchronous)"""
        out = np.empty((self._master_shape[0], self._master_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_read_master(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def read_master_pcm16(self):
        """the last master output as interleaved 16-bit PCM, converted on the device: [n_buffers * 513][C] int16"""
        out = np.empty((self._master_nb * self.B, self._master_shape[0]), dtype=np.int16)
        self._chk(self._l.pbso_read_master_pcm16(self._h, out.ctypes.data_as(C.POINTER(C.c_int16)), out.size))
        return out

    def read_master_meters(self):
        """the last call's meters: a structured array [n_buffers][C] (in_peak, out_peak, min_gain, n_limited, sumsq)"""
        out = np.empty((self._master_nb, self._master_shape[0]), dtype=np.dtype(capi.MasterMeter))
        self._chk(self._l.pbso_read_master_meters(self._h, out.ctypes.data_as(C.POINTER(capi.MasterMeter)), out.size))
        return out

    def master_window(self):
        """the L taps of the smoothing window in force, float32"""
        out = np.empty(self._master_shape[1], dtype=np.float32)
        self._chk(self._l.pbso_master_window(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def master_reset(self):
        self._chk(self._l.pbso_master_reset(self._h))

    def master_info(self):
        """pbso_master_info: t of the next processed sample, the first t at which the gain ramp is over, calls, sets"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_master_info(self._h, v))
        return {"t": v[0], "ramp_end": v[1], "calls": v[2], "sets": v[3]}

    # -- resampler bus: a device buffer [C][n] at the engine's rate out at another rate, history kept across steps ----------------
    def resample_enable(self, rate_out, n_channels, taps=32, beta=9.0, cutoff=0.9):
        """pbso_resample_enable: from the next step on, every step is processed exactly once (resample)"""
        self._chk(self._l.pbso_resample_enable(self._h, n_channels, rate_out, taps, beta, cutoff))
        self._rs_channels, self._rs_n_out = n_channels, 0

    def resample(self, d_in, d_out=None, out_stride=0):
        """pbso_resample: the device buffer d_in [C][n_buffers * frames] f32 of the last step at the output rate into d_out
        [C][out_stride] (None: the engine's own, stride n_out; must not overlap d_in).  Device pointers as integers.  Returns n_out,
        the number of output samples per channel, which differs from call to call."""
        vp = lambda p: None if p is None else C.c_void_p(p)
        n_out = C.c_int64(0)
        self._chk(self._l.pbso_resample(self._h, vp(d_in), vp(d_out), out_stride, C.byref(n_out)))
        self._rs_n_out = n_out.value
        return n_out.value

    def resample_max_out(self, n_buffers):
        """ceil(n L / M): the most outputs per channel a step of n_buffers can have"""
        v = C.c_int64(0)
        self._chk(self._l.pbso_resample_max_out(self._h, n_buffers, C.byref(v)))
        return v.value

    def read_resample(self):
        """the last resampler output: [C][n_out] float32 (synchronous)"""
        out = np.empty((self._rs_channels, self._rs_n_out), dtype=np.float32)
        self._chk(self._l.pbso_read_resample(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def read_resample_pcm16(self):
        """the last resampler output as interleaved 16-bit PCM, saturated and converted on the device: [n_out][C] int16"""
        out = np.empty((self._rs_n_out, self._rs_channels), dtype=np.int16)
        self._chk(self._l.pbso_read_resample_pcm16(self._h, out.ctypes.data_as(C.POINTER(C.c_int16)), out.size))
        return out

    def read_resample_meters(self):
        """the last call's meters: a structured array [C] (out_peak, n_over)"""
        out = np.empty(self._rs_channels, dtype=np.dtype(capi.ResampleMeter))
        self._chk(self._l.pbso_read_resample_meters(self._h, out.ctypes.data_as(C.POINTER(capi.ResampleMeter)), out.size))
        return out

    def resample_taps(self):
        """the phase table in force: [L][T] float32"""
        i = self.resample_info()
        out = np.empty((i["L"], i["T"]), dtype=np.float32)
        self._chk(self._l.pbso_resample_taps(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def resample_reset(self):
        self._chk(self._l.pbso_resample_reset(self._h))

    def resample_info(self):
        """pbso_resample_info: t, m, calls, L, M, T, N - 1 (the delay is that over 2 L input samples), n_out of the last call"""
        v = (C.c_int64 * 8)()
        self._chk(self._l.pbso_resample_info(self._h, v))
        return {"t": v[0], "m": v[1], "calls": v[2], "L": v[3], "M": v[4], "T": v[5], "delay_num": v[6], "n_out": v[7]}

    # -- EQ bus: biquad cascades per channel of a device buffer [C][n], block-parallel in fp64, state kept across steps -----------
    def eq_enable(self, n_channels, n_sections, xfade_samples=0):
        """pbso_eq_enable: the identity cascade; from the next step on, every step is processed exactly once (eq)"""
        self._chk(self._l.pbso_eq_enable(self._h, n_channels, n_sections, xfade_samples))
        self._eq_shape, self._eq_nb = (n_channels, n_sections), 0

    def eq_set(self, sos):
        """pbso_eq_set: sos [C][S][5] = b0 b1 b2 a1 a2 in fp64; takes effect at the first sample of the next processed step"""
        c = np.ascontiguousarray(sos, dtype=np.float64)
        if c.size != self._eq_shape[0] * self._eq_shape[1] * 5:
            raise PbsoError(capi.ERR_INVALID, "eq_set: sos must be [n_channels][n_sections][5]")
        self._chk(self._l.pbso_eq_set(self._h, c.ctypes.data_as(C.POINTER(C.c_double))))

    def eq_set_at(self, t_set, sos):
        """pbso_eq_set_at: as eq_set, taking effect at the absolute sample t_set (inside a step or not)"""
        self.eq_schedule([int(t_set)], np.ascontiguousarray(sos, dtype=np.float64)[None], _one=True)

    def eq_schedule(self, t_set, sos, _one=False):
        """pbso_eq_schedule: t_set [n_sets] ascending absolute samples, sos [n_sets][C][S][5].  All or nothing."""
        t = np.ascontiguousarray(t_set, dtype=np.int64)
        c = np.ascontiguousarray(sos, dtype=np.float64)
        shape = getattr(self, "_eq_shape", None)                     # (not enabled yet: the call itself says so)
        if shape is not None and c.size != t.size * shape[0] * shape[1] * 5:
            raise PbsoError(capi.ERR_INVALID, "eq_schedule: sos must be [n_sets][n_channels][n_sections][5]")
        tp, dp = t.ctypes.data_as(C.POINTER(C.c_int64)), c.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self._l.pbso_eq_set_at(self._h, int(t[0]), dp) if _one else self._l.pbso_eq_schedule(self._h, t.size, tp, dp))

    def eq_clear_schedule(self):
        """pbso_eq_clear_schedule: drops the scheduled sets not yet in force"""
        self._chk(self._l.pbso_eq_clear_schedule(self._h))

    def eq_schedule_info(self):
        """pbso_eq_schedule_info: t of the next processed sample, scheduled sets pending, the smallest t_set the next scheduled set may
        have, the sets that took effect inside the last processed step"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_eq_schedule_info(self._h, v))
        return {"t": v[0], "pending": v[1], "next_t_min": v[2], "sets_in_step": v[3]}

    def eq(self, d_in, d_out=None):
        """pbso_eq: the device buffer d_in [C][n_buffers * frames] f32 of the last step through the cascades into d_out (None: the
        engine's own; may be d_in).  Device pointers as integers."""
        vp = lambda p: None if p is None else C.c_void_p(p)
        self._chk(self._l.pbso_eq(self._h, vp(d_in), vp(d_out)))
        self._eq_nb = self._last_nb

    def read_eq(self):
        """the last EQ output: [C][n_buffers * frames] float32 (synchronous)"""
        out = np.empty((self._eq_shape[0], self._eq_nb * self.B), dtype=np.float32)
        self._chk(self._l.pbso_read_eq(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def eq_tables(self):
        """the block tables in force: [C][S][5][PBSO_EQ_BLOCK] float64, in the order h r s p q"""
        out = np.empty(self._eq_shape + (5, capi.EQ_BLOCK), dtype=np.float64)
        self._chk(self._l.pbso_eq_tables(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def eq_reset(self):
        self._chk(self._l.pbso_eq_reset(self._h))

    def eq_info(self):
        """pbso_eq_info: t of the next processed sample, the first t at which the running fade is over, calls, sets"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_eq_info(self._h, v))
        return {"t": v[0], "fade_end": v[1], "calls": v[2], "sets": v[3]}

    # -- loudness bus: BS.1770 energies and true peaks per 100 ms of a device buffer [C][n], logged on the device ----------------
    def loudness_enable(self, n_channels, weight=None, max_blocks=36000, true_peak=True):
        """pbso_loudness_enable: weight [C] doubles or None (all 1); max_blocks records of 100 ms per channel (36000 is an hour);
        from the next step on, every step is measured exactly once (loudness)"""
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        if w is not None and w.size != n_channels:
            raise PbsoError(capi.ERR_INVALID, "loudness_enable: weight must be [n_channels]")
        self._chk(self._l.pbso_loudness_enable(self._h, n_channels, None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)),
                                               max_blocks, 1 if true_peak else 0))
        self._loud_channels = n_channels

    def loudness(self, d_in):
        """pbso_loudness: measures the device buffer d_in [C][n_buffers * frames] f32 of the last step (read only).  A device
        pointer as an integer."""
        self._chk(self._l.pbso_loudness(self._h, None if d_in is None else C.c_void_p(d_in)))

    def read_loudness_blocks(self, first=0, n=None):
        """records [first, first + n) of the log (n None: all behind first): a structured array [n][C] (energy, true_peak, sample_peak)"""
        if n is None:
            n = self.loudness_info()["blocks"] - first
        channels = getattr(self, "_loud_channels", 1)                # (not enabled yet: the call itself says so)
        out = np.empty((max(n, 0), channels), dtype=np.dtype(capi.LOUDNESS_BLOCK))
        self._chk(self._l.pbso_read_loudness_blocks(self._h, first, n, out.ctypes.data_as(C.POINTER(capi.LoudnessBlock))))
        return out

    def loudness_report(self):
        """pbso_loudness_report: integrated, momentary, short_term, their maxima, relative_threshold (LUFS), true_peak and
        sample_peak (linear), n_blocks, n_gated"""
        r = capi.LoudnessSummary()
        self._chk(self._l.pbso_loudness_report(self._h, C.byref(r)))
        return capi.loudness_summary(r)

    def loudness_taps(self):
        """the true peak's phase table: [O][12] float32, O = 4 below 80 kHz and 2 from there up"""
        O = 4 if self.sample_rate < 80000 else 2
        out = np.empty((O, 12), dtype=np.float32)
        self._chk(self._l.pbso_loudness_taps(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def loudness_reset(self):
        self._chk(self._l.pbso_loudness_reset(self._h))

    def loudness_info(self):
        """pbso_loudness_info: t of the next measured sample, blocks logged, calls, max_blocks"""
        v = (C.c_int64 * 4)()
        self._chk(self._l.pbso_loudness_info(self._h, v))
        return {"t": v[0], "blocks": v[1], "calls": v[2], "max_blocks": v[3]}

    def info(self):
        i = capi.EngineInfo()
        self._chk(self._l.pbso_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in capi.EngineInfo._fields_}


class ModalSolver:
    """One-object facade with the reference's ModalSolver<double> method names
    (modal_solver.h:100-179).  step() produces one 513-sample buffer."""

    def __init__(self, omega_squared, density, alpha, beta, N_modes=None, mode_shapes=None, **engine_kw):
        self.engine = Engine(**engine_kw)
        self.obj = self.engine.add_object(omega_squared, density, alpha, beta, N_modes, mode_shapes)
        self._N_modes = self.engine.n_modes[self.obj]
        self._queue_sound = collections.deque()       # ReaderWriterQueue(2): 3 usable slots
        self._queue_qnorm = collections.deque()
        self._pending_maps = None
        self._final = False
        self._host = None                             # pinned [1][513]: the bank stores the buffer's samples straight into it

    def readFFATMaps(self, maps_or_dir):
        if isinstance(maps_or_dir, str):
            self.engine.read_ffat_maps(self.obj, maps_or_dir)
        else:
            self.engine.set_ffat_maps(self.obj, maps_or_dir)

    def _ensure(self):
        if not self._final:
            self.engine.finalize()
            self._final = True

    def enqueueForceMessage(self, mess):
        self._ensure()
        return self.engine.enqueue_force(self.obj, mess)

    def enqueueForceMessageNoFail(self, mess, maxIte=-1):
        return self.enqueueForceMessage(mess)

    def enqueueArprmMessageNoFail(self, a, sigma, mu, maxIte=-1):
        self._ensure()
        return self.engine.enqueue_arprm(self.obj, a, sigma, mu)

    def computeTransfer(self, pos, out=None):
        self._ensure()
        if out is None:
            return self.engine.compute_transfer(self.obj, pos)
        ok, vals = self.engine.compute_transfer_batch(self.obj, pos, out.size)
        if ok:
            out[:] = vals[0]
        return ok

    def setUseTransfer(self, s):
        self._ensure()
        self.engine.set_use_transfer(self.obj, s)

    def getLatestTransfer(self):
        self._ensure()
        return self.engine.latest_transfer(self.obj)

    def step(self):
        self._ensure()
        if self._host is None:
            self._host = self.engine.host_buffer(1)
        # the buffer's samples arrive in pinned host memory with the kernel's own stores (pbso_step_to_host): no copy call
        # between the oscillator bank and the SoundMessage
        self.engine.step_to_host(1, self._host)
        self.engine.host_wait()
        if not self.engine.emitted()[0, 0]:
            return                                   # clearAllForces: no SoundMessage (modal_solver.h:186-189)
        if self.engine.qnorm_mode != capi.QNORM_OFF and len(self._queue_qnorm) < 3:
            self._queue_qnorm.append(self.engine.qnorm(0, 0))     # try_enqueue, may drop (:273)
        self._queue_sound.append(self._host[0].copy())            # enqueueSoundMessageNoFail (:275)

    def dequeueSoundMessage(self):
        if not self._queue_sound:
            return None
        return self._queue_sound.popleft()

    def getQBufferNorm(self):
        if self._queue_qnorm:
            return self._queue_qnorm.popleft()
        return np.zeros(self._N_modes, dtype=np.float32)
