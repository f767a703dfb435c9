"""ctypes binding of include/openpbso_amd.h (libopenpbso_amd.so).

Fails loudly when the library is missing -- the HIP path is the only path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBSO_LIB") or os.path.join(_HERE, "libopenpbso_amd.so")      # PBSO_LIB: A/B runs of two builds in one process tree

ABI_VERSION = 6
OK = 0
ERR_INVALID, ERR_HIP, ERR_STATE, ERR_IO, ERR_MISSING_MAP, ERR_ASSERT, ERR_NOMEM = -1, -2, -3, -4, -5, -6, -7
POINT_FORCE, GAUSSIAN_FORCE, AUTOREGRESSIVE_FORCE, TRACK_FORCE = 0, 1, 2, 3
DATA_EXPLICIT, DATA_VERTEX, DATA_FACE, DATA_ZERO = 0, 1, 2, 3
FORM_BLOCK, FORM_VELOCITY, FORM_DIRECT, FORM_BLOCK_BF16 = 0, 1, 2, 3
QNORM_OFF, QNORM_ALL, QNORM_CLOSED = 0, 1, 2

# every symbol include/openpbso_amd.h declares
EXPORTS = [
    "pbso_abi_version", "pbso_status_string", "pbso_engine_create", "pbso_engine_destroy",
    "pbso_last_error", "pbso_add_object", "pbso_add_object_from_files", "pbso_object_set_ffat_maps",
    "pbso_object_read_ffat_maps", "pbso_fatcube_parse", "pbso_ffat_map_free", "pbso_finalize",
    "pbso_enqueue_force", "pbso_enqueue_force_batch", "pbso_enqueue_vertex_hits", "pbso_enqueue_strokes", "pbso_stroke_stats", "pbso_enqueue_arprm", "pbso_compute_transfer", "pbso_compute_transfer_batch", "pbso_object_n_maps", "pbso_listeners_enable", "pbso_mix_listeners",
    "pbso_set_use_transfer", "pbso_get_latest_transfer", "pbso_step", "pbso_step_into", "pbso_sync",
    "pbso_read_audio", "pbso_read_emitted", "pbso_read_qnorm", "pbso_read_state", "pbso_write_state",
    "pbso_audio_device_ptr", "pbso_pa_convert", "pbso_get_info",
    "pbso_modes_read", "pbso_num_modes_audible", "pbso_material_read", "pbso_free", "pbso_read_census", "pbso_obj_read", "pbso_arprm_pending", "pbso_flush",
    "pbso_mix_objects", "pbso_read_audio_rows", "pbso_compute_transfer_path",
    "pbso_step_to_host", "pbso_host_wait", "pbso_host_alloc", "pbso_host_free",
    # the scene mix (C channels, a ramped gain and fractional delay per channel and object)
    "pbso_scene_mix_enable", "pbso_scene_mix_set", "pbso_scene_mix", "pbso_read_scene_mix", "pbso_scene_mix_reset",
    # ... and its schedule (sets that take effect at absolute samples, any number of them inside one step)
    "pbso_scene_mix_set_at", "pbso_scene_mix_schedule", "pbso_scene_mix_clear_schedule", "pbso_scene_mix_info",
    "pbso_group_scene_mix_set_at", "pbso_group_scene_mix_schedule", "pbso_group_scene_mix_clear_schedule",
    # the scene filter mix (C channels, K taps per channel and object behind an onset per object)
    "pbso_scene_fir_enable", "pbso_scene_fir_set", "pbso_scene_fir", "pbso_read_scene_fir", "pbso_scene_fir_reset", "pbso_scene_fir_info",
    "pbso_group_scene_fir_enable", "pbso_group_scene_fir_set",
    # ... and its delay stage (a ramped fractional delay per object in front of the filters)
    "pbso_scene_fir_delay_enable", "pbso_scene_fir_set_delay", "pbso_scene_fir_delay_info",
    "pbso_group_scene_fir_delay_enable", "pbso_group_scene_fir_set_delay",
    # ... and the schedule of its filter and delay sets (sets that take effect at absolute samples, any number inside one step)
    "pbso_scene_fir_set_at", "pbso_scene_fir_schedule", "pbso_scene_fir_set_delay_at", "pbso_scene_fir_delay_schedule",
    "pbso_scene_fir_clear_schedule", "pbso_scene_fir_schedule_info",
    "pbso_group_scene_fir_set_at", "pbso_group_scene_fir_schedule", "pbso_group_scene_fir_set_delay_at",
    "pbso_group_scene_fir_delay_schedule", "pbso_group_scene_fir_clear_schedule",
    # ... and its bank (the filters stay on the device; a set is J (index, weight) pairs per object)
    "pbso_scene_fir_bank_create", "pbso_scene_fir_bank_info", "pbso_scene_fir_set_bank", "pbso_scene_fir_set_bank_at",
    "pbso_scene_fir_bank_schedule", "pbso_group_scene_fir_bank_create", "pbso_group_scene_fir_set_bank",
    "pbso_group_scene_fir_set_bank_at", "pbso_group_scene_fir_bank_schedule",
    # the scene reverb (n_in bus signals through K taps, up to 1 << 17, per output channel and input)
    "pbso_scene_reverb_enable", "pbso_scene_reverb_set", "pbso_scene_reverb", "pbso_read_scene_reverb", "pbso_scene_reverb_reset",
    "pbso_scene_reverb_info",
    # the master bus (gain, look-ahead limiter, meters and 16-bit PCM on a bus [C][n])
    "pbso_master_enable", "pbso_master_set_gain", "pbso_master", "pbso_read_master", "pbso_read_master_pcm16",
    "pbso_read_master_meters", "pbso_master_window", "pbso_master_reset", "pbso_master_info",
    # the resampler bus (a bus [C][n] at sample_rate out at another rate: rational polyphase, meters and 16-bit PCM)
    "pbso_resample_enable", "pbso_resample", "pbso_resample_max_out", "pbso_read_resample", "pbso_read_resample_pcm16",
    "pbso_read_resample_meters", "pbso_resample_taps", "pbso_resample_reset", "pbso_resample_info",
    # the EQ bus (biquad cascades per channel of a bus [C][n], block-parallel in fp64; the cookbook designs)
    "pbso_eq_enable", "pbso_eq_set", "pbso_eq", "pbso_read_eq", "pbso_eq_tables", "pbso_eq_reset", "pbso_eq_info", "pbso_eq_design",
    # ... and its schedule (sets at absolute samples, any number of them inside one step)
    "pbso_eq_set_at", "pbso_eq_schedule", "pbso_eq_clear_schedule", "pbso_eq_schedule_info",
    # the loudness bus (BS.1770 energies and true peaks per 100 ms of a bus [C][n], logged on the device; the gating on the host)
    "pbso_loudness_enable", "pbso_loudness", "pbso_read_loudness_blocks", "pbso_loudness_report", "pbso_loudness_taps",
    "pbso_loudness_reset", "pbso_loudness_info", "pbso_loudness_design", "pbso_loudness_report_from_blocks",
    # the device group (one engine per GPU, RCCL gather called from C++)
    "pbso_group_unique_id", "pbso_group_create", "pbso_group_destroy", "pbso_group_last_error", "pbso_group_plan",
    "pbso_group_rank_span", "pbso_group_owner", "pbso_group_add_object", "pbso_group_finalize", "pbso_group_engine",
    "pbso_group_enqueue_force", "pbso_group_step", "pbso_group_gather", "pbso_group_sync", "pbso_group_result_device_ptr",
    "pbso_group_read_result", "pbso_shard_by_modes", "pbso_group_scene_mix_enable", "pbso_group_scene_mix_set",
    # force tracks (caller-supplied force signals played by PBSO_TRACK_FORCE messages)
    "pbso_track_create", "pbso_enqueue_track_force", "pbso_track_stats",
    # retune: a new material for objects of a finalized engine, tables rebuilt on the device
    "pbso_set_material", "pbso_get_material", "pbso_material_stats", "pbso_group_set_material",
]
STROKE_START, STROKE_END, STROKE_ZERO = 1, 2, 4      # pbso_enqueue_strokes flags
GATHER_ALL, GATHER_ROOT, GATHER_MIX, GATHER_SCENE, GATHER_FIR = 1, 2, 3, 4, 5
GROUP_ID_BYTES = 128


class GroupDesc(C.Structure):
    pass          # (fields follow EngineDesc: set below)


class EngineDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int), ("device", C.c_int), ("frames_per_buffer", C.c_int),
                ("sample_rate", C.c_int), ("recurrence_form", C.c_int), ("qnorm_mode", C.c_int),
                ("modes_per_lane", C.c_int), ("stream", C.c_void_p),
                # ABI 4: kernel / path selection per engine (0 = the engine's policy)
                ("bank_kernel", C.c_int), ("time_chunks", C.c_int), ("direct_hits", C.c_int), ("forced_block", C.c_int),
                ("dense_launches", C.c_int), ("device_profiles", C.c_int), ("profile_kernel", C.c_int),
                ("profile_margin_pct", C.c_int), ("profile_priority", C.c_int), ("team_waves", C.c_int),
                ("pipe_consumers", C.c_int), ("pipe_max_teams", C.c_longlong), ("chunk_buffers", C.c_int),
                ("plan_threads", C.c_int), ("plan_pin", C.c_int), ("timing_every", C.c_int), ("warm_copies", C.c_int),
                ("stream_sync", C.c_int), ("latency_path", C.c_int), ("time_chunk_shape", C.c_int), ("scan_kernel", C.c_int), ("fuse_short_launches", C.c_int), ("submit_thread", C.c_int)]
BANK_AUTO, BANK_BLOCK, BANK_PIPE = 0, 1, 2


class ObjectDesc(C.Structure):
    _fields_ = [("n_modes", C.c_int), ("n_omega", C.c_int), ("omega_squared", C.POINTER(C.c_double)),
                ("density", C.c_double), ("alpha", C.c_double), ("beta", C.c_double),
                ("n_dof", C.c_int), ("mode_shapes", C.POINTER(C.c_double))]


class FfatMap(C.Structure):
    _fields_ = [("mode_id", C.c_int), ("k", C.c_double), ("center3", C.c_double * 3),
                ("cell_size", C.c_double), ("low_corners", (C.c_double * 3) * 6),
                ("n_elements", (C.c_int * 2) * 6), ("strides", C.c_int * 6),
                ("center", C.c_double * 3), ("bbox_low", C.c_double * 3), ("bbox_top", C.c_double * 3),
                ("n_psi", C.c_int), ("psi", C.POINTER(C.c_double))]


class ForceMsg(C.Structure):
    _fields_ = [("force_type", C.c_int), ("gaussian_width_us", C.c_double),
                ("sustained_force_start", C.c_int), ("sustained_force_end", C.c_int),
                ("clear_all_forces", C.c_int), ("data_kind", C.c_int),
                ("data", C.POINTER(C.c_double)), ("n_data", C.c_int), ("vids", C.c_int * 3),
                ("coords", C.c_double * 3), ("vn", C.c_double * 3)]


class TrackPlay(C.Structure):
    """pbso_track_play: which part of which track a PBSO_TRACK_FORCE message plays"""
    _fields_ = [("track", C.c_int), ("loop", C.c_int), ("start_sample", C.c_int), ("reserved", C.c_int),
                ("n_samples", C.c_int64), ("first", C.c_double), ("rate", C.c_double), ("gain", C.c_double)]


class Material(C.Structure):
    """pbso_material: what pbso_set_material gives an object, 24 bytes"""
    _fields_ = [("density", C.c_double), ("alpha", C.c_double), ("beta", C.c_double)]


class MasterMeter(C.Structure):
    """pbso_master_meter: one record per (buffer, channel) of a pbso_master call, 24 bytes"""
    _fields_ = [("in_peak", C.c_float), ("out_peak", C.c_float), ("min_gain", C.c_float), ("n_limited", C.c_int32),
                ("sumsq", C.c_double)]


class ResampleMeter(C.Structure):
    """pbso_resample_meter: one record per channel of a pbso_resample call, 8 bytes"""
    _fields_ = [("out_peak", C.c_float), ("n_over", C.c_int32)]


class LoudnessBlock(C.Structure):
    """pbso_loudness_block: one record per (sub-block of 100 ms, channel) of the loudness bus's log, 16 bytes"""
    _fields_ = [("energy", C.c_double), ("true_peak", C.c_float), ("sample_peak", C.c_float)]


class LoudnessSummary(C.Structure):
    """pbso_loudness_summary: what pbso_loudness_report fills, 80 bytes"""
    _fields_ = [("integrated", C.c_double), ("momentary", C.c_double), ("short_term", C.c_double), ("max_momentary", C.c_double),
                ("max_short_term", C.c_double), ("relative_threshold", C.c_double), ("true_peak", C.c_double),
                ("sample_peak", C.c_double), ("n_blocks", C.c_int64), ("n_gated", C.c_int64)]


class EngineInfo(C.Structure):
    _fields_ = [("n_objects", C.c_int), ("frames_per_buffer", C.c_int), ("modes_padded", C.c_int),
                ("modes_per_lane", C.c_int), ("waves_per_object", C.c_int),
                ("lds_bytes_per_workgroup", C.c_int), ("buffers_done", C.c_int64),
                ("last_step_kernel_ms", C.c_double), ("last_step_device_ms", C.c_double),
                ("last_step_host_plan_ms", C.c_double), ("last_step_forced_rows", C.c_int64),
                ("last_step_transfer_rows", C.c_int64),
                ("total_kernel_ms", C.c_double), ("total_device_ms", C.c_double),
                ("total_host_plan_ms", C.c_double), ("total_steps", C.c_int64), ("n_teams", C.c_int),
                ("recurrence_form", C.c_int), ("total_block_launches", C.c_int64), ("total_sample_launches", C.c_int64),
                ("total_timed_launches", C.c_int64), ("total_split_launches", C.c_int64),
                ("total_time_chunk_launches", C.c_int64), ("total_dropped_hits", C.c_int64), ("total_one_stream_launches", C.c_int64),
                ("total_dense_increment_launches", C.c_int64), ("total_segmented_scans", C.c_int64), ("last_time_chunk_shape", C.c_int), ("last_time_chunk_buffers", C.c_int),
                ("last_time_chunk_teams", C.c_int), ("start_gate", C.c_int), ("total_gate_timeouts", C.c_int64),
                ("total_host_submit_ms", C.c_double), ("total_ffat_shared_events", C.c_int64), ("total_ffat_general_events", C.c_int64)]


GroupDesc._fields_ = [("abi_version", C.c_int), ("devices", C.POINTER(C.c_int)), ("n_devices", C.c_int), ("world_size", C.c_int),
                      ("first_rank", C.c_int), ("unique_id", C.c_void_p), ("engine", EngineDesc), ("transport", C.c_int)]
GROUP_RCCL, GROUP_RCCL_ALWAYS, GROUP_LOOPBACK = 0, 1, 2

_lib = None


def lib():
    """Load libopenpbso_amd.so (raises if it is not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP engine first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    l = C.CDLL(LIB_PATH)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    l.pbso_abi_version.restype = C.c_int
    l.pbso_status_string.restype = C.c_char_p
    l.pbso_status_string.argtypes = [C.c_int]
    l.pbso_engine_create.argtypes = [C.POINTER(EngineDesc), C.POINTER(vp)]
    l.pbso_engine_destroy.argtypes = [vp]
    l.pbso_engine_destroy.restype = None
    l.pbso_last_error.restype = C.c_char_p
    l.pbso_last_error.argtypes = [vp]
    l.pbso_add_object.argtypes = [vp, C.POINTER(ObjectDesc), ip]
    l.pbso_add_object_from_files.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, ip, ip]
    l.pbso_object_set_ffat_maps.argtypes = [vp, C.c_int, C.POINTER(FfatMap), C.c_int]
    l.pbso_object_read_ffat_maps.argtypes = [vp, C.c_int, C.c_char_p]
    l.pbso_fatcube_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(FfatMap)]
    l.pbso_ffat_map_free.argtypes = [C.POINTER(FfatMap)]
    l.pbso_ffat_map_free.restype = None
    l.pbso_finalize.argtypes = [vp]
    l.pbso_enqueue_force.argtypes = [vp, C.c_int, C.POINTER(ForceMsg), C.c_int64]
    l.pbso_enqueue_vertex_hits.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    l.pbso_enqueue_strokes.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_ubyte), C.c_int]
    l.pbso_stroke_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_track_create"):
        # (an older build picked with PBSO_LIB for an A/B run has no tracks: using them fails there, where the call is made)
        l.pbso_track_create.argtypes = [vp, C.POINTER(C.c_float), C.c_int64, ip]
        l.pbso_enqueue_track_force.argtypes = [vp, C.c_int, C.POINTER(ForceMsg), C.POINTER(TrackPlay), C.c_int64]
        l.pbso_track_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    l.pbso_enqueue_force_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(ForceMsg), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_ubyte)]
    l.pbso_enqueue_arprm.argtypes = [vp, C.c_int, dp, C.c_double, C.c_double, C.c_int64]
    l.pbso_arprm_pending.argtypes = [vp, C.c_int]
    l.pbso_flush.argtypes = [vp]
    l.pbso_compute_transfer.argtypes = [vp, C.c_int, dp, C.c_int64]
    l.pbso_compute_transfer_batch.argtypes = [vp, C.c_int, dp, C.c_int, dp, C.c_int]
    l.pbso_object_n_maps.argtypes = [vp, C.c_int]
    l.pbso_listeners_enable.argtypes = [vp, C.c_int]
    l.pbso_mix_listeners.argtypes = [vp, C.c_int, dp, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    l.pbso_set_use_transfer.argtypes = [vp, C.c_int, C.c_int, C.c_int64]
    l.pbso_get_latest_transfer.argtypes = [vp, C.c_int, dp]
    l.pbso_step.argtypes = [vp, C.c_int]
    l.pbso_step_into.argtypes = [vp, C.c_int, vp]
    l.pbso_sync.argtypes = [vp]
    l.pbso_read_audio.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
    l.pbso_read_emitted.argtypes = [vp, C.POINTER(C.c_ubyte), C.c_size_t]
    l.pbso_read_qnorm.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]
    l.pbso_read_state.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    l.pbso_write_state.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    l.pbso_audio_device_ptr.restype = vp
    l.pbso_audio_device_ptr.argtypes = [vp]
    l.pbso_pa_convert.argtypes = [C.POINTER(C.c_float), C.c_ulong, C.POINTER(C.c_float)]
    l.pbso_pa_convert.restype = None
    l.pbso_get_info.argtypes = [vp, C.POINTER(EngineInfo)]
    l.pbso_modes_read.argtypes = [C.c_char_p, ip, ip, C.POINTER(dp), C.POINTER(dp)]
    l.pbso_num_modes_audible.argtypes = [dp, C.c_int, C.c_double, C.c_double]
    l.pbso_material_read.argtypes = [C.c_char_p, dp]
    l.pbso_obj_read.argtypes = [C.c_char_p, ip, ip, C.POINTER(dp), C.POINTER(ip), C.POINTER(dp)]
    l.pbso_read_census.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t]
    l.pbso_free.argtypes = [vp]
    l.pbso_free.restype = None
    l.pbso_mix_objects.argtypes = [vp, vp]
    fp = C.POINTER(C.c_float)
    l.pbso_scene_mix_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    l.pbso_scene_mix_set.argtypes = [vp, fp, fp]
    l.pbso_scene_mix.argtypes = [vp, vp]
    l.pbso_read_scene_mix.argtypes = [vp, fp, C.c_size_t]
    l.pbso_scene_mix_reset.argtypes = [vp]
    l.pbso_group_scene_mix_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    l.pbso_group_scene_mix_set.argtypes = [vp, fp, fp]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_scene_mix_schedule"):
        l.pbso_scene_mix_set_at.argtypes = [vp, C.c_int64, fp, fp]
        l.pbso_scene_mix_schedule.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), fp, fp]
        l.pbso_scene_mix_clear_schedule.argtypes = [vp]
        l.pbso_scene_mix_info.argtypes = [vp, C.POINTER(C.c_int64)]
        l.pbso_group_scene_mix_set_at.argtypes = [vp, C.c_int64, fp, fp]
        l.pbso_group_scene_mix_schedule.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), fp, fp]
        l.pbso_group_scene_mix_clear_schedule.argtypes = [vp]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_scene_fir"):
        # (as the tracks above: an older build picked with PBSO_LIB has no filter mix)
        l.pbso_scene_fir_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        l.pbso_scene_fir_set.argtypes = [vp, fp, ip]
        l.pbso_scene_fir.argtypes = [vp, vp]
        l.pbso_read_scene_fir.argtypes = [vp, fp, C.c_size_t]
        l.pbso_scene_fir_reset.argtypes = [vp]
        l.pbso_scene_fir_info.argtypes = [vp, C.POINTER(C.c_int64)]
        l.pbso_group_scene_fir_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        l.pbso_group_scene_fir_set.argtypes = [vp, fp, ip]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_scene_fir_delay_enable"):
        l.pbso_scene_fir_delay_enable.argtypes = [vp, C.c_int, C.c_int]
        l.pbso_scene_fir_set_delay.argtypes = [vp, fp]
        l.pbso_scene_fir_delay_info.argtypes = [vp, C.POINTER(C.c_int64)]
        l.pbso_group_scene_fir_delay_enable.argtypes = [vp, C.c_int, C.c_int]
        l.pbso_group_scene_fir_set_delay.argtypes = [vp, fp]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_scene_fir_schedule"):
        tp = C.POINTER(C.c_int64)
        l.pbso_scene_fir_set_at.argtypes = [vp, C.c_int64, fp, ip]
        l.pbso_scene_fir_schedule.argtypes = [vp, C.c_int, tp, fp, ip]
        l.pbso_scene_fir_set_delay_at.argtypes = [vp, C.c_int64, fp]
        l.pbso_scene_fir_delay_schedule.argtypes = [vp, C.c_int, tp, fp]
        l.pbso_scene_fir_clear_schedule.argtypes = [vp]
        l.pbso_scene_fir_schedule_info.argtypes = [vp, tp]
        l.pbso_group_scene_fir_set_at.argtypes = [vp, C.c_int64, fp, ip]
        l.pbso_group_scene_fir_schedule.argtypes = [vp, C.c_int, tp, fp, ip]
        l.pbso_group_scene_fir_set_delay_at.argtypes = [vp, C.c_int64, fp]
        l.pbso_group_scene_fir_delay_schedule.argtypes = [vp, C.c_int, tp, fp]
        l.pbso_group_scene_fir_clear_schedule.argtypes = [vp]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_scene_fir_bank_create"):
        tp = C.POINTER(C.c_int64)
        l.pbso_scene_fir_bank_create.argtypes = [vp, C.c_int, fp]
        l.pbso_scene_fir_bank_info.argtypes = [vp, tp]
        l.pbso_scene_fir_set_bank.argtypes = [vp, C.c_int, ip, fp, ip]
        l.pbso_scene_fir_set_bank_at.argtypes = [vp, C.c_int64, C.c_int, ip, fp, ip]
        l.pbso_scene_fir_bank_schedule.argtypes = [vp, C.c_int, tp, C.c_int, ip, fp, ip]
        l.pbso_group_scene_fir_bank_create.argtypes = [vp, C.c_int, fp]
        l.pbso_group_scene_fir_set_bank.argtypes = [vp, C.c_int, ip, fp, ip]
        l.pbso_group_scene_fir_set_bank_at.argtypes = [vp, C.c_int64, C.c_int, ip, fp, ip]
        l.pbso_group_scene_fir_bank_schedule.argtypes = [vp, C.c_int, tp, C.c_int, ip, fp, ip]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_scene_reverb"):
        l.pbso_scene_reverb_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        l.pbso_scene_reverb_set.argtypes = [vp, fp]
        l.pbso_scene_reverb.argtypes = [vp, vp, vp, vp]
        l.pbso_read_scene_reverb.argtypes = [vp, fp, C.c_size_t]
        l.pbso_scene_reverb_reset.argtypes = [vp]
        l.pbso_scene_reverb_info.argtypes = [vp, C.POINTER(C.c_int64)]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_master"):
        l.pbso_master_enable.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
        l.pbso_master_set_gain.argtypes = [vp, C.c_float]
        l.pbso_master.argtypes = [vp, vp, vp]
        l.pbso_read_master.argtypes = [vp, fp, C.c_size_t]
        l.pbso_read_master_pcm16.argtypes = [vp, C.POINTER(C.c_int16), C.c_size_t]
        l.pbso_read_master_meters.argtypes = [vp, C.POINTER(MasterMeter), C.c_size_t]
        l.pbso_master_window.argtypes = [vp, fp, C.c_size_t]
        l.pbso_master_reset.argtypes = [vp]
        l.pbso_master_info.argtypes = [vp, C.POINTER(C.c_int64)]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_resample"):
        l.pbso_resample_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
        l.pbso_resample.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        l.pbso_resample_max_out.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
        l.pbso_read_resample.argtypes = [vp, fp, C.c_size_t]
        l.pbso_read_resample_pcm16.argtypes = [vp, C.POINTER(C.c_int16), C.c_size_t]
        l.pbso_read_resample_meters.argtypes = [vp, C.POINTER(ResampleMeter), C.c_size_t]
        l.pbso_resample_taps.argtypes = [vp, fp, C.c_size_t]
        l.pbso_resample_reset.argtypes = [vp]
        l.pbso_resample_info.argtypes = [vp, C.POINTER(C.c_int64)]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_eq"):
        l.pbso_eq_enable.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        l.pbso_eq_set.argtypes = [vp, dp]
        l.pbso_eq.argtypes = [vp, vp, vp]
        l.pbso_read_eq.argtypes = [vp, fp, C.c_size_t]
        l.pbso_eq_tables.argtypes = [vp, dp, C.c_size_t]
        l.pbso_eq_reset.argtypes = [vp]
        l.pbso_eq_info.argtypes = [vp, C.POINTER(C.c_int64)]
        l.pbso_eq_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, dp]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_eq_schedule"):
        l.pbso_eq_set_at.argtypes = [vp, C.c_int64, dp]
        l.pbso_eq_schedule.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), dp]
        l.pbso_eq_clear_schedule.argtypes = [vp]
        l.pbso_eq_schedule_info.argtypes = [vp, C.POINTER(C.c_int64)]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_loudness"):
        l.pbso_loudness_enable.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int]
        l.pbso_loudness.argtypes = [vp, vp]
        l.pbso_read_loudness_blocks.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(LoudnessBlock)]
        l.pbso_loudness_report.argtypes = [vp, C.POINTER(LoudnessSummary)]
        l.pbso_loudness_taps.argtypes = [vp, fp, C.c_size_t]
        l.pbso_loudness_reset.argtypes = [vp]
        l.pbso_loudness_info.argtypes = [vp, C.POINTER(C.c_int64)]
        l.pbso_loudness_design.argtypes = [C.c_double, dp]
        l.pbso_loudness_report_from_blocks.argtypes = [C.POINTER(LoudnessBlock), C.c_int64, C.c_int, dp, C.c_int, C.POINTER(LoudnessSummary)]
    if "PBSO_LIB" not in os.environ or hasattr(l, "pbso_set_material"):
        l.pbso_set_material.argtypes = [vp, C.c_int, ip, C.POINTER(Material), C.c_int]
        l.pbso_get_material.argtypes = [vp, C.c_int, C.POINTER(Material)]
        l.pbso_material_stats.argtypes = [vp, C.POINTER(C.c_int64)]
        l.pbso_group_set_material.argtypes = [vp, C.c_int, ip, C.POINTER(Material), C.c_int]
    l.pbso_step_to_host.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    l.pbso_host_wait.argtypes = [vp]
    l.pbso_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    l.pbso_host_free.argtypes = [vp]
    l.pbso_host_free.restype = None
    l.pbso_compute_transfer_path.argtypes = [vp, C.c_int, ip, dp, C.POINTER(C.c_int64), C.POINTER(C.c_ubyte)]
    l.pbso_read_audio_rows.argtypes = [vp, ip, C.c_int, C.POINTER(C.c_float)]
    l.pbso_shard_by_modes.argtypes = [ip, C.c_int, C.c_int, ip]
    l.pbso_group_unique_id.argtypes = [vp]
    l.pbso_group_create.argtypes = [C.POINTER(GroupDesc), C.POINTER(vp)]
    l.pbso_group_destroy.argtypes = [vp]
    l.pbso_group_destroy.restype = None
    l.pbso_group_last_error.argtypes = [vp]
    l.pbso_group_last_error.restype = C.c_char_p
    l.pbso_group_plan.argtypes = [vp, ip, C.c_int]
    l.pbso_group_rank_span.argtypes = [vp, C.c_int, ip, ip]
    l.pbso_group_owner.argtypes = [vp, C.c_int, ip, ip]
    l.pbso_group_add_object.argtypes = [vp, C.c_int, C.POINTER(ObjectDesc)]
    l.pbso_group_finalize.argtypes = [vp]
    l.pbso_group_engine.argtypes = [vp, C.c_int]
    l.pbso_group_engine.restype = vp
    l.pbso_group_enqueue_force.argtypes = [vp, C.c_int, C.POINTER(ForceMsg), C.c_int64]
    l.pbso_group_step.argtypes = [vp, C.c_int]
    l.pbso_group_gather.argtypes = [vp, C.c_int]
    l.pbso_group_sync.argtypes = [vp]
    l.pbso_group_result_device_ptr.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    l.pbso_group_result_device_ptr.restype = vp
    l.pbso_group_read_result.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    _lib = l
    return l


EQ_BLOCK = 64                                         # PBSO_EQ_BLOCK: part of the EQ bus's definition
EQ_LOWPASS, EQ_HIGHPASS, EQ_PEAK, EQ_LOWSHELF, EQ_HIGHSHELF = 0, 1, 2, 3, 4
EQ_KINDS = {"lowpass": EQ_LOWPASS, "highpass": EQ_HIGHPASS, "peak": EQ_PEAK, "lowshelf": EQ_LOWSHELF, "highshelf": EQ_HIGHSHELF}


def eq_design(kind, rate, f0, q=0.7071067811865476, gain_db=0.0):
    """pbso_eq_design: one Audio-EQ-Cookbook section, b0 b1 b2 a1 a2 (a0 = 1) as five doubles; kind: a name of EQ_KINDS or its number"""
    out = (C.c_double * 5)()
    rc = lib().pbso_eq_design(EQ_KINDS[kind] if isinstance(kind, str) else int(kind), rate, f0, q, gain_db, out)
    if rc != 0:
        raise ValueError(f"pbso_eq_design({kind!r}, {rate}, {f0}, {q}, {gain_db}): status {rc}")
    return [float(v) for v in out]


LOUDNESS_BLOCK = [("energy", "<f8"), ("true_peak", "<f4"), ("sample_peak", "<f4")]      # pbso_loudness_block as a numpy dtype


def loudness_design(rate):
    """pbso_loudness_design: the two K-weighting sections of BS.1770 at `rate`, [2][5] = b0 b1 b2 a1 a2 as doubles"""
    out = (C.c_double * 10)()
    rc = lib().pbso_loudness_design(rate, out)
    if rc != 0:
        raise ValueError(f"pbso_loudness_design({rate}): status {rc}")
    return [[float(out[5 * s + k]) for k in range(5)] for s in range(2)]


def loudness_summary(r):
    """a LoudnessSummary as a dict"""
    return {k: getattr(r, k) for k, _ in LoudnessSummary._fields_}


def loudness_report_from_blocks(blocks, hop, weight=None):
    """pbso_loudness_report_from_blocks: the gating of BS.1770 / Tech 3341 over blocks [n_blocks][C] (a structured array of
    LOUDNESS_BLOCK, or anything with the fields energy, true_peak, sample_peak); hop = rate / 10; weight [C] or None (all 1)"""
    import numpy as np
    b = np.ascontiguousarray(blocks, dtype=np.dtype(LOUDNESS_BLOCK))
    if b.ndim != 2:
        raise ValueError("blocks must be [n_blocks][n_channels]")
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    if w is not None and w.size != b.shape[1]:
        raise ValueError("weight must be [n_channels]")
    out = LoudnessSummary()
    rc = lib().pbso_loudness_report_from_blocks(b.ctypes.data_as(C.POINTER(LoudnessBlock)), b.shape[0], b.shape[1],
                                                None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)), int(hop), C.byref(out))
    if rc != 0:
        raise ValueError(f"pbso_loudness_report_from_blocks: status {rc}")
    return loudness_summary(out)
