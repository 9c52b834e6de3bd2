"""ctypes binding of the product library stvo-pl_amd/libstvo_hip.so (include/stvo_hip.h).

Plumbing for tests and bench only.  There is NO fallback: if the library is missing or no gfx950
device is visible, loading / context creation raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .ctypes_types import Cam, GridWindow, MatchParams, OptParams, PoseResult, POSE_RESULT_DTYPE, RectCalib, RectCamera, TrajParams, \
    TRAJ_RECORD_DTYPE, TRAJ_STATE_DTYPE, TRACK_DTYPE, KF_HEADER_DTYPE

PKG_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # stvo-pl_amd/
LIB_PATH = os.environ.get("STVO_LIB") or os.path.join(PKG_DIR, "libstvo_hip.so")   # STVO_LIB: A/B runs of two builds (developer)

EXPORTS = ["stvo_backend_name", "stvo_abi_version", "stvo_error_string", "stvo_ctx_last_error", "stvo_ctx_create",
           "stvo_ctx_destroy", "stvo_ctx_set_stream", "stvo_ctx_synchronize", "stvo_ctx_set_overlap", "stvo_match_nnr_mutual",
           "stvo_match_grid_points", "stvo_match_grid_lines", "stvo_normal_eq", "stvo_optimize_pose",
           "stvo_track_batched_dev", "stvo_match_nnr_mutual_batched_dev", "stvo_optimize_pose_batched_dev",
           "stvo_time_stage_dev", "stvo_valu_peak_probe", "stvo_last_reverse_counts", "stvo_last_reverse_plan", "stvo_ctx_set_kernel_timing", "stvo_ctx_get_kernel_timing", "stvo_seq_create", "stvo_seq_destroy", "stvo_seq_enable_fetch", "stvo_seq_fetch_matches", "stvo_seq_fetch_inliers", "stvo_seq_strides",
           "stvo_seq_push", "stvo_seq_upload", "stvo_seq_step_dev", "stvo_seq_read", "stvo_seq_create_multi", "stvo_seq_set_slots",
           "stvo_seq_set_stage_timing", "stvo_seq_get_stage_timing", "stvo_seq_last_schedule", "stvo_seq_set_motion_model", "stvo_seq_debug_grid", "stvo_seq_debug_point_route", "stvo_seq_debug_stereo", "stvo_orb_create", "stvo_orb_destroy",
           "stvo_orb_set_pattern", "stvo_orb_get_pattern", "stvo_orb_detect", "stvo_orb_detect_dev", "stvo_orb_detect_levels",
           "stvo_orb_detect_levels_dev", "stvo_orb_set_fast_threshold", "stvo_orb_set_score_type", "stvo_seq_upload_dev", "stvo_lbd_create", "stvo_lbd_destroy",
           "stvo_lbd_compute", "stvo_lbd_compute_dev", "stvo_debug_reparse_env", "stvo_lsd_create", "stvo_lsd_destroy", "stvo_lsd_detect",
           "stvo_lsd_detect_dev", "stvo_lsd_segments", "stvo_lsd_counts", "stvo_lsd_geometry", "stvo_lsd_scaled_image", "stvo_fld_create", "stvo_fld_destroy", "stvo_fld_detect",
           "stvo_fld_detect_dev", "stvo_fld_counts", "stvo_fld_segments", "stvo_fld_edges", "stvo_keylines_xy_dev", "stvo_rectify_compute",
           "stvo_rectify_create", "stvo_rectify_create_from_maps", "stvo_rectify_destroy", "stvo_rectify_camera", "stvo_rectify_images",
           "stvo_rectify_images_dev", "stvo_orb_set_fast_thresholds", "stvo_orb_set_fast_thresholds_dev", "stvo_fast_adapt_dev",
           "stvo_seq_adapt_fast_dev", "stvo_traj_init_dev", "stvo_traj_update_dev", "stvo_seq_set_trajectory", "stvo_seq_read_trajectory",
           "stvo_seq_trajectory_state_dev", "stvo_seq_read_trajectory_state", "stvo_seq_control_next_step", "stvo_seq_restart_fast_dev",
           "stvo_seq_set_tracks", "stvo_seq_read_tracks", "stvo_seq_tracks_dev", "stvo_seq_keyframe_headers", "stvo_seq_read_keyframe",
           "stvo_color_to_gray", "stvo_color_to_gray_dev", "stvo_rectify_color_images", "stvo_rectify_color_images_dev",
           "stvo_rectify_color_to_gray_dev", "stvo_seq_snapshot_layout", "stvo_seq_snapshot_info", "stvo_seq_export_streams_dev",
           "stvo_seq_export_streams", "stvo_seq_import_streams_dev", "stvo_seq_import_streams", "stvo_orb_set_descriptor",
           "stvo_orb_pattern", "stvo_orb_set_image_sizes", "stvo_seq_restart_cameras", "stvo_rectify_bank_create",
           "stvo_rectify_bank_destroy", "stvo_rectify_bank_camera", "stvo_rectify_bank_assign", "stvo_rectify_bank_images_dev",
           "stvo_rectify_bank_color_to_gray_dev", "stvo_lsd_set_image_sizes", "stvo_lbd_set_image_sizes", "stvo_fld_set_image_sizes",
           "stvo_lsd_set_table_route", "stvo_lsd_search_route"]

SEQ_NSTAGE = 5  # include/stvo_hip.h: STVO_SEQ_NSTAGE
SEQ_STAGE_NAMES = ("stereo_points_stage", "grid_scan", "hamming_knn2", "reverse_check", "pose")
# include/stvo_hip.h: STVO_SCHED_* (pose_kernel: 0 none, 1 latency, 2 batch; pose_waves: 2 / 4 for the batch kernel; the rest 0 / 1)
SEQ_SCHEDULE_FIELDS = ("pose_kernel", "pose_waves", "fused_cells", "cells_ahead", "lines_ahead", "gate", "mid_fork", "line_fused")
SCHED_POSE_LATENCY, SCHED_POSE_BATCH = 1, 2
STREAM_RUN, STREAM_RESTART, STREAM_PARK = 0, 1, 2  # include/stvo_hip.h: STVO_STREAM_* (Sequences.control_next_step)
SNAP_MOTION, SNAP_TRAJ, SNAP_TRAJ_KF, SNAP_TRACKS, SNAP_KF_SETS = 1, 2, 4, 8, 16  # include/stvo_hip.h: STVO_SNAP_*
# the sections of a snapshot blob in the order they are cut (csrc/stream_snapshot.h): name, dtype of a row, "K" / "M" rows or one record
_SET_SECTIONS = (("rc", ("<f4", (4,)), "K"), ("desc", ("u1", (32,)), "K"), ("spl", ("<f8", (2,)), "M"), ("epl", ("<f8", (2,)), "M"),
                 ("sP", ("<f8", (3,)), "M"), ("eP", ("<f8", (3,)), "M"), ("le", ("<f8", (3,)), "M"), ("s2l", "<f8", "M"), ("s2lm", "<f8", "M"),
                 ("ldesc", ("u1", (32,)), "M"))
SNAP_SECTIONS = (("header", None, 1),) + _SET_SECTIONS + (("motion", ("<f8", (16,)), 1), ("traj", TRAJ_STATE_DTYPE, 1),
                                                           ("tracks_p", TRACK_DTYPE, "K"), ("tracks_l", TRACK_DTYPE, "M")) + \
    tuple(("kf_" + n, d, r) for n, d, r in _SET_SECTIONS)
_CAM_DTYPE = np.dtype([(n, "<f8") for n in ("fx", "fy", "cx", "cy", "b")])
SNAP_HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("bytes", "<i8"), ("K", "<i4"), ("M", "<i4"), ("flags", "<i4"), ("n", "<i4"),
                              ("nl", "<i4"), ("reserved", "<i4"), ("kf", KF_HEADER_DTYPE), ("cam", _CAM_DTYPE), ("cols", "<i4"), ("rows", "<i4"),
                              ("mp", "u1", (C.sizeof(MatchParams),)), ("op", "u1", (C.sizeof(OptParams),))])
assert SNAP_HEADER_DTYPE.itemsize == 256
SNAP_MAGIC, SNAP_VERSION = 0x53567453, 1

u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")


class Matched(C.Structure):
    _fields_ = [("np", C.c_int32), ("P", C.c_void_p), ("pl_obs", C.c_void_p), ("sigma2p", C.c_void_p),
                ("inlier_p", C.c_void_p), ("nl", C.c_int32), ("sP", C.c_void_p), ("eP", C.c_void_p),
                ("le_obs", C.c_void_p), ("spl", C.c_void_p), ("epl", C.c_void_p), ("sigma2l", C.c_void_p),
                ("inlier_l", C.c_void_p)]


class TrackBatchDev(C.Structure):
    _fields_ = [("B", C.c_int32), ("max_pts", C.c_int32), ("max_lines", C.c_int32), ("reserved", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("n_prev_pts", "prev_pdesc", "prev_P", "prev_sigma2p", "n_curr_pts",
                                          "curr_pdesc", "curr_pl", "n_prev_lines", "prev_ldesc", "prev_sP", "prev_eP",
                                          "prev_spl", "prev_epl", "prev_sigma2l", "n_curr_lines", "curr_ldesc",
                                          "curr_le", "init_T", "m12_pts", "m12_lines", "inlier_pts", "inlier_lines",
                                          "results")]


class FrameFeatures(C.Structure):
    _fields_ = [("stride_kp", C.c_int32), ("stride_kl", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("n_kp_l", "n_kp_r", "kp_l", "oct_l", "desc_l", "kp_r", "desc_r", "n_kl_l", "n_kl_r",
                                          "kl_l", "oct_ll", "ldesc_l", "kl_r", "ldesc_r")]


class StvoError(RuntimeError):
    pass


class SnapshotLayout(C.Structure):  # stvo_snapshot_layout
    _fields_ = [("bytes", C.c_int64)] + [("off_" + n, C.c_int64) for n, _, _ in SNAP_SECTIONS] + \
               [("K", C.c_int32), ("M", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


def snapshot_layout(K, M, flags):
    """{"bytes", "K", "M", "flags", "off": {section name: offset or -1}} of a snapshot blob cut at capacities K, M with the feature
    flags SNAP_* (stvo_seq_snapshot_layout: host only, no device)."""
    lay = SnapshotLayout()
    rc = load().stvo_seq_snapshot_layout(K, M, flags, C.byref(lay))
    if rc != 0:
        raise StvoError(f"stvo_seq_snapshot_layout({K}, {M}, {flags}): {rc}")
    return dict(bytes=lay.bytes, K=lay.K, M=lay.M, flags=lay.flags, off={n: getattr(lay, "off_" + n) for n, _, _ in SNAP_SECTIONS})


def snapshot_views(blob):
    """Numpy views into ONE blob (uint8 [bytes]): "header" (a SNAP_HEADER_DTYPE record) and, for every section that is cut, its valid
    rows — [n] / [nl] rows of the stereo set and the track state, [kf.n_pts] / [kf.n_lines] of the key-frame set, one record of the seed
    and of the trajectory state.  "live" is a bool mask of the bytes these views cover (every other byte of a blob is zero)."""
    blob = np.ascontiguousarray(blob, np.uint8).reshape(-1)
    h = blob[:256].view(SNAP_HEADER_DTYPE)[0]
    lay = snapshot_layout(int(h["K"]), int(h["M"]), int(h["flags"]))
    assert lay["bytes"] == int(h["bytes"]) == blob.size, (lay["bytes"], int(h["bytes"]), blob.size)
    out = dict(header=h, layout=lay)
    live = np.zeros(blob.size, bool)
    live[:256] = True
    for name, dt, rows in SNAP_SECTIONS[1:]:
        off = lay["off"][name]
        if off < 0:
            continue
        dt = np.dtype(dt)
        kf = name.startswith("kf_")
        cnt = 1 if rows == 1 else int((h["kf"]["n_pts"] if kf else h["n"]) if rows == "K" else (h["kf"]["n_lines"] if kf else h["nl"]))
        out[name] = blob[off:off + cnt * dt.itemsize].view(dt.base).reshape((cnt,) + dt.shape)
        live[off:off + cnt * dt.itemsize] = True
    out["live"] = live
    return out


class FastAdapt(C.Structure):  # stvo_fast_adapt
    _fields_ = [("min_th", C.c_int32), ("max_th", C.c_int32), ("inc_th", C.c_int32), ("feat_th", C.c_int32), ("err_th", C.c_float)]


def fast_adapt_params(preset="kitti", **overrides):
    """Config::fastMinTh / fastMaxTh / fastIncTh / fastFeatTh / fastErrTh as the reference's YAML files ship them: "kitti" =
    config_kitti.yaml (7, 30, 5, 50, 0.5), "euroc" = every other file (5, 50, 5, 50, 0.5).  overrides: min_th, max_th, inc_th, feat_th, err_th."""
    base = {"kitti": dict(min_th=7, max_th=30), "euroc": dict(min_th=5, max_th=50)}[preset]
    base.update(inc_th=5, feat_th=50, err_th=0.5)
    unknown = set(overrides) - set(base)
    if unknown:
        raise TypeError(f"fast_adapt_params: unknown field(s) {sorted(unknown)}")
    base.update(overrides)
    return FastAdapt(**base)


def fast_adapt_dev(ctx, results, prm, th):
    """updateFrame's adaptive FAST rule for len(th) streams, on the context's stream (stvo_fast_adapt_dev): results = a torch uint8
    device tensor holding that many stvo_pose_result records (POSE_RESULT_DTYPE), th = a torch int32 device tensor, moved in place."""
    B = th.numel()
    if str(th.dtype) != "torch.int32" or not th.is_cuda or not th.is_contiguous() or not results.is_contiguous() or \
            results.numel() * results.element_size() < B * POSE_RESULT_DTYPE.itemsize:
        raise ValueError("fast_adapt_dev: th must be a contiguous int32 tensor and results hold one record per threshold")
    ctx._chk(ctx.lib.stvo_fast_adapt_dev(ctx.h, B, results.data_ptr(), C.byref(prm), th.data_ptr()))


def traj_params(preset="kitti", keyframes=True, **overrides):
    """Config::minEntropyRatio / maxKFTDist / maxKFRDist as the reference ships them (config_euroc.yaml: 0.85, 5.0, 15.0; the files that
    do not name them take the same values from src/config.cpp, so every preset agrees).  keyframes=False: the pose is composed and never
    reset.  overrides: min_entropy_ratio, max_kf_t_dist, max_kf_r_dist."""
    if preset not in ("kitti", "euroc", "default"):
        raise KeyError(preset)
    base = dict(min_entropy_ratio=0.85, max_kf_t_dist=5.0, max_kf_r_dist=15.0)
    unknown = set(overrides) - set(base)
    if unknown:
        raise TypeError(f"traj_params: unknown field(s) {sorted(unknown)}")
    base.update(overrides)
    return TrajParams(keyframes=1 if keyframes else 0, reserved=0, **base)


def _dev_bytes(t, n, itemsize, what):
    if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < n * itemsize:
        raise ValueError(f"{what}: a contiguous device tensor of at least {n} records of {itemsize} bytes is needed")


def traj_init_dev(ctx, state):
    """The state `initialize` leaves, for every record of `state` (a torch uint8 device tensor of B * TRAJ_STATE_DTYPE.itemsize bytes),
    on the context's stream (stvo_traj_init_dev)."""
    B = state.numel() * state.element_size() // TRAJ_STATE_DTYPE.itemsize
    _dev_bytes(state, max(B, 1), TRAJ_STATE_DTYPE.itemsize, "traj_init_dev")
    ctx._chk(ctx.lib.stvo_traj_init_dev(ctx.h, B, state.data_ptr()))


def traj_update_dev(ctx, results, prm, state, records=None):
    """One trajectory / key-frame update for B streams on the context's stream (stvo_traj_update_dev): results = torch uint8 device
    tensor of B stvo_pose_result records, state = B TRAJ_STATE_DTYPE records (in / out), records = None or B TRAJ_RECORD_DTYPE records."""
    B = state.numel() * state.element_size() // TRAJ_STATE_DTYPE.itemsize
    _dev_bytes(state, max(B, 1), TRAJ_STATE_DTYPE.itemsize, "traj_update_dev: state")
    _dev_bytes(results, B, POSE_RESULT_DTYPE.itemsize, "traj_update_dev: results")
    if records is not None:
        _dev_bytes(records, B, TRAJ_RECORD_DTYPE.itemsize, "traj_update_dev: records")
    ctx._chk(ctx.lib.stvo_traj_update_dev(ctx.h, B, results.data_ptr(), C.byref(prm), state.data_ptr(),
                                          records.data_ptr() if records is not None else None))


def build(force=False):
    """Compile libstvo_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "clean"])
    subprocess.check_call(["make", "-s", "-C", PKG_DIR, "-j4"])
    return LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StvoError(f"{LIB_PATH} is missing: run `make -C stvo-pl_amd` (python __graft_entry__.py). "
                        "The product has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64; if this library pulled in
    # /opt/rocm's copy first, torch would later find "No HIP GPUs".  Import torch first when it exists so
    # both resolve to the same already-loaded runtime (torch is only plumbing: HBM buffers + streams).
    try:
        import torch  # noqa: F401
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.stvo_backend_name.restype = C.c_char_p
    L.stvo_error_string.restype = C.c_char_p
    L.stvo_error_string.argtypes = [C.c_int]
    L.stvo_ctx_last_error.restype = C.c_char_p
    L.stvo_ctx_last_error.argtypes = [C.c_void_p]
    L.stvo_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.stvo_ctx_destroy.argtypes = [C.c_void_p]
    L.stvo_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.stvo_ctx_synchronize.argtypes = [C.c_void_p]
    L.stvo_ctx_set_overlap.argtypes = [C.c_void_p, C.c_int]
    L.stvo_match_nnr_mutual.argtypes = [C.c_void_p, u8p, C.c_int, u8p, C.c_int, C.c_float, C.c_int, i32p,
                                        C.POINTER(C.c_int32)]
    L.stvo_match_grid_points.argtypes = [C.c_void_p, i32p, u8p, C.c_int, i32p, i32p, u8p, C.c_int,
                                         C.POINTER(GridWindow), C.c_double, C.c_int, i32p, C.POINTER(C.c_int32)]
    L.stvo_match_grid_lines.argtypes = [C.c_void_p, i32p, u8p, C.c_int, i32p, i32p, u8p, C.c_int, f64p,
                                        C.POINTER(GridWindow), C.c_double, C.c_double, C.c_int, i32p,
                                        C.POINTER(C.c_int32)]
    L.stvo_normal_eq.argtypes = [C.c_void_p, f64p, C.POINTER(Cam), C.POINTER(OptParams), C.POINTER(Matched), C.c_int,
                                 f64p, f64p, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.stvo_optimize_pose.argtypes = [C.c_void_p, f64p, C.POINTER(Cam), C.POINTER(OptParams), C.POINTER(Matched),
                                     C.POINTER(PoseResult)]
    L.stvo_track_batched_dev.argtypes = [C.c_void_p, C.POINTER(TrackBatchDev), C.POINTER(Cam), C.POINTER(OptParams),
                                         C.c_float, C.c_float, C.c_int]
    L.stvo_match_nnr_mutual_batched_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    L.stvo_optimize_pose_batched_dev.argtypes = [C.c_void_p, C.POINTER(TrackBatchDev), C.POINTER(Cam),
                                                 C.POINTER(OptParams)]
    L.stvo_time_stage_dev.argtypes = [C.c_void_p, C.POINTER(TrackBatchDev), C.POINTER(Cam), C.POINTER(OptParams),
                                      C.c_float, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.stvo_valu_peak_probe.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.stvo_seq_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Cam),
                                  C.POINTER(MatchParams), C.POINTER(OptParams), C.POINTER(C.c_void_p)]
    L.stvo_seq_create_multi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p, i32p, C.c_void_p, C.POINTER(MatchParams),
                                        C.POINTER(OptParams), C.POINTER(C.c_void_p)]
    L.stvo_seq_set_slots.argtypes = [C.c_void_p, C.c_int]
    L.stvo_seq_set_stage_timing.argtypes = [C.c_void_p, C.c_int]
    L.stvo_seq_set_motion_model.argtypes = [C.c_void_p, C.c_int]
    L.stvo_seq_get_stage_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    L.stvo_seq_debug_grid.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, i32p, C.c_int32, i32p, i32p, i32p, C.c_int32,
                                      C.POINTER(C.c_int32)]
    L.stvo_seq_debug_point_route.argtypes = [C.c_void_p, i32p]
    L.stvo_orb_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(OrbParams), C.POINTER(C.c_void_p)]
    L.stvo_orb_destroy.argtypes = [C.c_void_p]
    i8p = np.ctypeslib.ndpointer(np.int8, flags="C_CONTIGUOUS")
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    L.stvo_seq_debug_stereo.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.POINTER(C.c_int32), f32p, u8p, C.c_int32, C.POINTER(C.c_int32),
                                        f64p, f64p, f64p, f64p, f64p, f64p, f64p, u8p]
    L.stvo_orb_set_pattern.argtypes = [C.c_void_p, i8p]
    L.stvo_orb_get_pattern.argtypes = [C.c_void_p, i8p]
    L.stvo_orb_detect.argtypes = [C.c_void_p, u8p, f32p, f32p, f32p, u8p, i32p]
    L.stvo_orb_detect_dev.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    L.stvo_orb_set_fast_threshold.argtypes = [C.c_void_p, C.c_int]
    L.stvo_orb_set_score_type.argtypes = [C.c_void_p, C.c_int]
    L.stvo_orb_set_descriptor.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.stvo_orb_pattern.argtypes = [C.c_int, C.c_int, C.c_void_p, i8p, C.POINTER(C.c_int32)]
    L.stvo_orb_set_fast_thresholds.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_orb_set_fast_thresholds_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_orb_set_image_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_fast_adapt_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(FastAdapt), C.c_void_p]
    L.stvo_seq_adapt_fast_dev.argtypes = [C.c_void_p, C.POINTER(FastAdapt), C.c_void_p]
    L.stvo_traj_init_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.stvo_traj_update_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(TrajParams), C.c_void_p, C.c_void_p]
    L.stvo_seq_set_trajectory.argtypes = [C.c_void_p, C.POINTER(TrajParams), C.c_int]
    L.stvo_seq_read_trajectory.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
    L.stvo_seq_trajectory_state_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.stvo_seq_read_trajectory_state.argtypes = [C.c_void_p, C.c_void_p]
    L.stvo_seq_control_next_step.argtypes = [C.c_void_p, C.c_void_p]
    L.stvo_seq_set_tracks.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.stvo_seq_read_tracks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.stvo_seq_tracks_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.stvo_seq_keyframe_headers.argtypes = [C.c_void_p, C.c_void_p]
    L.stvo_seq_read_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, f32p, u8p, C.c_int32, f64p, f64p, f64p, f64p, f64p,
                                         f64p, f64p, u8p]
    L.stvo_seq_restart_fast_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_seq_restart_cameras.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.stvo_seq_snapshot_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(SnapshotLayout)]
    L.stvo_seq_snapshot_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.stvo_seq_export_streams_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.stvo_seq_export_streams.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.stvo_seq_import_streams_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    L.stvo_seq_import_streams.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    L.stvo_orb_detect_levels.argtypes = [C.c_void_p, u8p, f32p, f32p, f32p, i32p, u8p, i32p, i32p]
    L.stvo_orb_detect_levels_dev.argtypes = [C.c_void_p] + [C.c_void_p] * 8
    L.stvo_lbd_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.stvo_lbd_destroy.argtypes = [C.c_void_p]
    L.stvo_lbd_compute.argtypes = [C.c_void_p, u8p, C.c_void_p, i32p, u8p, C.c_void_p]
    L.stvo_lbd_compute_dev.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    L.stvo_lsd_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LsdParams), C.POINTER(C.c_void_p)]
    L.stvo_lsd_destroy.argtypes = [C.c_void_p]
    L.stvo_lsd_detect.argtypes = [C.c_void_p, u8p, C.c_void_p, C.c_void_p, i32p]
    L.stvo_lsd_detect_dev.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    L.stvo_lsd_segments.argtypes = [C.c_void_p, u8p, f32p, C.c_int, i32p]
    L.stvo_lsd_counts.argtypes = [C.c_void_p, i32p, i32p]
    L.stvo_lsd_geometry.argtypes = [C.POINTER(LsdParams), C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                    C.POINTER(C.c_int32), i32p]
    L.stvo_lsd_scaled_image.argtypes = [C.c_void_p, u8p, u8p]
    L.stvo_lsd_debug.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.stvo_lsd_set_image_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_lsd_set_table_route.argtypes = [C.c_void_p, C.c_int]
    L.stvo_lsd_search_route.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.stvo_lbd_set_image_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_fld_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FldParams), C.POINTER(C.c_void_p)]
    L.stvo_fld_destroy.argtypes = [C.c_void_p]
    L.stvo_fld_detect.argtypes = [C.c_void_p, u8p, C.c_void_p, C.c_void_p, i32p]
    L.stvo_fld_detect_dev.argtypes = [C.c_void_p] + [C.c_void_p] * 4
    L.stvo_fld_counts.argtypes = [C.c_void_p, i32p]
    L.stvo_fld_segments.argtypes = [C.c_void_p, u8p, f32p, C.c_int, i32p]
    L.stvo_fld_edges.argtypes = [C.c_void_p, u8p, u8p]
    L.stvo_fld_set_image_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.stvo_keylines_xy_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.stvo_seq_destroy.argtypes = [C.c_void_p]
    L.stvo_rectify_compute.argtypes = [C.POINTER(RectCalib), C.POINTER(RectCamera), C.c_void_p, C.c_void_p]
    L.stvo_rectify_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(RectCalib), C.POINTER(C.c_void_p)]
    L.stvo_rectify_create_from_maps.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.stvo_rectify_destroy.argtypes = [C.c_void_p]
    L.stvo_rectify_camera.argtypes = [C.c_void_p, C.POINTER(RectCamera)]
    L.stvo_rectify_images.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.stvo_rectify_images_dev.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    L.stvo_color_to_gray.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    L.stvo_color_to_gray_dev.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3
    L.stvo_rectify_color_images.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.stvo_rectify_color_images_dev.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.stvo_rectify_color_to_gray_dev.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 6
    L.stvo_rectify_bank_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    L.stvo_rectify_bank_destroy.argtypes = [C.c_void_p]
    L.stvo_rectify_bank_camera.argtypes = [C.c_void_p, C.c_int, C.POINTER(RectCamera)]
    L.stvo_rectify_bank_assign.argtypes = [C.c_void_p, C.c_void_p]
    L.stvo_rectify_bank_images_dev.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.stvo_rectify_bank_color_to_gray_dev.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 6
    L.stvo_seq_push.argtypes = [C.c_void_p, C.POINTER(FrameFeatures), C.c_void_p, i32p]
    L.stvo_seq_upload.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameFeatures)]
    L.stvo_seq_upload_dev.argtypes = [C.c_void_p, C.c_int, C.POINTER(FrameFeatures)]
    L.stvo_seq_step_dev.argtypes = [C.c_void_p, C.c_int]
    L.stvo_seq_read.argtypes = [C.c_void_p, C.c_void_p, i32p]
    pp32 = C.POINTER(C.POINTER(C.c_int32))
    L.stvo_seq_enable_fetch.argtypes = [C.c_void_p, C.c_int]
    L.stvo_seq_fetch_matches.argtypes = [C.c_void_p, pp32, pp32, pp32, pp32]
    L.stvo_seq_fetch_inliers.argtypes = [C.c_void_p, pp32, pp32]
    L.stvo_seq_strides.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.stvo_seq_last_schedule.argtypes = [C.c_void_p, i32p]
    L.stvo_last_reverse_counts.argtypes = [C.c_void_p, C.c_int, i32p]
    L.stvo_last_reverse_plan.argtypes = [C.c_void_p, C.c_int, i32p]
    L.stvo_ctx_set_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    L.stvo_ctx_get_kernel_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One stvo_ctx.  Raises StvoError on any non-zero status."""

    def __init__(self, device_id=0, max_rows=4096, max_batch=64):
        self.lib = load()
        self.h = C.c_void_p()
        rc = self.lib.stvo_ctx_create(device_id, max_rows, max_batch, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise StvoError(f"stvo_ctx_create failed: {self.lib.stvo_error_string(rc).decode()} ({rc})")

    def close(self):
        if self.h:
            self.lib.stvo_ctx_destroy(self.h)
            self.h = None

    def _chk(self, rc):
        if rc != 0:
            raise StvoError(f"{self.lib.stvo_error_string(rc).decode()} ({rc}): "
                            f"{self.lib.stvo_ctx_last_error(self.h).decode()}")

    def set_stream(self, stream_handle):
        self._chk(self.lib.stvo_ctx_set_stream(self.h, C.c_void_p(stream_handle)))

    def synchronize(self):
        self._chk(self.lib.stvo_ctx_synchronize(self.h))

    def set_overlap(self, enable):
        self._chk(self.lib.stvo_ctx_set_overlap(self.h, 1 if enable else 0))

    # ---- host-buffer seams ----
    def match(self, d1, d2, nnr, mutual=1):
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        m12 = np.empty(max(len(d1), 1), np.int32)
        n = C.c_int32()
        self._chk(self.lib.stvo_match_nnr_mutual(self.h, d1 if len(d1) else np.zeros((1, 32), np.uint8), len(d1),
                                                 d2 if len(d2) else np.zeros((1, 32), np.uint8), len(d2), nnr, mutual,
                                                 m12, C.byref(n)))
        return m12[:len(d1)], n.value

    def match_grid_points(self, cell_xy1, d1, start, items, d2, w, ratio, mutual=1):
        n1 = len(d1)
        m12 = np.empty(max(n1, 1), np.int32)
        n = C.c_int32()
        gw = GridWindow(*w)
        items_ = np.ascontiguousarray(items, np.int32) if len(items) else np.zeros(1, np.int32)
        d1_ = d1 if n1 else np.zeros((1, 32), np.uint8)
        d2_ = d2 if len(d2) else np.zeros((1, 32), np.uint8)
        xy = np.ascontiguousarray(cell_xy1, np.int32).reshape(-1) if n1 else np.zeros(2, np.int32)
        self._chk(self.lib.stvo_match_grid_points(self.h, xy, d1_, n1, np.ascontiguousarray(start, np.int32), items_,
                                                  d2_, len(d2), C.byref(gw), ratio, mutual, m12, C.byref(n)))
        return m12[:n1], n.value

    def match_grid_lines(self, cell_xy1, d1, start, items, d2, dir2, w, ratio, line_sim_th, mutual=1):
        n1 = len(d1)
        m12 = np.empty(max(n1, 1), np.int32)
        n = C.c_int32()
        gw = GridWindow(*w)
        items_ = np.ascontiguousarray(items, np.int32) if len(items) else np.zeros(1, np.int32)
        d1_ = d1 if n1 else np.zeros((1, 32), np.uint8)
        d2_ = d2 if len(d2) else np.zeros((1, 32), np.uint8)
        xy = np.ascontiguousarray(cell_xy1, np.int32).reshape(-1) if n1 else np.zeros(4, np.int32)
        dr = np.ascontiguousarray(dir2, np.float64).reshape(-1) if len(d2) else np.zeros(2)
        self._chk(self.lib.stvo_match_grid_lines(self.h, xy, d1_, n1, np.ascontiguousarray(start, np.int32), items_,
                                                 d2_, len(d2), dr, C.byref(gw), ratio, line_sim_th, mutual, m12,
                                                 C.byref(n)))
        return m12[:n1], n.value

    @staticmethod
    def _matched(rec):
        keep = {k: np.ascontiguousarray(rec[k], np.float64)
                for k in ("P", "pl_obs", "sigma2p", "sP", "eP", "le_obs", "spl", "epl", "sigma2l")}
        keep["inlier_p"] = np.ascontiguousarray(rec["inlier_p"], np.int32).copy()
        keep["inlier_l"] = np.ascontiguousarray(rec["inlier_l"], np.int32).copy()
        m = Matched(len(keep["sigma2p"]), _ptr(keep["P"]), _ptr(keep["pl_obs"]), _ptr(keep["sigma2p"]),
                    _ptr(keep["inlier_p"]), len(keep["sigma2l"]), _ptr(keep["sP"]), _ptr(keep["eP"]),
                    _ptr(keep["le_obs"]), _ptr(keep["spl"]), _ptr(keep["epl"]), _ptr(keep["sigma2l"]),
                    _ptr(keep["inlier_l"]))
        return m, keep

    def normal_eq(self, T, cam, params, rec, robust=0):
        m, keep = self._matched(rec)
        H = np.empty(36)
        g = np.empty(6)
        e = C.c_double()
        n = C.c_int32()
        camc = Cam.from_dict(cam)
        self._chk(self.lib.stvo_normal_eq(self.h, np.ascontiguousarray(T, np.float64).reshape(-1), C.byref(camc),
                                          C.byref(params), C.byref(m), robust, H, g, C.byref(e), C.byref(n)))
        return H.reshape(6, 6), g, e.value, n.value

    def optimize_pose(self, init_T, cam, params, rec):
        m, keep = self._matched(rec)
        res = PoseResult()
        camc = Cam.from_dict(cam)
        self._chk(self.lib.stvo_optimize_pose(self.h, np.ascontiguousarray(init_T, np.float64).reshape(-1),
                                              C.byref(camc), C.byref(params), C.byref(m), C.byref(res)))
        d = res.as_dict()
        d["inlier_p"] = keep["inlier_p"]
        d["inlier_l"] = keep["inlier_l"]
        return d

    def valu_peak(self):
        v = C.c_double()
        self._chk(self.lib.stvo_valu_peak_probe(self.h, C.byref(v)))
        return v.value

    def set_kernel_timing(self, enable):
        self._chk(self.lib.stvo_ctx_set_kernel_timing(self.h, 1 if enable else 0))

    def get_kernel_timing(self):
        f = C.c_float(); r = C.c_float(); n = C.c_int32()
        self._chk(self.lib.stvo_ctx_get_kernel_timing(self.h, C.byref(f), C.byref(r), C.byref(n)))
        return f.value, r.value, n.value

    def last_reverse_counts(self, B):
        out = np.empty(B, np.int32)
        self._chk(self.lib.stvo_last_reverse_counts(self.h, B, out))
        return out

    def last_reverse_plan(self, B):
        """[5][B]: claimed, light, heavy columns, |S|, tau of the last mutual match's reverse check (matrix-core path)."""
        out = np.empty((5, B), np.int32)
        self._chk(self.lib.stvo_last_reverse_plan(self.h, B, out))
        return out

    # ---- batched device-resident path ----
    def track_batched(self, batch, cam, params, nnr_p, nnr_l, mutual=1):
        camc = Cam.from_dict(cam)
        self._chk(self.lib.stvo_track_batched_dev(self.h, C.byref(batch.struct), C.byref(camc), C.byref(params), nnr_p,
                                                  nnr_l, mutual))

    def optimize_pose_batched(self, batch, cam, params):
        camc = Cam.from_dict(cam)
        self._chk(self.lib.stvo_optimize_pose_batched_dev(self.h, C.byref(batch.struct), C.byref(camc), C.byref(params)))

    def time_stage(self, batch, cam, params, nnr, stage, iters):
        camc = Cam.from_dict(cam)
        ms = C.c_float()
        self._chk(self.lib.stvo_time_stage_dev(self.h, C.byref(batch.struct), C.byref(camc), C.byref(params), nnr,
                                               stage, iters, C.byref(ms)))
        return ms.value


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("fast_threshold", C.c_int32), ("edge_threshold", C.c_int32), ("nlevels", C.c_int32),
                ("scale_factor", C.c_double)]


class Orb:
    """The ORB point front-end for B images of one size (stvo_orb_*)."""

    def __init__(self, ctx, B, cols, rows, max_keypoints=2048, nfeatures=2000, fast_threshold=20, edge_threshold=19, nlevels=1,
                 scale_factor=1.2, score=1, wta_k=2, patch_size=31):
        """score: Config::orbScore() with OpenCV's values — 1 FAST_SCORE (the default), 0 HARRIS_SCORE.  wta_k, patch_size:
        Config::orbWtaK() (2, 3, 4) and Config::orbPatchSize() (2 .. 63; other than 31 it needs edge_threshold >= ceil(patch_size // 2 *
        sqrt 2)): stvo_orb_set_descriptor."""
        self.ctx, self.B, self.cols, self.rows, self.K = ctx, B, cols, rows, max_keypoints
        self.h = C.c_void_p()
        prm = OrbParams(nfeatures, fast_threshold, edge_threshold, nlevels, scale_factor)
        ctx._chk(ctx.lib.stvo_orb_create(ctx.h, B, cols, rows, max_keypoints, C.byref(prm), C.byref(self.h)))
        try:
            if score != 1:
                self.set_score_type(score)
            if (wta_k, patch_size) != (2, 31):
                self.set_descriptor(wta_k, patch_size)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.h:
            self.ctx.lib.stvo_orb_destroy(self.h)
            self.h = None

    def pattern(self):
        """The effective point list of the setting in force as [256, 4] (x0, y0, x1, y1): 512 / 384 / 512 points for wta_k 2 / 3 / 4,
        zero beyond them."""
        p = np.zeros(1024, np.int8)
        self.ctx._chk(self.ctx.lib.stvo_orb_get_pattern(self.h, p))
        return p.reshape(256, 4)

    def set_descriptor(self, wta_k, patch_size):
        self.ctx._chk(self.ctx.lib.stvo_orb_set_descriptor(self.h, wta_k, patch_size))

    def set_pattern(self, pattern):
        self.ctx._chk(self.ctx.lib.stvo_orb_set_pattern(self.h, np.ascontiguousarray(pattern, np.int8).reshape(-1)))

    def set_fast_threshold(self, th):
        self.ctx._chk(self.ctx.lib.stvo_orb_set_fast_threshold(self.h, th))

    def set_fast_thresholds(self, th):
        """One FAST threshold per image, image i takes th[i % len(th)] (len(th) divides B).  A numpy array / sequence: host form, the
        detector keeps its own device copy (stvo_orb_set_fast_thresholds).  A torch int32 device tensor: device form, the tensor is
        read by every later detection when it runs and must outlive them (stvo_orb_set_fast_thresholds_dev).  None: back to the scalar."""
        lib = self.ctx.lib
        if th is None:
            self.ctx._chk(lib.stvo_orb_set_fast_thresholds_dev(self.h, None, 0))
            self._th_keep = None
        elif hasattr(th, "data_ptr"):
            if str(th.dtype) != "torch.int32" or not th.is_cuda or not th.is_contiguous():
                raise ValueError("Orb.set_fast_thresholds: the device form takes a contiguous int32 device tensor")
            self.ctx._chk(lib.stvo_orb_set_fast_thresholds_dev(self.h, th.data_ptr(), th.numel()))
            self._th_keep = th
        else:
            a = np.ascontiguousarray(th, np.int32).reshape(-1)
            self.ctx._chk(lib.stvo_orb_set_fast_thresholds(self.h, _ptr(a), a.size))
            self._th_keep = None

    def set_image_sizes(self, sizes):
        """One image size per image: sizes [n][2] = (cols, rows), image i takes sizes[i % n] (n divides B) and occupies the top-left of
        its slot of the size given at creation, whose row pitch it keeps (stvo_orb_set_image_sizes).  None: every image fills its slot."""
        if sizes is None:
            self.ctx._chk(self.ctx.lib.stvo_orb_set_image_sizes(self.h, None, 0))
            return
        a = np.ascontiguousarray(sizes, np.int32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("Orb.set_image_sizes: sizes is [n][2] = (cols, rows)")
        self.ctx._chk(self.ctx.lib.stvo_orb_set_image_sizes(self.h, _ptr(a), a.shape[0]))

    def set_score_type(self, score):
        self.ctx._chk(self.ctx.lib.stvo_orb_set_score_type(self.h, score))

    def detect(self, images):
        """images: uint8 [B, rows, cols] -> list of B dicts(kp [n,2] float32, response, angle, desc [n,32])."""
        images = np.ascontiguousarray(images, np.uint8).reshape(self.B, self.rows, self.cols)
        kp = np.zeros((self.B, self.K, 2), np.float32); resp = np.zeros((self.B, self.K), np.float32)
        ang = np.zeros((self.B, self.K), np.float32); desc = np.zeros((self.B, self.K, 32), np.uint8); n = np.zeros(self.B, np.int32)
        octv = np.zeros((self.B, self.K), np.int32); ntot = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_orb_detect_levels(self.h, images.reshape(-1), kp.reshape(-1), resp.reshape(-1), ang.reshape(-1),
                                                          octv.reshape(-1), desc.reshape(-1), n, ntot))
        return [dict(kp=kp[b, :n[b]].copy(), response=resp[b, :n[b]].copy(), angle=ang[b, :n[b]].copy(), desc=desc[b, :n[b]].copy(),
                     octave=octv[b, :n[b]].copy(), n_total=int(ntot[b])) for b in range(self.B)]

    def detect_dev(self, img, kp, resp, ang, desc, n, octave=None, n_total=None):
        """Device buffers (integers = device addresses): images in, key-points / descriptors out, on the context's stream."""
        self.ctx._chk(self.ctx.lib.stvo_orb_detect_levels_dev(self.h, img, kp, resp, ang, octave, desc, n, n_total))


def orb_pattern(wta_k, patch_size, pool=None):
    """stvo_orb_pattern (host only, no context): the effective point list [n_points, 2] int8 of a descriptor setting.  pool: the
    1024-byte pattern of patch size 31 (None: the seeded stand-in).  Raises StvoError with the library's verdict."""
    lib = load()
    out, n = np.zeros(1024, np.int8), C.c_int32(0)
    p = None if pool is None else np.ascontiguousarray(pool, np.int8).reshape(-1)
    if p is not None and p.size != 1024:
        raise ValueError("orb_pattern: the pool holds 1024 bytes")
    rc = lib.stvo_orb_pattern(wta_k, patch_size, None if p is None else p.ctypes.data, out, C.byref(n))
    if rc != 0:
        raise StvoError(f"{lib.stvo_error_string(rc).decode()} ({rc}): stvo_orb_pattern({wta_k}, {patch_size})")
    assert not out[2 * n.value:].any()
    return out[:2 * n.value].reshape(-1, 2).copy()


KEYLINE_DTYPE = np.dtype([("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"), ("angle", "<f4"), ("num_pixels", "<i4")])  # stvo_keyline


class LsdParams(C.Structure):  # stvo_lsd_params
    _fields_ = [("refine", C.c_int32), ("n_bins", C.c_int32), ("scale", C.c_double), ("sigma_scale", C.c_double), ("quant", C.c_double),
                ("ang_th", C.c_double), ("log_eps", C.c_double), ("density_th", C.c_double), ("min_length", C.c_double),
                ("nfeatures", C.c_int32), ("flags", C.c_int32)]


LSD_SIZES_ANY_RADIUS = 1  # STVO_LSD_SIZES_ANY_RADIUS
LSD_TABLE_ONE_WAVE, LSD_TABLE_BY_BATCH = 0, 1  # STVO_LSD_TABLE_*: what a size table does to the route of the search (Lsd.set_table_route)
LSD_SEARCH_ONE_WAVE, LSD_SEARCH_ONE_WAVE_PLAIN, LSD_SEARCH_MANY_WAVES = 0, 1, 2  # STVO_LSD_SEARCH_*: the search kernel (Lsd.search_route)


def lsd_params(min_length=0.0, nfeatures=300, refine=0, scale=1.2, sigma_scale=0.6, quant=2.0, ang_th=22.5, n_bins=1024,
               sizes_any_radius=False):
    """src/config.cpp:104-112 (every shipped yaml has the same values).  sizes_any_radius: Lsd.set_image_sizes also takes the detector
    at a scale other than 1 with a blur radius other than 3 (STVO_LSD_SIZES_ANY_RADIUS; nothing else changes)."""
    return LsdParams(refine, n_bins, scale, sigma_scale, quant, ang_th, 1.0, 0.6, min_length, nfeatures,
                     LSD_SIZES_ANY_RADIUS if sizes_any_radius else 0)


LSD_MAX_RADIUS = 15  # STVO_LSD_MAX_RADIUS


def lsd_geometry(prm, cols, rows):
    """stvo_lsd_geometry (host only, no context): what a parameter set means for cols x rows images — the scaled size, sigma and radius
    of the blur and the 1 + 2 radius integer weights of one pass; StvoError where stvo_lsd_create would refuse."""
    lib = load()
    w, h, radius, sigma = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
    k = np.zeros(1 + 2 * LSD_MAX_RADIUS, np.int32)
    rc = lib.stvo_lsd_geometry(C.byref(prm), cols, rows, C.byref(w), C.byref(h), C.byref(sigma), C.byref(radius), k)
    if rc != 0:
        raise StvoError(f"{lib.stvo_error_string(rc).decode()} ({rc}): stvo_lsd_geometry")
    return dict(cols=w.value, rows=h.value, sigma=sigma.value, radius=radius.value, weights=k[:1 + 2 * radius.value].copy())


class Lsd:
    """The LSD key-line detector for B images of one size (stvo_lsd_*)."""

    def __init__(self, ctx, B, cols, rows, prm, max_keylines=512):
        self.ctx, self.B, self.cols, self.rows, self.M = ctx, B, cols, rows, max_keylines
        self.h = C.c_void_p()
        ctx._chk(ctx.lib.stvo_lsd_create(ctx.h, B, cols, rows, max_keylines, C.byref(prm), C.byref(self.h)))
        self.geometry = lsd_geometry(prm, cols, rows)

    def close(self):
        if self.h:
            self.ctx.lib.stvo_lsd_destroy(self.h)
            self.h = None

    def detect(self, images):
        """images uint8 [B, rows, cols] -> list of B (key-lines as KEYLINE_DTYPE records, responses float32)."""
        images = np.ascontiguousarray(images, np.uint8).reshape(self.B, self.rows, self.cols)
        rec = np.zeros((self.B, self.M), KEYLINE_DTYPE)
        resp = np.zeros((self.B, self.M), np.float32)
        n = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_lsd_detect(self.h, images.reshape(-1), rec.ctypes.data_as(C.c_void_p), resp.ctypes.data_as(C.c_void_p), n))
        return [(rec[b, :n[b]].copy(), resp[b, :n[b]].copy()) for b in range(self.B)]

    def detect_dev(self, img_ptr, lines_ptr, resp_ptr, n_ptr):
        """Device pointers (uint8 [B, rows, cols]; stvo_keyline [B, M]; float32 [B, M] or None; int32 [B]); asynchronous."""
        self.ctx._chk(self.ctx.lib.stvo_lsd_detect_dev(self.h, img_ptr, lines_ptr, resp_ptr, n_ptr))

    def counts(self):
        """(segments found, segments longer than min_length) per image of the last detection, before the top-N / capacity cut."""
        ns = np.zeros(self.B, np.int32); npass = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_lsd_counts(self.h, ns, npass))
        return ns, npass

    def segments(self, images, cap=8192):
        """The raw segments of the detector core: list of B float32 [n_b, 4] (detection order)."""
        images = np.ascontiguousarray(images, np.uint8).reshape(self.B, self.rows, self.cols)
        seg = np.zeros((self.B, cap, 4), np.float32)
        n = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_lsd_segments(self.h, images.reshape(-1), seg.reshape(-1), cap, n))
        return [seg[b, :min(n[b], cap)].copy() for b in range(self.B)], n

    def debug(self, enable):
        """Developer aid (stvo_lsd_debug): switches the probe instances of the search kernels on or off for the calls that follow, and
        returns what the last detection under them left for image 0 as float64 [8192, 8] — per segment of a one-wave kernel the row
        (cx, cy, Ixx, Iyy, Ixy, theta, l_min, l_max) in the scaled image, counter rows at the end (tools/lsd_probe.py reads them);
        zeros before the first such detection.  StvoError for lsd_refine = 1, which has no probe instance."""
        rows = np.zeros((8192, 8), np.float64)
        self.ctx._chk(self.ctx.lib.stvo_lsd_debug(self.h, 1 if enable else 0, _ptr(rows)))
        return rows

    def set_image_sizes(self, sizes, min_lengths=None):
        """One image size per image: sizes [n][2] = (cols, rows), image i takes sizes[i % n] (n divides B) and occupies the top-left of
        its slot of the size given at creation, whose row pitch it keeps; min_lengths [n] (None: the detector's min_length for all) is
        the minimum line length per entry (stvo_lsd_set_image_sizes).  sizes None: every image fills its slot."""
        if sizes is None:
            self.ctx._chk(self.ctx.lib.stvo_lsd_set_image_sizes(self.h, None, None, 0))
            return
        a = np.ascontiguousarray(sizes, np.int32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("Lsd.set_image_sizes: sizes is [n][2] = (cols, rows)")
        ml = None if min_lengths is None else np.ascontiguousarray(min_lengths, np.float64).reshape(-1)
        if ml is not None and ml.size != a.shape[0]:
            raise ValueError("Lsd.set_image_sizes: one minimum length per entry of sizes")
        self.ctx._chk(self.ctx.lib.stvo_lsd_set_image_sizes(self.h, _ptr(a), None if ml is None else _ptr(ml), a.shape[0]))

    def set_table_route(self, route):
        """What a size table does to the route of the search from the next detection on (stvo_lsd_set_table_route, host only):
        LSD_TABLE_ONE_WAVE (the default) — one wavefront per image under a table; LSD_TABLE_BY_BATCH — the route the detector takes with
        no table, the many-wave search for a detector of up to 128 images.  The results are the same bytes.  It survives
        set_image_sizes; StvoError for another value, and the route in force stays."""
        self.ctx._chk(self.ctx.lib.stvo_lsd_set_table_route(self.h, int(route)))

    def search_route(self):
        """The search kernel the next detection launches (stvo_lsd_search_route, host only): LSD_SEARCH_ONE_WAVE, LSD_SEARCH_ONE_WAVE_PLAIN
        (lsd_refine 1, STVO_LSD_GROW=0) or LSD_SEARCH_MANY_WAVES."""
        r = C.c_int32(-1)
        self.ctx._chk(self.ctx.lib.stvo_lsd_search_route(self.h, C.byref(r)))
        return r.value

    def scaled_image(self, images):
        """The image the detector core sees (blurred and resized; the input itself at scale 1): uint8 [B, scaled rows, scaled cols]
        (under set_image_sizes: the top-left scaled size of every image, at the slot's scaled pitch)."""
        images = np.ascontiguousarray(images, np.uint8).reshape(self.B, self.rows, self.cols)
        out = np.zeros((self.B, self.geometry["rows"], self.geometry["cols"]), np.uint8)
        self.ctx._chk(self.ctx.lib.stvo_lsd_scaled_image(self.h, images.reshape(-1), out.reshape(-1)))
        return out


class FldParams(C.Structure):  # stvo_fld_params
    _fields_ = [("length_threshold", C.c_int32), ("distance_threshold", C.c_float), ("canny_th1", C.c_double), ("canny_th2", C.c_double),
                ("canny_aperture_size", C.c_int32), ("do_merge", C.c_int32), ("nfeatures", C.c_int32), ("reserved", C.c_int32)]


def fld_params(length_threshold, nfeatures=300, distance_threshold=1.414213562, canny_th1=50.0, canny_th2=50.0, canny_aperture_size=3,
               do_merge=0):
    """createFastLineDetector(length_threshold) with every other parameter at its default (stereoFrame.cpp:257);
    length_threshold = int(min_line_length x min(cols, rows)), nfeatures = Config::lsdNFeatures()."""
    return FldParams(int(length_threshold), distance_threshold, canny_th1, canny_th2, canny_aperture_size, do_merge, nfeatures, 0)


class Fld:
    """The FLD key-line detector for B images of one size, or one size per image under set_image_sizes (stvo_fld_*)."""

    def __init__(self, ctx, B, cols, rows, prm, max_keylines=512):
        self.ctx, self.B, self.cols, self.rows, self.M = ctx, B, cols, rows, max_keylines
        self.h = C.c_void_p()
        ctx._chk(ctx.lib.stvo_fld_create(ctx.h, B, cols, rows, max_keylines, C.byref(prm), C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.lib.stvo_fld_destroy(self.h)
            self.h = None

    def _images(self, images):
        return np.ascontiguousarray(images, np.uint8).reshape(self.B, self.rows, self.cols)

    def detect(self, images):
        """images uint8 [B, rows, cols] -> list of B (key-lines as KEYLINE_DTYPE records, responses float32)."""
        images = self._images(images)
        rec = np.zeros((self.B, self.M), KEYLINE_DTYPE)
        resp = np.zeros((self.B, self.M), np.float32)
        n = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_fld_detect(self.h, images.reshape(-1), rec.ctypes.data_as(C.c_void_p), resp.ctypes.data_as(C.c_void_p), n))
        return [(rec[b, :n[b]].copy(), resp[b, :n[b]].copy()) for b in range(self.B)]

    def set_image_sizes(self, sizes, length_thresholds=None):
        """One image size per image: sizes [n][2] = (cols, rows), image i takes sizes[i % n] (n divides B) and occupies the top-left of
        its slot of the size given at creation, whose row pitch it keeps; length_thresholds [n] (None: the detector's for all) is the
        length threshold per entry (stvo_fld_set_image_sizes).  sizes None: every image fills its slot."""
        if sizes is None:
            self.ctx._chk(self.ctx.lib.stvo_fld_set_image_sizes(self.h, None, None, 0))
            return
        a = np.ascontiguousarray(sizes, np.int32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("Fld.set_image_sizes: sizes is [n][2] = (cols, rows)")
        lt = None if length_thresholds is None else np.ascontiguousarray(length_thresholds, np.int32).reshape(-1)
        if lt is not None and lt.size != a.shape[0]:
            raise ValueError("Fld.set_image_sizes: one length threshold per entry of sizes")
        self.ctx._chk(self.ctx.lib.stvo_fld_set_image_sizes(self.h, _ptr(a), None if lt is None else _ptr(lt), a.shape[0]))

    def detect_dev(self, img_ptr, lines_ptr, resp_ptr, n_ptr):
        """Device pointers (uint8 [B, rows, cols]; stvo_keyline [B, M]; float32 [B, M] or None; int32 [B]); asynchronous."""
        self.ctx._chk(self.ctx.lib.stvo_fld_detect_dev(self.h, img_ptr, lines_ptr, resp_ptr, n_ptr))

    def counts(self):
        """Segments found per image by the last detection, before the top-N / capacity cut."""
        ns = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_fld_counts(self.h, ns))
        return ns

    def segments(self, images, cap=8192):
        """The raw segments of FastLineDetector::detect: (list of B float32 [n_b, 4] in detection order, counts [B])."""
        images = self._images(images)
        seg = np.zeros((self.B, cap, 4), np.float32)
        n = np.zeros(self.B, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_fld_segments(self.h, images.reshape(-1), seg.reshape(-1), cap, n))
        return [seg[b, :min(n[b], cap)].copy() for b in range(self.B)], n

    def edges(self, images):
        """The edge map the chains are walked on: uint8 [B, rows, cols] 0 / 255 (under set_image_sizes: every image's own edge map
        top-left in its slot, 0 around it)."""
        images = self._images(images)
        out = np.zeros((self.B, self.rows, self.cols), np.uint8)
        self.ctx._chk(self.ctx.lib.stvo_fld_edges(self.h, images.reshape(-1), out.reshape(-1)))
        return out


class Lbd:
    """The LBD line descriptor for B images of one size with up to M key-lines each (stvo_lbd_*)."""

    def __init__(self, ctx, B, cols, rows, max_keylines=512):
        self.ctx, self.B, self.cols, self.rows, self.M = ctx, B, cols, rows, max_keylines
        self.h = C.c_void_p()
        ctx._chk(ctx.lib.stvo_lbd_create(ctx.h, B, cols, rows, max_keylines, C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.lib.stvo_lbd_destroy(self.h)
            self.h = None

    def set_image_sizes(self, sizes):
        """One image size per image, as Lsd.set_image_sizes (stvo_lbd_set_image_sizes).  None: every image fills its slot."""
        if sizes is None:
            self.ctx._chk(self.ctx.lib.stvo_lbd_set_image_sizes(self.h, None, 0))
            return
        a = np.ascontiguousarray(sizes, np.int32)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("Lbd.set_image_sizes: sizes is [n][2] = (cols, rows)")
        self.ctx._chk(self.ctx.lib.stvo_lbd_set_image_sizes(self.h, _ptr(a), a.shape[0]))

    def compute_dev(self, img_ptr, lines_ptr, n_ptr, desc_ptr, desc_float_ptr=None):
        """Device pointers (uint8 [B, rows, cols]; stvo_keyline [B, M]; int32 [B]; uint8 [B, M, 32]; float32 [B, M, 72] or None)."""
        self.ctx._chk(self.ctx.lib.stvo_lbd_compute_dev(self.h, img_ptr, lines_ptr, n_ptr, desc_ptr, desc_float_ptr))

    def compute(self, images, lines, num_pixels, want_float=False):
        """images uint8 [B, rows, cols]; lines: list of B arrays [n_b, 5] (sx, sy, ex, ey, angle); num_pixels: list of B int arrays.
        -> list of B uint8 [n_b, 32] (and float32 [n_b, 72])."""
        images = np.ascontiguousarray(images, np.uint8).reshape(self.B, self.rows, self.cols)
        rec = np.zeros((self.B, self.M), KEYLINE_DTYPE)
        n = np.zeros(self.B, np.int32)
        for b in range(self.B):
            ln = np.asarray(lines[b], np.float32).reshape(-1, 5)
            n[b] = len(ln)
            for k, f in enumerate(("sx", "sy", "ex", "ey", "angle")):
                rec[f][b, :len(ln)] = ln[:, k]
            rec["num_pixels"][b, :len(ln)] = num_pixels[b]
        desc = np.zeros((self.B, self.M, 32), np.uint8)
        df = np.zeros((self.B, self.M, 72), np.float32) if want_float else None
        self.ctx._chk(self.ctx.lib.stvo_lbd_compute(self.h, images.reshape(-1), rec.ctypes.data_as(C.c_void_p), n, desc.reshape(-1),
                                                    df.ctypes.data_as(C.c_void_p) if want_float else None))
        out = [desc[b, :n[b]].copy() for b in range(self.B)]
        return (out, [df[b, :n[b]].copy() for b in range(self.B)]) if want_float else out


class Sequences:
    """B independent stereo sequences on the device-resident per-frame pipeline (stvo_seq_*)."""

    def __init__(self, ctx, B, max_kp, max_kl, cam, mp, op):
        """cam: one camera dict for all B sequences, or a list of B dicts (stvo_seq_create_multi)."""
        self.ctx, self.B = ctx, B
        self.h = C.c_void_p()
        if isinstance(cam, dict):
            camc = Cam.from_dict(cam)
            ctx._chk(ctx.lib.stvo_seq_create(ctx.h, B, max_kp, max_kl, cam["width"], cam["height"], C.byref(camc), C.byref(mp),
                                             C.byref(op), C.byref(self.h)))
        else:
            assert len(cam) == B
            cams = (Cam * B)(*[Cam.from_dict(c) for c in cam])
            cols = np.array([c["width"] for c in cam], np.int32)
            rows = np.array([c["height"] for c in cam], np.int32)
            ctx._chk(ctx.lib.stvo_seq_create_multi(ctx.h, B, max_kp, max_kl, cols, rows, C.cast(cams, C.c_void_p), C.byref(mp),
                                                   C.byref(op), C.byref(self.h)))

    def set_slots(self, n):
        self.ctx._chk(self.ctx.lib.stvo_seq_set_slots(self.h, n))

    def set_motion_model(self, on=True):
        """Config::useMotionModel(): the initial DT of a frame pair = the increment committed for the previous pair if it was good."""
        self.ctx._chk(self.ctx.lib.stvo_seq_set_motion_model(self.h, 1 if on else 0))

    def set_stage_timing(self, on=True):
        """True / 1: an event pair around every stage; 2: "light" — only the grid matcher, the forward scan and the pose kernel (the
        step otherwise as untimed); False: off."""
        self.ctx._chk(self.ctx.lib.stvo_seq_set_stage_timing(self.h, int(on)))

    def get_stage_timing(self):
        """({stage name: average ms per step}, number of steps measured) since the last call."""
        ms = (C.c_float * SEQ_NSTAGE)()
        n = C.c_int32()
        self.ctx._chk(self.ctx.lib.stvo_seq_get_stage_timing(self.h, ms, C.byref(n)))
        return {k: float(ms[i]) for i, k in enumerate(SEQ_STAGE_NAMES)}, n.value

    def debug_grid(self, b, lines):
        """Device-built grid of sequence b after the last step: (cell_start[3073], cell_items, cells_left, cand_off, cand)."""
        K, M = self.strides()
        cap_items = (M * 116) if lines else K
        cap_cand = (M * M) if lines else (K * 256)
        start = np.empty(64 * 48 + 1, np.int32); items = np.empty(cap_items, np.int32)
        cells = np.empty((M if lines else K) * (4 if lines else 2), np.int32)
        off = np.empty((M if lines else K) + 1, np.int32); cand = np.empty(cap_cand, np.int32)
        n = C.c_int32()
        self.ctx._chk(self.ctx.lib.stvo_seq_debug_grid(self.h, b, 1 if lines else 0, start, items, cap_items, cells, off, cand, cap_cand,
                                                      C.byref(n)))
        nl = n.value
        return (start, items[:start[-1]].copy(), cells[:nl * (4 if lines else 2)].reshape(nl, -1).copy(), off[:nl + 1].copy(),
                cand[:off[nl]].copy())

    def debug_point_route(self):
        """int32 [B, 2] = (misfit, ovf) of the stereo point matcher of the last step (stvo_seq_debug_point_route); copies only.  Call it
        before debug_grid, whose kernels clear ovf."""
        out = np.zeros((self.B, 2), np.int32)
        self.ctx._chk(self.ctx.lib.stvo_seq_debug_point_route(self.h, out.reshape(-1)))
        return out

    def debug_stereo(self, b):
        """The stereo sets the last step built from its frame for sequence b (stvo_seq_debug_stereo): dict of n, rc [n, 4] float32
        {u, v, disparity, level}, desc [n, 32]; nl, spl, epl [nl, 2], sP, eP, le [nl, 3], s2l, s2lm [nl], ldesc [nl, 32]."""
        K, M = self.strides()
        rc = np.empty((K, 4), np.float32); desc = np.empty((K, 32), np.uint8); ldesc = np.empty((M, 32), np.uint8)
        spl, epl = np.empty((M, 2)), np.empty((M, 2))
        sP, eP, le = np.empty((M, 3)), np.empty((M, 3)), np.empty((M, 3))
        s2l, s2lm = np.empty(M), np.empty(M)
        n, nl = C.c_int32(), C.c_int32()
        self.ctx._chk(self.ctx.lib.stvo_seq_debug_stereo(self.h, b, K, C.byref(n), rc.reshape(-1), desc.reshape(-1), M, C.byref(nl),
                                                        spl.reshape(-1), epl.reshape(-1), sP.reshape(-1), eP.reshape(-1), le.reshape(-1),
                                                        s2l, s2lm, ldesc.reshape(-1)))
        n, nl = n.value, nl.value
        return dict(n=n, rc=rc[:n].copy(), desc=desc[:n].copy(), nl=nl, spl=spl[:nl].copy(), epl=epl[:nl].copy(), sP=sP[:nl].copy(),
                    eP=eP[:nl].copy(), le=le[:nl].copy(), s2l=s2l[:nl].copy(), s2lm=s2lm[:nl].copy(), ldesc=ldesc[:nl].copy())

    def close(self):
        if self.h:
            self.ctx.lib.stvo_seq_destroy(self.h)
            self.h = None

    def _pack(self, frames):
        B = self.B
        assert len(frames) == B
        skp = max(max(len(f["kp_l"]), len(f["kp_r"])) for f in frames) or 1
        skl = max(max(len(f["kl_l"]), len(f["kl_r"])) for f in frames) or 1
        a = dict(n_kp_l=np.array([len(f["kp_l"]) for f in frames], np.int32), n_kp_r=np.array([len(f["kp_r"]) for f in frames], np.int32),
                 n_kl_l=np.array([len(f["kl_l"]) for f in frames], np.int32), n_kl_r=np.array([len(f["kl_r"]) for f in frames], np.int32),
                 kp_l=np.zeros((B, skp, 2), np.float32), oct_l=np.zeros((B, skp), np.int32), desc_l=np.zeros((B, skp, 32), np.uint8),
                 kp_r=np.zeros((B, skp, 2), np.float32), desc_r=np.zeros((B, skp, 32), np.uint8),
                 kl_l=np.zeros((B, skl, 4), np.float32), oct_ll=np.zeros((B, skl), np.int32), ldesc_l=np.zeros((B, skl, 32), np.uint8),
                 kl_r=np.zeros((B, skl, 4), np.float32), ldesc_r=np.zeros((B, skl, 32), np.uint8))
        for b, f in enumerate(frames):
            n = len(f["kp_l"]); a["kp_l"][b, :n] = f["kp_l"]; a["oct_l"][b, :n] = f["oct_l"]; a["desc_l"][b, :n] = f["desc_l"]
            n = len(f["kp_r"]); a["kp_r"][b, :n] = f["kp_r"]; a["desc_r"][b, :n] = f["desc_r"]
            n = len(f["kl_l"]); a["kl_l"][b, :n] = f["kl_l"]; a["oct_ll"][b, :n] = f["oct_ll"]; a["ldesc_l"][b, :n] = f["ldesc_l"]
            n = len(f["kl_r"]); a["kl_r"][b, :n] = f["kl_r"]; a["ldesc_r"][b, :n] = f["ldesc_r"]
        ff = FrameFeatures()
        ff.stride_kp, ff.stride_kl = skp, skl
        for k, v in a.items():
            setattr(ff, k, v.ctypes.data_as(C.c_void_p))
        return ff, a  # `a` keeps the arrays alive

    def push(self, frames):
        """frames: list of B per-sequence frame dicts as produced by synth.make_stereo_sequence."""
        ff, keep = self._pack(frames)
        res = np.zeros(self.B, dtype=POSE_RESULT_DTYPE)
        counts = np.zeros(self.B * 4, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_seq_push(self.h, C.byref(ff), res.ctypes.data_as(C.c_void_p), counts))
        return res, counts.reshape(self.B, 4)

    def upload(self, slot, frames):
        ff, keep = self._pack(frames)
        self.ctx._chk(self.ctx.lib.stvo_seq_upload(self.h, slot, C.byref(ff)))
        self.ctx.synchronize()

    def upload_dev(self, slot, ff):
        """ff: FrameFeatures whose pointers (count arrays included) are DEVICE pointers; asynchronous."""
        self.ctx._chk(self.ctx.lib.stvo_seq_upload_dev(self.h, slot, C.byref(ff)))

    def step_dev(self, slot):
        self.ctx._chk(self.ctx.lib.stvo_seq_step_dev(self.h, slot))

    def adapt_fast_dev(self, prm, th):
        """updateFrame's adaptive FAST rule behind the last enqueued step (stvo_seq_adapt_fast_dev): th = torch int32 [B] device tensor,
        moved in place by that step's results; asynchronous.  A sequence's first frame leaves it alone."""
        if str(th.dtype) != "torch.int32" or not th.is_cuda or not th.is_contiguous() or th.numel() != self.B:
            raise ValueError("Sequences.adapt_fast_dev: th must be a contiguous int32 device tensor of B entries")
        self.ctx._chk(self.ctx.lib.stvo_seq_adapt_fast_dev(self.h, C.byref(prm), th.data_ptr()))

    def control_next_step(self, ctl):
        """One control word per stream for the NEXT step only (stvo_seq_control_next_step): STREAM_RUN, STREAM_RESTART (the frame in
        the slot starts a new sequence: StereoFrameHandler::initialize) or STREAM_PARK (no sequence at the moment: nothing of the
        stream is reported or advanced).  ctl: B integers; staged on the context's stream at once, no synchronisation."""
        ctl = np.ascontiguousarray(np.asarray(ctl).reshape(-1), dtype=np.int32)
        if ctl.size != self.B:
            raise ValueError("Sequences.control_next_step: one control word per stream")
        self.ctx._chk(self.ctx.lib.stvo_seq_control_next_step(self.h, _ptr(ctl)))

    def restart_fast_dev(self, th, th0):
        """th[b] = th0 for the streams the staged control restarts (stvo_seq_restart_fast_dev), before their first frame is detected;
        th = torch int32 [B] device tensor.  Nothing is launched when no control is staged."""
        if str(th.dtype) != "torch.int32" or not th.is_cuda or not th.is_contiguous() or th.numel() != self.B:
            raise ValueError("Sequences.restart_fast_dev: th must be a contiguous int32 device tensor of B entries")
        self.ctx._chk(self.ctx.lib.stvo_seq_restart_fast_dev(self.h, th.data_ptr(), int(th0)))

    def restart_cameras(self, cams):
        """The cameras of the sequences the staged control's RESTART streams begin (stvo_seq_restart_cameras), after control_next_step for
        the same step: cams = B entries, a camera dict (fx, fy, cx, cy, b, width, height) for every stream that restarts, None (or
        anything) for the others, which are not read.  No synchronisation."""
        if len(cams) != self.B:
            raise ValueError("Sequences.restart_cameras: one entry per stream")
        arr = (Cam * self.B)(*[Cam.from_dict(c) if c is not None else Cam() for c in cams])
        cols = np.array([c["width"] if c is not None else 0 for c in cams], np.int32)
        rows = np.array([c["height"] if c is not None else 0 for c in cams], np.int32)
        self.ctx._chk(self.ctx.lib.stvo_seq_restart_cameras(self.h, C.cast(arr, C.c_void_p), _ptr(cols), _ptr(rows)))

    def set_trajectory(self, prm, log_steps=1):
        """Trajectory and key-frame decision per stream behind every tracked step (stvo_seq_set_trajectory): prm = traj_params(...) or
        None (off); the last log_steps steps' records stay readable.  Only before the first step."""
        self.ctx._chk(self.ctx.lib.stvo_seq_set_trajectory(self.h, C.byref(prm) if prm is not None else None, log_steps))
        self._traj_log_steps = log_steps if prm is not None else 0

    def read_trajectory(self, n_last=1):
        """TRAJ_RECORD_DTYPE array [n, B]: the last n = min(n_last, log_steps, tracked steps) steps, oldest first; synchronises."""
        rows = max(1, min(n_last, getattr(self, "_traj_log_steps", 0)))   # the library returns no more than the ring holds
        rec = np.zeros((rows, self.B), dtype=TRAJ_RECORD_DTYPE)
        n = C.c_int32()
        self.ctx._chk(self.ctx.lib.stvo_seq_read_trajectory(self.h, n_last, rec.ctypes.data_as(C.c_void_p), C.byref(n)))
        return rec[:n.value].copy()

    def trajectory_state(self):
        """Host copy of the B stream states (TRAJ_STATE_DTYPE) after everything enqueued so far; synchronises."""
        out = np.zeros(self.B, dtype=TRAJ_STATE_DTYPE)
        self.ctx._chk(self.ctx.lib.stvo_seq_read_trajectory_state(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_tracks(self, log_steps=1, keyframe_sets=False):
        """Feature tracks per stream behind every step (stvo_seq_set_tracks): the TRACK_DTYPE records of the last log_steps steps stay
        readable; keyframe_sets: every stream also keeps the stereo set of its last key-frame.  log_steps = 0: off.  Only before the
        first step."""
        self.ctx._chk(self.ctx.lib.stvo_seq_set_tracks(self.h, 1 if keyframe_sets else 0, int(log_steps)))
        self._track_log_steps = int(log_steps)

    def read_tracks(self, n_last=1):
        """(pts [n, B, K], lines [n, B, M] as TRACK_DTYPE, counts [n, B, 2]) of the last n = min(n_last, log_steps, steps) steps, oldest
        first; rows [0, count) of a stream are meaningful.  Synchronises."""
        K, M = self.strides()
        rows = max(1, min(n_last, getattr(self, "_track_log_steps", 0)))
        pts, lines = np.zeros((rows, self.B, K), TRACK_DTYPE), np.zeros((rows, self.B, M), TRACK_DTYPE)
        counts = np.zeros((rows, self.B, 2), np.int32)
        n = C.c_int32()
        self.ctx._chk(self.ctx.lib.stvo_seq_read_tracks(self.h, n_last, pts.ctypes.data_as(C.c_void_p), lines.ctypes.data_as(C.c_void_p),
                                                       counts.ctypes.data_as(C.c_void_p), C.byref(n)))
        return pts[:n.value].copy(), lines[:n.value].copy(), counts[:n.value].copy()

    def tracks_dev(self):
        """Device addresses (points, lines, counts) of the last step's records (stvo_seq_tracks_dev), for chained kernels."""
        ps = [C.c_void_p() for _ in range(3)]
        self.ctx._chk(self.ctx.lib.stvo_seq_tracks_dev(self.h, *[C.byref(p) for p in ps]))
        return tuple(p.value for p in ps)

    def keyframe_headers(self):
        """KF_HEADER_DTYPE array [B] (stvo_seq_keyframe_headers); serial == 0: the stream has no key-frame set yet.  Synchronises."""
        hdr = np.zeros(self.B, KF_HEADER_DTYPE)
        self.ctx._chk(self.ctx.lib.stvo_seq_keyframe_headers(self.h, hdr.ctypes.data_as(C.c_void_p)))
        return hdr

    def read_keyframe(self, b):
        """Stream b's key-frame set (stvo_seq_read_keyframe): the dict of debug_stereo plus frame and serial of the header."""
        K, M = self.strides()
        rc = np.empty((K, 4), np.float32); desc = np.empty((K, 32), np.uint8); ldesc = np.empty((M, 32), np.uint8)
        spl, epl = np.empty((M, 2)), np.empty((M, 2))
        sP, eP, le = np.empty((M, 3)), np.empty((M, 3)), np.empty((M, 3))
        s2l, s2lm = np.empty(M), np.empty(M)
        hdr = np.zeros(1, KF_HEADER_DTYPE)
        self.ctx._chk(self.ctx.lib.stvo_seq_read_keyframe(self.h, b, hdr.ctypes.data_as(C.c_void_p), K, rc.reshape(-1), desc.reshape(-1), M,
                                                         spl.reshape(-1), epl.reshape(-1), sP.reshape(-1), eP.reshape(-1), le.reshape(-1),
                                                         s2l, s2lm, ldesc.reshape(-1)))
        n, nl = int(hdr["n_pts"][0]), int(hdr["n_lines"][0])
        return dict(n=n, rc=rc[:n].copy(), desc=desc[:n].copy(), nl=nl, spl=spl[:nl].copy(), epl=epl[:nl].copy(), sP=sP[:nl].copy(),
                    eP=eP[:nl].copy(), le=le[:nl].copy(), s2l=s2l[:nl].copy(), s2lm=s2lm[:nl].copy(), ldesc=ldesc[:nl].copy(),
                    frame=int(hdr["frame"][0]), serial=int(hdr["serial"][0]))

    def snapshot_info(self):
        """{"K", "M", "flags" (SNAP_*), "bytes" of one stream's blob} of this pipeline (stvo_seq_snapshot_info)."""
        k, m, f, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx._chk(self.ctx.lib.stvo_seq_snapshot_info(self.h, C.byref(k), C.byref(m), C.byref(f), C.byref(b)))
        return dict(K=k.value, M=m.value, flags=f.value, bytes=b.value)

    @staticmethod
    def _streams(streams):
        return np.ascontiguousarray(np.asarray(streams).reshape(-1), dtype=np.int32)

    def export_streams(self, streams):
        """uint8 [n, bytes]: blob i = everything stream streams[i] carries into the next step (stvo_seq_export_streams); synchronises."""
        st = self._streams(streams)
        out = np.zeros((st.size, self.snapshot_info()["bytes"]), np.uint8)
        self.ctx._chk(self.ctx.lib.stvo_seq_export_streams(self.h, st.size, _ptr(st), out.ctypes.data_as(C.c_void_p)))
        return out

    def export_streams_dev(self, streams, blob_ptr):
        """The same into device memory at blob_ptr (n * bytes, 16-byte aligned), enqueued on the context's stream; no synchronisation."""
        st = self._streams(streams)
        self.ctx._chk(self.ctx.lib.stvo_seq_export_streams_dev(self.h, st.size, _ptr(st), C.c_void_p(blob_ptr)))

    def import_streams(self, streams, blobs):
        """Stream streams[i] holds the state of blobs[i] (uint8 [n, stride], as export_streams returns them, of this or another pipeline);
        refusals raise StvoError and change nothing (stvo_seq_import_streams)."""
        st = self._streams(streams)
        blobs = np.ascontiguousarray(blobs, np.uint8).reshape(st.size, -1)
        self.ctx._chk(self.ctx.lib.stvo_seq_import_streams(self.h, st.size, _ptr(st), blobs.ctypes.data_as(C.c_void_p), blobs.shape[1]))

    def import_streams_dev(self, streams, blob_ptr, blob_stride):
        """The same from device memory (blob i at blob_ptr + i * blob_stride); synchronises once for the headers, then enqueues."""
        st = self._streams(streams)
        self.ctx._chk(self.ctx.lib.stvo_seq_import_streams_dev(self.h, st.size, _ptr(st), C.c_void_p(blob_ptr), int(blob_stride)))

    def read(self):
        res = np.zeros(self.B, dtype=POSE_RESULT_DTYPE)
        counts = np.zeros(self.B * 4, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_seq_read(self.h, res.ctypes.data_as(C.c_void_p), counts))
        return res, counts.reshape(self.B, 4)

    def last_schedule(self):
        """{field of SEQ_SCHEDULE_FIELDS: value}: what the last enqueued step decided on the host (no launch, no synchronisation)."""
        out = np.zeros(8, np.int32)
        self.ctx._chk(self.ctx.lib.stvo_seq_last_schedule(self.h, out))
        return {k: int(out[i]) for i, k in enumerate(SEQ_SCHEDULE_FIELDS)}

    def enable_fetch(self, on=True):
        self.ctx._chk(self.ctx.lib.stvo_seq_enable_fetch(self.h, 1 if on else 0))

    def strides(self):
        k, m = C.c_int32(), C.c_int32()
        self.ctx._chk(self.ctx.lib.stvo_seq_strides(self.h, C.byref(k), C.byref(m)))
        return k.value, m.value

    def fetch_matches(self):
        """(stereo m12 points [B,K], stereo m12 lines [B,M], f2f m12 points [B,K], f2f m12 lines [B,M]) of the last step."""
        K, M = self.strides()
        ps = [C.POINTER(C.c_int32)() for _ in range(4)]
        self.ctx._chk(self.ctx.lib.stvo_seq_fetch_matches(self.h, *[C.byref(p) for p in ps]))
        shapes = [(self.B, K), (self.B, M), (self.B, K), (self.B, M)]
        return tuple(np.ctypeslib.as_array(p, shape=sh).copy() for p, sh in zip(ps, shapes))

    def fetch_inliers(self):
        K, M = self.strides()
        ps = [C.POINTER(C.c_int32)() for _ in range(2)]
        self.ctx._chk(self.ctx.lib.stvo_seq_fetch_inliers(self.h, *[C.byref(p) for p in ps]))
        return tuple(np.ctypeslib.as_array(p, shape=sh).copy() for p, sh in zip(ps, [(self.B, K), (self.B, M)]))


# ---- stereo rectification (stvo_rectify_*) ------------------------------------------------------------------------------------

RECT_FORM_KITTI, RECT_FORM_RADTAN, RECT_FORM_FISHEYE = 0, 1, 2


def parse_dataset_yaml(text):
    """The YAML subset of the dataset parameter files (config/dataset_params/*.yaml of the reference): `key: value` lines, one level
    of blocks (`cam0:`), scalars, and flow lists `[a, b, ...]` that may span lines; `#` starts a comment.  -> nested dict of str /
    float / list of float."""
    root, block, pending = {}, None, None
    for raw in text.splitlines():
        line = raw.split("#", 1)[0].rstrip()
        if pending is not None:
            pending[1].append(line.strip())
            if "]" in line:
                key, parts, target = pending
                target[key] = [float(v) for v in " ".join(parts).strip()[1:-1].replace(",", " ").split()]
                pending = None
            continue
        if not line.strip():
            continue
        indented = line[0] in " \t"
        key, sep, val = line.strip().partition(":")
        if not sep:
            raise ValueError(f"dataset parameters: cannot read line {raw!r}")
        key, val = key.strip(), val.strip()
        target = block if indented and block is not None else root
        if not indented:
            block = None
        if val == "":
            if indented:
                raise ValueError(f"dataset parameters: nested blocks are not supported ({raw!r})")
            block = root[key] = {}
        elif val.startswith("["):
            if "]" in val:
                target[key] = [float(v) for v in val[1:val.index("]")].replace(",", " ").split()]
            else:
                pending = (key, [val], target)
        else:
            try:
                target[key] = float(val)
            except ValueError:
                target[key] = val
    if pending is not None:
        raise ValueError(f"dataset parameters: unterminated list for {pending[0]}")
    return root


def calib_from_params(params):
    """The cam0 block of a parsed dataset parameter file -> RectCalib, selecting the branch the reference's constructor takes
    (src/pinholeStereoCamera.cpp:38-125): Kl present -> rad-tan stereo (fisheye when a dtype key is present), else KITTI-style."""
    cam = params["cam0"]
    if cam.get("cam_model") != "Pinhole":
        raise ValueError("dataset parameters: cam_model must be Pinhole")
    c = RectCalib()
    c.width, c.height, c.b = int(cam["cam_width"]), int(cam["cam_height"]), float(cam["cam_bl"])
    if "Kl" in cam:
        c.form = RECT_FORM_FISHEYE if "dtype" in cam else RECT_FORM_RADTAN
        nd = len(cam["Dl"])
        if len(cam["Dr"]) != nd or len(cam["Kl"]) != 4 or len(cam["Kr"]) != 4 or len(cam["R"]) != 9 or len(cam["t"]) != 3:
            raise ValueError("dataset parameters: Kl / Kr need 4 values, Dl / Dr the same count, R 9 and t 3")
        c.n_dist = nd
        c.Kl[:], c.Kr[:] = cam["Kl"], cam["Kr"]
        c.Dl[:nd], c.Dr[:nd] = cam["Dl"], cam["Dr"]
        c.R[:], c.t[:] = cam["R"], cam["t"]
    else:
        c.form = RECT_FORM_KITTI
        c.fx, c.fy, c.cx, c.cy = cam["cam_fx"], cam["cam_fy"], cam["cam_cx"], cam["cam_cy"]
        c.d[:] = [cam["cam_d0"], cam["cam_d1"], cam["cam_d2"], cam["cam_d3"]]
    return c


def read_dataset_params(path):
    """A dataset parameter file (euroc_params.yaml, kitti00-02.yaml, ...) -> RectCalib."""
    with open(path) as f:
        return calib_from_params(parse_dataset_yaml(f.read()))


def camera_dict(rc):
    """RectCamera -> dict of numpy arrays (R1, R2 3x3; P1, P2 3x4), the pipeline camera (fx, fy, cx, cy, b, width, height), dist."""
    return dict(R1=np.array(rc.R1[:]).reshape(3, 3), R2=np.array(rc.R2[:]).reshape(3, 3), P1=np.array(rc.P1[:]).reshape(3, 4),
                P2=np.array(rc.P2[:]).reshape(3, 4), dist=int(rc.dist),
                cam=dict(fx=rc.cam.fx, fy=rc.cam.fy, cx=rc.cam.cx, cy=rc.cam.cy, b=rc.cam.b, width=rc.width, height=rc.height))


def rectify_compute(calib, maps=True):
    """Host-only rectification (no device): (camera_dict, map1 int16 [2, rows, cols, 2], map2 uint16 [2, rows, cols]) or, with
    maps=False, the camera dict alone."""
    L = load()
    rc = RectCamera()
    m1 = m2 = None
    if maps:
        m1 = np.zeros((2, calib.height, calib.width, 2), np.int16)
        m2 = np.zeros((2, calib.height, calib.width), np.uint16)
    rcode = L.stvo_rectify_compute(C.byref(calib), C.byref(rc), _ptr(m1) if maps else None, _ptr(m2) if maps else None)
    if rcode != 0:
        raise StvoError(f"stvo_rectify_compute: {L.stvo_error_string(rcode).decode()} ({rcode})")
    return (camera_dict(rc), m1, m2) if maps else camera_dict(rc)


GRAY_WEIGHTS = {"q14": 0, "q15": 1}  # include/stvo_hip.h: STVO_GRAY_*
GRAY_ORDERS = {"bgr": 0, "rgb": 1}    # STVO_ORDER_*


def color_to_gray(ctx, img, order="bgr", weights="q14", swapped=False):
    """Host colour images uint8 [n, rows, cols, ch] (or [rows, cols, ch]), ch = 3 (B, G, R) or 4 (B, G, R, A) -> the grey plane(s)
    uint8 [n, rows, cols] of cvtColor's integer form (stvo_color_to_gray, synchronous).  swapped: also the plane with the red and
    blue weights exchanged, from the same launch: returns (plane, swapped plane)."""
    img = np.ascontiguousarray(img, np.uint8)
    single = img.ndim == 3
    if single:
        img = img[None]
    if img.ndim != 4:
        raise ValueError("color_to_gray: images must be [n, rows, cols, channels]")
    n, rows, cols, ch = img.shape
    a = np.empty((n, rows, cols), np.uint8)
    b = np.empty((n, rows, cols), np.uint8) if swapped else None
    ctx._chk(ctx.lib.stvo_color_to_gray(ctx.h, n, rows, cols, ch, GRAY_ORDERS[order], GRAY_WEIGHTS[weights], _ptr(img), _ptr(a),
                                        _ptr(b) if swapped else None))
    if single:
        a, b = a[0], (b[0] if swapped else None)
    return (a, b) if swapped else a


def color_to_gray_dev(ctx, n, rows, cols, ch, src, gray, gray_swapped=None, order="bgr", weights="q14"):
    """Device pointers; asynchronous on the context's stream (stvo_color_to_gray_dev)."""
    ctx._chk(ctx.lib.stvo_color_to_gray_dev(ctx.h, n, rows, cols, ch, GRAY_ORDERS[order], GRAY_WEIGHTS[weights], src, gray, gray_swapped))


class Rectifier:
    """The GPU rectifier for up to B stereo pairs of one size (stvo_rectify_*): calib = RectCalib (read_dataset_params) or
    maps = (map1 int16 [2, rows, cols, 2], map2 uint16 [2, rows, cols]), left side first."""

    def __init__(self, ctx, B, calib=None, maps=None):
        if (calib is None) == (maps is None):
            raise ValueError("Rectifier: pass exactly one of calib and maps")
        self.ctx, self.B = ctx, B
        self.h = C.c_void_p()
        if calib is not None:
            ctx._chk(ctx.lib.stvo_rectify_create(ctx.h, B, C.byref(calib), C.byref(self.h)))
        else:
            m1 = np.ascontiguousarray(maps[0], np.int16)
            m2 = np.ascontiguousarray(maps[1], np.uint16)
            if m1.ndim != 4 or m1.shape[0] != 2 or m1.shape[3] != 2 or m2.shape != m1.shape[:3]:
                raise ValueError("Rectifier: maps must be int16 [2, rows, cols, 2] and uint16 [2, rows, cols]")
            ctx._chk(ctx.lib.stvo_rectify_create_from_maps(ctx.h, B, m1.shape[2], m1.shape[1], _ptr(m1), _ptr(m2), C.byref(self.h)))
        rc = RectCamera()
        ctx._chk(ctx.lib.stvo_rectify_camera(self.h, C.byref(rc)))
        info = camera_dict(rc)
        self.cols, self.rows, self.dist = rc.width, rc.height, info["dist"]
        self.camera = info["cam"]  # the rectified pipeline camera (zeros for caller maps)
        self.info = info

    def close(self):
        if self.h:
            self.ctx.lib.stvo_rectify_destroy(self.h)
            self.h = None

    def rectify(self, left, right):
        """Host images uint8 [n, rows, cols] each (n <= B) -> (left, right) rectified, synchronous."""
        left = np.ascontiguousarray(left, np.uint8).reshape(-1, self.rows, self.cols)
        right = np.ascontiguousarray(right, np.uint8).reshape(-1, self.rows, self.cols)
        if len(left) != len(right):
            raise ValueError("Rectifier.rectify: as many right images as left ones")
        out_l, out_r = np.empty_like(left), np.empty_like(right)
        self.ctx._chk(self.ctx.lib.stvo_rectify_images(self.h, len(left), _ptr(left), _ptr(right), _ptr(out_l), _ptr(out_r)))
        return out_l, out_r

    def rectify_dev(self, n, src_l, src_r, dst_l, dst_r):
        """Device pointers (n images each, rows * cols bytes apart); asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.stvo_rectify_images_dev(self.h, n, src_l, src_r, dst_l, dst_r))

    def rectify_color(self, left, right):
        """Host colour images uint8 [n, rows, cols, ch] each (n <= B, ch = 3 or 4) -> (left, right) rectified with all their
        channels, synchronous."""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        if left.ndim != 4 or left.shape[1:3] != (self.rows, self.cols) or right.shape != left.shape:
            raise ValueError("Rectifier.rectify_color: left and right must both be [n, rows, cols, channels] of the rectifier's size")
        out_l, out_r = np.empty_like(left), np.empty_like(right)
        self.ctx._chk(self.ctx.lib.stvo_rectify_color_images(self.h, len(left), left.shape[3], _ptr(left), _ptr(right), _ptr(out_l), _ptr(out_r)))
        return out_l, out_r

    def rectify_color_dev(self, n, ch, src_l, src_r, dst_l, dst_r):
        """Device pointers (n images each, rows * cols * ch bytes apart); asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.stvo_rectify_color_images_dev(self.h, n, ch, src_l, src_r, dst_l, dst_r))

    def rectify_color_to_gray_dev(self, n, ch, src_l, src_r, gray_l, gray_r, swapped_l=None, swapped_r=None, order="bgr", weights="q14"):
        """Raw colour pairs -> the grey planes of the rectified colour images, one kernel (device pointers, asynchronous); swapped_*:
        the planes of the other channel order, both or neither."""
        self.ctx._chk(self.ctx.lib.stvo_rectify_color_to_gray_dev(self.h, n, ch, GRAY_ORDERS[order], GRAY_WEIGHTS[weights], src_l, src_r,
                                                                  gray_l, gray_r, swapped_l, swapped_r))


class RectifierBank:
    """One rectifier for mixed cameras (stvo_rectify_bank_*): up to B pairs per call in slots of slot_cols x slot_rows, every pair under
    one of the K calibrations `rectifiers` (capi.Rectifier objects of the same context, each no larger than the slot).  The bank borrows
    their resident maps: keep the rectifiers open until the bank is closed.  Buffers are slot-shaped, [n, slot_rows, slot_cols(, ch)],
    image b the top-left cols_k x rows_k of its slot — what Orb.set_image_sizes reads.  Every pair starts on calibration 0."""

    def __init__(self, ctx, B, slot_cols, slot_rows, rectifiers):
        rectifiers = list(rectifiers)
        if not rectifiers or any(r.ctx is not ctx or not r.h for r in rectifiers):
            raise ValueError("RectifierBank: rectifiers is a non-empty list of open Rectifier objects of the same context")
        self.ctx, self.B, self.slot_cols, self.slot_rows = ctx, B, slot_cols, slot_rows
        self.rectifiers = rectifiers  # (kept alive: the bank reads their maps)
        self.K = len(rectifiers)
        self.sizes = [(r.cols, r.rows) for r in rectifiers]
        self.calibs = [0] * B
        self.h = C.c_void_p()
        hs = (C.c_void_p * self.K)(*[r.h for r in rectifiers])
        ctx._chk(ctx.lib.stvo_rectify_bank_create(ctx.h, B, slot_cols, slot_rows, hs, self.K, C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.lib.stvo_rectify_bank_destroy(self.h)
            self.h = None

    def assign(self, calibs):
        """Pair b takes calibration calibs[b] (B entries, 0 .. K - 1) for the calls that follow; travels on the context's stream behind
        the calls already enqueued, no synchronisation.  An index out of range raises and nothing changes."""
        a = np.ascontiguousarray(calibs, np.int32).reshape(-1)
        if a.size != self.B:
            raise ValueError("RectifierBank.assign: one calibration index per pair (B entries)")
        self.ctx._chk(self.ctx.lib.stvo_rectify_bank_assign(self.h, _ptr(a)))
        self.calibs = [int(v) for v in a]

    def camera(self, k):
        """What Rectifier.camera gives for calibration k: the rectified pipeline camera (zeros for caller maps)."""
        rc = RectCamera()
        self.ctx._chk(self.ctx.lib.stvo_rectify_bank_camera(self.h, k, C.byref(rc)))
        return camera_dict(rc)["cam"]

    def rectify_dev(self, n, ch, src_l, src_r, dst_l, dst_r):
        """Device pointers to slot-shaped buffers (n slots each, ch = 1, 3 or 4); one launch, asynchronous on the context's stream."""
        self.ctx._chk(self.ctx.lib.stvo_rectify_bank_images_dev(self.h, n, ch, src_l, src_r, dst_l, dst_r))

    def rectify_color_to_gray_dev(self, n, ch, src_l, src_r, gray_l, gray_r, swapped_l=None, swapped_r=None, order="bgr", weights="q14"):
        """Raw colour slots -> the grey planes of the rectified colour images, one launch (device pointers, asynchronous); swapped_*:
        the planes of the other channel order, both or neither."""
        self.ctx._chk(self.ctx.lib.stvo_rectify_bank_color_to_gray_dev(self.h, n, ch, GRAY_ORDERS[order], GRAY_WEIGHTS[weights], src_l, src_r,
                                                                       gray_l, gray_r, swapped_l, swapped_r))

    def _slots(self, imgs, ch, torch):
        """per-pair host arrays of each pair's own size -> a device tensor of slots (zeros beyond the images)"""
        shape = (len(imgs), self.slot_rows, self.slot_cols) + ((ch,) if ch > 1 else ())
        host = np.zeros(shape, np.uint8)
        for b, im in enumerate(imgs):
            cols, rows = self.sizes[self.calibs[b]]
            im = np.asarray(im, np.uint8)
            if im.shape != (rows, cols) + ((ch,) if ch > 1 else ()):
                raise ValueError(f"RectifierBank: pair {b} takes images of {cols} x {rows}")
            host[b, :rows, :cols] = im
        return torch.as_tensor(host).cuda()

    def _run(self, left, right, ch):
        import torch  # (the device buffers of this convenience only; every computation is behind the C-ABI)
        if len(left) != len(right) or not 1 <= len(left) <= self.B:
            raise ValueError("RectifierBank: as many right images as left ones, 1 .. B pairs")
        sl, sr = self._slots(left, ch, torch), self._slots(right, ch, torch)
        dl, dr = torch.zeros_like(sl), torch.zeros_like(sr)
        torch.cuda.synchronize()  # the copies ran on torch's stream, the library uses its own
        self.rectify_dev(len(left), ch, sl.data_ptr(), sr.data_ptr(), dl.data_ptr(), dr.data_ptr())
        self.ctx.synchronize()
        out = []
        for d in (dl.cpu().numpy(), dr.cpu().numpy()):
            out.append([d[b, :self.sizes[self.calibs[b]][1], :self.sizes[self.calibs[b]][0]].copy() for b in range(len(left))])
        return out[0], out[1]

    def rectify(self, left, right):
        """Host images: two lists of n <= B uint8 arrays [rows_b, cols_b] of each pair's own size (its calibration's) -> (left, right)
        lists of the rectified images, synchronous."""
        return self._run(left, right, 1)

    def rectify_color(self, left, right):
        """The same for colour images [rows_b, cols_b, ch], ch = 3 or 4, every channel remapped."""
        ch = np.asarray(left[0]).shape[-1] if len(left) and np.asarray(left[0]).ndim == 3 else 0
        if ch not in (3, 4):
            raise ValueError("RectifierBank.rectify_color: images are [rows, cols, 3] or [rows, cols, 4]")
        return self._run(left, right, ch)
