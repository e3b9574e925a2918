"""ctypes binding of librt_hip.so (include/rt_abi.h).

The library must be built in-tree (``make -C gpu-ray-tracing_amd`` or
``__graft_entry__.build()``).  There is no fallback: if the HIP library is missing or
fails to load, every entry point raises.

``torch`` is imported before the library is opened so that the HIP runtime torch ships
(soname libamdhip64.so.7) is the one librt_hip.so binds to; streams and device pointers
from torch are then valid inside the library.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch  # noqa: F401  (load order: torch's HIP runtime first)

PKG_ROOT = Path(__file__).resolve().parent.parent          # gpu-ray-tracing_amd/
LIB_PATH = PKG_ROOT / "build" / "librt_hip.so"

F = ctypes.c_float
U32 = ctypes.c_uint32


class RtError(RuntimeError):
    """A librt_hip.so entry point returned a non-zero rt_status."""

    def __init__(self, status: int, func: str, message: str):
        super().__init__(f"{func} failed with status {status} ({STATUS_NAMES.get(status, '?')}): "
                         f"{message}")
        self.status = status


STATUS_NAMES = {
    0: "RT_OK",
    1: "RT_ERR_INVALID_ARGUMENT",
    2: "RT_ERR_INVALID_SIZE",
    3: "RT_ERR_INVALID_DEVICE",
    4: "RT_ERR_HIP",
    5: "RT_ERR_NO_MEMORY",
    6: "RT_ERR_INVALID_CONTEXT",
    7: "RT_ERR_COMM",
}
RT_COMM_ID_BYTES = 128
RT_STRIPE_ROWS = 8
RT_SCAN_EXHAUSTIVE = 0
RT_SCAN_CULLED = 1
RT_ENCODE_LINEAR = 0
RT_ENCODE_SRGB = 1


class SceneCameraC(ctypes.Structure):
    """rt_scene_camera == SceneCamera (camera.rs:256-291), 176 bytes."""

    _fields_ = [
        ("center", F * 3), ("viewport_height", F),
        ("viewport_upper_left", F * 3), ("viewport_width", F),
        ("pixel_delta_u", F * 3), ("defocus_angle", F),
        ("pixel_delta_v", F * 3), ("aspect_ratio", F),
        ("defocus_disk_u", F * 3), ("_padding0", F),
        ("viewport_u", F * 3), ("_padding1", F),
        ("defocus_disk_v", F * 3), ("max_depth", F),
        ("look_from", F * 3), ("samples_per_pixel", F),
        ("look_at", F * 3), ("camera_has_moved", F),
        ("vup", F * 3), ("random_seed", F),
        ("viewport_v", F * 3), ("defocus_radius", F),
    ]


class SphereC(ctypes.Structure):
    """rt_sphere == GpuSphere (sphere.rs:20-26), 32 bytes."""

    _fields_ = [("position", F * 3), ("radius", F), ("color", F * 4)]


class CameraSettingsC(ctypes.Structure):
    """rt_camera_settings == CameraSettings (camera.rs:9-28)."""

    _fields_ = [
        ("field_of_view", F), ("samples_per_pixel", U32), ("camera_has_moved", U32),
        ("max_depth", U32), ("vup", F * 3), ("look_from", F * 3), ("look_at", F * 3),
        ("defocus_angle", F), ("focus_distance", F),
    ]


assert ctypes.sizeof(SceneCameraC) == 176
assert ctypes.sizeof(SphereC) == 32

P = ctypes.c_void_p
_SIGS = {
    "rt_abi_version": (U32, []),
    "rt_last_error": (ctypes.c_char_p, []),
    "rt_kernel_name": (ctypes.c_char_p, [ctypes.c_int]),
    "rt_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(P)]),
    "rt_destroy": (ctypes.c_int, [P]),
    "rt_set_scan_mode": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_set_spheres": (ctypes.c_int, [P, P, U32, P]),
    "rt_init_image": (ctypes.c_int, [P, P, U32, U32, P]),
    "rt_update": (ctypes.c_int, [P, P, P, U32, U32, P, P, U32, P]),
    "rt_render": (ctypes.c_int, [P, P, P, U32, U32, P, P, U32, U32, P, P]),
    "rt_render_stripes": (ctypes.c_int, [P, P, P, U32, U32, U32, U32, P, P, U32, U32, P, P]),
    "rt_update_frames": (ctypes.c_int, [P, P, P, U32, U32, U32, U32, P, P, U32, U32, P, P,
                                        ctypes.POINTER(ctypes.c_int)]),
    "rt_stripe_local_rows": (U32, [U32, U32, U32]),
    "rt_deinterleave_stripes": (ctypes.c_int, [P, P, P, U32, U32, U32, P]),
    "rt_camera_settings_default": (None, [P]),
    "rt_camera_from_settings": (ctypes.c_int, [P, U32, U32, F, P]),
    "rt_scene_generate": (ctypes.c_int, [U32, U32, ctypes.c_uint64, P, U32, ctypes.POINTER(U32)]),
    "rt_frame_seeds": (None, [ctypes.c_uint64, U32, P]),
    "rt_driver_create": (ctypes.c_int, [P, P, P, U32, U32, ctypes.POINTER(P)]),
    "rt_driver_destroy": (ctypes.c_int, [P]),
    "rt_driver_frame": (ctypes.c_int, [P, P, P, U32, P, ctypes.POINTER(ctypes.c_int)]),
    "rt_driver_state": (ctypes.c_int, [P]),
    "rt_present_rgba8": (ctypes.c_int, [P, P, P, U32, U32, ctypes.c_int, P]),
    "rt_srgb_thresholds": (None, [P]),
    "rt_selftest_fastmath": (ctypes.c_int, [P, ctypes.c_uint64, P]),
    "rt_set_frames_per_launch": (ctypes.c_int, [P, U32]),
    "rt_get_frames_per_launch": (ctypes.c_int, [P, P, ctypes.POINTER(U32)]),
    "rt_set_frame_pairs": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_set_tile_order": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_set_update_queues": (ctypes.c_int, [P, U32]),
    "rt_set_update_submit": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_set_frame_images": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_update_submit_status": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(U32),
                                               ctypes.POINTER(ctypes.c_uint64)]),
    "rt_last_launch_info": (ctypes.c_int, [P, P]),
    "rt_set_path_compaction": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_set_single_kernel": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_candidate_stats": (ctypes.c_int, [P, P]),
    "rt_comm_unique_id": (ctypes.c_int, [P]),
    "rt_comm_create": (ctypes.c_int, [P, P, U32, U32, ctypes.POINTER(P)]),
    "rt_comm_create_all": (ctypes.c_int, [U32, P, P]),
    "rt_comm_destroy": (ctypes.c_int, [P]),
    "rt_comm_info": (ctypes.c_int, [P, ctypes.POINTER(U32), ctypes.POINTER(U32),
                                    ctypes.POINTER(ctypes.c_int)]),
    "rt_comm_group_start": (ctypes.c_int, []),
    "rt_comm_group_end": (ctypes.c_int, []),
    "rt_gather_stripes": (ctypes.c_int, [P, P, P, P, P, U32, U32, U32, P]),
    "rt_update_frames_bands": (ctypes.c_int, [P, P, P, U32, U32, P, P, P, U32, U32, P, P,
                                              ctypes.POINTER(ctypes.c_int)]),
    "rt_band_costs": (ctypes.c_int, [P, U32, U32, P, P]),
    "rt_partition_bands": (ctypes.c_int, [P, U32, U32, P]),
    "rt_deinterleave_bands": (ctypes.c_int, [P, P, P, U32, U32, U32, P, U32, P]),
    "rt_gather_bands": (ctypes.c_int, [P, P, P, P, P, U32, U32, P, U32, P]),
    "rt_set_launch_timing": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_last_call_kernel_time": (ctypes.c_int, [P, ctypes.POINTER(F), ctypes.POINTER(U32)]),
}

# include/rt_chain_parts.h (the additions to rt_abi.h's boundary)
_SIGS_CHAIN_PARTS = {
    "rt_set_chain_parts": (ctypes.c_int, [P, U32]),
    "rt_chain_schedule": (ctypes.c_int, [U32, U32, ctypes.c_int, P, U32, ctypes.POINTER(U32)]),
}

# include/rt_occlusion_cull.h
_SIGS_OCCLUSION = {
    "rt_set_occlusion_cull": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_occlusion_cull_stats": (ctypes.c_int, [P, P]),
}

# include/rt_certain_tiles.h
_SIGS_CERTAIN = {
    "rt_set_certain_tiles": (ctypes.c_int, [P, ctypes.c_int]),
    "rt_certain_tiles_stats": (ctypes.c_int, [P, P]),
}

# include/rt_tile_lists.h
_SIGS_TILE_LISTS = {
    "rt_tile_lists": (ctypes.c_int, [P, P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
    "rt_set_tight_bundle": (ctypes.c_int, [P, ctypes.c_int]),
}
RT_TILE_LIST_MAX = 19
RT_TILE_LIST_NONE = 0xFFFFFFFF
RT_TILE_CERTAIN = 1


class TileListC(ctypes.Structure):
    """rt_tile_list (rt_tile_lists.h)."""
    _fields_ = [("count", U32), ("removed", U32), ("flags", U32), ("reserved", U32),
                ("records", (ctypes.c_float * 4) * RT_TILE_LIST_MAX)]


# include/rt_selftest_roots.h
_SIGS_SELFTEST_ROOTS = {
    "rt_selftest_roots": (ctypes.c_int, [P, ctypes.c_uint64, P]),
}
RT_ROOTS_FAMILIES = 2
RT_ROOTS_STRATA = 4

# include/rt_aov.h (first-hit G-buffer and picking)
_SIGS_AOV = {
    "rt_trace_aov": (ctypes.c_int, [P, P, U32, U32, P, P, U32, P]),
    "rt_trace_aov_bands": (ctypes.c_int, [P, P, U32, U32, P, P, P, U32, P]),
    "rt_pick": (ctypes.c_int, [P, U32, U32, U32, U32, P, P, U32, P, P]),
}
RT_AOV_MISS = 0xFFFFFFFF
AOV_PLANES = ("sphere_id", "hit", "normal", "material")


class AovPlanesC(ctypes.Structure):
    """rt_aov_planes (rt_aov.h): device pointers, NULL = plane not wanted."""
    _fields_ = [("sphere_id", P), ("hit", P), ("normal", P), ("material", P)]


class PickResultC(ctypes.Structure):
    """rt_pick_result (rt_aov.h)."""
    _fields_ = [("sphere_id", U32), ("t", F), ("p", F * 3), ("normal", F * 3),
                ("front_face", U32), ("color", F * 4)]


# include/rt_denoise.h (the a-trous denoiser guided by rt_aov.h's planes)
_SIGS_DENOISE = {
    "rt_denoise_params_default": (None, [P]),
    "rt_denoise": (ctypes.c_int, [P, P, P, P, U32, U32, P, P, P, P, P]),
}
RT_DENOISE_MAX_ITERATIONS = 8


class DenoiseParamsC(ctypes.Structure):
    """rt_denoise_params (rt_denoise.h), 16 bytes."""
    _fields_ = [("iterations", U32), ("normal_power_log2", U32), ("inv_sigma_color2", F),
                ("inv_sigma_position2", F)]


# include/rt_reproject.h (carrying the accumulator across camera moves)
_SIGS_REPROJECT = {
    "rt_reproject_params_default": (None, [P]),
    "rt_reproject_basis": (ctypes.c_int, [P, P]),
    "rt_reproject": (ctypes.c_int, [P, P, P, U32, U32, P, P, P, P]),
}


class ReprojectParamsC(ctypes.Structure):
    """rt_reproject_params (rt_reproject.h), 16 bytes."""
    _fields_ = [("max_history", U32), ("lambertian_only", U32), ("position_tolerance2", F),
                ("_reserved", U32)]


class ReprojectPlanesC(ctypes.Structure):
    """rt_reproject_planes (rt_reproject.h): device pointers, 48 bytes."""
    _fields_ = [("prev_sphere_id", P), ("prev_hit", P), ("sphere_id", P), ("hit", P),
                ("normal", P), ("material", P)]


# include/rt_resize.h (carrying the accumulator across image sizes)
_SIGS_RESIZE = {
    "rt_resize_params_default": (None, [P]),
    "rt_resize_carry": (ctypes.c_int, [P, P, U32, U32, U32, U32, P, P, P, P, P]),
}
RT_RESIZE_FILL_NONE = 0
RT_RESIZE_FILL_NEAREST = 1


class ResizeParamsC(ctypes.Structure):
    """rt_resize_params (rt_resize.h), 32 bytes."""
    _fields_ = [("max_history", U32), ("lambertian_only", U32), ("position_tolerance2", F),
                ("sky", U32), ("fill", U32), ("_reserved", U32 * 3)]


class ResizeImagesC(ctypes.Structure):
    """rt_resize_images (rt_resize.h): device pointers, 32 bytes."""
    _fields_ = [("prev_rgba", P), ("dst_rgba", P), ("prev_second", P), ("dst_second", P)]


# include/rt_variance.h (luminance moments and the variance-guided filter)
_SIGS_VARIANCE = {
    "rt_variance_filter_params_default": (None, [P]),
    "rt_moments_update": (ctypes.c_int, [P, P, P, P, U32, U32, P]),
    "rt_variance_filter": (ctypes.c_int, [P, P, P, P, P, P, P, U32, U32, P, P, P, P, P]),
}
RT_VARIANCE_MAX_ITERATIONS = 8


class VarianceFilterParamsC(ctypes.Structure):
    """rt_variance_filter_params (rt_variance.h), 24 bytes."""
    _fields_ = [("iterations", U32), ("normal_power_log2", U32), ("inv_sigma_luminance2", F),
                ("inv_sigma_position2", F), ("min_history", U32), ("fallback_variance", F)]


# include/rt_adaptive.h (variance-driven adaptive sampling)
_SIGS_ADAPTIVE = {
    "rt_adaptive_params_default": (None, [P]),
    "rt_adaptive_error": (ctypes.c_int, [P, P, P, P, U32, U32, U32, P]),
    "rt_update_adaptive": (ctypes.c_int, [P, P, P, P, P, U32, U32, P, P, U32, P, P]),
    "rt_update_adaptive_bands": (ctypes.c_int, [P, P, P, P, P, U32, U32, P, P, P, U32, P, P]),
}


class AdaptiveParamsC(ctypes.Structure):
    """rt_adaptive_params (rt_adaptive.h), 12 bytes."""
    _fields_ = [("min_samples", U32), ("abs_tolerance2", F), ("rel_tolerance2", F)]


# include/rt_converge.h (the adaptive round as one multi-frame launch)
_SIGS_CONVERGE = {
    "rt_converge_frames": (ctypes.c_int, [P, P, P, P, P, P, U32, U32, P, P, U32, U32, P, P, U32,
                                          P]),
    "rt_converge_frames_bands": (ctypes.c_int, [P, P, P, P, P, P, U32, U32, P, P, P, U32, U32, P,
                                                P, U32, P]),
}
RT_CONVERGE_MAX_FRAMES_PER_LAUNCH = 64


# include/rt_progress.h (convergence reports and render-to-tolerance)
_SIGS_PROGRESS = {
    "rt_progress_stats": (ctypes.c_int, [P, P, P, P, P, U32, U32, U32, P, U32, P, P]),
    "rt_progress_stats_bands": (ctypes.c_int, [P, P, P, P, P, U32, U32, P, U32, P, U32, P, P]),
    "rt_progress_run": (ctypes.c_int, [P, P, P, P, U32, U32, P, P, U32, P, P, U32, P, P, P, P]),
}


class ProgressReportC(ctypes.Structure):
    """rt_progress_report (rt_progress.h), 96 bytes."""
    _fields_ = [("pixels", ctypes.c_uint64), ("active", ctypes.c_uint64),
                ("converged", ctypes.c_uint64), ("capped", ctypes.c_uint64),
                ("below_min", ctypes.c_uint64), ("no_history", ctypes.c_uint64),
                ("nonfinite", ctypes.c_uint64), ("samples", ctypes.c_uint64),
                ("active_tiles", ctypes.c_uint64), ("min_count", U32), ("max_count", U32),
                ("max_error", F), ("_reserved", U32 * 3)]


class ProgressGoalC(ctypes.Structure):
    """rt_progress_goal (rt_progress.h), 16 bytes."""
    _fields_ = [("max_active", ctypes.c_uint64), ("max_frames", U32), ("check_every", U32)]


# include/rt_scene_edit.h (carrying the accumulator across scene edits)
_SIGS_EDIT = {
    "rt_edit_params_default": (None, [P]),
    "rt_edit_plan_bytes": (ctypes.c_size_t, [U32]),
    "rt_edit_plan": (ctypes.c_int, [P, U32, P, U32, P, P, P, ctypes.c_size_t, P]),
    "rt_edit_carry": (ctypes.c_int, [P, P, P, U32, U32, P, P, P, U32, U32, P, P]),
}
RT_EDIT_NONE = 0xFFFFFFFF
RT_EDIT_MOVED = 0x80000000
RT_EDIT_MAX_BALLS = 32
RT_EDIT_MAX_SPHERES = 1 << 20


class EditRecordC(ctypes.Structure):
    """rt_edit_record (rt_scene_edit.h), 32 bytes."""
    _fields_ = [("prev_center", F * 3), ("scale", F), ("center", F * 3), ("link", U32)]


class EditBallC(ctypes.Structure):
    """rt_edit_ball (rt_scene_edit.h), 32 bytes."""
    _fields_ = [("center", F * 3), ("radius2", F), ("owner", U32), ("_pad", U32 * 3)]


class EditParamsC(ctypes.Structure):
    """rt_edit_params (rt_scene_edit.h), 32 bytes."""
    _fields_ = [("carry", ReprojectParamsC), ("edit_history", U32), ("influence", F),
                ("_reserved", U32 * 2)]


class EditInfoC(ctypes.Structure):
    """rt_edit_info (rt_scene_edit.h), 32 bytes."""
    _fields_ = [("n_records", U32), ("n_balls", U32), ("n_changed", U32), ("n_moved", U32),
                ("n_restart", U32), ("n_deleted", U32), ("full_restart", U32), ("_reserved", U32)]


# include/rt_matte.h (sample-coverage ID mattes)
_SIGS_MATTE = {
    "rt_matte_frames": (ctypes.c_int, [P, P, U32, U32, P, P, U32, P, U32, P]),
    "rt_matte_frames_bands": (ctypes.c_int, [P, P, U32, U32, P, P, P, U32, P, U32, P]),
    "rt_matte_resolve": (ctypes.c_int, [P, P, ctypes.c_uint64, P, U32, P, P, P]),
    "rt_matte_last_info": (ctypes.c_int, [P, P]),
}
RT_MATTE_SLOTS = 4
RT_MATTE_MAX_FRAMES = 65536
RT_MATTE_LIST_CAPACITY = 64
MATTE_PLANES = ("ids", "counts", "tally")


class MattePlanesC(ctypes.Structure):
    """rt_matte_planes (rt_matte.h): device pointers, 24 bytes."""
    _fields_ = [("ids", P), ("counts", P), ("tally", P)]


class MatteInfoC(ctypes.Structure):
    """rt_matte_info (rt_matte.h), 16 bytes."""
    _fields_ = [("list_tiles", U32), ("fallback_tiles", U32), ("longest_list", U32),
                ("overflow_tiles", U32)]


# include/rt_query.h (ray queries: closest hit and occlusion for rays the caller chooses)
_SIGS_QUERY = {
    "rt_cast_rays": (ctypes.c_int, [P, P, ctypes.c_uint64, U32, P, P, U32, P, P]),
    "rt_cast_ray": (ctypes.c_int, [P, P, P, U32, P, P]),
}
RT_QUERY_CLOSEST = 0
RT_QUERY_OCCLUSION = 1
QUERY_ROUTES = ("grid", "cone", "exhaustive")


class RayC(ctypes.Structure):
    """rt_ray (rt_query.h), 32 bytes."""
    _fields_ = [("o", F * 3), ("tmax", F), ("d", F * 3), ("_reserved", U32)]


class QueryPlanesC(ctypes.Structure):
    """rt_query_planes (rt_query.h): device pointers, 40 bytes."""
    _fields_ = [("sphere_id", P), ("hit", P), ("normal", P), ("material", P), ("occluded", P)]


class BandSetC(ctypes.Structure):
    """rt_band_set (rt_abi.h, ABI 7): global bands first + j * step, j < count."""
    _fields_ = [("first", U32), ("step", U32), ("count", U32)]


def band_sets(sets) -> ctypes.Array:
    """A ctypes array of rt_band_set from (first, step, count) triples."""
    arr = (BandSetC * len(sets))()
    for i, (f, st, c) in enumerate(sets):
        arr[i].first, arr[i].step, arr[i].count = int(f), int(st), int(c)
    return arr


class LaunchInfoC(ctypes.Structure):
    """rt_launch_info (rt_abi.h)."""
    _fields_ = [("launches", U32), ("frames", U32), ("max_frames_per_launch", U32),
                ("kernel", ctypes.c_int32), ("queues", U32), ("submit", U32),
                ("normal_rn", U32), ("chain_parts", U32)]


class ChainLaunchC(ctypes.Structure):
    """rt_chain_launch (rt_abi.h): frames [first, first + frames) of a call for part `part`."""
    _fields_ = [("part", U32), ("first", U32), ("frames", U32)]


class RootsTallyC(ctypes.Structure):
    """rt_roots_tally (rt_selftest_roots.h): one family and stratum of rt_selftest_roots."""
    _fields_ = [("mismatches", ctypes.c_uint64), ("drawn", ctypes.c_uint64),
                ("compared", ctypes.c_uint64), ("rooted", ctypes.c_uint64)]


_lib = None


def lib() -> ctypes.CDLL:
    """Open librt_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("RT_HIP_LIB", LIB_PATH))
        if not path.exists():
            raise RuntimeError(f"librt_hip.so not found at {path}: build it with "
                               f"`make -C {PKG_ROOT}` (no CPU fallback exists)")
        handle = ctypes.CDLL(str(path))
        for name, (res, args) in {**_SIGS, **_SIGS_CHAIN_PARTS, **_SIGS_SELFTEST_ROOTS,
                                  **_SIGS_AOV, **_SIGS_DENOISE, **_SIGS_REPROJECT,
                                  **_SIGS_VARIANCE, **_SIGS_ADAPTIVE, **_SIGS_CONVERGE,
                                  **_SIGS_PROGRESS, **_SIGS_EDIT, **_SIGS_OCCLUSION,
                                  **_SIGS_MATTE, **_SIGS_QUERY, **_SIGS_CERTAIN,
                                  **_SIGS_TILE_LISTS, **_SIGS_RESIZE}.items():
            if "RT_HIP_LIB" in os.environ and not hasattr(handle, name):
                continue  # an older experiment build (tools/ab_variants.py)
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


_fast = False


def fastcall():
    """The CPython binding of rt_update_frames (build/_rt_fastcall*.so, csrc/host/rt_fastcall.c:
    the same library entry point without ctypes' per-call conversion), or None when it has
    not been built or an experiment build of the library is selected (RT_HIP_LIB: the binding
    links the in-tree librt_hip.so)."""
    global _fast
    if _fast is False:
        _fast = None
        if "RT_HIP_LIB" not in os.environ:
            import importlib.machinery
            import importlib.util
            import sysconfig
            path = PKG_ROOT / "build" / ("_rt_fastcall" + sysconfig.get_config_var("EXT_SUFFIX"))
            if path.exists():
                lib()                      # (the library first: the same mapping)
                loader = importlib.machinery.ExtensionFileLoader("_rt_fastcall", str(path))
                spec = importlib.util.spec_from_file_location("_rt_fastcall", path,
                                                              loader=loader)
                mod = importlib.util.module_from_spec(spec)
                loader.exec_module(mod)
                _fast = mod
    return _fast


def exported_symbols() -> list[str]:
    return list(_SIGS)


def chain_parts_symbols() -> list[str]:
    return list(_SIGS_CHAIN_PARTS)


def occlusion_symbols() -> list[str]:
    return list(_SIGS_OCCLUSION)


def certain_symbols() -> list[str]:
    return list(_SIGS_CERTAIN)


def tile_lists_symbols() -> list[str]:
    return list(_SIGS_TILE_LISTS)


def selftest_roots_symbols() -> list[str]:
    return list(_SIGS_SELFTEST_ROOTS)


def aov_symbols() -> list[str]:
    return list(_SIGS_AOV)


def denoise_symbols() -> list[str]:
    return list(_SIGS_DENOISE)


def reproject_symbols() -> list[str]:
    return list(_SIGS_REPROJECT)


def resize_symbols() -> list[str]:
    return list(_SIGS_RESIZE)


def variance_symbols() -> list[str]:
    return list(_SIGS_VARIANCE)


def adaptive_symbols() -> list[str]:
    return list(_SIGS_ADAPTIVE)


def converge_symbols() -> list[str]:
    return list(_SIGS_CONVERGE)


def progress_symbols() -> list[str]:
    return list(_SIGS_PROGRESS)


def edit_symbols() -> list[str]:
    return list(_SIGS_EDIT)


def matte_symbols() -> list[str]:
    return list(_SIGS_MATTE)


def query_symbols() -> list[str]:
    return list(_SIGS_QUERY)


def check(status: int, func: str) -> None:
    if status != 0:
        msg = lib().rt_last_error()
        raise RtError(status, func, msg.decode() if msg else "")


def call(func: str, *args) -> None:
    check(getattr(lib(), func)(*args), func)
