"""MI355X-native per-pixel ray tracer (Sur091/GPU-Ray-Tracing hot path, rebuilt for gfx950).

Python surface over librt_hip.so (include/rt_abi.h).  Names follow the reference crate
``gpu_ray_tracing`` (Cargo.toml:2): camera (src/camera.rs), scene (src/scene/sphere.rs),
compute_shader (the plugin in src/lib.rs).  The HIP library is the only compute path:
importing this package does not load it; the first call does, and raises if it is absent.
"""
from . import _lib
from .camera import CameraSettings, SceneCamera
from . import image_io
from .compute_shader import (ADAPTIVE_DEFAULTS, DENOISE_DEFAULTS, EDIT_DEFAULTS, GUIDED_DEFAULTS, REPROJECT_DEFAULTS,
                             RESIZE_FILL_NEAREST, RESIZE_FILL_NONE, RT_STRIPE_ROWS,
                             ComputeShaderImages, ComputeShaderNode,
                             ComputeShaderPipeline, chain_schedule, edit_plan, partition_bands,
                             reproject_basis, srgb_thresholds,
                             stripe_band_set, stripe_local_rows)
from .scene import (SCENE_DEFAULT, SCENE_N, SCENE_THREE, SphereCollection,
                    create_default_spheres, frame_seeds, synthetic_scene, three_spheres)

RtError = _lib.RtError
# first-hit G-buffer (include/rt_aov.h): the plane names of ComputeShaderPipeline.trace_aov
# and the sphere_id of a miss (-1 as the plane's int32)
AOV_PLANES = _lib.AOV_PLANES
RT_AOV_MISS = _lib.RT_AOV_MISS
# the denoiser (include/rt_denoise.h): ComputeShaderPipeline.denoise's default parameters
RT_DENOISE_MAX_ITERATIONS = _lib.RT_DENOISE_MAX_ITERATIONS
# moments and the variance-guided filter (include/rt_variance.h)
RT_VARIANCE_MAX_ITERATIONS = _lib.RT_VARIANCE_MAX_ITERATIONS
# scene edits (include/rt_scene_edit.h): edit_plan and ComputeShaderPipeline.carry_edit
RT_EDIT_NONE = _lib.RT_EDIT_NONE
RT_EDIT_MOVED = _lib.RT_EDIT_MOVED
RT_EDIT_MAX_BALLS = _lib.RT_EDIT_MAX_BALLS
# coverage mattes (include/rt_matte.h): ComputeShaderPipeline.new_matte / matte_frames / matte_resolve
RT_MATTE_SLOTS = _lib.RT_MATTE_SLOTS
# ray queries (include/rt_query.h): ComputeShaderPipeline.cast_rays / occluded / cast_ray; the
# names of cast_rays' route counters, in order
QUERY_ROUTES = _lib.QUERY_ROUTES

__all__ = [
    "CameraSettings", "SceneCamera", "ComputeShaderPipeline", "ComputeShaderImages",
    "ComputeShaderNode", "SphereCollection", "create_default_spheres", "synthetic_scene",
    "three_spheres", "frame_seeds", "stripe_local_rows", "RT_STRIPE_ROWS", "RtError",
    "SCENE_THREE", "SCENE_DEFAULT", "SCENE_N", "srgb_thresholds", "image_io",
    "partition_bands", "chain_schedule", "stripe_band_set", "AOV_PLANES", "RT_AOV_MISS",
    "DENOISE_DEFAULTS", "RT_DENOISE_MAX_ITERATIONS", "REPROJECT_DEFAULTS", "reproject_basis",
    "GUIDED_DEFAULTS", "RT_VARIANCE_MAX_ITERATIONS", "ADAPTIVE_DEFAULTS",
    "EDIT_DEFAULTS", "edit_plan", "RT_EDIT_NONE", "RT_EDIT_MOVED", "RT_EDIT_MAX_BALLS",
    "RT_MATTE_SLOTS", "QUERY_ROUTES", "RESIZE_FILL_NONE", "RESIZE_FILL_NEAREST",
]
