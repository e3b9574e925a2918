"""Time of rt_reproject at K3's shape (1920x1080, the 500-sphere bench scene) in one process with
two yardsticks: the bytes a pixel is expected to move at 8 TB/s (current planes 36 B, plus 16 B
with the material plane; previous planes and accumulator about 36 B; 16 B out) and one rt_update
dispatch (at max_depth 1, as tools/time_denoise.py, and at the default depth).  The previous view
is the default camera with a 16-sample accumulator, the current view has look_at moved by
(0.3, 0.1, 0); the planes of both come from rt_trace_aov.  Per repetition every configuration is
warmed up and then timed with device events around CALLS back-to-back calls through the C entry
point with prebuilt arguments; the repetitions alternate the configurations.  Configurations:
"lambertian" (the default: the material plane is read, non-Lambertian pixels restart), "all"
(lambertian_only 0) and "identity" (the current view is the previous one, lambertian_only 1).
Prints one JSON line: per configuration the median, min and max over the repetitions in
microseconds, the share of its floor (floor / time), the bytes per second that is and the call in
update dispatches, and the share of pixels that received history.
usage: python tools/time_reproject.py [--calls 50] [--reps 9]"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "gpu-ray-tracing_amd"), str(ROOT)]
import numpy as np
import torch

import gpu_ray_tracing as rt
from gpu_ray_tracing import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

W, H, NSPH, HISTORY = 1920, 1080, 500, 16
PEAK = 8e12
BYTES = {"lambertian": 36 + 16 + 36 + 16, "all": 36 + 36 + 16, "identity": 36 + 16 + 36 + 16}
scene = rt.synthetic_scene(NSPH)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
cams = {"rt_update_depth1": rt.CameraSettings(max_depth=1, samples_per_pixel=65536),
        "rt_update_default_depth": rt.CameraSettings(samples_per_pixel=65536)}
prev_cam = rt.SceneCamera.from_settings(cams["rt_update_default_depth"], W, H, 0.5)
cur_cam = rt.SceneCamera.from_settings(
    rt.CameraSettings(samples_per_pixel=65536, look_at=(0.3, 0.1, 0.0)), W, H, 0.5)
a, b = pipe.new_image(W, H), pipe.new_image(W, H)
images = (a, b)
newest = pipe.update_frames(a, b, W, H, prev_cam, scene,
                            np.array(rt.frame_seeds(3, HISTORY), np.float32))
prev = images[newest].clone()                              # the 16-sample accumulator
prev_guides = pipe.trace_aov(W, H, prev_cam, scene)
guides = pipe.trace_aov(W, H, cur_cam, scene)
dst = torch.empty_like(prev)
torch.cuda.synchronize()


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def reproject_call(cur, lamb):
    params = _lib.ReprojectParamsC()
    L.rt_reproject_params_default(ctypes.byref(params))
    params.lambertian_only = lamb
    planes = _lib.ReprojectPlanesC(prev_guides["sphere_id"].data_ptr(),
                                   prev_guides["hit"].data_ptr(), cur["sphere_id"].data_ptr(),
                                   cur["hit"].data_ptr(), cur["normal"].data_ptr(),
                                   cur["material"].data_ptr() if lamb else None)
    cam = prev_cam.to_c()
    argv = (pipe._ctx, P(prev), P(dst), W, H, ctypes.byref(cam), ctypes.byref(planes),
            ctypes.byref(params), stream)

    def run(_k):
        return L.rt_reproject(*argv)
    run.keep = (params, planes, cam)
    return run


def update_call(settings):
    c = rt.SceneCamera.from_settings(settings, W, H, 0.5)
    pipe.update(a, b, W, H, c, scene)
    still = c.with_fields(camera_has_moved=0.0).to_c()
    pa, pb, pstill = P(a), P(b), ctypes.byref(still)

    def run(k):
        # ping-pong: out of one call is the in of the next (b holds the newest image first)
        i, o = (pb, pa) if k % 2 == 0 else (pa, pb)
        return L.rt_update(pipe._ctx, i, o, W, H, pstill, sp, n, stream)
    run.keep = still
    return run


CONFIGS = {"lambertian": reproject_call(guides, 1), "all": reproject_call(guides, 0),
           "identity": reproject_call(prev_guides, 1)}
history = {}
for name, fn in CONFIGS.items():
    assert fn(0) == 0, name
    torch.cuda.synchronize()
    history[name] = round(float((dst[..., 3] > 0).float().mean()), 4)
CONFIGS.update({name: update_call(s) for name, s in cams.items()})
st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, fn in CONFIGS.items():
        for k in range(10):
            assert fn(k) == 0, name
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for k in range(args.calls):
            fn(k)
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)


def stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
            "max_us": round(max(t), 2)}


out = {"shape": f"{W}x{H}, {NSPH} spheres", "calls": args.calls, "reps": args.reps,
       "history_samples": HISTORY, "peak": f"{PEAK / 1e12:g} TB/s"}
for name in cams:
    out[name] = stats(times[name])
unit = out["rt_update_depth1"]["median_us"]
unit_full = out["rt_update_default_depth"]["median_us"]
for name, nbytes in BYTES.items():
    s = stats(times[name])
    floor_us = nbytes * W * H / PEAK * 1e6
    s["bytes_per_pixel"] = nbytes
    s["floor_us"] = round(floor_us, 2)
    s["share_of_floor"] = round(floor_us / s["median_us"], 3)
    s["tb_per_s"] = round(nbytes * W * H / s["median_us"] / 1e6, 2)
    s["call_in_updates_depth1"] = round(s["median_us"] / unit, 2)
    s["call_in_updates_default_depth"] = round(s["median_us"] / unit_full, 2)
    s["pixels_with_history"] = history[name]
    out[name] = s
print(json.dumps(out))
