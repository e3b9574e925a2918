"""Time of rt_matte_frames at K3's shape (1920x1080, the 500-sphere bench scene, the default
lens) in one process with its neighbours: 64-frame matte calls on the list route and on the
per-frame scan route (RT_MATTE_ROUTE=scan), one id-only rt_trace_aov call (the nearest capability
before the matte: one pinhole ray per pixel), rt_matte_resolve (alpha and dominant) and
rt_update_frames at max_depth 1 in 64-frame calls.  Per repetition every configuration is warmed
up and then timed with device events around CALLS back-to-back calls through the C entry points
with prebuilt arguments; the repetitions alternate the configurations.  Prints one JSON line: per
configuration the median, min and max over the repetitions of the time per frame (per call for
the one-launch configurations), the host's time to issue a call, and the matte's list statistics.
usage: python tools/time_matte.py [--calls 8] [--reps 9] [--scan culled|exhaustive]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "gpu-ray-tracing_amd"), str(ROOT)]
import numpy as np
import torch

import gpu_ray_tracing as rt
from gpu_ray_tracing import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=8)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scan", default="culled", choices=["culled", "exhaustive"])
args = ap.parse_args()

W, H, NSPH, FRAMES = 1920, 1080, 500, 64
scene = rt.synthetic_scene(NSPH)
cam = rt.SceneCamera.from_settings(rt.CameraSettings(max_depth=1, samples_per_pixel=1 << 24),
                                   W, H, 0.5)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_scan_mode(args.scan)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
seeds = np.ascontiguousarray(rt.frame_seeds(11, FRAMES), np.float32)
pseeds = ctypes.c_void_p(seeds.ctypes.data)
camc = cam.to_c()
still = cam.with_fields(camera_has_moved=0.0).to_c()
pstill = ctypes.byref(still)

os.environ.pop("RT_MATTE_ROUTE", None)
matte = pipe.matte_frames(pipe.new_matte(W, H), W, H, cam, scene, seeds)
info = pipe.matte_info()
mplanes = _lib.MattePlanesC(*[matte[k].data_ptr() for k in _lib.MATTE_PLANES])
pm = ctypes.byref(mplanes)
alpha = torch.empty((H, W), dtype=torch.float32, device=pipe.torch_device)
dominant = torch.empty((H, W), dtype=torch.int32, device=pipe.torch_device)
selected = (ctypes.c_uint32 * 3)(1, 2, 0xFFFFFFFF)
ids = torch.empty((H, W), dtype=torch.int32, device=pipe.torch_device)
aov = _lib.AovPlanesC()
aov.sphere_id = ids.data_ptr()
paov = ctypes.byref(aov)
a, b = pipe.new_image(W, H), pipe.new_image(W, H)
pipe.update_frames(a, b, W, H, cam, scene, seeds)
pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
newest = ctypes.c_int(-1)
torch.cuda.synchronize()


def matte_call(route):
    def run(_k):
        return L.rt_matte_frames(pipe._ctx, pm, W, H, pstill, sp, n, pseeds, FRAMES, stream)

    def enter():
        if route == "scan":
            os.environ["RT_MATTE_ROUTE"] = "scan"
        else:
            os.environ.pop("RT_MATTE_ROUTE", None)
    run.enter = enter
    return run


def aov_call(_k):
    return L.rt_trace_aov(pipe._ctx, paov, W, H, ctypes.byref(camc), sp, n, stream)


def resolve_call(_k):
    return L.rt_matte_resolve(pipe._ctx, pm, W * H, selected, 3, alpha.data_ptr(),
                              dominant.data_ptr(), stream)


def update_call(_k):
    return L.rt_update_frames(pipe._ctx, pa, pb, W, H, 0, 1, pstill, sp, n, FRAMES, pseeds, stream,
                              ctypes.byref(newest))


# name: (call, frames per call)
CONFIGS = {
    "matte_list": (matte_call("list"), FRAMES),
    "matte_scan": (matte_call("scan"), FRAMES),
    "aov_sphere_id": (aov_call, 1),
    "matte_resolve": (resolve_call, 1),
    "update_frames_depth1": (update_call, FRAMES),
}
st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
issue = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, (fn, per) in CONFIGS.items():
        getattr(fn, "enter", lambda: None)()
        calls = args.calls if per > 1 else args.calls * 16
        for k in range(2):
            assert fn(k) == 0, name
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        for k in range(calls):
            fn(k)
        t1 = time.perf_counter()
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / (calls * per))
        issue[name].append((t1 - t0) * 1e6 / calls)
os.environ.pop("RT_MATTE_ROUTE", None)
out = {"shape": f"{W}x{H}, {NSPH} spheres, default lens", "scan": args.scan,
       "frames_per_call": FRAMES, "calls": args.calls, "reps": args.reps, "matte_info": info,
       "update_kernel": pipe.last_launch_info()["kernel_name"],
       "unit": "us per frame (aov_sphere_id, matte_resolve: per call)"}
for name in CONFIGS:
    t = times[name]
    out[name] = {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
                 "max_us": round(max(t), 2),
                 "host_issue_us": round(statistics.median(issue[name]), 2)}
ml, ao, up = out["matte_list"], out["aov_sphere_id"], out["update_frames_depth1"]
out["list_cheaper_than_aov_ranges_apart"] = ml["max_us"] < ao["min_us"]
out["matte_list_over_update_frame"] = round(ml["median_us"] / up["median_us"], 3)
print(json.dumps(out))
