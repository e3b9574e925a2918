"""Time of rt_trace_aov at K3's shape (1920x1080, the 500-sphere bench scene) against one
rt_update dispatch at max_depth 1 of the same tree, in one process: all four planes, sphere_id
only, hit only, and the update (one camera ray per pixel each).  Per repetition every
configuration is warmed up and then timed with device events around CALLS back-to-back calls
through the C entry points with prebuilt arguments; the repetitions alternate the
configurations.  Prints one JSON line: per configuration the median, min and max over the
repetitions of the time per call, and the host's time to issue a call (a kernel time at or
below it would be host-bound).  usage: python tools/time_aov.py [--calls 100] [--reps 9]
[--scan culled|exhaustive]"""
import argparse
import ctypes
import json
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
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scan", default="culled", choices=["culled", "exhaustive"])
args = ap.parse_args()

W, H, NSPH = 1920, 1080, 500
scene = rt.synthetic_scene(NSPH)
cam = rt.SceneCamera.from_settings(rt.CameraSettings(max_depth=1, samples_per_pixel=65536),
                                   W, H, 0.5)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_scan_mode(args.scan)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
a, b = pipe.new_image(W, H), pipe.new_image(W, H)
pipe.update(a, b, W, H, cam, scene)
still = cam.with_fields(camera_has_moved=0.0).to_c()
camc = cam.to_c()
planes = pipe.trace_aov(W, H, cam, scene)
torch.cuda.synchronize()


def planes_c(names):
    c = _lib.AovPlanesC()
    for k in names:
        setattr(c, k, planes[k].data_ptr())
    return c


def aov_call(names):
    c = planes_c(names)
    pc, pcam = ctypes.byref(c), ctypes.byref(camc)

    def run(_k):
        return L.rt_trace_aov(pipe._ctx, pc, W, H, pcam, sp, n, stream)
    run.keep = c
    return run


pa, pb, pstill = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.byref(still)


def update_call(k):
    # ping-pong: out of one call is the in of the next (b holds the newest image first)
    i, o = (pb, pa) if k % 2 == 0 else (pa, pb)
    return L.rt_update(pipe._ctx, i, o, W, H, pstill, sp, n, stream)


CONFIGS = {
    "aov_all_planes": aov_call(_lib.AOV_PLANES),
    "aov_sphere_id": aov_call(("sphere_id",)),
    "aov_hit": aov_call(("hit",)),
    "rt_update_depth1": update_call,
}
st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
issue = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, fn in CONFIGS.items():
        for k in range(10):
            assert fn(k) == 0, name
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        for k in range(args.calls):
            fn(k)
        t1 = time.perf_counter()
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        issue[name].append((t1 - t0) * 1e6 / args.calls)
out = {"shape": f"{W}x{H}, {NSPH} spheres", "scan": args.scan, "calls": args.calls,
       "reps": args.reps, "update_kernel": pipe.last_launch_info()["kernel_name"],
       "bytes_per_pixel": {"aov_all_planes": 52, "aov_sphere_id": 4, "aov_hit": 16,
                           "rt_update_depth1": 32}}
for name in CONFIGS:
    t = times[name]
    out[name] = {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
                 "max_us": round(max(t), 2),
                 "host_issue_us": round(statistics.median(issue[name]), 2)}
print(json.dumps(out))
