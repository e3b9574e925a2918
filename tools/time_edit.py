"""Time of rt_edit_carry at K3's shape (1920x1080, the 500-sphere bench scene) against rt_reproject
with the same planes in the same process, by tools/time_reproject.py's method: per repetition
every configuration is warmed up and then timed with device events around CALLS back-to-back calls
through the C entry point with prebuilt arguments; the repetitions alternate the configurations.
The edit moves one small sphere (the first of radius 0.2 the default view shows) and the radius-1
Lambertian sphere by (0.5 R, 0, 0.25 R) each: 4 balls.  The previous accumulator holds 16 samples
of the previous scene; the planes of both scenes come from rt_trace_aov, camera unmoved.
Configurations: "reproject" (rt_reproject over the edited scene's planes: what a host could do
before, wrong on the moved spheres), "carry" (rt_edit_carry with the plan), "carry_identity" (an
identity plan over the same planes: the record gather alone), "carry_32_balls" (16 small spheres
moved: the ball loop at its longest).  The expectation is rt_reproject's loads plus one 32-byte
record gather per pixel and up to 32 ball tests of scalar-cached data.
Prints one JSON line and, with --out, writes it to that file: per configuration the median, min
and max over the repetitions in microseconds, the ratio to "reproject", and the share of pixels
that received history.
usage: python tools/time_edit.py [--calls 50] [--reps 9] [--out profiles/scene_edit/time_edit.json]"""
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
ap.add_argument("--out", type=Path, default=None)
args = ap.parse_args()

W, H, NSPH, HISTORY = 1920, 1080, 500, 16
base = np.ascontiguousarray(rt.synthetic_scene(NSPH).spheres, np.float32).reshape(-1, 8)
pipe = rt.ComputeShaderPipeline(0)
L = _lib.lib()
stream = pipe._stream()
cam = rt.SceneCamera.from_settings(rt.CameraSettings(samples_per_pixel=65536), W, H, 0.5)
prev_scene = rt.SphereCollection(base)
a, b = pipe.new_image(W, H), pipe.new_image(W, H)
images = (a, b)
newest = pipe.update_frames(a, b, W, H, cam, prev_scene,
                            np.array(rt.frame_seeds(3, HISTORY), np.float32))
prev = images[newest].clone()                              # the 16-sample accumulator
prev_guides = pipe.trace_aov(W, H, cam, prev_scene)
torch.cuda.synchronize()
seen = np.unique(prev_guides["sphere_id"].cpu().numpy())
small = [int(i) for i in seen if i >= 0 and abs(base[i, 3]) < 0.5]
big = [int(i) for i in seen if i >= 0 and base[i, 3] == 1.0 and base[i, 7] < -1.0]
assert small and big, "the view shows no small or no radius-1 Lambertian sphere"


def edited(indices):
    s = base.copy()
    for i in indices:
        s[i, 0:3] += s[i, 3] * np.array([0.5, 0.0, 0.25], np.float32)
    return s


def P(t):
    return ctypes.c_void_p(t.data_ptr())


dst = torch.empty_like(prev)
keep = []


def planes_of(guides):
    return _lib.ReprojectPlanesC(prev_guides["sphere_id"].data_ptr(),
                                 prev_guides["hit"].data_ptr(), guides["sphere_id"].data_ptr(),
                                 guides["hit"].data_ptr(), guides["normal"].data_ptr(),
                                 guides["material"].data_ptr())


def reproject_call(guides):
    params = _lib.ReprojectParamsC()
    L.rt_reproject_params_default(ctypes.byref(params))
    planes, c = planes_of(guides), cam.to_c()
    argv = (pipe._ctx, P(prev), P(dst), W, H, ctypes.byref(c), ctypes.byref(planes),
            ctypes.byref(params), stream)
    keep.append((params, planes, c))
    return lambda: L.rt_reproject(*argv)


def carry_call(guides, plan):
    table, info = plan
    params = _lib.EditParamsC()
    L.rt_edit_params_default(ctypes.byref(params))
    planes, c = planes_of(guides), cam.to_c()
    dev = torch.from_numpy(table.view(np.int32).copy()).to(pipe.torch_device)
    argv = (pipe._ctx, P(prev), P(dst), W, H, ctypes.byref(c), ctypes.byref(planes), P(dev),
            info["n_records"], info["n_balls"], ctypes.byref(params), stream)
    keep.append((params, planes, c, dev))
    return lambda: L.rt_edit_carry(*argv)


two = edited([small[0], big[0]])
many = edited(small[:16])
g_two = pipe.trace_aov(W, H, cam, rt.SphereCollection(two))
g_many = pipe.trace_aov(W, H, cam, rt.SphereCollection(many))
plans = {"carry": rt.edit_plan(base, two), "carry_identity": rt.edit_plan(two, two),
         "carry_32_balls": rt.edit_plan(base, many)}
CONFIGS = {"reproject": reproject_call(g_two), "carry": carry_call(g_two, plans["carry"]),
           "carry_identity": carry_call(g_two, plans["carry_identity"]),
           "carry_32_balls": carry_call(g_many, plans["carry_32_balls"])}
history = {}
for name, fn in CONFIGS.items():
    assert fn() == 0, name
    torch.cuda.synchronize()
    history[name] = round(float((dst[..., 3] > 0).float().mean()), 4)
st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, fn in CONFIGS.items():
        for k in range(10):
            assert fn() == 0, name
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for k in range(args.calls):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)

out = {"shape": f"{W}x{H}, {NSPH} spheres", "calls": args.calls, "reps": args.reps,
       "history_samples": HISTORY, "moved": {"small": small[0], "radius_1": big[0]}}
for name, t in times.items():
    out[name] = {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
                 "max_us": round(max(t), 2), "pixels_with_history": history[name]}
    if name in plans:
        out[name]["balls"] = plans[name][1]["n_balls"]
for name in plans:
    out[name]["ratio_to_reproject"] = round(out[name]["median_us"] /
                                            out["reproject"]["median_us"], 3)
line = json.dumps(out)
print(line)
if args.out:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(line + "\n")
pipe.close()
