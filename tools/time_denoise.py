"""Time of rt_denoise at K3's shape (1920x1080, the 500-sphere bench scene, guides from
rt_trace_aov, a 1-spp accumulator as input) in one process with two yardsticks: the 68 bytes
per pixel every iteration must move (16 colour in, 16 colour out, 16 hit, 16 normal, 4 id) at
8 TB/s, and one rt_update dispatch (at max_depth 1, as tools/time_aov.py, and at the default
depth).  Per repetition every configuration is warmed up and then timed with device events
around CALLS back-to-back calls through the C entry point with prebuilt arguments; the
repetitions alternate the configurations.  A configuration is a route ("auto": the library's
choice; "direct": every step without LDS, through RT_DENOISE_ROUTE) and a number of iterations
1..ITER; iteration i alone (tap spacing 1 << i) is the call of i + 1 iterations minus the call
of i iterations of the same repetition.  Prints one JSON line: per configuration the median,
min and max over the repetitions in microseconds, per iteration also the share of its floor
(floor / time) and the bytes per second that is, and the 5-iteration call in update dispatches.
usage: python tools/time_denoise.py [--calls 50] [--reps 9] [--iterations 5]
[--routes auto,direct]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "gpu-ray-tracing_amd"), str(ROOT)]
import torch

import gpu_ray_tracing as rt
from gpu_ray_tracing import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iterations", type=int, default=5)
ap.add_argument("--routes", default="auto,direct")
args = ap.parse_args()

W, H, NSPH = 1920, 1080, 500
BYTES_PER_PIXEL, PEAK = 68, 8e12
FLOOR_US = BYTES_PER_PIXEL * W * H / PEAK * 1e6
scene = rt.synthetic_scene(NSPH)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
cams = {"rt_update_depth1": rt.CameraSettings(max_depth=1, samples_per_pixel=65536),
        "rt_update_default_depth": rt.CameraSettings(samples_per_pixel=65536)}
cam = rt.SceneCamera.from_settings(cams["rt_update_default_depth"], W, H, 0.5)
a, b = pipe.new_image(W, H), pipe.new_image(W, H)
src = pipe.new_image(W, H)
pipe.update(a, src, W, H, cam, scene)                      # the 1-spp accumulator
guides = pipe.trace_aov(W, H, cam, scene, planes=("sphere_id", "hit", "normal"))
dst, scratch = torch.empty_like(src), torch.empty_like(src)
torch.cuda.synchronize()


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def denoise_call(route, iterations):
    params = _lib.DenoiseParamsC()
    L.rt_denoise_params_default(ctypes.byref(params))
    params.iterations = iterations
    argv = (pipe._ctx, P(src), P(dst), P(scratch), W, H, P(guides["hit"]), P(guides["normal"]),
            P(guides["sphere_id"]), ctypes.byref(params), stream)

    def run(_k):
        return L.rt_denoise(*argv)
    run.keep = params
    run.route = route
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
    run.route = None
    return run


ROUTES = args.routes.split(",")
CONFIGS = {f"{r}_{k}": denoise_call(r, k) for r in ROUTES for k in range(1, args.iterations + 1)}
CONFIGS.update({name: update_call(s) for name, s in cams.items()})
st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, fn in CONFIGS.items():
        os.environ.pop("RT_DENOISE_ROUTE", None)
        if fn.route not in (None, "auto"):
            os.environ["RT_DENOISE_ROUTE"] = fn.route
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
os.environ.pop("RT_DENOISE_ROUTE", None)


def stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
            "max_us": round(max(t), 2)}


out = {"shape": f"{W}x{H}, {NSPH} spheres", "calls": args.calls, "reps": args.reps,
       "floor": f"{BYTES_PER_PIXEL} B/pixel at {PEAK / 1e12:g} TB/s", "floor_us": round(FLOOR_US, 2)}
for name in cams:
    out[name] = stats(times[name])
unit = out["rt_update_depth1"]["median_us"]
unit_full = out["rt_update_default_depth"]["median_us"]
for r in ROUTES:
    res = {}
    for k in range(1, args.iterations + 1):
        alone = [t - (times[f"{r}_{k - 1}"][j] if k > 1 else 0.0)
                 for j, t in enumerate(times[f"{r}_{k}"])]
        s = stats(alone)
        s["share_of_floor"] = round(FLOOR_US / s["median_us"], 3)
        s["tb_per_s"] = round(BYTES_PER_PIXEL * W * H / s["median_us"] / 1e6, 2)
        res[f"step_{1 << (k - 1)}"] = s
        res[f"call_{k}_iterations"] = stats(times[f"{r}_{k}"])
    whole = res[f"call_{args.iterations}_iterations"]["median_us"]
    res["call_in_updates_depth1"] = round(whole / unit, 2)
    res["call_in_updates_default_depth"] = round(whole / unit_full, 2)
    out[r] = res
print(json.dumps(out))
