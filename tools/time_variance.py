"""Time of rt_moments_update and rt_variance_filter at K3's shape (1920x1080, the 500-sphere
bench scene, guides from rt_trace_aov, a 5-spp accumulator and its moments as input) in one
process with their yardsticks: rt_moments_update against the 64 bytes per pixel it must move
(16 in, 16 out, 16 moments read, 16 moments written) at 8 TB/s and against one rt_update dispatch
(at max_depth 1 and at the default depth); rt_variance_filter against rt_denoise, the fixed-sigma
filter, with the same number of iterations, and per iteration against the 76 bytes per pixel an
iteration must move (rt_denoise's 68 and 4 of variance in, 4 out).  Per repetition every
configuration is warmed up and then timed with device events around CALLS back-to-back calls
through the C entry point with prebuilt arguments; the repetitions alternate the configurations.
Iteration i alone (tap spacing 1 << i) is the call of i + 1 iterations minus the call of i
iterations of the same repetition.  Back-to-back calls of rt_moments_update find their three
images (100 MB) in the Infinity Cache, as DESIGN.md §4.8 notes for rt_reproject.  Prints one JSON
line: per configuration the median, min and max over the repetitions in microseconds.
usage: python tools/time_variance.py [--calls 50] [--reps 9] [--iterations 5]"""
import argparse
import ctypes
import json
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
args = ap.parse_args()

W, H, NSPH, FRAMES = 1920, 1080, 500, 5
PEAK = 8e12
MOMENTS_BYTES, FILTER_BYTES = 64, 76
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
prev, src, moments = pipe.new_image(W, H), pipe.new_image(W, H), pipe.new_image(W, H)
for k, seed in enumerate(rt.frame_seeds(5, FRAMES)):       # the 5-spp accumulator and its moments
    c = cam.with_fields(random_seed=float(seed), camera_has_moved=1.0 if k == 0 else 0.0)
    pipe.update(prev, src, W, H, c, scene)
    pipe.moments_update(prev, src, moments, W, H)
    if k + 1 < FRAMES:
        prev, src = src, prev
guides = pipe.trace_aov(W, H, cam, scene, planes=("sphere_id", "hit", "normal"))
dst, scratch = torch.empty_like(src), torch.empty_like(src)
variance = torch.empty((H, W), dtype=torch.float32, device=pipe.torch_device)
variance_scratch = torch.empty_like(variance)
timed_moments = moments.clone()
torch.cuda.synchronize()


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def moments_call():
    argv = (pipe._ctx, P(prev), P(src), P(timed_moments), W, H, stream)

    def run(_k):
        return L.rt_moments_update(*argv)
    return run


def guided_call(iterations):
    params = _lib.VarianceFilterParamsC()
    L.rt_variance_filter_params_default(ctypes.byref(params))
    params.iterations = iterations
    argv = (pipe._ctx, P(src), P(dst), P(scratch), P(moments), P(variance), P(variance_scratch),
            W, H, P(guides["hit"]), P(guides["normal"]), P(guides["sphere_id"]),
            ctypes.byref(params), stream)

    def run(_k):
        return L.rt_variance_filter(*argv)
    run.keep = params
    return run


def denoise_call(iterations):
    params = _lib.DenoiseParamsC()
    L.rt_denoise_params_default(ctypes.byref(params))
    params.iterations = iterations
    argv = (pipe._ctx, P(src), P(dst), P(scratch), W, H, P(guides["hit"]), P(guides["normal"]),
            P(guides["sphere_id"]), ctypes.byref(params), stream)

    def run(_k):
        return L.rt_denoise(*argv)
    run.keep = params
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


ITER = range(1, args.iterations + 1)
CONFIGS = {"rt_moments_update": moments_call()}
for k in ITER:
    CONFIGS[f"guided_{k}"] = guided_call(k)
    CONFIGS[f"denoise_{k}"] = denoise_call(k)
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


def floor_us(bytes_per_pixel):
    return bytes_per_pixel * W * H / PEAK * 1e6


out = {"shape": f"{W}x{H}, {NSPH} spheres, {FRAMES} spp", "calls": args.calls, "reps": args.reps}
for name in cams:
    out[name] = stats(times[name])
m = stats(times["rt_moments_update"])
m["floor"] = f"{MOMENTS_BYTES} B/pixel at {PEAK / 1e12:g} TB/s"
m["floor_us"] = round(floor_us(MOMENTS_BYTES), 2)
m["share_of_floor"] = round(floor_us(MOMENTS_BYTES) / m["median_us"], 3)
m["tb_per_s"] = round(MOMENTS_BYTES * W * H / m["median_us"] / 1e6, 2)
m["in_updates_depth1"] = round(m["median_us"] / out["rt_update_depth1"]["median_us"], 3)
m["in_updates_default_depth"] = round(m["median_us"] / out["rt_update_default_depth"]["median_us"], 3)
out["rt_moments_update"] = m
for kind, bpp in (("guided", FILTER_BYTES), ("denoise", 68)):
    res = {"floor": f"{bpp} B/pixel at {PEAK / 1e12:g} TB/s", "floor_us": round(floor_us(bpp), 2)}
    for k in ITER:
        alone = [t - (times[f"{kind}_{k - 1}"][j] if k > 1 else 0.0)
                 for j, t in enumerate(times[f"{kind}_{k}"])]
        s = stats(alone)
        s["share_of_floor"] = round(floor_us(bpp) / s["median_us"], 3)
        res[f"step_{1 << (k - 1)}"] = s
        res[f"call_{k}_iterations"] = stats(times[f"{kind}_{k}"])
    out[kind] = res
ratio = {f"step_{1 << (k - 1)}": round(out["guided"][f"step_{1 << (k - 1)}"]["median_us"]
                                       / out["denoise"][f"step_{1 << (k - 1)}"]["median_us"], 3)
         for k in ITER}
ratio["call"] = round(out["guided"][f"call_{args.iterations}_iterations"]["median_us"]
                      / out["denoise"][f"call_{args.iterations}_iterations"]["median_us"], 3)
out["guided_over_denoise"] = ratio
out["guided_call_in_updates_default_depth"] = round(
    out["guided"][f"call_{args.iterations}_iterations"]["median_us"]
    / out["rt_update_default_depth"]["median_us"], 2)
print(json.dumps(out))
