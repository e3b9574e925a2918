"""Time of rt_update_adaptive at K3's shape (1920x1080, the 500-sphere bench scene) against
rt_update on the same input in the same process, at max_depth 1 and at the default depth.  The
input is a 16-spp accumulator (16 rt_update frames), so with the default parameters a pixel is
sampled exactly where its error is above the tolerance.  Synthetic error planes (0 = converged,
+inf = active) make 100, 50, 25, 10 and 0 % of the pixels active in two layouts: `tiles` (whole
8x8 tiles active, chosen at random) and `pixels` (random pixels, and at least one in every tile,
so that every tile is partly active and no wave can skip its trace).  `real` is the plane and the
accumulator a 16-round chain of update_adaptive + moments_update + adaptive_error leaves behind.
Per repetition every configuration is warmed up and then timed with device events around CALLS
back-to-back calls through the C entry point with prebuilt arguments; the repetitions alternate
the configurations.  Per point: the median, min and max in microseconds, the active pixels and
tiles (from the call's own tile mask) and the occupancy of the active tiles; the 0 % point against
the 36 bytes per pixel it must move (16 in, 4 error, 16 out) at 8 TB/s; the all-active point's
ratio to rt_update; and the break-even active fraction of the `tiles` layout (linear between the
measured points).  Prints one JSON line (profiles/adaptive/time_adaptive.json).
usage: python tools/time_adaptive.py [--calls 50] [--reps 9]"""
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

W, H, NSPH, SPP0, ROUNDS = 1920, 1080, 500, 16, 16
TX, TY = (W + 7) // 8, (H + 7) // 8
PEAK, IDLE_BYTES = 8e12, 36
FRACTIONS = (100, 50, 25, 10, 0)
scene = rt.synthetic_scene(NSPH)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
dev = pipe.torch_device
params = _lib.AdaptiveParamsC()
L.rt_adaptive_params_default(ctypes.byref(params))
DEPTHS = {"depth1": rt.CameraSettings(max_depth=1, samples_per_pixel=65536),
          "default_depth": rt.CameraSettings(samples_per_pixel=65536)}


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def synthetic_planes():
    """{name: (H, W) float32 device plane}: +inf where a pixel is active, else 0."""
    rng = np.random.default_rng(3)
    out = {}
    for f in FRACTIONS:
        tiles = rng.random((TY, TX)) < f / 100
        whole = np.repeat(np.repeat(tiles, 8, 0), 8, 1)[:H, :W]
        px = rng.random((H, W)) < f / 100
        if 0 < f < 100:
            # one pixel of every tile active: no tile is idle (and at these fractions none is
            # full: the mask's occupancy shows it)
            ys = np.minimum(np.arange(TY)[:, None] * 8 + rng.integers(0, 8, (TY, TX)), H - 1)
            xs = np.minimum(np.arange(TX)[None, :] * 8 + rng.integers(0, 8, (TY, TX)), W - 1)
            px[ys, xs] = True
        for layout, m in (("tiles", whole), ("pixels", px)):
            if f in (0, 100) and layout == "pixels":
                continue                                     # the same plane as `tiles`
            plane = np.where(m, np.float32(np.inf), np.float32(0.0)).astype(np.float32)
            out[f"{layout}_{f}"] = torch.from_numpy(plane).to(dev)
    return out


def accumulate(cam, frames):
    """The accumulator after `frames` rt_update frames from a reset."""
    a, b = pipe.new_image(W, H), pipe.new_image(W, H)
    for k, seed in enumerate(rt.frame_seeds(5, frames)):
        c = cam.with_fields(random_seed=float(seed), camera_has_moved=1.0 if k == 0 else 0.0)
        pipe.update(a, b, W, H, c, scene)
        a, b = b, a
    return a


def real_chain(cam):
    """(accumulator, error plane) after ROUNDS rounds of the adaptive loop from a reset."""
    a, b, m = pipe.new_image(W, H), pipe.new_image(W, H), pipe.new_image(W, H)
    e = torch.full((H, W), float("inf"), dtype=torch.float32, device=dev)
    for k, seed in enumerate(rt.frame_seeds(7, ROUNDS)):
        c = cam.with_fields(random_seed=float(seed), camera_has_moved=1.0 if k == 0 else 0.0)
        pipe.update_adaptive(a, b, W, H, c, scene, e)
        pipe.moments_update(a, b, m, W, H)
        pipe.adaptive_error(b, m, W, H, out=e)
        a, b = b, a
    return a, e


def popcount(words):
    return int(np.unpackbits(words.cpu().numpy().view(np.uint8)).sum())


CONFIGS, ACTIVE = {}, {}
planes = synthetic_planes()
keep = []
for depth, settings in DEPTHS.items():
    cam = rt.SceneCamera.from_settings(settings, W, H, 0.5)
    still = cam.with_fields(camera_has_moved=0.0)
    cstill = still.to_c()
    src, dst = accumulate(cam, SPP0), pipe.new_image(W, H)
    real_src, real_err = real_chain(cam)
    keep += [cstill, src, dst, real_src, real_err]

    def update_call(src=src, dst=dst, cstill=cstill):
        argv = (pipe._ctx, P(src), P(dst), W, H, ctypes.byref(cstill), sp, n, stream)
        return lambda: L.rt_update(*argv)

    def adaptive_call(inp, err, dst=dst, cstill=cstill):
        argv = (pipe._ctx, P(inp), P(dst), P(err), None, W, H, ctypes.byref(cstill), sp, n,
                ctypes.byref(params), stream)
        return lambda: L.rt_update_adaptive(*argv)

    CONFIGS[f"{depth}/rt_update"] = update_call()
    for name, (inp, err) in {**{k: (src, v) for k, v in planes.items()},
                             "real": (real_src, real_err)}.items():
        CONFIGS[f"{depth}/{name}"] = adaptive_call(inp, err)
        words = pipe.update_adaptive(inp, dst, W, H, still, scene, err, tile_mask=True)
        torch.cuda.synchronize()
        tiles = int((words != 0).sum().item())
        px = popcount(words)
        ACTIVE[f"{depth}/{name}"] = {
            "active_pixels": px, "active_fraction": round(px / (W * H), 4),
            "active_tiles": tiles, "active_tile_fraction": round(tiles / (TX * TY), 4),
            "occupancy_of_active_tiles": round(px / (64 * tiles), 4) if tiles else 0.0}

st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, fn in CONFIGS.items():
        for _ in range(10):
            assert fn() == 0, name
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.calls):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)


def stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
            "max_us": round(max(t), 2)}


out = {"shape": f"{W}x{H}, {NSPH} spheres, {SPP0}-spp input", "calls": args.calls,
       "reps": args.reps, "params": [params.min_samples, params.abs_tolerance2,
                                     params.rel_tolerance2]}
floor_us = IDLE_BYTES * W * H / PEAK * 1e6
for depth in DEPTHS:
    res = {"rt_update": stats(times[f"{depth}/rt_update"])}
    upd = res["rt_update"]
    for name in list(planes) + ["real"]:
        s = stats(times[f"{depth}/{name}"])
        s.update(ACTIVE[f"{depth}/{name}"])
        s["over_rt_update"] = round(s["median_us"] / upd["median_us"], 3)
        res[name] = s
    idle = res["tiles_0"]
    idle["floor"] = f"{IDLE_BYTES} B/pixel at {PEAK / 1e12:g} TB/s"
    idle["floor_us"] = round(floor_us, 2)
    idle["share_of_floor"] = round(floor_us / idle["median_us"], 3)
    q = res["tiles_25"]
    res["tiles_25_faster_than_rt_update"] = bool(q["max_us"] < upd["min_us"])
    # break-even of the whole-tile layout: where the line through two neighbouring measured
    # points crosses rt_update's median
    pts = sorted((res[f"tiles_{f}"]["active_fraction"], res[f"tiles_{f}"]["median_us"])
                 for f in FRACTIONS)
    even = None
    for (f0, t0), (f1, t1) in zip(pts, pts[1:]):
        if t0 <= upd["median_us"] <= t1 and t1 > t0:
            even = round(f0 + (upd["median_us"] - t0) / (t1 - t0) * (f1 - f0), 4)
    res["break_even_active_fraction_tiles"] = even if even is not None else (
        "above 1" if pts[-1][1] < upd["median_us"] else "below the smallest point")
    out[depth] = res
print(json.dumps(out))
