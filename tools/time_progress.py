"""Time of rt_progress_stats and rt_progress_run at K3's shape (1920x1080, the 500-sphere bench
scene), with the default parameters and min_history 4, on tools/time_adaptive.py's `real` state:
the accumulator and moments that 16 rounds of the three calls leave from a reset (16 spp
everywhere: min_samples is 16).

(a) `device`: rt_progress_stats (from the moments; with and without tile_active) and
    rt_adaptive_error on the same two images in the same process, each CALLS times back to back
    between device events, microseconds per call.  rt_adaptive_error reads the same 32 bytes per
    pixel and writes 4 more; it is asynchronous, so its calls queue up behind each other, while
    every rt_progress_stats call ends with a copy of the report and a wait for it.  Also the ratio
    of each to 32 bytes per pixel at 8 TB/s.
(b) `host`: the wall time of one synchronous rt_progress_stats call, which is what a check costs
    the host.
(c) `run`: rt_progress_run from the state to the goal (at most 0.1 % of the pixels active, a check
    every CHECK frames, at most MAX_FRAMES frames), against one rt_converge_frames call of the
    same frames_run and against a fixed 64-frame call, all from fresh copies of the state, wall
    time around the call and a synchronise; the tool checks once that the run and the single call
    leave the same bits.  overhead_per_check_us = (run - single call) / reports taken.

Per repetition every configuration is warmed up once and then timed; the repetitions alternate the
configurations.  Per point: the median, min and max in microseconds.

`--step kernels` is for a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/time_progress.py --step kernels; profiles/progress/kernel_stats.csv): on the depth-1 state,
TRACE_CALLS times rt_progress_stats and rt_adaptive_error in turn, nothing timed here.

Each depth runs in a child process of its own under a time limit (--limit seconds); after a child
that fails or runs out of time no further one is started.  Prints one JSON line
(profiles/progress/time_progress.json).
usage: python tools/time_progress.py [--calls 20] [--reps 9] [--limit 240]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
DEPTH_NAMES = ("depth1", "default_depth")

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--step", choices=DEPTH_NAMES + ("kernels",),
                help="(internal) time one depth in this process; kernels: the calls of a trace")
args = ap.parse_args()

if args.step is None:
    out = {}
    for depth in DEPTH_NAMES:
        try:
            r = subprocess.run([sys.executable, __file__, "--step", depth, "--calls",
                                str(args.calls), "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{depth}: no result within {args.limit} s; nothing more is started")
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"{depth}: exit status {r.returncode}; nothing more is started")
        step = json.loads(r.stdout.strip().splitlines()[-1])
        out.update(step.pop("common"))
        out[depth] = step
    print(json.dumps(out))
    sys.exit(0)

sys.path[:0] = [str(ROOT / "gpu-ray-tracing_amd"), str(ROOT)]
import ctypes      # noqa: E402
import statistics  # noqa: E402
import time        # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpu_ray_tracing as rt  # noqa: E402
from gpu_ray_tracing import _lib  # noqa: E402

W, H, NSPH, ROUNDS, MIN_HISTORY = 1920, 1080, 500, 16, 4
CHECK, MAX_FRAMES, FIXED, TRACE_CALLS = 16, 512, 64, 50
MAX_ACTIVE = W * H // 1000
TILES = ((W + 7) // 8) * ((H + 7) // 8)
PEAK, READ_BYTES = 8e12, 32
SPP = 65536
scene = rt.synthetic_scene(NSPH)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
dev = pipe.torch_device
params = _lib.AdaptiveParamsC()
L.rt_adaptive_params_default(ctypes.byref(params))
settings = {"depth1": rt.CameraSettings(max_depth=1, samples_per_pixel=SPP),
            "default_depth": rt.CameraSettings(samples_per_pixel=SPP)}[
                "depth1" if args.step == "kernels" else args.step]
cam = rt.SceneCamera.from_settings(settings, W, H, 0.5)
cstill = cam.with_fields(camera_has_moved=0.0).to_c()
seeds = np.ascontiguousarray(rt.frame_seeds(9, MAX_FRAMES), np.float32)
SEEDS = ctypes.c_void_p(seeds.ctypes.data)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def real_chain():
    """(accumulator, moments) after ROUNDS rounds of the three calls from a reset."""
    a, b, m = pipe.new_image(W, H), pipe.new_image(W, H), pipe.new_image(W, H)
    m.zero_()
    e = torch.full((H, W), float("inf"), dtype=torch.float32, device=dev)
    for k, seed in enumerate(rt.frame_seeds(7, ROUNDS)):
        c = cam.with_fields(random_seed=float(seed), camera_has_moved=1.0 if k == 0 else 0.0)
        pipe.update_adaptive(a, b, W, H, c, scene, e)
        pipe.moments_update(a, b, m, W, H)
        pipe.adaptive_error(b, m, W, H, out=e)
        a, b = b, a
    return a, m


src, src_m = real_chain()
work, work_m = pipe.new_image(W, H), pipe.new_image(W, H)
plane = torch.empty((H, W), dtype=torch.float32, device=dev)
mask = torch.empty((TILES,), dtype=torch.int64, device=dev)
report = _lib.ProgressReportC()
goal = _lib.ProgressGoalC(MAX_ACTIVE, MAX_FRAMES, CHECK)
done = ctypes.c_uint32(0)
st = torch.cuda.current_stream()


def restore():
    work.copy_(src)
    work_m.copy_(src_m)


def stats_call(with_mask):
    argv = (pipe._ctx, P(src), P(src_m), None, P(mask) if with_mask else None, W, H, SPP,
            ctypes.byref(params), MIN_HISTORY, stream, ctypes.byref(report))
    return lambda: L.rt_progress_stats(*argv)


def error_call():
    argv = (pipe._ctx, P(src), P(src_m), P(plane), W, H, MIN_HISTORY, stream)
    return lambda: L.rt_adaptive_error(*argv)


def run_call():
    argv = (pipe._ctx, P(work), P(work_m), None, W, H, ctypes.byref(cstill), sp, n, SEEDS,
            ctypes.byref(params), MIN_HISTORY, ctypes.byref(goal), stream, ctypes.byref(done),
            ctypes.byref(report))
    return lambda: L.rt_progress_run(*argv)


def converge_call(frames):
    argv = (pipe._ctx, P(work), P(work_m), None, None, None, W, H, ctypes.byref(cstill), sp, n,
            frames, SEEDS, ctypes.byref(params), MIN_HISTORY, stream)
    return lambda: L.rt_converge_frames(*argv)


def fields(r):
    return {f: getattr(r, f) for f, _ in _lib.ProgressReportC._fields_ if f != "_reserved"}


if args.step == "kernels":
    check, error = stats_call(False), error_call()
    for _ in range(TRACE_CALLS):
        assert check() == 0 and error() == 0
    torch.cuda.synchronize()
    print(json.dumps(fields(report)))
    sys.exit(0)

# once, untimed: the state's report, where the run stops, and that a single call leaves its bits
assert stats_call(True)() == 0
start = fields(report)
assert int((mask != 0).sum()) == start["active_tiles"]
restore()
assert run_call()() == 0
FRAMES_RUN, end = int(done.value), fields(report)
assert FRAMES_RUN > 0, "the state already meets the goal"
run_img, run_m = work.clone(), work_m.clone()
restore()
assert converge_call(FRAMES_RUN)() == 0
torch.cuda.synchronize()
assert (torch.equal(work.view(torch.int32), run_img.view(torch.int32))
        and torch.equal(work_m.view(torch.int32), run_m.view(torch.int32))), \
    "rt_progress_run and one rt_converge_frames call leave different bits"
REPORTS = 1 + (FRAMES_RUN + CHECK - 1) // CHECK


def device_us(fn):
    """CALLS back-to-back calls between device events, microseconds per call."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(args.calls):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.calls


def host_us(fn):
    """The median wall time of one call that returns with its result, microseconds."""
    torch.cuda.synchronize()
    t = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def wall_us(fn):
    """One call from a fresh copy of the state and a synchronise, microseconds."""
    restore()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert fn() == 0
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


CONFIGS = {"device/progress_stats": (device_us, stats_call(False)),
           "device/progress_stats_with_mask": (device_us, stats_call(True)),
           "device/adaptive_error": (device_us, error_call()),
           "host/progress_stats": (host_us, stats_call(False)),
           "run/progress_run": (wall_us, run_call()),
           "run/converge_frames_run": (wall_us, converge_call(FRAMES_RUN)),
           f"run/converge_{FIXED}": (wall_us, converge_call(FIXED))}
times = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, (how, fn) in CONFIGS.items():
        how(fn) if how is wall_us else fn()              # warm-up
        times[name].append(how(fn))


def stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
            "max_us": round(max(t), 2)}


res = {"common": {"shape": f"{W}x{H}, {NSPH} spheres, {ROUNDS}-spp input", "calls": args.calls,
                  "reps": args.reps, "min_history": MIN_HISTORY,
                  "params": [params.min_samples, params.abs_tolerance2, params.rel_tolerance2],
                  "goal": {"max_active": MAX_ACTIVE, "check_every": CHECK,
                           "max_frames": MAX_FRAMES}}}
for name, t in times.items():
    part, point = name.split("/")
    res.setdefault(part, {})[point] = stats(t)
d = res["device"]
floor_us = READ_BYTES * W * H / PEAK * 1e6
d["floor"] = f"{READ_BYTES} B/pixel at {PEAK / 1e12:g} TB/s"
d["floor_us"] = round(floor_us, 2)
for k in ("progress_stats", "progress_stats_with_mask", "adaptive_error"):
    d[k]["over_floor"] = round(d[k]["median_us"] / floor_us, 2)
ranges = sum(d[k]["max_us"] - d[k]["min_us"] for k in ("progress_stats", "adaptive_error"))
d["stats_minus_error_us"] = round(d["progress_stats"]["median_us"]
                                  - d["adaptive_error"]["median_us"], 2)
d["both_ranges_us"] = round(ranges, 2)
d["stats_within_ranges_of_error"] = bool(d["stats_minus_error_us"] <= ranges)
r = res["run"]
r.update(start=start, end=end, frames_run=FRAMES_RUN, reports=REPORTS, same_bits=True)
r["overhead_per_check_us"] = round((r["progress_run"]["median_us"]
                                    - r["converge_frames_run"]["median_us"]) / REPORTS, 2)
r[f"run_over_converge_{FIXED}"] = round(r["progress_run"]["median_us"]
                                        / r[f"converge_{FIXED}"]["median_us"], 3)
print(json.dumps(res))
