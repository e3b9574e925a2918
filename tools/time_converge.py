"""Time of rt_converge_frames at K3's shape (1920x1080, the 500-sphere bench scene) against the
three-call loop it fuses (rt_adaptive_error was already applied; per round rt_update_adaptive,
rt_moments_update, rt_adaptive_error) on the same input in the same process, at max_depth 1 and at
the default depth, with the default parameters.

`real` is tools/time_adaptive.py's state: the accumulator, moments and error plane that 16 rounds
of the three calls leave from a reset (16 spp everywhere: min_samples is 16).  From it, FRAMES
more rounds are timed both ways: one rt_converge_frames call, and FRAMES rounds of the three calls
back to back.  Both start from a fresh copy of the state (copied outside the timed region), and
the tool checks once that they leave the same bits.  The synthetic points run through the fused
call only: the 16-spp accumulator with moments that keep a pixel idle (variance 0) or active
(variance 1e6 over a history too long for FRAMES samples to move) in time_adaptive's layouts —
`tiles` (whole 8x8 tiles at random: 100, 25, 10 and 0 %) and `pixels` (25 % random pixels, at
least one in every tile).  The 0 % call is set against 64 bytes per pixel at 8 TB/s (a tile that
changes nothing is loaded, 32 bytes per pixel, and not stored).

Per repetition every configuration is warmed up once and then timed CALLS times, each time with
device events around the back-to-back calls of one FRAMES-round sequence through the C entry
points with prebuilt arguments; the repetitions alternate the configurations.  Per point: the
median, min and max in microseconds per sequence and per frame, and the samples taken.

Each depth runs in a child process of its own under a time limit (--limit seconds); after a child
that fails or runs out of time no further one is started.  Prints one JSON line
(profiles/converge/time_converge.json).
usage: python tools/time_converge.py [--calls 5] [--reps 9] [--limit 240]"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
DEPTH_NAMES = ("depth1", "default_depth")

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--step", choices=DEPTH_NAMES, help="(internal) time one depth in this process")
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpu_ray_tracing as rt  # noqa: E402
from gpu_ray_tracing import _lib  # noqa: E402

W, H, NSPH, ROUNDS, FRAMES, MIN_HISTORY = 1920, 1080, 500, 16, 16, 4
TX, TY = (W + 7) // 8, (H + 7) // 8
PEAK, IDLE_BYTES = 8e12, 64
SYNTHETIC = (("tiles", 100), ("tiles", 25), ("tiles", 10), ("tiles", 0), ("pixels", 25))
IDLE_M, ACTIVE_M = (0.5, 0.25, 0.0, 16.0), (0.0, 1e6, 0.0, 1e6)
scene = rt.synthetic_scene(NSPH)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_spheres(scene)
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
dev = pipe.torch_device
params = _lib.AdaptiveParamsC()
L.rt_adaptive_params_default(ctypes.byref(params))
settings = {"depth1": rt.CameraSettings(max_depth=1, samples_per_pixel=65536),
            "default_depth": rt.CameraSettings(samples_per_pixel=65536)}[args.step]
cam = rt.SceneCamera.from_settings(settings, W, H, 0.5)
still = cam.with_fields(camera_has_moved=0.0)
seeds = np.ascontiguousarray(rt.frame_seeds(9, FRAMES), np.float32)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def synthetic_moments():
    """{name: (H, W, 4) float32 device moments}: ACTIVE_M where a pixel is active, else IDLE_M."""
    rng = np.random.default_rng(3)
    out = {}
    for layout, f in SYNTHETIC:
        if layout == "tiles":
            tiles = rng.random((TY, TX)) < f / 100
            m = np.repeat(np.repeat(tiles, 8, 0), 8, 1)[:H, :W]
        else:
            m = rng.random((H, W)) < f / 100
            ys = np.minimum(np.arange(TY)[:, None] * 8 + rng.integers(0, 8, (TY, TX)), H - 1)
            xs = np.minimum(np.arange(TX)[None, :] * 8 + rng.integers(0, 8, (TY, TX)), W - 1)
            m[ys, xs] = True                                 # no tile is idle
        mom = np.where(m[..., None], np.float32(ACTIVE_M), np.float32(IDLE_M)).astype(np.float32)
        out[f"{layout}_{f}"] = torch.from_numpy(mom).to(dev)
    return out


def real_chain():
    """(accumulator, moments, error plane) after ROUNDS rounds of the three calls from a reset."""
    a, b, m = pipe.new_image(W, H), pipe.new_image(W, H), pipe.new_image(W, H)
    m.zero_()
    e = torch.full((H, W), float("inf"), dtype=torch.float32, device=dev)
    for k, seed in enumerate(rt.frame_seeds(7, ROUNDS)):
        c = cam.with_fields(random_seed=float(seed), camera_has_moved=1.0 if k == 0 else 0.0)
        pipe.update_adaptive(a, b, W, H, c, scene, e)
        pipe.moments_update(a, b, m, W, H)
        pipe.adaptive_error(b, m, W, H, out=e)
        a, b = b, a
    return a, m, e


src, src_m, src_e = real_chain()
work, work_b, work_m = pipe.new_image(W, H), pipe.new_image(W, H), pipe.new_image(W, H)
work_e = torch.empty((H, W), dtype=torch.float32, device=dev)
taken = torch.zeros((TY * TX,), dtype=torch.int32, device=dev)
cams = [still.with_fields(random_seed=float(s)).to_c() for s in seeds]
cstill = still.to_c()


def restore_from(mom):
    def restore():
        work.copy_(src)
        work_m.copy_(mom)
        work_e.copy_(src_e)
    return restore


def fused_call(samples=None):
    argv = (pipe._ctx, P(work), P(work_m), None, None, P(samples) if samples is not None else None,
            W, H, ctypes.byref(cstill), sp, n, FRAMES, ctypes.c_void_p(seeds.ctypes.data),
            ctypes.byref(params), MIN_HISTORY, stream)
    return lambda: L.rt_converge_frames(*argv)


def loop_calls():
    """FRAMES rounds of the three calls from (work, work_m, work_e), ping-ponging into work_b."""
    img = [work, work_b]
    calls = []
    for f in range(FRAMES):
        a, b = img[f & 1], img[1 - (f & 1)]
        calls.append((L.rt_update_adaptive, (pipe._ctx, P(a), P(b), P(work_e), None, W, H,
                                             ctypes.byref(cams[f]), sp, n, ctypes.byref(params),
                                             stream)))
        calls.append((L.rt_moments_update, (pipe._ctx, P(a), P(b), P(work_m), W, H, stream)))
        calls.append((L.rt_adaptive_error, (pipe._ctx, P(b), P(work_m), P(work_e), W, H,
                                            MIN_HISTORY, stream)))

    def run():
        status = 0
        for fn, argv in calls:
            status |= fn(*argv)
        return status
    return run, img[FRAMES & 1]


loop, loop_result = loop_calls()
CONFIGS = {"real/three_calls": (restore_from(src_m), loop),
           "real/fused": (restore_from(src_m), fused_call())}
synthetic = synthetic_moments()
for name, mom in synthetic.items():
    CONFIGS[f"{name}/fused"] = (restore_from(mom), fused_call())

# once, untimed: the two ways leave the same bits, and the samples each point takes
restore_from(src_m)()
assert loop() == 0
torch.cuda.synchronize()
want_img, want_m = loop_result.clone(), work_m.clone()
SAMPLES = {}
for name, mom in {"real": src_m, **synthetic}.items():
    restore_from(mom)()
    assert fused_call(taken)() == 0
    torch.cuda.synchronize()
    t = taken.cpu().numpy().astype(np.int64)
    SAMPLES[name] = {"samples": int(t.sum()), "active_tiles": int((t != 0).sum()),
                     "mean_active_fraction": round(float(t.sum()) / (FRAMES * W * H), 4)}
    if name == "real":
        same = (torch.equal(work.view(torch.int32), want_img.view(torch.int32))
                and torch.equal(work_m.view(torch.int32), want_m.view(torch.int32)))
        assert same, "the fused call and the three-call loop leave different bits"

st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, (restore, fn) in CONFIGS.items():
        restore()
        assert fn() == 0, name
        total = 0.0
        for _ in range(args.calls):
            restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1) * 1e3
        times[name].append(total / args.calls)


def stats(t):
    return {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
            "max_us": round(max(t), 2),
            "median_us_per_frame": round(statistics.median(t) / FRAMES, 2)}


res = {"common": {"shape": f"{W}x{H}, {NSPH} spheres, {ROUNDS}-spp input, {FRAMES} frames",
                  "calls": args.calls, "reps": args.reps, "min_history": MIN_HISTORY,
                  "params": [params.min_samples, params.abs_tolerance2, params.rel_tolerance2]}}
for name, t in times.items():
    point, how = name.split("/")
    res.setdefault(point, dict(SAMPLES[point]))[how] = stats(t)
real = res["real"]
real["same_bits"] = True
real["fused_over_three_calls"] = round(real["fused"]["median_us"]
                                       / real["three_calls"]["median_us"], 3)
real["ranges_apart_fused_faster"] = bool(real["fused"]["max_us"] < real["three_calls"]["min_us"])
idle = res["tiles_0"]
floor_us = IDLE_BYTES * W * H / PEAK * 1e6
idle["floor"] = f"{IDLE_BYTES} B/pixel at {PEAK / 1e12:g} TB/s"
idle["floor_us"] = round(floor_us, 2)
idle["share_of_floor"] = round(floor_us / idle["fused"]["median_us"], 3)
res["tiles_10_above_tiles_25"] = bool(res["tiles_10"]["fused"]["median_us"]
                                      > res["tiles_25"]["fused"]["median_us"])
print(json.dumps(res))
