"""Time of rt_cast_rays (include/rt_query.h) at K3's shape (1920x1080, the 500-sphere bench
scene), in one process with rt_trace_aov as the yardstick:
  (a) the image's centre rays, RT_QUERY_CLOSEST with sphere_id + hit, against rt_trace_aov with
      the same two planes (the query reads 32 B of ray per pixel that the G-buffer computes);
  (b) the same rays in a fixed random permutation (incoherent waves), the same call;
  (c) 2 M segments between points on neighbouring spheres' surfaces (tmax = 1):
      RT_QUERY_OCCLUSION against RT_QUERY_CLOSEST with sphere_id only, on the same rays.  The
      early exit's rule: occlusion's median must not lie above closest's by more than closest's
      own min-max spread ("early_exit_rule_holds").
Per repetition every configuration is warmed up and then timed with device events around CALLS
back-to-back calls through the C entry point with prebuilt arguments; the repetitions alternate
the configurations.  Writes one JSON object (also printed): per configuration the median, min
and max over the repetitions of the time per call, the host's time to issue a call, and the
waves per route.  usage: python tools/time_query.py [--calls 20] [--reps 9]
[--scan culled|exhaustive] [--out profiles/query/time_query.json]"""
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
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scan", default="culled", choices=["culled", "exhaustive"])
ap.add_argument("--out", default=str(ROOT / "profiles" / "query" / "time_query.json"))
args = ap.parse_args()

W, H, NSPH, NSEG = 1920, 1080, 500, 1 << 21
scene = rt.synthetic_scene(NSPH)
cam = rt.SceneCamera.from_settings(rt.CameraSettings(max_depth=1, samples_per_pixel=65536),
                                   W, H, 0.5)
pipe = rt.ComputeShaderPipeline(0)
pipe.set_scan_mode(args.scan)
pipe.set_spheres(scene)
dev = pipe.torch_device
L = _lib.lib()
stream = pipe._stream()
sp, n = pipe._spheres(scene)
camc = cam.to_c()


def camera_rays():
    """The centre rays of every pixel, row-major, made on the device."""
    b = torch.from_numpy(np.array(cam.blob, np.float32)).to(dev)
    o, vul, pdu, pdv = b[0:3], b[4:7], b[8:11], b[12:15]
    sy = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5)[:, None, None]
    sx = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5)[None, :, None]
    pc = sy * pdv + (sx * pdu + vul)
    rays = torch.zeros((H, W, 8), dtype=torch.float32, device=dev)
    rays[..., 0:3] = o
    rays[..., 3] = float("inf")
    rays[..., 4:7] = pc - o
    return rays.reshape(-1, 8).contiguous()


def segment_rays():
    """o on one sphere's surface pushed out by 1 %, d to a point on one of its three nearest
    neighbours' surfaces, tmax = 1 (the ground is neither end)."""
    rng = np.random.default_rng(5)
    s = np.asarray(scene.spheres, np.float64)
    s = s[np.abs(s[:, 3]) < 100.0]
    dist = np.linalg.norm(s[:, None, :3] - s[None, :, :3], axis=2)
    np.fill_diagonal(dist, np.inf)
    near = np.argsort(dist, axis=1)[:, :3]

    def units(k):
        v = rng.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    i = rng.integers(0, s.shape[0], NSEG)
    j = near[i, rng.integers(0, 3, NSEG)]
    o = s[i, :3] + 1.01 * s[i, 3:4] * units(NSEG)
    target = s[j, :3] + s[j, 3:4] * units(NSEG)
    rays = np.zeros((NSEG, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = o, 1.0, target - o
    return torch.from_numpy(rays).to(dev)


RAYS = {"camera": camera_rays()}
gen = torch.Generator(device="cpu")
gen.manual_seed(7)
RAYS["permuted"] = RAYS["camera"][torch.randperm(W * H, generator=gen).to(dev)].contiguous()
RAYS["segments"] = segment_rays()
NMAX = max(r.shape[0] for r in RAYS.values())
ids = torch.empty(NMAX, dtype=torch.int32, device=dev)
hit = torch.empty((NMAX, 4), dtype=torch.float32, device=dev)
occ = torch.empty(NMAX, dtype=torch.int32, device=dev)
routes = torch.zeros(3, dtype=torch.int32, device=dev)


def query_call(rays, mode, names):
    c = _lib.QueryPlanesC()
    for k in names:
        setattr(c, k, {"sphere_id": ids, "hit": hit, "occluded": occ}[k].data_ptr())
    pc, pr, count = ctypes.byref(c), ctypes.c_void_p(rays.data_ptr()), rays.shape[0]

    def run(_k, rc=None):
        return L.rt_cast_rays(pipe._ctx, pr, count, mode, pc, sp, n, rc, stream)
    run.keep = (c, rays)
    return run


def aov_call(names):
    c = _lib.AovPlanesC()
    for k in names:
        setattr(c, k, {"sphere_id": ids, "hit": hit}[k].data_ptr())
    pc, pcam = ctypes.byref(c), ctypes.byref(camc)

    def run(_k, rc=None):
        return L.rt_trace_aov(pipe._ctx, pc, W, H, pcam, sp, n, stream)
    run.keep = c
    return run


CLOSEST, OCCLUSION = _lib.RT_QUERY_CLOSEST, _lib.RT_QUERY_OCCLUSION
CONFIGS = {
    "aov_id_hit": aov_call(("sphere_id", "hit")),
    "a_camera_closest_id_hit": query_call(RAYS["camera"], CLOSEST, ("sphere_id", "hit")),
    "b_permuted_closest_id_hit": query_call(RAYS["permuted"], CLOSEST, ("sphere_id", "hit")),
    "c_segments_closest_id": query_call(RAYS["segments"], CLOSEST, ("sphere_id",)),
    "c_segments_occlusion": query_call(RAYS["segments"], OCCLUSION, ("occluded",)),
}
st = torch.cuda.current_stream()
times = {k: [] for k in CONFIGS}
issue = {k: [] for k in CONFIGS}
for rep in range(args.reps):
    for name, fn in CONFIGS.items():
        for k in range(3):
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

out = {"shape": f"{W}x{H} camera rays, {NSEG} segments, {NSPH} spheres", "scan": args.scan,
       "calls": args.calls, "reps": args.reps}
for name, fn in CONFIGS.items():
    t = times[name]
    out[name] = {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2),
                 "max_us": round(max(t), 2),
                 "host_issue_us": round(statistics.median(issue[name]), 2)}
    if name != "aov_id_hit":
        routes.zero_()
        assert fn(0, ctypes.c_void_p(routes.data_ptr())) == 0
        torch.cuda.synchronize()
        out[name]["waves"] = dict(zip(_lib.QUERY_ROUTES, routes.cpu().tolist()))
aov = out["aov_id_hit"]["median_us"]
out["a_ratio_to_aov"] = round(out["a_camera_closest_id_hit"]["median_us"] / aov, 3)
out["b_ratio_to_aov"] = round(out["b_permuted_closest_id_hit"]["median_us"] / aov, 3)
clo, oc = out["c_segments_closest_id"], out["c_segments_occlusion"]
out["c_occlusion_to_closest"] = round(oc["median_us"] / clo["median_us"], 3)
out["c_segments_occluded"] = int(occ[:NSEG].sum().item())
out["early_exit_rule_holds"] = bool(oc["median_us"] <= clo["median_us"]
                                    + (clo["max_us"] - clo["min_us"]))
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps(out))
