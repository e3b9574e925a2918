"""Per-rank frame time of the stripe partition on ONE GPU (diagnostic, not the bench): times
rank 0's share of a W x H progressive render for world sizes 1, 2, 4, 8, i.e. what each rank
of `bench.py --gpus N` computes per step, to predict strong-scaling efficiency without an
8-GPU node.  usage: [RT_FRAME_PAIRS=auto|off|on] [RT_TILE_ORDER=auto|off] [RT_FPL=n] [RT_IMAGES=last_two|every] [RT_QUEUES=q] [RT_CHAIN_PARTS=0|1|2] [RT_SUBMIT=auto|hip|aql] [RT_REPS=r] [RT_WARM_MS=50] [RT_PATHS=auto|per_wave|pair|compact] python tools/rank_sim.py [K3|K2|K5] [steps]"""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "gpu-ray-tracing_amd"), str(ROOT)]
import torch  # noqa: E402

import gpu_ray_tracing as rt  # noqa: E402
from gpu_ray_tracing.distributed import StripeRenderer  # noqa: E402

CONF = {"K2": (1920, 1080, rt.SCENE_THREE, 3, 1), "K3": (1920, 1080, rt.SCENE_N, 500, 1),
        "K5": (3840, 2160, rt.SCENE_N, 500, 8)}


def main(cfg="K3", steps=50):
    w, h, kind, n, depth = CONF[cfg]
    sc = rt.SphereCollection.generate(kind, n, 1)
    reps = int(os.environ.get("RT_REPS", "1"))
    seeds = rt.frame_seeds(0x5EED, steps * reps + 69)
    settings = rt.CameraSettings(max_depth=depth, samples_per_pixel=1000)
    cam = rt.SceneCamera.from_settings(settings, w, h, float(seeds[0]))
    pipe = rt.ComputeShaderPipeline(0)
    pipe.set_spheres(sc)
    pipe.set_frame_pairs(os.environ.get("RT_FRAME_PAIRS", "auto"))
    # RT_FPL=1: one launch per frame (the reference's dispatch structure)
    pipe.set_frames_per_launch(int(os.environ.get("RT_FPL", "0")))
    pipe.set_path_compaction(os.environ.get("RT_PATHS", "auto"))   # bounce launches
    if hasattr(rt._lib.lib(), "rt_set_frame_images"):
        pipe.set_frame_images(os.environ.get("RT_IMAGES", "last_two"))
    if hasattr(rt._lib.lib(), "rt_set_single_kernel"):
        pipe.set_single_kernel(os.environ.get("RT_SINGLE", "auto"))
    if hasattr(rt._lib.lib(), "rt_set_tile_order"):
        pipe.set_tile_order(os.environ.get("RT_TILE_ORDER", "auto"))
    if hasattr(rt._lib.lib(), "rt_set_update_queues"):
        pipe.set_update_queues(int(os.environ.get("RT_QUEUES", "0")))
    if hasattr(rt._lib.lib(), "rt_set_chain_parts"):
        pipe.set_chain_parts(int(os.environ.get("RT_CHAIN_PARTS", "0")))
    if hasattr(rt._lib.lib(), "rt_set_update_submit"):
        pipe.set_update_submit(os.environ.get("RT_SUBMIT", "auto"))
    # untimed warm-up (as bench.py --warm-ms): the whole image for RT_WARM_MS ms
    warm = StripeRenderer(pipe, w, h, 0, 1)
    torch.cuda.synchronize()
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < float(os.environ.get("RT_WARM_MS", "50")) / 1e3:
        warm.frames(cam, sc, seeds[:20])
        torch.cuda.synchronize()
    del warm
    base = None
    for world in (1, 2, 4, 8):
        r = StripeRenderer(pipe, w, h, 0, world)
        r.frames(cam, sc, seeds[:5])                       # reset frame + warmup
        cam_t = cam.with_fields(camera_has_moved=0.0)
        r.frames(cam_t, sc, seeds[5:69])                   # (tile costs of a long launch)
        # RT_REPS timed blocks of `steps` frames (the median reported, all listed)
        runs, host = [], []
        for rep in range(reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            off = 69 + rep * steps
            r.frames(cam_t, sc, seeds[off:off + steps])
            host.append((time.perf_counter() - t0) * 1e6 / steps)  # the issuing call's time
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / steps)
        us = sorted(runs)[len(runs) // 2]
        host_us = sorted(host)[len(host) // 2]
        base = base or us
        print(json.dumps({"cfg": cfg, "world": world, "rank0_rows": r.rows,
                          "us_per_step": round(us, 2), "ideal_us": round(base / world, 2),
                          "predicted_efficiency": round(base / world / us, 3),
                          "host_issue_us_per_step": round(host_us, 2),
                          "runs_us": [round(x, 2) for x in runs],
                          "queues": pipe.last_launch_info().get("queues"),
                          "chain_parts": pipe.last_launch_info().get("chain_parts"),
                          "launches": pipe.last_launch_info().get("launches"),
                          "kernel": pipe.last_launch_info().get("kernel_name"),
                          "frames_per_launch": pipe.last_launch_info().get("max_frames_per_launch"),
                          "submit": pipe.last_launch_info().get("submit")}), flush=True)
    pipe.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "K3",
         int(sys.argv[2]) if len(sys.argv) > 2 else 50)
