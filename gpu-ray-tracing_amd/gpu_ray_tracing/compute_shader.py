"""The compute-shader plugin surface (src/lib.rs), bound to the HIP kernels.

Reference -> here:
  ComputeShaderPipeline::from_world (lib.rs:240-324)   -> ComputeShaderPipeline(device)
  ComputeShaderImages {texture_a, texture_b} (138-142)  -> ComputeShaderImages
  `init` dispatch (lib.rs:398-407, wgsl:65-70)          -> ComputeShaderPipeline.init_image
  `update` dispatch (lib.rs:408-417, wgsl:333-364)      -> ComputeShaderPipeline.update
  ComputeShaderNode state machine (lib.rs:326-421)      -> ComputeShaderNode (C++ driver)
Extensions the reference lacks: fused multi-frame accumulation (``render``), the stripe
partition for multi-GPU (``render_stripes`` / ``deinterleave``).

Images are torch float32 tensors of shape (H, W, 4) on the pipeline's device (RGBA32F,
row-major, alpha = sample count).  Every call is enqueued on torch's current stream.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .camera import SceneCamera
from .scene import SphereCollection

RT_STRIPE_ROWS = _lib.RT_STRIPE_ROWS
# ComputeShaderPipeline.denoise's defaults: rt_denoise_params_default's (1 / 0.5^2 = 4)
DENOISE_DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_color": 1.0,
                    "sigma_position": 0.5}


# ComputeShaderPipeline.reproject's defaults: rt_reproject_params_default's
REPROJECT_DEFAULTS = {"max_history": 64, "position_tolerance2": 1e-5, "lambertian_only": True}


# ComputeShaderPipeline.resize_carry's `fill`: rt_resize.h's RT_RESIZE_FILL_*
RESIZE_FILL_NONE = _lib.RT_RESIZE_FILL_NONE
RESIZE_FILL_NEAREST = _lib.RT_RESIZE_FILL_NEAREST


# ComputeShaderPipeline.denoise_guided's defaults: rt_variance_filter_params_default's
GUIDED_DEFAULTS = {"iterations": 5, "normal_power_log2": 5, "sigma_luminance": 1.0,
                   "sigma_position": 0.5, "min_history": 4, "fallback_variance": 1.0}


# ComputeShaderPipeline.update_adaptive's defaults: rt_adaptive_params_default's
ADAPTIVE_DEFAULTS = {"min_samples": 16, "abs_tolerance2": 1e-5, "rel_tolerance2": 2.5e-4}


def reproject_basis(camera: SceneCamera) -> np.ndarray:
    """rt_reproject_basis: the 3 x 3 float32 rows that take a world point's offset from
    camera.center to (a, b, c), the point lying on the view's ray through sample position
    (a / c, b / c) at c > 0 (rt_reproject.h).  Host only; raises RtError for a degenerate
    camera."""
    out = np.zeros(9, np.float32)
    cam = camera.to_c()
    _lib.call("rt_reproject_basis", ctypes.byref(cam), _np_ptr(out))
    return out.reshape(3, 3)


# edit_plan's and ComputeShaderPipeline.carry_edit's defaults: rt_edit_params_default's (the two
# numbers come from the CPU prototype DESIGN.md 4.13 reports)
EDIT_DEFAULTS = {"edit_history": 4, "influence": 3.0}


def _edit_params(max_history, lambertian_only, position_tolerance2, edit_history, influence):
    p = _lib.EditParamsC()
    p.carry = _lib.ReprojectParamsC(int(max_history), 1 if lambertian_only else 0,
                                    float(position_tolerance2), 0)
    p.edit_history = int(edit_history)
    p.influence = float(influence)
    return p


def _sphere_rows(spheres) -> np.ndarray:
    arr = spheres.spheres if isinstance(spheres, SphereCollection) else spheres
    arr = np.ascontiguousarray(arr, np.float32)
    if arr.size % 8:
        raise ValueError("sphere records are 8 float32 each")
    return arr.reshape(-1, 8)


def edit_plan(prev_spheres, spheres, prev_index=None, *,
              influence: float = EDIT_DEFAULTS["influence"],
              edit_history: int = EDIT_DEFAULTS["edit_history"],
              max_history: int = REPROJECT_DEFAULTS["max_history"]) -> tuple[np.ndarray, dict]:
    """rt_edit_plan (rt_scene_edit.h): compares the previous scene with the current one
    (SphereCollections or (n, 8) float32 arrays) and returns (table, info) for
    ComputeShaderPipeline.carry_edit.  prev_index[i] is the index current sphere i had in the
    previous scene, RT_EDIT_NONE for a new one; None is the identity.  `table` is a
    (n_cur + 32, 8) uint32 array of 32-byte rows: info["n_records"] records, then
    info["n_balls"] balls, the rest zeros.  Host only; raises RtError for what the header
    refuses."""
    prev, cur = _sphere_rows(prev_spheres), _sphere_rows(spheres)
    index = None
    if prev_index is not None:
        index = np.ascontiguousarray(np.asarray(prev_index, np.int64).astype(np.uint32))
        if index.shape != (cur.shape[0],):
            raise ValueError("prev_index holds one entry per current sphere")
    table = np.zeros((cur.shape[0] + _lib.RT_EDIT_MAX_BALLS, 8), np.uint32)
    info = _lib.EditInfoC()
    params = _edit_params(max_history, True, REPROJECT_DEFAULTS["position_tolerance2"],
                          edit_history, influence)
    _lib.call("rt_edit_plan", _np_ptr(prev), prev.shape[0], _np_ptr(cur), cur.shape[0],
              _np_ptr(index) if index is not None else None, ctypes.byref(params),
              _np_ptr(table), table.nbytes, ctypes.byref(info))
    return table, {f: int(getattr(info, f)) for f, _ in _lib.EditInfoC._fields_
                   if not f.startswith("_")}


def inv_sigma2(sigma: float) -> float:
    """1 / sigma^2 in float32, as denoise passes a sigma to rt_denoise (inf for sigma 0,
    which the library refuses; 0 for an infinite sigma: that weight term is off)."""
    with np.errstate(divide="ignore", over="ignore"):
        s = np.float32(sigma)
        return float(np.float32(1.0) / (s * s))


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


def _np_ptr(a: np.ndarray) -> ctypes.c_void_p:
    # (the array interface's address: ndarray.ctypes builds a helper object per access,
    # several microseconds of host time on every call)
    return ctypes.c_void_p(a.__array_interface__["data"][0])


# torch's current stream as a raw handle without building a Stream object per call
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _is_f32c(a) -> bool:
    return isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous


def _cam_blob(camera: SceneCamera) -> np.ndarray:
    """The camera's 44 f32 as one contiguous array: the rt_scene_camera layout itself."""
    blob = camera.blob
    if not _is_f32c(blob) or blob.size != 44:
        blob = np.ascontiguousarray(blob, np.float32)
        if blob.size != 44:
            raise ValueError("a SceneCamera blob holds 44 f32 (176 bytes)")
    return blob


def _check_image(t: torch.Tensor, width: int, height: int, name: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise ValueError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous float32")
    if t.numel() < width * height * 4:
        raise ValueError(f"{name} holds {t.numel()} floats, need {width * height * 4}")


def _check_plane(t, n: int, dtype, name: str):
    if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
            or not t.is_contiguous() or t.numel() < n):
        raise ValueError(f"{name} must be a contiguous CUDA (HIP) {dtype} tensor of at least "
                         f"{n} elements")
    return t


def stripe_local_rows(height: int, rank: int, nranks: int) -> int:
    return int(_lib.lib().rt_stripe_local_rows(height, rank, nranks))


def stripe_band_set(height: int, rank: int, nranks: int) -> tuple[int, int, int]:
    """The round-robin stripes of rank / nranks as a band set (first, step, count)."""
    bands = (height + RT_STRIPE_ROWS - 1) // RT_STRIPE_ROWS
    return (rank, nranks, (bands - rank + nranks - 1) // nranks if bands > rank else 0)


def chain_schedule(frames: int, cap: int, variant: int = 0) -> list[tuple[int, int, int]]:
    """rt_chain_schedule: the (part, first frame, frames) launches of an update_frames call of
    `frames` frames at `cap` frames per launch, in issue order (host only)."""
    n = _lib.U32(0)
    out = (_lib.ChainLaunchC * (2 * (int(frames) // max(1, int(cap)) + 4)))()
    _lib.call("rt_chain_schedule", int(frames), int(cap), int(variant), out, len(out),
              ctypes.byref(n))
    return [(int(l.part), int(l.first), int(l.frames)) for l in out[:n.value]]


def partition_bands(band_cost, nranks: int) -> list[tuple[int, int, int]]:
    """rt_partition_bands: the bands cut into nranks contiguous ranges (first, 1, count)
    whose largest cost is the smallest possible (host-only, exact)."""
    c = np.ascontiguousarray(band_cost, np.float64)
    out = (_lib.BandSetC * nranks)()
    _lib.call("rt_partition_bands", _np_ptr(c), c.size, nranks, out)
    return [(b.first, b.step, b.count) for b in out]


class ComputeShaderPipeline:
    """One librt_hip.so context on one HIP device (lib.rs:231-324)."""

    def __init__(self, device: int | torch.device = 0):
        if isinstance(device, torch.device):
            device = device.index if device.index is not None else torch.cuda.current_device()
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        ctx = ctypes.c_void_p()
        _lib.call("rt_create", self.device, ctypes.byref(ctx))
        self._ctx = ctx
        self._sphere_keep = None
        self.scan_mode = "culled"

    # ---- lifetime ---------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            _lib.call("rt_destroy", self._ctx)
            self._ctx = ctypes.c_void_p()

    def set_frames_per_launch(self, n: int) -> None:
        """rt_set_frames_per_launch: update_frames' frames per launch (0 = automatic,
        1 = one `update` dispatch per frame, n = up to n)."""
        _lib.call("rt_set_frames_per_launch", self._ctx, int(n))

    def set_frame_pairs(self, mode: str) -> None:
        """rt_set_frame_pairs: 'auto' | 'off' | 'on' (two waves per tile, alternate frames)
        | 'quad' (four waves per tile) | 'on2' / 'quad2' (two / four waves per pair of tiles,
        two pixels per lane)."""
        _lib.call("rt_set_frame_pairs", self._ctx,
                  {"auto": 0, "off": 1, "on": 2, "quad": 3, "on2": 4, "quad2": 5}[mode])

    def set_frame_images(self, mode: str) -> None:
        """rt_set_frame_images: the images a fused multi-frame launch writes — "last_two"
        (default: the two that survive the call) or "every" (every frame's image to the
        ping-pong buffer its chained update writes, as the reference's dispatches do);
        identical pixels."""
        _lib.call("rt_set_frame_images", self._ctx, {"last_two": 0, "every": 1}[mode])

    def set_tile_order(self, mode: str) -> None:
        """rt_set_tile_order: "auto" (costliest tiles first, from the first launch's
        per-tile durations) or "off" (raster order)."""
        _lib.call("rt_set_tile_order", self._ctx, {"auto": 0, "off": 1}[mode])

    def set_update_queues(self, queues: int) -> None:
        """rt_set_update_queues: one-frame updates of update_frames as `queues` concurrent
        parts on their own streams (0 = automatic, 1 = one launch per update)."""
        _lib.call("rt_set_update_queues", self._ctx, int(queues))

    def set_chain_parts(self, parts: int) -> None:
        """rt_set_chain_parts: update_frames calls of several fused frame-group launches as
        two staggered chains over halves of the image (0 = automatic, 1 = one chain, 2 = two
        parts wherever the conditions hold); identical pixels."""
        _lib.call("rt_set_chain_parts", self._ctx, int(parts))

    def set_occlusion_cull(self, on: bool) -> None:
        """rt_set_occlusion_cull: whether the candidate-list build drops the entries another
        entry hides from every camera ray of the tile (default on); identical pixels."""
        _lib.call("rt_set_occlusion_cull", self._ctx, 1 if on else 0)

    def set_certain_tiles(self, on: bool) -> None:
        """rt_set_certain_tiles: whether the list build marks the tiles one sphere certainly
        covers and the pair frame loops trace them straight-line (default on); identical
        pixels."""
        if hasattr(_lib.lib(), "rt_set_certain_tiles"):       # (absent from older builds)
            _lib.call("rt_set_certain_tiles", self._ctx, 1 if on else 0)

    def certain_tiles_stats(self) -> dict:
        """rt_certain_tiles_stats: certain tiles of the lists built last, and pairs of two
        certain tiles in the last tile-pair launch."""
        out = (ctypes.c_uint64 * 2)()
        if hasattr(_lib.lib(), "rt_certain_tiles_stats"):     # (absent from older builds)
            _lib.call("rt_certain_tiles_stats", self._ctx, out)
        return {"certain_tiles": int(out[0]), "certain_pairs": int(out[1])}

    def set_tight_bundle(self, on: bool) -> None:
        """rt_set_tight_bundle: whether the lists are built against the two-slope beam of a
        tile's camera rays (default on) or the single cone used before it; identical pixels."""
        if hasattr(_lib.lib(), "rt_set_tight_bundle"):        # (absent from older builds)
            _lib.call("rt_set_tight_bundle", self._ctx, 1 if on else 0)

    def tile_lists(self) -> dict:
        """rt_tile_lists: the candidate lists built last, copied to the host — per tile (local
        band by local band, (width + 7) // 8 tiles each) "count" (RT_TILE_LIST_NONE: no list),
        "removed", "flags" (u32 arrays) and "records" (tiles x 19 x 4 f32: centre and radius
        squared of entry j < count, zero beyond)."""
        n = ctypes.c_uint64(0)
        _lib.call("rt_tile_lists", self._ctx, None, 0, ctypes.byref(n))
        buf = np.zeros((int(n.value), 4 + 4 * _lib.RT_TILE_LIST_MAX), np.uint32)
        assert buf.shape[1] * buf.itemsize == ctypes.sizeof(_lib.TileListC)
        if n.value:
            _lib.call("rt_tile_lists", self._ctx, buf.ctypes.data, n.value, ctypes.byref(n))
        return {"count": buf[:, 0].copy(), "removed": buf[:, 1].copy(), "flags": buf[:, 2].copy(),
                "records": buf[:, 4:].copy().view(np.float32).reshape(-1, _lib.RT_TILE_LIST_MAX, 4)}

    def set_update_submit(self, mode: str) -> None:
        """rt_set_update_submit: how update_frames submits one-frame updates — "auto" (HIP
        launches; AQL is opt-in), "hip" or "aql" (AQL packets on the context's own HSA
        queues, an error if unavailable; after a failed AQL segment, reported once as an
        error, the context runs HIP launches); identical pixels."""
        _lib.call("rt_set_update_submit", self._ctx, {"auto": 0, "hip": 1, "aql": 2}[mode])

    def submit_status(self) -> dict:
        """rt_update_submit_status: whether AQL submission is available (and why not), the go
        waits that gave up (0 in a correct run) and the AQL packets submitted so far."""
        avail, give_ups, packets = ctypes.c_int(0), _lib.U32(0), ctypes.c_uint64(0)
        _lib.call("rt_update_submit_status", self._ctx, ctypes.byref(avail),
                  ctypes.byref(give_ups), ctypes.byref(packets))
        why = "" if avail.value else _lib.lib().rt_last_error().decode()
        return {"aql_available": bool(avail.value), "go_give_ups": int(give_ups.value),
                "packets": int(packets.value), "why": why}

    def set_path_compaction(self, mode: str) -> None:
        """rt_set_path_compaction for bounce launches: "auto" (default: "split" with four
        chunks for launches of at most 20 000 tiles once their tile costs are measured, else
        "per_wave"), "per_wave", "compact" (paths repacked across four waves after every
        bounce), "pair" (two waves per tile on alternate frames) or "split" (a tile's frames in
        chunks on separate waves, the last finisher accumulating; with measured costs only
        the costliest tiles split, every unit dispatched by its own cost)."""
        _lib.call("rt_set_path_compaction", self._ctx,
                  {"auto": 0, "per_wave": 1, "compact": 2, "pair": 3, "split": 4}[mode])

    def set_single_kernel(self, mode: str) -> None:
        """rt_set_single_kernel: "auto" (one-frame launches of the camera-ray-only case run
        rt_single_kernel: two tiles per wave, one for small launches), "pair", "one" (force
        either) or "off" (the general rt_trace_kernel<2>); identical pixels."""
        _lib.call("rt_set_single_kernel", self._ctx,
                  {"auto": 0, "off": 1, "pair": 2, "one": 3}[mode])

    def frames_per_launch(self, camera) -> int:
        """rt_get_frames_per_launch: frames update_frames fuses per launch for `camera`."""
        out = _lib.U32(0)
        cam = camera.to_c()
        _lib.call("rt_get_frames_per_launch", self._ctx, ctypes.byref(cam), ctypes.byref(out))
        return int(out.value)

    def last_launch_info(self) -> dict:
        """rt_last_launch_info: what the last trace call launched — launches, frames,
        max_frames_per_launch, kernel (RT_KERNEL_* id) and its rocprofv3 name, the parts
        (queues) and the submission ("hip" or "aql")."""
        info = _lib.LaunchInfoC()
        _lib.call("rt_last_launch_info", self._ctx, ctypes.byref(info))
        d = {k: int(getattr(info, k)) for k, _ in info._fields_}
        d["kernel_name"] = _lib.lib().rt_kernel_name(d["kernel"]).decode()
        d["submit"] = {1: "hip", 2: "aql"}.get(d["submit"], "none")
        if d["submit"] == "aql" and d["kernel_name"].startswith("rt_single_kernel"):
            # the AQL path dispatches the chain instances of the same kernel
            d["kernel_name"] = d["kernel_name"].replace("rt_single_kernel", "rt_chain_kernel")
        return d

    def set_launch_timing(self, enable: bool) -> None:
        """rt_set_launch_timing: the fused launches of each update_frames call carry timing
        events in their own dispatch packets (no marker packets on the stream)."""
        _lib.call("rt_set_launch_timing", self._ctx, 1 if enable else 0)

    def last_call_kernel_time(self) -> tuple[float, int]:
        """rt_last_call_kernel_time: (seconds from the start of the last call's first timed
        launch to the end of its last, launches timed); waits for that launch."""
        ms, n = ctypes.c_float(0.0), _lib.U32(0)
        _lib.call("rt_last_call_kernel_time", self._ctx, ctypes.byref(ms), ctypes.byref(n))
        return ms.value / 1e3, int(n.value)

    def candidate_stats(self) -> dict:
        """rt_candidate_stats: the camera rays' per-tile candidate lists built last."""
        out = (ctypes.c_uint64 * 5)()
        _lib.call("rt_candidate_stats", self._ctx, out)
        t, none, entries, mx, cap = (int(v) for v in out)
        listed = t - none
        stats = {"tiles": t, "tiles_without_list": none,
                 "no_list_frac": round(none / t, 6) if t else 0.0,
                 "mean_entries": round(entries / listed, 3) if listed else 0.0,
                 "max_entries": mx, "capacity": cap}
        if hasattr(_lib.lib(), "rt_occlusion_cull_stats"):   # (absent from older builds)
            occ = (ctypes.c_uint64 * 2)()
            _lib.call("rt_occlusion_cull_stats", self._ctx, occ)
            stats["entries"] = entries
            stats["occlusion_removed"] = int(occ[0])
            stats["occlusion_tiles"] = int(occ[1])
        return stats

    def selftest_fastmath(self, n_random: int = 1 << 26) -> list[int]:
        """rt_selftest_fastmath: [defocus, division, sqrt, root-selection mismatches,
        cases run]."""
        out = (ctypes.c_uint64 * 5)()
        _lib.call("rt_selftest_fastmath", self._ctx, n_random, out)
        return list(out)

    ROOT_FAMILIES = ("consider_fast", "consider_any_fast")
    ROOT_STRATA = ("bulk", "far", "edge", "far_edge")

    def selftest_roots(self, n_random: int = 1 << 26) -> dict:
        """rt_selftest_roots: {(family, stratum): {mismatches, drawn, compared, rooted}} of
        the fast root selections against the IEEE ones on n_random generated cases."""
        out = (_lib.RootsTallyC * (_lib.RT_ROOTS_FAMILIES * _lib.RT_ROOTS_STRATA))()
        _lib.call("rt_selftest_roots", self._ctx, n_random, out)
        return {(fam, st): {k: int(getattr(out[f * _lib.RT_ROOTS_STRATA + s], k))
                            for k, _ in _lib.RootsTallyC._fields_}
                for f, fam in enumerate(self.ROOT_FAMILIES)
                for s, st in enumerate(self.ROOT_STRATA)}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- helpers ----------------------------------------------------------------------
    def _stream(self) -> ctypes.c_void_p:
        if _raw_stream is not None:
            return ctypes.c_void_p(_raw_stream(self.device))
        return ctypes.c_void_p(torch.cuda.current_stream(self.torch_device).cuda_stream)

    def _spheres(self, spheres: SphereCollection):
        arr = np.ascontiguousarray(spheres.spheres, np.float32)
        self._sphere_keep = arr
        return _np_ptr(arr), arr.shape[0]

    def new_image(self, width: int, height: int) -> torch.Tensor:
        return torch.zeros((height, width, 4), dtype=torch.float32, device=self.torch_device)

    # ---- the plugin operations --------------------------------------------------------
    def set_scan_mode(self, mode: str) -> None:
        """"culled" (default, exact wave-level culling) or "exhaustive" (linear walk)."""
        code = {"exhaustive": _lib.RT_SCAN_EXHAUSTIVE, "culled": _lib.RT_SCAN_CULLED}[mode]
        _lib.call("rt_set_scan_mode", self._ctx, code)
        self.scan_mode = mode

    def set_spheres(self, spheres: SphereCollection) -> None:
        p, n = self._spheres(spheres)
        _lib.call("rt_set_spheres", self._ctx, p, n, self._stream())

    def init_image(self, out: torch.Tensor, width: int, height: int) -> None:
        _check_image(out, width, height, "out")
        _lib.call("rt_init_image", self._ctx, _ptr(out), width, height, self._stream())

    def update(self, inp: torch.Tensor, out: torch.Tensor, width: int, height: int,
               camera: SceneCamera, spheres: SphereCollection) -> None:
        _check_image(inp, width, height, "in")
        _check_image(out, width, height, "out")
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        _lib.call("rt_update", self._ctx, _ptr(inp), _ptr(out), width, height,
                  ctypes.byref(cam), p, n, self._stream())

    def render(self, inp: torch.Tensor, out: torch.Tensor, width: int, height: int,
               camera: SceneCamera, spheres: SphereCollection, seeds) -> None:
        _check_image(inp, width, height, "in")
        _check_image(out, width, height, "out")
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        s = np.ascontiguousarray(seeds, np.float32)
        _lib.call("rt_render", self._ctx, _ptr(inp), _ptr(out), width, height,
                  ctypes.byref(cam), p, n, s.size, _np_ptr(s),
                  self._stream())

    def render_stripes(self, inp: torch.Tensor, out: torch.Tensor, width: int, height: int,
                       rank: int, nranks: int, camera: SceneCamera,
                       spheres: SphereCollection, seeds) -> None:
        rows = stripe_local_rows(height, rank, nranks)
        _check_image(inp, width, rows, "in")
        _check_image(out, width, rows, "out")
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        s = np.ascontiguousarray(seeds, np.float32)
        _lib.call("rt_render_stripes", self._ctx, _ptr(inp), _ptr(out), width, height, rank,
                  nranks, ctypes.byref(cam), p, n, s.size, _np_ptr(s),
                  self._stream())

    def update_frames(self, image_a: torch.Tensor, image_b: torch.Tensor, width: int,
                      height: int, camera: SceneCamera, spheres: SphereCollection, seeds,
                      rank: int = 0, nranks: int = 1) -> int:
        """len(seeds) progressive `update` dispatches ping-ponging a -> b -> a ... (the
        reference's per-frame loop, lib.rs:366-417); returns 0 if image_a holds the
        result, 1 for image_b.  Frame 0 honours camera.camera_has_moved."""
        rows = stripe_local_rows(height, rank, nranks) if nranks > 1 else height
        _check_image(image_a, width, rows, "image_a")
        _check_image(image_b, width, rows, "image_b")
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        s = np.ascontiguousarray(seeds, np.float32)
        newest = ctypes.c_int(-1)
        _lib.call("rt_update_frames", self._ctx, _ptr(image_a), _ptr(image_b), width, height,
                  rank, nranks, ctypes.byref(cam), p, n, s.size, _np_ptr(s), self._stream(),
                  ctypes.byref(newest))
        return newest.value

    def bind_update_frames(self, image_a: torch.Tensor, image_b: torch.Tensor, width: int,
                           height: int, rank: int = 0, nranks: int = 1):
        """update_frames with the images, size and stripe fixed: the images are checked once
        here, and the returned run(camera, spheres, seeds) -> newest issues the call with no
        per-call validation or lookups (the host time before a call's first launch is part of
        a short timed region).  The images must stay allocated while run is used."""
        rows = stripe_local_rows(height, rank, nranks) if nranks > 1 else height
        _check_image(image_a, width, rows, "image_a")
        _check_image(image_b, width, rows, "image_b")
        fn = _lib.lib().rt_update_frames
        ctx, pa, pb = self._ctx, _ptr(image_a), _ptr(image_b)
        newest = ctypes.c_int(-1)
        pnew = ctypes.byref(newest)
        stream = self._stream
        # the CPython binding (rt_fastcall.c) when built: the same call with plain ints and
        # the arrays' buffers, ≈ 1 µs of host time against ≈ 8 µs through ctypes
        fast = _lib.fastcall()
        ictx, ia, ib = ctx.value, pa.value, pb.value
        dev = self.device if fast is not None else None
        raw = _raw_stream
        # the caller's spheres array when it can be passed as it is (contiguous float32
        # (N, 8)), its data pointer and count; `held` keeps the array the pointer points into
        # alive until the next call replaces it (a converted copy included)
        last = {"arr": None, "ptr": None, "n": 0, "held": None}

        # arrays the binding refused (by identity): they take the converting path below from
        # then on instead of raising and catching on every call
        refused = {"arr": None, "seeds": None}

        def run(camera: SceneCamera, spheres: SphereCollection, seeds) -> int:
            arr = spheres.spheres
            # the binding takes exactly what the ctypes path passes unconverted: contiguous
            # float32 (N, 8) spheres (an (N, 16) array would otherwise be read as N records of
            # a 32-byte stride) and contiguous float32 seeds
            if (fast is not None and arr is not refused["arr"] and seeds is not refused["seeds"]
                    and _is_f32c(arr) and arr.ndim == 2 and arr.shape[1] == 8
                    and _is_f32c(seeds)):
                try:
                    r = fast.update_frames(ictx, ia, ib, width, height, rank, nranks,
                                           camera.blob, arr, len(arr), seeds,
                                           raw(dev) if raw else stream().value)
                except (TypeError, ValueError, BufferError):
                    refused.update(arr=arr, seeds=seeds)
                    r = None
                if r is not None:
                    if r < 0:
                        _lib.check(-r, "rt_update_frames")
                    return r
            # the camera blob itself is the 176-byte rt_scene_camera (no struct copy).  A
            # spheres array that is contiguous float32 (N, 8) is passed as it is, its pointer
            # re-read only when the array object or its length changes; any other array is
            # converted on every call.  (The library compares the contents on every call, so
            # an array edited in place is still uploaded.)
            blob = _cam_blob(camera)
            arr = spheres.spheres
            if arr is not last["arr"] or arr.shape[0] != last["n"]:
                direct = _is_f32c(arr) and arr.ndim == 2 and arr.shape[1] == 8
                held = arr if direct else np.ascontiguousarray(arr, np.float32).reshape(-1, 8)
                last.update(arr=arr if direct else None, held=held, n=held.shape[0],
                            ptr=held.__array_interface__["data"][0])
            s = seeds if _is_f32c(seeds) else np.ascontiguousarray(seeds, np.float32)
            rc = fn(ctx, pa, pb, width, height, rank, nranks, blob.__array_interface__["data"][0],
                    last["ptr"], last["n"], s.size, s.__array_interface__["data"][0], stream(),
                    pnew)
            if rc:
                _lib.check(rc, "rt_update_frames")
            return newest.value

        run.images = (image_a, image_b)
        return run

    def update_frames_bands(self, image_a: torch.Tensor, image_b: torch.Tensor, width: int,
                            height: int, bands, camera: SceneCamera,
                            spheres: SphereCollection, seeds) -> int:
        """rt_update_frames_bands: update_frames over the band set bands = (first, step,
        count) — local band j is global band first + j * step; the images hold count * 8
        rows.  Returns 0 if image_a holds the result, 1 for image_b."""
        rows = int(bands[2]) * RT_STRIPE_ROWS
        _check_image(image_a, width, rows, "image_a")
        _check_image(image_b, width, rows, "image_b")
        bs = _lib.band_sets([bands])
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        sd = np.ascontiguousarray(seeds, np.float32)
        newest = ctypes.c_int(-1)
        _lib.call("rt_update_frames_bands", self._ctx, _ptr(image_a), _ptr(image_b), width,
                  height, bs, ctypes.byref(cam), p, n, sd.size, _np_ptr(sd), self._stream(),
                  ctypes.byref(newest))
        return newest.value

    def band_costs(self, width: int, height: int, bands) -> np.ndarray:
        """rt_band_costs: per local band of `bands` the tile costs (device clock ticks) the
        context's last cost-recording launch measured for that share."""
        out = np.zeros(int(bands[2]), np.float64)
        _lib.call("rt_band_costs", self._ctx, width, height, _lib.band_sets([bands]),
                  _np_ptr(out))
        return out

    def deinterleave_bands(self, gathered: torch.Tensor, out: torch.Tensor, width: int,
                           height: int, sets, rows_per_rank: int) -> None:
        """rt_deinterleave_bands: nranks = len(sets) compact buffers of rows_per_rank rows
        each (rank order) scattered into the width x height image."""
        _check_image(gathered, width, rows_per_rank * len(sets), "gathered")
        _check_image(out, width, height, "out")
        _lib.call("rt_deinterleave_bands", self._ctx, _ptr(gathered), _ptr(out), width,
                  height, len(sets), _lib.band_sets(sets), rows_per_rank, self._stream())

    def deinterleave(self, gathered: torch.Tensor, out: torch.Tensor, width: int, height: int,
                     nranks: int) -> None:
        rows = stripe_local_rows(height, 0, nranks)
        _check_image(gathered, width, rows * nranks, "gathered")
        _check_image(out, width, height, "out")
        _lib.call("rt_deinterleave_stripes", self._ctx, _ptr(gathered), _ptr(out), width,
                  height, nranks, self._stream())

    # ---- first-hit G-buffer and picking (rt_aov.h) -------------------------------------
    def trace_aov(self, width: int, height: int, camera: SceneCamera,
                  spheres: SphereCollection, planes=_lib.AOV_PLANES, bands=None,
                  out: dict | None = None) -> dict[str, torch.Tensor]:
        """rt_trace_aov / rt_trace_aov_bands: the first hit of each pixel's centre ray from
        camera.center (no jitter, no lens), bit-identical to the oracle's sphere_hit.
        planes: any non-empty subset of "sphere_id" ((rows, W) int32, a miss reads -1: the
        bits of RT_AOV_MISS), "hit" ((rows, W, 4) float32: p, t; a miss 0, 0, 0, +inf),
        "normal" (n, front ? 1 : 0; a miss zeros) and "material" (the sphere's color[4]; a
        miss zeros).  bands = (first, step, count): compact local buffers of count * 8 rows
        with global pixel coordinates, as update_frames_bands.  Buffers come from `out` (by
        plane name) where given, else they are allocated on the pipeline's device; a buffer
        of a plane not in `planes` is not touched.  Enqueued on torch's current stream."""
        planes = tuple(planes)
        unknown = [k for k in planes if k not in _lib.AOV_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose from {_lib.AOV_PLANES}")
        rows = height if bands is None else int(bands[2]) * RT_STRIPE_ROWS
        res: dict[str, torch.Tensor] = {}
        c = _lib.AovPlanesC()
        for name in planes:
            is_id = name == "sphere_id"
            dtype = torch.int32 if is_id else torch.float32
            t = out.get(name) if out else None
            if t is None:
                shape = (rows, width) if is_id else (rows, width, 4)
                t = torch.empty(shape, dtype=dtype, device=self.torch_device)
            need = rows * width * (1 if is_id else 4)
            if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
                    or not t.is_contiguous() or t.numel() < need):
                raise ValueError(f"out[{name!r}] must be a contiguous CUDA (HIP) {dtype} tensor "
                                 f"of at least {need} elements")
            setattr(c, name, t.data_ptr())
            res[name] = t
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        if bands is None:
            _lib.call("rt_trace_aov", self._ctx, ctypes.byref(c), width, height,
                      ctypes.byref(cam), p, n, self._stream())
        else:
            _lib.call("rt_trace_aov_bands", self._ctx, ctypes.byref(c), width, height,
                      _lib.band_sets([bands]), ctypes.byref(cam), p, n, self._stream())
        return res

    def pick(self, width: int, height: int, x: int, y: int, camera: SceneCamera,
             spheres: SphereCollection) -> dict | None:
        """rt_pick: what is under pixel (x, y) — {"sphere_id", "t", "p", "normal",
        "front_face", "color"}, the texel trace_aov writes there — or None for a miss.  One
        wave is launched (the pixel's tile); returns once the record is on the host."""
        r = _lib.PickResultC()
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        _lib.call("rt_pick", self._ctx, width, height, x, y, ctypes.byref(cam), p, n,
                  self._stream(), ctypes.byref(r))
        if r.sphere_id == _lib.RT_AOV_MISS:
            return None
        return {"sphere_id": int(r.sphere_id), "t": np.float32(r.t),
                "p": np.array(r.p, np.float32), "normal": np.array(r.normal, np.float32),
                "front_face": bool(r.front_face), "color": np.array(r.color, np.float32)}

    # ---- ray queries (rt_query.h) ---------------------------------------------------------
    def _rays(self, rays) -> tuple[torch.Tensor, int]:
        """The (N, 8) float32 ray records on the device: o, tmax, d, a reserved word."""
        if isinstance(rays, np.ndarray):
            arr = np.ascontiguousarray(rays, np.float32)
            if arr.ndim != 2 or arr.shape[1] != 8:
                raise ValueError("rays must be (N, 8) float32: o, tmax, d, reserved")
            # (from_numpy refuses to share a read-only array quietly: copy that one)
            rays = torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(
                self.torch_device)
        if (not isinstance(rays, torch.Tensor) or rays.device.type != "cuda"
                or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.dim() != 2
                or rays.shape[1] != 8):
            raise ValueError("rays must be a contiguous (N, 8) float32 CUDA (HIP) tensor or a "
                             "NumPy array")
        return rays, int(rays.shape[0])

    def cast_rays(self, rays, spheres: SphereCollection,
                  planes=("sphere_id", "hit", "normal"), out: dict | None = None,
                  route_counts: torch.Tensor | None = None) -> dict[str, torch.Tensor]:
        """rt_cast_rays, RT_QUERY_CLOSEST: the closest hit of each ray below its own tmax,
        bit-identical to the oracle's sphere_hit chained in index order.  rays: a contiguous
        (N, 8) float32 CUDA tensor (o, tmax, d, a reserved word per row), or a NumPy array that
        is uploaded.  planes: any non-empty subset of trace_aov's, one element per ray
        ("sphere_id" (N,) int32, the others (N, 4) float32, the same values and miss records).
        Buffers come from `out` (by plane name) where given, else they are allocated; a buffer
        of a plane not in `planes` is not touched.  route_counts: a zeroed int32 CUDA tensor of
        3 words that receives the waves per route (QUERY_ROUTES).  Enqueued on torch's current
        stream."""
        planes = tuple(planes)
        unknown = [k for k in planes if k not in _lib.AOV_PLANES]
        if unknown:
            raise ValueError(f"unknown planes {unknown}: choose from {_lib.AOV_PLANES}")
        rays, n_rays = self._rays(rays)
        res: dict[str, torch.Tensor] = {}
        c = _lib.QueryPlanesC()
        for name in planes:
            is_id = name == "sphere_id"
            dtype = torch.int32 if is_id else torch.float32
            t = out.get(name) if out else None
            if t is None:
                t = torch.empty((n_rays,) if is_id else (n_rays, 4), dtype=dtype,
                                device=self.torch_device)
            _check_plane(t, n_rays * (1 if is_id else 4), dtype, f"out[{name!r}]")
            setattr(c, name, t.data_ptr())
            res[name] = t
        self._cast(rays, n_rays, _lib.RT_QUERY_CLOSEST, c, spheres, route_counts)
        return res

    def occluded(self, rays, spheres: SphereCollection, out: torch.Tensor | None = None,
                 route_counts: torch.Tensor | None = None) -> torch.Tensor:
        """rt_cast_rays, RT_QUERY_OCCLUSION: per ray 1 where cast_rays reports a hit below the
        ray's tmax, else 0 ((N,) int32); the scan stops at the first sphere accepted.  rays,
        route_counts and the stream as cast_rays."""
        rays, n_rays = self._rays(rays)
        if out is None:
            out = torch.empty((n_rays,), dtype=torch.int32, device=self.torch_device)
        _check_plane(out, n_rays, torch.int32, "out")
        c = _lib.QueryPlanesC()
        c.occluded = out.data_ptr()
        self._cast(rays, n_rays, _lib.RT_QUERY_OCCLUSION, c, spheres, route_counts)
        return out

    def _cast(self, rays, n_rays, mode, c, spheres, route_counts) -> None:
        if route_counts is not None:
            _check_plane(route_counts, 3, torch.int32, "route_counts")
        p, n = self._spheres(spheres)
        _lib.call("rt_cast_rays", self._ctx, _ptr(rays) if n_rays else None, n_rays, mode,
                  ctypes.byref(c), p, n,
                  _ptr(route_counts) if route_counts is not None else None, self._stream())

    def cast_ray(self, origin, direction, spheres: SphereCollection,
                 tmax: float = float("inf")) -> dict | None:
        """rt_cast_ray: the closest hit of one ray below tmax — the record `pick` returns
        ({"sphere_id", "t", "p", "normal", "front_face", "color"}), or None for a miss.  One
        wave is launched; returns once the record is on the host."""
        ray = _lib.RayC()
        ray.o = tuple(float(np.float32(v)) for v in origin)
        ray.d = tuple(float(np.float32(v)) for v in direction)
        ray.tmax = float(np.float32(tmax))
        r = _lib.PickResultC()
        p, n = self._spheres(spheres)
        _lib.call("rt_cast_ray", self._ctx, ctypes.byref(ray), p, n, self._stream(),
                  ctypes.byref(r))
        if r.sphere_id == _lib.RT_AOV_MISS:
            return None
        return {"sphere_id": int(r.sphere_id), "t": np.float32(r.t),
                "p": np.array(r.p, np.float32), "normal": np.array(r.normal, np.float32),
                "front_face": bool(r.front_face), "color": np.array(r.color, np.float32)}

    # ---- sample-coverage ID mattes (rt_matte.h) ------------------------------------------
    def new_matte(self, width: int, height: int) -> dict[str, torch.Tensor]:
        """The empty matte state of a width x height image (or of a band buffer of `height`
        rows): "ids" and "counts" ((H, W, 4) int32, the u32 words of rt_matte.h; the background id
        RT_AOV_MISS reads -1, as trace_aov's sphere_id plane) and "tally" ((H, W, 2) int32:
        samples taken, samples that found no slot)."""
        return {"ids": torch.zeros((height, width, 4), dtype=torch.int32, device=self.torch_device),
                "counts": torch.zeros((height, width, 4), dtype=torch.int32,
                                      device=self.torch_device),
                "tally": torch.zeros((height, width, 2), dtype=torch.int32,
                                     device=self.torch_device)}

    @staticmethod
    def _matte_planes(matte: dict, pixels: int) -> "_lib.MattePlanesC":
        c = _lib.MattePlanesC()
        for name in _lib.MATTE_PLANES:
            t = matte.get(name) if isinstance(matte, dict) else None
            if t is None:
                raise ValueError(f"matte[{name!r}] is missing (the planes of new_matte)")
            _check_plane(t, pixels * (2 if name == "tally" else 4), torch.int32,
                         f"matte[{name!r}]")
            setattr(c, name, t.data_ptr())
        return c

    def matte_frames(self, matte: dict, width: int, height: int, camera: SceneCamera,
                     spheres: SphereCollection, seeds) -> dict:
        """rt_matte_frames: len(seeds) frames of first-hit counting over the planes of
        new_matte, in place (returned).  Frame f traces, per pixel, the camera ray `update`
        traces for that pixel's sample count and seeds[f] — jitter and lens included — and
        counts the sphere it hits first (the background as RT_AOV_MISS) in the pixel's four
        slots.  Frame 0 honours camera.camera_has_moved (a reset).  Enqueued on torch's current
        stream."""
        c = self._matte_planes(matte, width * height)
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        s = np.ascontiguousarray(seeds, np.float32)
        _lib.call("rt_matte_frames", self._ctx, ctypes.byref(c), width, height,
                  ctypes.byref(cam), p, n, _np_ptr(s), s.size, self._stream())
        return matte

    def matte_frames_bands(self, matte: dict, width: int, height: int, bands,
                           camera: SceneCamera, spheres: SphereCollection, seeds) -> dict:
        """rt_matte_frames_bands: matte_frames over the band set bands = (first, step, count);
        the planes are compact local buffers of count * 8 rows with global pixel coordinates,
        as update_frames_bands."""
        c = self._matte_planes(matte, width * int(bands[2]) * RT_STRIPE_ROWS)
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        s = np.ascontiguousarray(seeds, np.float32)
        _lib.call("rt_matte_frames_bands", self._ctx, ctypes.byref(c), width, height,
                  _lib.band_sets([bands]), ctypes.byref(cam), p, n, _np_ptr(s), s.size,
                  self._stream())
        return matte

    def matte_resolve(self, matte: dict, selected, *, alpha: bool = True,
                      dominant: bool = False, out: dict | None = None) -> dict:
        """rt_matte_resolve over every pixel the planes hold (a whole image or a band buffer).
        selected: sphere indices (below 2^20) and / or RT_AOV_MISS (-1 is accepted) for the
        background.  Returns {"alpha": (H, W) float32 — the fraction of the pixel's samples
        that saw a selected id, 0 where no sample was taken} and / or {"dominant": (H, W) int32
        — the id of the fullest slot, -1 (RT_AOV_MISS) where no sample was taken}.  Buffers
        come from `out` where given."""
        t = matte.get("tally") if isinstance(matte, dict) else None
        if not isinstance(t, torch.Tensor) or t.numel() % 2:
            raise ValueError("matte['tally'] is missing (the planes of new_matte)")
        pixels = t.numel() // 2
        shape = tuple(t.shape[:-1]) if t.dim() > 1 else (pixels,)
        c = self._matte_planes(matte, pixels)
        sel = np.ascontiguousarray(np.asarray(selected, np.int64).reshape(-1) & 0xFFFFFFFF,
                                   np.uint32)
        res = {}
        for name, want, dtype in (("alpha", alpha, torch.float32),
                                  ("dominant", dominant, torch.int32)):
            if not want:
                continue
            buf = out.get(name) if out else None
            if buf is None:
                buf = torch.empty(shape, dtype=dtype, device=self.torch_device)
            res[name] = _check_plane(buf, pixels, dtype, f"out[{name!r}]")
        _lib.call("rt_matte_resolve", self._ctx, ctypes.byref(c), pixels,
                  _np_ptr(sel) if sel.size else None, sel.size,
                  _ptr(res["alpha"]) if "alpha" in res else None,
                  _ptr(res["dominant"]) if "dominant" in res else None, self._stream())
        return res

    def matte_info(self) -> dict:
        """rt_matte_last_info: how the last matte_frames call found its first hits — tiles that
        walked their own sphere list, tiles that fell back to the per-frame scan (and how many
        of those because the list overflowed), the longest list."""
        r = _lib.MatteInfoC()
        _lib.call("rt_matte_last_info", self._ctx, ctypes.byref(r))
        return {k: int(getattr(r, k)) for k, _ in _lib.MatteInfoC._fields_}

    # ---- the denoiser (rt_denoise.h) -----------------------------------------------------
    def denoise(self, image: torch.Tensor, width: int, height: int, guides: dict, *,
                iterations: int = DENOISE_DEFAULTS["iterations"],
                normal_power_log2: int = DENOISE_DEFAULTS["normal_power_log2"],
                sigma_color: float = DENOISE_DEFAULTS["sigma_color"],
                sigma_position: float = DENOISE_DEFAULTS["sigma_position"],
                use_ids: bool = True, out: torch.Tensor | None = None,
                scratch: torch.Tensor | None = None) -> torch.Tensor:
        """rt_denoise: the edge-avoiding a-trous filter of rt_denoise.h over `image` (an
        accumulator of width x height, left as it is), guided by the planes trace_aov returns
        for the same view: guides["hit"], guides["normal"] and, with use_ids,
        guides["sphere_id"].  Iteration i filters with tap spacing 1 << i; the sigmas go to the
        library as float32 1 / sigma^2 (sigma_color is iteration 0's and halves every
        iteration).  `out` and `scratch` (needed from two iterations on) are allocated when
        not given; returns `out`, whose alpha is the image's.  Every bit equals the NumPy
        restatement in tests/test_denoise.py.  Enqueued on torch's current stream."""
        need = width * height * 4

        def image_like(t, what, dtype=torch.float32, n=need):
            if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
                    or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) {dtype} tensor of at "
                                 f"least {n} elements")
            return t

        image_like(image, "image")
        names = ("hit", "normal") + (("sphere_id",) if use_ids else ())
        missing = [k for k in names if guides.get(k) is None]
        if missing:
            raise ValueError(f"guides lacks {missing} (the planes of trace_aov)")
        image_like(guides["hit"], 'guides["hit"]')
        image_like(guides["normal"], 'guides["normal"]')
        ids = None
        if use_ids:
            ids = image_like(guides["sphere_id"], 'guides["sphere_id"]', torch.int32,
                             width * height)
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=self.torch_device)
        image_like(out, "out")
        if scratch is None and iterations >= 2:
            scratch = torch.empty((height, width, 4), dtype=torch.float32,
                                  device=self.torch_device)
        if scratch is not None:
            image_like(scratch, "scratch")
        params = _lib.DenoiseParamsC(int(iterations), int(normal_power_log2),
                                     inv_sigma2(sigma_color), inv_sigma2(sigma_position))
        _lib.call("rt_denoise", self._ctx, _ptr(image), _ptr(out),
                  _ptr(scratch) if scratch is not None else None, width, height,
                  _ptr(guides["hit"]), _ptr(guides["normal"]),
                  _ptr(ids) if ids is not None else None, ctypes.byref(params), self._stream())
        return out

    # ---- reprojection (rt_reproject.h) ---------------------------------------------------
    def reproject(self, prev_image: torch.Tensor, width: int, height: int,
                  prev_camera: SceneCamera, prev_guides: dict, guides: dict, *,
                  max_history: int = REPROJECT_DEFAULTS["max_history"],
                  position_tolerance2: float = REPROJECT_DEFAULTS["position_tolerance2"],
                  lambertian_only: bool = REPROJECT_DEFAULTS["lambertian_only"],
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """rt_reproject: carries `prev_image`, the accumulator of the view `prev_camera`
        (left as it is), into the current view of the same scene.  prev_guides holds
        trace_aov's "sphere_id" and "hit" for the previous view, guides its "sphere_id",
        "hit", "normal" and, with lambertian_only, "material" for the current one.  Each pixel
        of `out` (allocated when not given; returned) gets the colour and the sample count,
        capped at max_history, of the previous pixels that saw the same surface point, or
        zeros (a restart) where none did: pass it to update / update_frames with
        camera_has_moved = 0, or to denoise.  Every bit equals the NumPy restatement in
        tests/test_reproject.py.  Enqueued on torch's current stream."""
        need = width * height * 4

        def image_like(t, what, dtype=torch.float32, n=need):
            if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
                    or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) {dtype} tensor of at "
                                 f"least {n} elements")
            return t

        image_like(prev_image, "prev_image")
        names = ("sphere_id", "hit", "normal") + (("material",) if lambertian_only else ())
        missing = [f"prev_guides[{k!r}]" for k in ("sphere_id", "hit")
                   if prev_guides.get(k) is None]
        missing += [f"guides[{k!r}]" for k in names if guides.get(k) is None]
        if missing:
            raise ValueError(f"missing {missing} (the planes of trace_aov)")
        c = _lib.ReprojectPlanesC()
        for field, src, k in [("prev_sphere_id", prev_guides, "sphere_id"),
                              ("prev_hit", prev_guides, "hit")] + \
                             [(k, guides, k) for k in names]:
            is_id = k == "sphere_id"
            what = ("prev_guides" if src is prev_guides else "guides") + f"[{k!r}]"
            t = image_like(src[k], what, torch.int32 if is_id else torch.float32,
                           width * height if is_id else need)
            setattr(c, field, t.data_ptr())
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=self.torch_device)
        image_like(out, "out")
        params = _lib.ReprojectParamsC(int(max_history), 1 if lambertian_only else 0,
                                       float(position_tolerance2), 0)
        cam = prev_camera.to_c()
        _lib.call("rt_reproject", self._ctx, _ptr(prev_image), _ptr(out), width, height,
                  ctypes.byref(cam), ctypes.byref(c), ctypes.byref(params), self._stream())
        return out

    # ---- carrying across image sizes (rt_resize.h) ---------------------------------------
    def resize_carry(self, prev_image: torch.Tensor, prev_size, size,
                     prev_camera: SceneCamera, camera: SceneCamera | None,
                     prev_guides: dict, guides: dict, *,
                     max_history: int = REPROJECT_DEFAULTS["max_history"],
                     position_tolerance2: float = REPROJECT_DEFAULTS["position_tolerance2"],
                     lambertian_only: bool = REPROJECT_DEFAULTS["lambertian_only"],
                     sky: bool = False, fill: int = RESIZE_FILL_NONE,
                     prev_second: torch.Tensor | None = None,
                     out: torch.Tensor | None = None, out_second: torch.Tensor | None = None):
        """rt_resize_carry: `reproject` from a previous view of prev_size = (width, height)
        into a current view of size = (width, height).  prev_guides are trace_aov's
        "sphere_id" and "hit" at the previous size, guides its "sphere_id", "hit", "normal"
        and, with lambertian_only, "material" at the current size.  With `sky` a pixel whose
        ray misses carries the previous sky pixels in its direction; with fill =
        RESIZE_FILL_NEAREST a pixel that gets no history shows the nearest previous texel's
        colour with a sample count of 0 (a restart for update).  `camera`, the current view's,
        is needed for either and may be None otherwise.  prev_second (a moments image, say) is
        carried by the same rules in the same launch into out_second.  Returns `out`
        (allocated when not given), or (out, out_second) with prev_second.  Every bit equals
        the NumPy restatement in tests/test_resize.py.  Enqueued on torch's current stream."""
        (pw, ph), (width, height) = (int(v) for v in prev_size), (int(v) for v in size)
        need, prev_need = width * height * 4, pw * ph * 4

        def image_like(t, what, dtype=torch.float32, n=need):
            if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
                    or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) {dtype} tensor of at "
                                 f"least {n} elements")
            return t

        image_like(prev_image, "prev_image", n=prev_need)
        if out_second is not None and prev_second is None:
            raise ValueError("out_second is given without prev_second")
        if (sky or fill) and camera is None:
            raise ValueError("sky and fill need the current view's camera")
        names = ("sphere_id", "hit", "normal") + (("material",) if lambertian_only else ())
        missing = [f"prev_guides[{k!r}]" for k in ("sphere_id", "hit")
                   if prev_guides.get(k) is None]
        missing += [f"guides[{k!r}]" for k in names if guides.get(k) is None]
        if missing:
            raise ValueError(f"missing {missing} (the planes of trace_aov)")
        c = _lib.ReprojectPlanesC()
        for field, src, k in [("prev_sphere_id", prev_guides, "sphere_id"),
                              ("prev_hit", prev_guides, "hit")] + \
                             [(k, guides, k) for k in names]:
            is_id = k == "sphere_id"
            is_prev = src is prev_guides
            what = ("prev_guides" if is_prev else "guides") + f"[{k!r}]"
            texels = pw * ph if is_prev else width * height
            t = image_like(src[k], what, torch.int32 if is_id else torch.float32,
                           texels if is_id else 4 * texels)
            setattr(c, field, t.data_ptr())
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=self.torch_device)
        image_like(out, "out")
        images = _lib.ResizeImagesC(prev_image.data_ptr(), out.data_ptr(), None, None)
        if prev_second is not None:
            image_like(prev_second, "prev_second", n=prev_need)
            if out_second is None:
                out_second = torch.empty((height, width, 4), dtype=torch.float32,
                                         device=self.torch_device)
            image_like(out_second, "out_second")
            images.prev_second, images.dst_second = prev_second.data_ptr(), out_second.data_ptr()
        params = _lib.ResizeParamsC(int(max_history), 1 if lambertian_only else 0,
                                    float(position_tolerance2), 1 if sky else 0, int(fill))
        prev_cam = prev_camera.to_c()
        cam = camera.to_c() if camera is not None else None
        _lib.call("rt_resize_carry", self._ctx, ctypes.byref(images), pw, ph, width, height,
                  ctypes.byref(prev_cam), ctypes.byref(cam) if cam is not None else None,
                  ctypes.byref(c), ctypes.byref(params), self._stream())
        return out if prev_second is None else (out, out_second)

    def upscale(self, image: torch.Tensor, size_small, size, camera_small: SceneCamera,
                camera: SceneCamera, guides_small: dict | None = None,
                guides: dict | None = None, *, spheres: SphereCollection | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
        """A size-sized picture of the accumulator `image` rendered at size_small (both
        (width, height)) for the view camera_small, as seen by `camera`: resize_carry with
        lambertian_only off, sky on and fill = RESIZE_FILL_NEAREST, so that every pixel shows a
        colour and the full-size G-buffer places every silhouette.  Whichever of guides_small /
        guides is not given is traced with trace_aov over `spheres`, the current scene, which
        is required then (the pipeline does not guess it from an earlier call).  Returns the
        full-size image (`out` when given), ready for `present`."""
        if (guides_small is None or guides is None) and spheres is None:
            raise ValueError("spheres is needed to trace the guides that are not given")
        if guides_small is None:
            guides_small = self.trace_aov(int(size_small[0]), int(size_small[1]), camera_small,
                                          spheres, planes=("sphere_id", "hit"))
        if guides is None:
            guides = self.trace_aov(int(size[0]), int(size[1]), camera, spheres,
                                    planes=("sphere_id", "hit", "normal"))
        return self.resize_carry(image, size_small, size, camera_small, camera, guides_small,
                                 guides, lambertian_only=False, sky=True,
                                 fill=RESIZE_FILL_NEAREST, out=out)

    # ---- carrying across scene edits (rt_scene_edit.h) -----------------------------------
    def carry_edit(self, prev_image: torch.Tensor, width: int, height: int,
                   prev_camera: SceneCamera, prev_guides: dict, guides: dict, plan, *,
                   max_history: int = REPROJECT_DEFAULTS["max_history"],
                   position_tolerance2: float = REPROJECT_DEFAULTS["position_tolerance2"],
                   lambertian_only: bool = REPROJECT_DEFAULTS["lambertian_only"],
                   edit_history: int = EDIT_DEFAULTS["edit_history"],
                   out: torch.Tensor | None = None) -> torch.Tensor:
        """rt_edit_carry: `reproject` across an edit of the scene.  prev_guides are trace_aov's
        planes for the previous scene and camera, guides those for the current scene and
        camera; `plan` is what edit_plan returned for the two scenes, (table, info), where
        `table` may also be a contiguous device tensor that already holds the table's bytes.
        A host table is copied to the device on torch's current stream, so the call touches no
        scene state of the pipeline.  A sphere that moved or was resized carries its own
        surface's history; pixels inside the plan's balls keep at most edit_history samples
        (0: they restart); recoloured and new spheres restart.  Every bit of `out` (allocated
        when not given; returned) equals the NumPy restatement in tests/test_scene_edit.py.
        Enqueued on torch's current stream."""
        need = width * height * 4

        def image_like(t, what, dtype=torch.float32, n=need):
            if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
                    or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) {dtype} tensor of at "
                                 f"least {n} elements")
            return t

        image_like(prev_image, "prev_image")
        names = ("sphere_id", "hit", "normal") + (("material",) if lambertian_only else ())
        missing = [f"prev_guides[{k!r}]" for k in ("sphere_id", "hit")
                   if prev_guides.get(k) is None]
        missing += [f"guides[{k!r}]" for k in names if guides.get(k) is None]
        if missing:
            raise ValueError(f"missing {missing} (the planes of trace_aov)")
        c = _lib.ReprojectPlanesC()
        for field, src, k in [("prev_sphere_id", prev_guides, "sphere_id"),
                              ("prev_hit", prev_guides, "hit")] + \
                             [(k, guides, k) for k in names]:
            is_id = k == "sphere_id"
            what = ("prev_guides" if src is prev_guides else "guides") + f"[{k!r}]"
            t = image_like(src[k], what, torch.int32 if is_id else torch.float32,
                           width * height if is_id else need)
            setattr(c, field, t.data_ptr())
        try:
            table, info = plan
            n_records, n_balls = int(info["n_records"]), int(info["n_balls"])
        except (TypeError, ValueError, KeyError):
            raise ValueError("plan is the (table, info) pair of edit_plan") from None
        rows = n_records + n_balls
        if isinstance(table, np.ndarray):
            if table.nbytes < 32 * rows:
                raise ValueError(f"plan's table holds {table.nbytes} bytes, need {32 * rows}")
            host = np.ascontiguousarray(table).reshape(-1).view(np.uint8)[:32 * rows]
            table_dev = torch.from_numpy(host.copy()).to(self.torch_device) if rows else None
        else:
            if (not isinstance(table, torch.Tensor) or table.device.type != "cuda"
                    or not table.is_contiguous()
                    or table.numel() * table.element_size() < 32 * rows):
                raise ValueError("plan's table must be a NumPy array or a contiguous CUDA (HIP) "
                                 f"tensor of at least {32 * rows} bytes")
            table_dev = table if rows else None
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=self.torch_device)
        image_like(out, "out")
        params = _edit_params(max_history, lambertian_only, position_tolerance2, edit_history,
                              EDIT_DEFAULTS["influence"])
        cam = prev_camera.to_c()
        _lib.call("rt_edit_carry", self._ctx, _ptr(prev_image), _ptr(out), width, height,
                  ctypes.byref(cam), ctypes.byref(c),
                  _ptr(table_dev) if table_dev is not None else None, n_records, n_balls,
                  ctypes.byref(params), self._stream())
        return out

    # ---- moments and the variance-guided filter (rt_variance.h) --------------------------
    def moments_update(self, inp: torch.Tensor, out: torch.Tensor, moments: torch.Tensor,
                       width: int, height: int) -> torch.Tensor:
        """rt_moments_update: folds the sample that one update added between its input image
        `inp` and its output image `out` (both left as they are) into `moments`, an image
        (m1, m2, 0, k) of the running means of luminance and luminance^2 and their sample
        count, rewritten in place and returned.  Start from zeros (new_image); reproject
        carries a moments image across a camera move like an accumulator.  Enqueued on torch's
        current stream."""
        for t, what in ((inp, "inp"), (out, "out"), (moments, "moments")):
            _check_image(t, width, height, what)
        _lib.call("rt_moments_update", self._ctx, _ptr(inp), _ptr(out), _ptr(moments), width,
                  height, self._stream())
        return moments

    def denoise_guided(self, image: torch.Tensor, width: int, height: int, guides: dict,
                       moments: torch.Tensor, *,
                       iterations: int = GUIDED_DEFAULTS["iterations"],
                       normal_power_log2: int = GUIDED_DEFAULTS["normal_power_log2"],
                       sigma_luminance: float = GUIDED_DEFAULTS["sigma_luminance"],
                       sigma_position: float = GUIDED_DEFAULTS["sigma_position"],
                       min_history: int = GUIDED_DEFAULTS["min_history"],
                       fallback_variance: float = GUIDED_DEFAULTS["fallback_variance"],
                       use_ids: bool = True, out: torch.Tensor | None = None,
                       scratch: torch.Tensor | None = None,
                       variance: torch.Tensor | None = None,
                       variance_scratch: torch.Tensor | None = None
                       ) -> tuple[torch.Tensor, torch.Tensor]:
        """rt_variance_filter: denoise's filter with a luminance term scaled by each pixel's
        own variance, from `moments` (moments_update's image for `image`), and taps weighted by
        their sample counts (rt_variance.h).  Guides and sigmas as in denoise (sigma_luminance
        is in units of the local standard deviation and does not change with the iteration).
        `out`, `variance` ((height, width) float32) and, from two iterations on, `scratch` and
        `variance_scratch` are allocated when not given; returns (out, variance), the filtered
        image and the variance of its luminance.  Every bit equals the NumPy restatement in
        tests/test_variance.py.  Enqueued on torch's current stream."""
        need = width * height * 4

        def image_like(t, what, dtype=torch.float32, n=need):
            if (not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype
                    or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous CUDA (HIP) {dtype} tensor of at "
                                 f"least {n} elements")
            return t

        image_like(image, "image")
        image_like(moments, "moments")
        names = ("hit", "normal") + (("sphere_id",) if use_ids else ())
        missing = [k for k in names if guides.get(k) is None]
        if missing:
            raise ValueError(f"guides lacks {missing} (the planes of trace_aov)")
        image_like(guides["hit"], 'guides["hit"]')
        image_like(guides["normal"], 'guides["normal"]')
        ids = None
        if use_ids:
            ids = image_like(guides["sphere_id"], 'guides["sphere_id"]', torch.int32,
                             width * height)
        dev = self.torch_device
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.float32, device=dev)
        if variance is None:
            variance = torch.empty((height, width), dtype=torch.float32, device=dev)
        if iterations >= 2:
            if scratch is None:
                scratch = torch.empty((height, width, 4), dtype=torch.float32, device=dev)
            if variance_scratch is None:
                variance_scratch = torch.empty((height, width), dtype=torch.float32, device=dev)
        image_like(out, "out")
        image_like(variance, "variance", n=width * height)
        if scratch is not None:
            image_like(scratch, "scratch")
        if variance_scratch is not None:
            image_like(variance_scratch, "variance_scratch", n=width * height)
        params = _lib.VarianceFilterParamsC(int(iterations), int(normal_power_log2),
                                            inv_sigma2(sigma_luminance),
                                            inv_sigma2(sigma_position), int(min_history),
                                            float(fallback_variance))
        _lib.call("rt_variance_filter", self._ctx, _ptr(image), _ptr(out),
                  _ptr(scratch) if scratch is not None else None, _ptr(moments),
                  _ptr(variance),
                  _ptr(variance_scratch) if variance_scratch is not None else None,
                  width, height, _ptr(guides["hit"]), _ptr(guides["normal"]),
                  _ptr(ids) if ids is not None else None, ctypes.byref(params), self._stream())
        return out, variance

    # ---- adaptive sampling (rt_adaptive.h) -----------------------------------------------
    def adaptive_error(self, image: torch.Tensor, moments: torch.Tensor, width: int,
                       height: int, *, min_history: int = 4,
                       out: torch.Tensor | None = None) -> torch.Tensor:
        """rt_adaptive_error: the error plane update_adaptive reads, a (height, width) float32
        tensor (`out`, allocated when not given; returned): the variance of the mean of each
        pixel's luminance from `moments` (moments_update's image for the accumulator `image`),
        +inf where the moments hold fewer than min_history samples.  Both inputs are left as
        they are.  Enqueued on torch's current stream."""
        _check_image(image, width, height, "image")
        _check_image(moments, width, height, "moments")
        if out is None:
            out = torch.empty((height, width), dtype=torch.float32, device=self.torch_device)
        _check_plane(out, width * height, torch.float32, "out")
        _lib.call("rt_adaptive_error", self._ctx, _ptr(image), _ptr(moments), _ptr(out), width,
                  height, int(min_history), self._stream())
        return out

    def update_adaptive(self, inp: torch.Tensor, out: torch.Tensor, width: int, height: int,
                        camera: SceneCamera, spheres: SphereCollection, error: torch.Tensor, *,
                        min_samples: int = ADAPTIVE_DEFAULTS["min_samples"],
                        abs_tolerance2: float = ADAPTIVE_DEFAULTS["abs_tolerance2"],
                        rel_tolerance2: float = ADAPTIVE_DEFAULTS["rel_tolerance2"],
                        tile_mask=False, bands=None) -> torch.Tensor | None:
        """rt_update_adaptive / rt_update_adaptive_bands: one `update` from `inp` into `out` in
        which a pixel takes a sample only while it has fewer than min_samples samples or its
        `error` (adaptive_error's plane, or denoise_guided's variance) is above abs_tolerance2 +
        rel_tolerance2 * luminance^2; every other pixel passes through.  A sampled pixel has
        update's bits.  tile_mask: True (allocated) or an int64 tensor of one word per 8 x 8
        tile, tile rows first, bit (y & 7) * 8 + (x & 7) set where pixel (x, y) was sampled;
        it is returned (else None).  bands = (first, step, count): compact local buffers of
        count * 8 rows with global pixel coordinates, as update_frames_bands.  Enqueued on
        torch's current stream."""
        rows = height if bands is None else int(bands[2]) * RT_STRIPE_ROWS
        _check_image(inp, width, rows, "in")
        _check_image(out, width, rows, "out")
        _check_plane(error, width * rows, torch.float32, "error")
        tiles = ((width + 7) // 8) * ((rows + 7) // 8)
        mask = None
        if tile_mask is True:
            mask = torch.empty((tiles,), dtype=torch.int64, device=self.torch_device)
        elif tile_mask is not False and tile_mask is not None:
            mask = _check_plane(tile_mask, tiles, torch.int64, "tile_mask")
        params = _lib.AdaptiveParamsC(int(min_samples), float(abs_tolerance2),
                                      float(rel_tolerance2))
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        head = (self._ctx, _ptr(inp), _ptr(out), _ptr(error),
                _ptr(mask) if mask is not None else None, width, height)
        tail = (ctypes.byref(cam), p, n, ctypes.byref(params), self._stream())
        if bands is None:
            _lib.call("rt_update_adaptive", *head, *tail)
        else:
            _lib.call("rt_update_adaptive_bands", *head, _lib.band_sets([bands]), *tail)
        return mask

    # ---- the adaptive round as one multi-frame launch (rt_converge.h) --------------------
    def converge(self, image: torch.Tensor, moments: torch.Tensor, width: int, height: int,
                 camera: SceneCamera, spheres: SphereCollection, seeds, *,
                 min_samples: int = ADAPTIVE_DEFAULTS["min_samples"],
                 abs_tolerance2: float = ADAPTIVE_DEFAULTS["abs_tolerance2"],
                 rel_tolerance2: float = ADAPTIVE_DEFAULTS["rel_tolerance2"],
                 min_history: int = 4, error=None, tile_mask=False, tile_samples=False,
                 bands=None):
        """rt_converge_frames / rt_converge_frames_bands: len(seeds) rounds of adaptive_error,
        update_adaptive and moments_update on `image` and `moments`, both rewritten in place,
        bit for bit what the three calls leave; frame 0 honours camera.camera_has_moved.
        Returns (error, tile_mask, tile_samples), None for each one not wanted: `error` (True:
        allocated, or a float32 tensor of width * rows elements) receives adaptive_error of the
        result, `tile_mask` (True, or an int64 tensor of one word per 8 x 8 tile) the pixels the
        last frame sampled in update_adaptive's layout, `tile_samples` (True, or an int32 tensor
        of one word per tile) the samples each tile took over the call.  bands = (first, step,
        count): compact local buffers, as update_adaptive.  Enqueued on torch's current
        stream."""
        rows = height if bands is None else int(bands[2]) * RT_STRIPE_ROWS
        _check_image(image, width, rows, "image")
        _check_image(moments, width, rows, "moments")
        tiles = ((width + 7) // 8) * ((rows + 7) // 8)

        def optional(t, shape, dtype, name):
            if t is None or t is False:
                return None
            if t is True:
                return torch.empty(shape, dtype=dtype, device=self.torch_device)
            return _check_plane(t, int(np.prod(shape)), dtype, name)

        err = optional(error, (rows, width), torch.float32, "error")
        mask = optional(tile_mask, (tiles,), torch.int64, "tile_mask")
        taken = optional(tile_samples, (tiles,), torch.int32, "tile_samples")
        s = np.ascontiguousarray(seeds, np.float32)
        params = _lib.AdaptiveParamsC(int(min_samples), float(abs_tolerance2),
                                      float(rel_tolerance2))
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        head = (self._ctx, _ptr(image), _ptr(moments), *(_ptr(t) if t is not None else None
                                                         for t in (err, mask, taken)),
                width, height)
        tail = (ctypes.byref(cam), p, n, s.size, _np_ptr(s), ctypes.byref(params),
                int(min_history), self._stream())
        if bands is None:
            _lib.call("rt_converge_frames", *head, *tail)
        else:
            _lib.call("rt_converge_frames_bands", *head, _lib.band_sets([bands]), *tail)
        return err, mask, taken

    # ---- convergence reports and render-to-tolerance (rt_progress.h) ---------------------
    @staticmethod
    def _report_dict(r) -> dict:
        return {name: getattr(r, name) for name, _ in _lib.ProgressReportC._fields_
                if name != "_reserved"}

    def progress_report(self, image: torch.Tensor, width: int, height: int, spp: int, *,
                        moments: torch.Tensor | None = None, error: torch.Tensor | None = None,
                        min_samples: int = ADAPTIVE_DEFAULTS["min_samples"],
                        abs_tolerance2: float = ADAPTIVE_DEFAULTS["abs_tolerance2"],
                        rel_tolerance2: float = ADAPTIVE_DEFAULTS["rel_tolerance2"],
                        min_history: int = 4, tile_active=False, bands=None):
        """rt_progress_stats / rt_progress_stats_bands: every pixel of `image` classified as
        update_adaptive and converge decide it for these parameters, a samples_per_pixel of `spp`
        and a camera that has not moved, from `moments` (adaptive_error's estimate) or from an
        `error` plane, exactly one of the two.  Returns (report, mask): the report a dict of
        rt_progress_report's fields (pixels, active, converged, capped, below_min, no_history,
        nonfinite, samples, active_tiles, min_count, max_count, max_error), the mask
        (tile_active: True, or an int64 tensor of one word per 8 x 8 tile; else None) the active
        pixels in update_adaptive's tile_mask layout.  bands = (first, step, count): compact
        local buffers, as update_adaptive.  The call runs on torch's current stream and waits
        for it: the report is on the host when it returns."""
        rows = height if bands is None else int(bands[2]) * RT_STRIPE_ROWS
        _check_image(image, width, rows, "image")
        if (moments is None) == (error is None):
            raise ValueError("exactly one of moments and error is given")
        if moments is not None:
            _check_image(moments, width, rows, "moments")
        else:
            _check_plane(error, width * rows, torch.float32, "error")
        tiles = ((width + 7) // 8) * ((rows + 7) // 8)
        mask = None
        if tile_active is True:
            mask = torch.empty((tiles,), dtype=torch.int64, device=self.torch_device)
        elif tile_active is not False and tile_active is not None:
            mask = _check_plane(tile_active, tiles, torch.int64, "tile_active")
        params = _lib.AdaptiveParamsC(int(min_samples), float(abs_tolerance2),
                                      float(rel_tolerance2))
        report = _lib.ProgressReportC()
        head = (self._ctx, _ptr(image), _ptr(moments) if moments is not None else None,
                _ptr(error) if error is not None else None,
                _ptr(mask) if mask is not None else None, width, height)
        tail = (int(spp), ctypes.byref(params), int(min_history), self._stream(),
                ctypes.byref(report))
        if bands is None:
            _lib.call("rt_progress_stats", *head, *tail)
        else:
            _lib.call("rt_progress_stats_bands", *head, _lib.band_sets([bands]), *tail)
        return self._report_dict(report), mask

    def render_to_tolerance(self, image: torch.Tensor, moments: torch.Tensor, width: int,
                            height: int, camera: SceneCamera, spheres: SphereCollection, seeds,
                            *, max_active: int = 0, check_every: int = 16,
                            min_samples: int = ADAPTIVE_DEFAULTS["min_samples"],
                            abs_tolerance2: float = ADAPTIVE_DEFAULTS["abs_tolerance2"],
                            rel_tolerance2: float = ADAPTIVE_DEFAULTS["rel_tolerance2"],
                            min_history: int = 4, tile_active=False):
        """rt_progress_run: `converge` on `image` and `moments` in calls of check_every frames,
        with a progress_report after each, until at most max_active pixels are active or
        len(seeds) frames have run.  A camera that has not moved is looked at first, and nothing
        runs when it is already there; a camera that has moved runs its first call unseen (its
        frame 0 is a reset).  Returns (frames_run, report, mask) with the last report and its
        mask as progress_report returns them; `image` and `moments` hold what one `converge` of
        frames_run frames leaves.  Runs on torch's current stream and waits for it."""
        _check_image(image, width, height, "image")
        _check_image(moments, width, height, "moments")
        tiles = ((width + 7) // 8) * ((height + 7) // 8)
        mask = None
        if tile_active is True:
            mask = torch.empty((tiles,), dtype=torch.int64, device=self.torch_device)
        elif tile_active is not False and tile_active is not None:
            mask = _check_plane(tile_active, tiles, torch.int64, "tile_active")
        s = np.ascontiguousarray(seeds, np.float32)
        params = _lib.AdaptiveParamsC(int(min_samples), float(abs_tolerance2),
                                      float(rel_tolerance2))
        goal = _lib.ProgressGoalC(int(max_active), s.size, int(check_every))
        cam = camera.to_c()
        p, n = self._spheres(spheres)
        report = _lib.ProgressReportC()
        done = ctypes.c_uint32(0)
        _lib.call("rt_progress_run", self._ctx, _ptr(image), _ptr(moments),
                  _ptr(mask) if mask is not None else None, width, height, ctypes.byref(cam), p,
                  n, _np_ptr(s), ctypes.byref(params), int(min_history), ctypes.byref(goal),
                  self._stream(), ctypes.byref(done), ctypes.byref(report))
        return int(done.value), self._report_dict(report), mask

    def present(self, image: torch.Tensor, width: int, height: int,
                encoding: str = "srgb", out: torch.Tensor | None = None) -> torch.Tensor:
        """8-bit RGBA of a float image (rt_present_rgba8), a (H, W, 4) uint8 device tensor:
        what the reference's sprite shows (lib.rs:79-102), ready for a PNG."""
        _check_image(image, width, height, "image")
        code = {"linear": _lib.RT_ENCODE_LINEAR, "srgb": _lib.RT_ENCODE_SRGB}[encoding]
        if out is None:
            out = torch.empty((height, width, 4), dtype=torch.uint8, device=self.torch_device)
        if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < width * height * 4:
            raise ValueError("out must be contiguous uint8 with width*height*4 elements")
        _lib.call("rt_present_rgba8", self._ctx, _ptr(image), _ptr(out), width, height, code,
                  self._stream())
        return out


def srgb_thresholds() -> np.ndarray:
    """The 256-entry f32 boundary table of the sRGB encoding (rt_srgb_thresholds)."""
    t = np.zeros(256, np.float32)
    _lib.lib().rt_srgb_thresholds(t.ctypes.data_as(ctypes.c_void_p))
    return t


class ComputeShaderImages:
    """texture_a / texture_b (lib.rs:60-93, 138-142): two zero-filled RGBA32F images."""

    def __init__(self, pipeline: ComputeShaderPipeline, width: int, height: int):
        self.width, self.height = width, height
        self.texture_a = pipeline.new_image(width, height)
        self.texture_b = pipeline.new_image(width, height)


class ComputeShaderNode:
    """Render-graph node (lib.rs:326-421) driving init + ping-pong updates per frame."""

    STATES = {0: "Loading", 1: "Init", 2: "Update(0)", 3: "Update(1)"}

    def __init__(self, pipeline: ComputeShaderPipeline, images: ComputeShaderImages):
        self.pipeline = pipeline
        self.images = images
        drv = ctypes.c_void_p()
        _lib.call("rt_driver_create", pipeline._ctx, _ptr(images.texture_a),
                  _ptr(images.texture_b), images.width, images.height, ctypes.byref(drv))
        self._drv = drv

    @property
    def state(self) -> str:
        return self.STATES[_lib.lib().rt_driver_state(self._drv)]

    def frame(self, camera: SceneCamera, spheres: SphereCollection) -> torch.Tensor:
        """One frame (node.update() + node.run()); returns the image written last."""
        cam = camera.to_c()
        p, n = self.pipeline._spheres(spheres)
        newest = ctypes.c_int(-1)
        _lib.call("rt_driver_frame", self._drv, ctypes.byref(cam), p, n,
                  self.pipeline._stream(), ctypes.byref(newest))
        return self.images.texture_a if newest.value == 0 else self.images.texture_b

    def close(self) -> None:
        if getattr(self, "_drv", None) and self._drv.value:
            _lib.call("rt_driver_destroy", self._drv)
            self._drv = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
