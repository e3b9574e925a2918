"""Convergence reports and render-to-tolerance (include/rt_progress.h): rt_progress_stats,
rt_progress_stats_bands, rt_progress_run.

The reference is NumPy, built from what the repository already has: tests/test_variance.py's
`initial_variance` with +inf as the fallback (err from the moments), tests/test_adaptive.py's
`f2u` and `tile_words`, the sampler's decision lines restated once (`report_ref`; the CPU tests
hold it against `adaptive_ref`'s own sampled pixels) and tests/test_converge.py's `chain_ref`
(`run_ref`, the header's loop).  Every GPU output is compared bit for bit, and a sentinel tail
follows every buffer the library writes.

The report inputs: test_adaptive's `mixed` planes (an error plane with values on and next to each
pixel's threshold, NaN, +inf, counts that u32() saturates or zeroes) at samples_per_pixel 20 and
10, test_converge's parity planes and test_adaptive's `error_inputs` (moments).  Shapes a tile
recipe cannot index (1 x 1, 65536 x 1, 1 x 65536) take the 256 x 256 `mixed` planes reshaped: a
pixel's class depends on its own values only.  The CPU tests count from the reference alone what
the inputs reach (printed with -s).
"""
import ctypes
import functools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import test_adaptive as ta
import test_converge as tc
import test_fast_domains as fd
import test_variance as tv
from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_progress.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
SENT, SENT_WORD, TAIL = ta.SENT, ta.SENT_WORD, ta.TAIL
COUNTS = ("pixels", "active", "converged", "capped", "below_min", "no_history", "nonfinite",
          "samples", "active_tiles")
FIELDS = COUNTS + ("min_count", "max_count", "max_error")
MIXED = dict(min_samples=ta.MIN_SAMPLES, abs_tolerance2=ta.ABS2, rel_tolerance2=ta.REL2)
SHAPES = [(24, 16), (21, 13), (193, 131), (1, 1), (65536, 1), (1, 65536)]
SHAPE_IDS = [f"{w}x{h}" for w, h in SHAPES]
# the run's stopping case (the issue's): test_converge's parity input
STOP = dict(w=48, h=32, depth=1, check_every=5, max_frames=40, max_active=0)


# ---- the reference ---------------------------------------------------------------------------------
def order_key(a):
    """float32 bits as unsigned keys of the floats' order, +0 above -0."""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_float(k):
    k = np.uint32(k)
    b = k ^ np.uint32(0x80000000) if k & np.uint32(0x80000000) else ~k
    return np.array([b], np.uint32).view(F32)[0]


def bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def classes(img, err, spp, min_samples, abs_tolerance2, rel_tolerance2):
    """rt_progress.h's classification of an (H, W, 4) image with the (H, W) estimate `err`."""
    I, err = np.ascontiguousarray(img, F32), np.ascontiguousarray(err, F32)
    n = ta.f2u(I[..., 3])
    with np.errstate(all="ignore"):
        lm = tv.lum(I)
        thr = F32(abs_tolerance2) + F32(rel_tolerance2) * (lm * lm)
        assert thr.dtype == F32
        le = err <= thr                                       # a NaN on either side: False
    capped = ~(n < np.uint64(spp))
    converged = ~capped & (n >= np.uint64(min_samples)) & le
    active = ~capped & ~converged
    below = active & (n < np.uint64(min_samples))
    return SimpleNamespace(n=n, capped=capped, converged=converged, active=active, below_min=below,
                           no_history=active & ~below & np.isposinf(err),
                           nonfinite=~np.isfinite(I[..., :3]).all(-1))


def report_of(k, err, words):
    """The report of a classification (a dict of Python ints and the float32 max_error)."""
    with np.errstate(all="ignore"):
        finite_side = err < F32(np.inf)
    keys = order_key(err)[finite_side]
    return {"pixels": int(k.n.size), "active": int(k.active.sum()),
            "converged": int(k.converged.sum()), "capped": int(k.capped.sum()),
            "below_min": int(k.below_min.sum()), "no_history": int(k.no_history.sum()),
            "nonfinite": int(k.nonfinite.sum()), "samples": int(k.n.sum(dtype=np.uint64)),
            "active_tiles": int((words != 0).sum()),
            "min_count": int(k.n.min()) if k.n.size else 0xFFFFFFFF,
            "max_count": int(k.n.max()) if k.n.size else 0,
            "max_error": key_float(keys.max()) if keys.size else F32(-np.inf)}


def report_ref(img, spp, params, *, err=None, mom=None, min_history=4):
    """(report, tile_active words, classification) of rt_progress_stats for these arguments."""
    if mom is not None:
        err = tv.initial_variance(img, mom, min_history, np.inf)[0]
    k = classes(img, err, spp, **params)
    words = ta.tile_words(k.active)
    return report_of(k, np.ascontiguousarray(err, F32), words), words, k


def same_report(got, want, what=""):
    for f in FIELDS[:-1]:
        assert got[f] == want[f], f"{what}: {f} is {got[f]}, the reference has {want[f]}"
    assert bits(got["max_error"]) == bits(want["max_error"]), \
        f"{what}: max_error is {got['max_error']!r}, the reference has {want['max_error']!r}"


def combined(reports):
    """Reports of band sets that partition an image, combined as the header says."""
    out = {f: sum(r[f] for r in reports) for f in COUNTS}
    out["min_count"] = min(r["min_count"] for r in reports)
    out["max_count"] = max(r["max_count"] for r in reports)
    out["max_error"] = key_float(max(int(order_key(F32(r["max_error"]))[0]) for r in reports))
    return out


def run_ref(oracle, img, mom, cam, spheres, seeds, params, min_history, max_active, check_every):
    """rt_progress.h's loop over chain_ref: (frames_run, image, moments, report, words, the
    active counts of every report taken)."""
    spp = int(ta.f2u(F32(cam.samples_per_pixel)))
    seen = []

    def stats():
        rep, words, _ = report_ref(img, spp, params, mom=mom, min_history=min_history)
        seen.append(rep["active"])
        return rep, words

    done, max_frames = 0, len(seeds)
    if not cam.camera_has_moved > 0.5:
        rep, words = stats()
        if rep["active"] <= max_active:
            return SimpleNamespace(frames=0, img=img, mom=mom, report=rep, words=words, seen=seen)
    while True:
        f = min(check_every, max_frames - done)
        c = cam if done == 0 else cam.with_fields(camera_has_moved=0.0)
        last = tc.chain_ref(oracle, img, mom, c, spheres, seeds[done:done + f], params,
                            min_history)[-1]
        img, mom = last.img, last.mom
        done += f
        rep, words = stats()
        if rep["active"] <= max_active or done == max_frames:
            break
    return SimpleNamespace(frames=done, img=img, mom=mom, report=rep, words=words, seen=seen)


# ---- inputs ----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def mixed_planes(w, h):
    """test_adaptive's `mixed` accumulator and error plane at any shape."""
    if h >= 11 and w >= 16:
        return ta.planes(w, h, "mixed")
    img, err = ta.planes(256, 256, "mixed")
    if (w, h) == (1, 1):
        return img[9:10, 3:4], err[9:10, 3:4]                 # the NaN count: a first sample
    assert w * h == 256 * 256
    return img.reshape(h, w, 4), err.reshape(h, w)


@functools.lru_cache(None)
def moment_planes(w, h, kind):
    if kind == "parity":
        return tc.parity_planes(w, h)
    img, mom = ta.error_inputs(w, h)
    img.setflags(write=False)
    mom.setflags(write=False)
    return img, mom


PARITY = dict(spp=tc.SPP, params=tc.PARAMS, min_history=tc.MIN_HISTORY)
# error_inputs: counts 0..22 and NaN, k 0..8 and NaN; a quarter or so of the variances negative
ERRIN = dict(spp=15, params=dict(min_samples=3, abs_tolerance2=2e-3, rel_tolerance2=1e-3),
             min_history=4)


@functools.lru_cache(None)
def settled_planes(w, h):
    """Counts 16..20 and moments whose error is 0: every pixel converged below the cap."""
    img = ta.planes(w, h, "converged")[0]
    mom = np.empty((h, w, 4), F32)
    mom[:] = (0.5, 0.25, 0.0, 20.0)
    mom.setflags(write=False)
    return img, mom


@functools.lru_cache(None)
def stop_case():
    """The stopping case and its reference."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    w, h = STOP["w"], STOP["h"]
    cam = ta.make_camera(rt, w, h, STOP["depth"], True, tc.SPP)
    img, mom = tc.parity_planes(w, h)
    seeds = np.array(rt.frame_seeds(tc.SEED_SET, STOP["max_frames"]), F32)
    ref = run_ref(oracle, img, mom, cam, ta.scene().spheres, seeds, tc.PARAMS, tc.MIN_HISTORY,
                  STOP["max_active"], STOP["check_every"])
    return SimpleNamespace(w=w, h=h, cam=cam, sc=ta.scene(), img=img, mom=mom, seeds=seeds,
                           ref=ref)


# ---- CPU tests -------------------------------------------------------------------------------------
def test_library_exports_the_progress_entry_points(rt):
    text = HEADER.read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_progress_stats", "rt_progress_stats_bands", "rt_progress_run"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert {s for s in exported if "progress" in s} == set(declared)
    for s in declared:
        assert not any(k in s for k in ("converge", "adaptive", "variance", "moments", "denoise",
                                        "reproject"))
    L = rt._lib
    assert L.progress_symbols() == declared
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.selftest_roots_symbols(), L.denoise_symbols(), L.reproject_symbols(),
                  L.variance_symbols(), L.adaptive_symbols(), L.converge_symbols()):
        assert not set(declared) & set(other)
    abi = (ROOT / "include" / "rt_abi.h").read_text()
    # (rt_abi.h says "progressive sample" of rt_update: the word and the symbols are what it lacks)
    assert not re.search(r"progress(?!ive\b)", abi)
    in_abi = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", abi, flags=re.M)
    assert sorted(L.exported_symbols()) == sorted(in_abi) and len(in_abi) == 52
    assert L.lib().rt_abi_version() == 7
    assert '#include "rt_adaptive.h"' in text
    assert callable(rt.ComputeShaderPipeline.progress_report)
    assert callable(rt.ComputeShaderPipeline.render_to_tolerance)


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(rt, lang, std, cc, tmp_path):
    L = rt._lib
    sizes = (ctypes.sizeof(L.ProgressReportC), ctypes.sizeof(L.ProgressGoalC))
    assert sizes == (96, 16)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "rt_progress.h"\n'
                   f"typedef char report_size[sizeof(rt_progress_report) == {sizes[0]} ? 1 : -1];\n"
                   f"typedef char goal_size[sizeof(rt_progress_goal) == {sizes[1]} ? 1 : -1];\n"
                   "typedef char samples_at_56[offsetof(rt_progress_report, samples) == "
                   f"{L.ProgressReportC.samples.offset} ? 1 : -1];\n"
                   "typedef char max_error_at_80[offsetof(rt_progress_report, max_error) == "
                   f"{L.ProgressReportC.max_error.offset} ? 1 : -1];\n"
                   "typedef char check_every_at_12[offsetof(rt_progress_goal, check_every) == "
                   f"{L.ProgressGoalC.check_every.offset} ? 1 : -1];\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [f for f, _ in L.ProgressReportC._fields_][:12] == list(FIELDS)
    assert [f for f, _ in L.ProgressGoalC._fields_] == ["max_active", "max_frames", "check_every"]


def refusals(rt, ctx, px=None):
    """{what: (status, call)} of the argument checks: `ctx` is only passed on, and the buffers
    are the addresses px gives (device tensors on the GPU; any non-NULL value on the CPU, where
    no check may read them)."""
    L = rt._lib
    A, Z = RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE
    px = px or dict(image=0x1000, moments=0x2000, error=0x3000, mask=0x4000)
    cam = ta.make_camera(rt, 24, 16, 1, True, 500).to_c()
    seeds = np.zeros(8, F32)
    keep = dict(cam=cam, seeds=seeds, report=L.ProgressReportC(), done=ctypes.c_uint32(0xDEAD))
    ctypes.memset(ctypes.byref(keep["report"]), 0xAB, 96)

    def stats(params=(4, 1e-4, 1e-2), bands=None, form="moments", out=True, **kw):
        v = dict(ctx=ctx, image=px["image"], moments=px["moments"] if form == "moments" else None,
                 error=px["error"] if form == "error" else None, mask=px["mask"], w=24, h=16,
                 min_history=4)
        v.update(kw)
        pc = L.AdaptiveParamsC(*params) if params is not None else None
        head = (v["ctx"], v["image"], v["moments"], v["error"], v["mask"], v["w"], v["h"])
        tail = (20, ctypes.byref(pc) if pc is not None else None, v["min_history"], None,
                ctypes.byref(keep["report"]) if out else None)
        if bands is None:
            return L.lib().rt_progress_stats(*head, *tail)
        return L.lib().rt_progress_stats_bands(*head, bands[0], *tail)

    def run(params=(4, 1e-4, 1e-2), goal=(0, 8, 4), out=True, done=True, **kw):
        v = dict(ctx=ctx, image=px["image"], moments=px["moments"], mask=px["mask"], w=24, h=16,
                 cam=ctypes.byref(cam), seeds=ctypes.c_void_p(seeds.ctypes.data), min_history=4)
        v.update(kw)
        pc = L.AdaptiveParamsC(*params) if params is not None else None
        gc = L.ProgressGoalC(*goal) if goal is not None else None
        return L.lib().rt_progress_run(
            v["ctx"], v["image"], v["moments"], v["mask"], v["w"], v["h"], v["cam"], None, 0,
            v["seeds"], ctypes.byref(pc) if pc is not None else None, v["min_history"],
            ctypes.byref(gc) if gc is not None else None, None,
            ctypes.byref(keep["done"]) if done else None,
            ctypes.byref(keep["report"]) if out else None)

    band = L.band_sets([(0, 1, 2)])
    rows = {"ctx NULL": (RT_ERR_INVALID_CONTEXT, lambda: stats(ctx=None)),
            "image NULL": (A, lambda: stats(image=None)),
            "params NULL": (A, lambda: stats(params=None)),
            "out_report NULL": (A, lambda: stats(out=False)),
            "neither moments nor error": (A, lambda: stats(moments=None)),
            "both moments and error": (A, lambda: stats(error=px["error"])),
            "tile_active == image": (A, lambda: stats(mask=px["image"])),
            "tile_active == moments": (A, lambda: stats(mask=px["moments"])),
            "tile_active == error": (A, lambda: stats(form="error", mask=px["error"])),
            "min_samples 2^24 + 1": (A, lambda: stats(params=((1 << 24) + 1, 1e-4, 1e-2))),
            "min_history 0": (A, lambda: stats(min_history=0)),
            "min_history 2^24 + 1": (A, lambda: stats(min_history=(1 << 24) + 1)),
            "width 0": (Z, lambda: stats(w=0)), "height 0": (Z, lambda: stats(h=0)),
            "width 65537": (Z, lambda: stats(w=65537)), "height 65537": (Z, lambda: stats(h=65537)),
            "bands NULL": (A, lambda: stats(bands=(None,))),
            "bands: ctx NULL": (RT_ERR_INVALID_CONTEXT, lambda: stats(bands=(band,), ctx=None)),
            "bands past the image": (A, lambda: stats(bands=(L.band_sets([(1, 1, 2)]),))),
            "bands: step 0": (A, lambda: stats(bands=(L.band_sets([(0, 0, 1)]),))),
            "bands: neither": (A, lambda: stats(bands=(band,), moments=None)),
            "run: ctx NULL": (RT_ERR_INVALID_CONTEXT, lambda: run(ctx=None)),
            "run: image NULL": (A, lambda: run(image=None)),
            "run: moments NULL": (A, lambda: run(moments=None)),
            "run: camera NULL": (A, lambda: run(cam=None)),
            "run: random_seeds NULL": (A, lambda: run(seeds=None)),
            "run: params NULL": (A, lambda: run(params=None)),
            "run: goal NULL": (A, lambda: run(goal=None)),
            "run: frames_run NULL": (A, lambda: run(done=False)),
            "run: out_report NULL": (A, lambda: run(out=False)),
            "run: image == moments": (A, lambda: run(moments=px["image"])),
            "run: tile_active == image": (A, lambda: run(mask=px["image"])),
            "run: tile_active == moments": (A, lambda: run(mask=px["moments"])),
            "run: max_frames 0": (A, lambda: run(goal=(0, 0, 4))),
            "run: max_frames 65537": (A, lambda: run(goal=(0, 65537, 4))),
            "run: check_every 0": (A, lambda: run(goal=(0, 8, 0))),
            "run: check_every 65537": (A, lambda: run(goal=(0, 8, 65537))),
            "run: min_history 0": (A, lambda: run(min_history=0)),
            "run: min_samples 2^24 + 1": (A, lambda: run(params=((1 << 24) + 1, 1e-4, 1e-2))),
            "run: width 0": (Z, lambda: run(w=0)), "run: height 65537": (Z, lambda: run(h=65537))}
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf")),
                      ("-inf", float("-inf"))]:
        rows[f"abs_tolerance2 {what}"] = (A, lambda bad=bad: stats(params=(4, bad, 1e-2)))
        rows[f"rel_tolerance2 {what}"] = (A, lambda bad=bad: stats(form="error",
                                                                    params=(4, 1e-4, bad)))
        rows[f"run: abs_tolerance2 {what}"] = (A, lambda bad=bad: run(params=(4, bad, 1e-2)))
    # with an error plane min_history is not read
    return rows, keep, SimpleNamespace(stats=stats, run=run)


def outputs_untouched(keep):
    assert bytes(keep["report"]) == b"\xab" * 96, "a refused call wrote *out_report"
    assert keep["done"].value == 0xDEAD, "a refused call wrote *frames_run"


def test_argument_checks_without_a_device(rt):
    """Every refusal comes before the context is used: a context that is no context (zeroed
    bytes) is enough, and the outputs stay as they were."""
    fake = ctypes.create_string_buffer(1 << 16)
    rows, keep, _ = refusals(rt, ctypes.cast(fake, ctypes.c_void_p))
    for what, (status, call) in rows.items():
        assert call() == status, what
    outputs_untouched(keep)
    assert bytes(fake) == bytes(1 << 16)


@pytest.mark.parametrize("spp", [20, 10])
@pytest.mark.parametrize("shape", SHAPES[:3], ids=SHAPE_IDS[:3])
def test_mixed_inputs_reach_every_class(shape, spp):
    """From the reference alone: every class and sub-count, the threshold's edges, NaN and the
    counts u32() saturates or zeroes; and `active` is adaptive_ref's own sampled pixels."""
    w, h = shape
    img, err = mixed_planes(w, h)
    rep, words, k = report_ref(img, spp, MIXED, err=err)
    print(f"{w}x{h} spp {spp}: " + ", ".join(f"{f} {rep[f]}" for f in FIELDS))
    for f in COUNTS:
        assert rep[f] >= 1, f"{f} is never reached"
    assert rep["pixels"] == w * h == rep["active"] + rep["converged"] + rep["capped"]
    assert rep["below_min"] + rep["no_history"] < rep["active"]         # by_error and NaN too
    assert (k.capped.astype(int) + k.converged + k.active == 1).all()
    assert rep["min_count"] == 0 and rep["max_count"] == 0xFFFFFFFF
    assert rep["samples"] > 0xFFFFFFFF
    assert np.isfinite(rep["max_error"]) and rep["max_error"] > 0
    c = ta.case(w, h, 1, False, "mixed" if spp == 20 else "low_spp")
    assert (k.active == c.sampled).all() and (words == c.words).all()
    assert rep["active"] == sum(c.tally[r] for r in ta.SAMPLED_RULES)
    assert rep["capped"] == c.tally["capped"] and rep["converged"] == c.tally["converged"]
    assert rep["below_min"] == c.tally["below_min"] and rep["no_history"] == c.tally["inf_error"]
    # the planted texels
    assert k.active[9, 3] and k.below_min[9, 3]                    # a NaN count
    assert k.converged[9, 4] and k.n[9, 4] == 7                    # 7.5 counts as 7
    assert k.active[9, 6] and k.nonfinite[9, 6]                    # a NaN threshold
    assert k.capped[10, 3] and k.capped[10, 4] and k.n[10, 4] == 0xFFFFFFFF
    assert (k.converged if spp == 20 else k.capped)[10, 5]         # error == threshold; count 13
    idle, full, part = ta.tile_kinds(words, w, h)
    assert idle >= 1 and full >= 1 and part >= 1
    assert rep["active_tiles"] == full + part


@pytest.mark.parametrize("kind,args", [("parity", PARITY), ("error_inputs", ERRIN)])
def test_moment_inputs_reach_every_class(kind, args):
    w, h = 193, 131
    img, mom = moment_planes(w, h, kind)
    rep, words, k = report_ref(img, args["spp"], args["params"], mom=mom,
                               min_history=args["min_history"])
    print(f"{w}x{h} {kind}: " + ", ".join(f"{f} {rep[f]}" for f in FIELDS))
    for f in ("active", "converged", "capped", "below_min", "no_history", "active_tiles"):
        assert rep[f] >= 1, f"{f} is never reached"
    assert rep["pixels"] == w * h == rep["active"] + rep["converged"] + rep["capped"]
    if kind == "error_inputs":
        assert rep["below_min"] + rep["no_history"] < rep["active"]     # active by its error
        assert rep["min_count"] == 0 and rep["max_error"] > 0


def test_max_error_orders_floats_with_signed_zeros():
    a = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 1.0, 3e38], F32)
    k = order_key(a)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert all(bits(key_float(x)) == bits(y) for x, y in zip(k, a))
    img = np.zeros((1, 2, 4), F32)
    rep = report_of(classes(img, np.array([[-0.0, 0.0]], F32), 5, 0, 0.0, 0.0),
                    np.array([[-0.0, 0.0]], F32), np.zeros((1, 1), np.uint64))
    assert bits(rep["max_error"]) == 0                             # +0 is above -0
    none = np.array([[np.nan, np.inf]], F32)
    rep = report_of(classes(img, none, 5, 0, 0.0, 0.0), none, np.zeros((1, 1), np.uint64))
    assert rep["max_error"] == -np.inf and rep["no_history"] == 1 and rep["active"] == 2


def test_the_stopping_case_stops_in_the_middle():
    c = stop_case()
    r = c.ref
    print(f"stopping case: frames_run {r.frames}, active at each report {r.seen}, last report "
          + ", ".join(f"{f} {r.report[f]}" for f in FIELDS))
    first, *_ = r.seen
    assert first > 0 and report_ref(c.img, tc.SPP, tc.PARAMS, mom=c.mom,
                                    min_history=tc.MIN_HISTORY)[0]["below_min"] > 0
    assert 0 < r.frames < STOP["max_frames"] and r.frames in (5, 10, 15)
    assert r.frames % STOP["check_every"] == 0 and len(r.seen) == 1 + r.frames // 5
    assert r.seen[-1] == 0 and all(a > 0 for a in r.seen[:-1])
    assert r.report["active"] == 0 and r.report["active_tiles"] == 0


def test_the_budget_case_is_still_active_at_its_budget():
    c = tc.cap_case()
    for k in (3, 6, 7):
        fr = c.frames[k - 1]
        rep = report_ref(fr.img, 500, tc.CAP_PARAMS, mom=fr.mom, min_history=c.min_history)[0]
        assert rep["active"] > 0, f"nothing is active after {k} frames"


def test_settled_planes_are_settled():
    img, mom = settled_planes(24, 16)
    rep = report_ref(img, 500, tc.CAP_PARAMS, mom=mom, min_history=2)[0]
    assert rep["converged"] == rep["pixels"] == 24 * 16 and rep["active"] == 0
    assert rep["max_error"] == 0


# ---- GPU side --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


guarded, guarded_words, to_dev = ta.guarded, ta.guarded_words, ta.to_dev
tail_intact = ta.tail_intact


def run_report(p, img, w, h, spp, params, *, err=None, mom=None, min_history=4, mask=True,
               bands=None):
    """progress_report on host planes (compact local ones for a band set): (report, tile_active
    words or None), after the checks every call must pass."""
    rows = img.shape[0]
    tiles_y, tiles_x = (rows + 7) // 8, (w + 7) // 8
    a = to_dev(p, img)
    m = to_dev(p, mom) if mom is not None else None
    e = to_dev(p, err) if err is not None else None
    words = guarded_words(p, tiles_y * tiles_x) if mask else False
    rep, res = p.progress_report(a, w, h, spp, moments=m, error=e, min_history=min_history,
                                 tile_active=words, bands=bands, **params)
    assert (res is words) if mask else (res is None)
    assert bits_equal(a.cpu().numpy(), img)[0], "image was written"
    if m is not None:
        assert bits_equal(m.cpu().numpy(), mom)[0], "moments was written"
    if e is not None:
        assert bits_equal(e.cpu().numpy(), err)[0], "error was written"
    got = None
    if mask:
        got = tail_intact(words, tiles_y * tiles_x, "tile_active").view(np.uint64).reshape(
            tiles_y, tiles_x)
    return rep, got


@gpu
@pytest.mark.parametrize("spp", [20, 10])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_report_matches_reference_with_an_error_plane(rt, pipe, shape, spp):
    w, h = shape
    img, err = mixed_planes(w, h)
    want, words, _ = report_ref(img, spp, MIXED, err=err)
    got, got_words = run_report(pipe, img, w, h, spp, MIXED, err=err)
    same_report(got, want, f"{w}x{h}")
    assert (got_words == words).all(), "tile_active differs from the reference"
    if shape == SHAPES[0]:
        again, none = run_report(pipe, img, w, h, spp, MIXED, err=err, mask=False)
        assert none is None
        same_report(again, want, "without tile_active")


@gpu
@pytest.mark.parametrize("kind,args", [("parity", PARITY), ("error_inputs", ERRIN)])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_report_matches_reference_with_moments(rt, pipe, shape, kind, args):
    w, h = shape
    if kind == "parity" and (w < 16 or h < 8):
        kind, args = "error_inputs", dict(ERRIN, min_history=1)    # the thin shapes: both histories
    img, mom = moment_planes(w, h, kind)
    want, words, _ = report_ref(img, args["spp"], args["params"], mom=mom,
                                min_history=args["min_history"])
    got, got_words = run_report(pipe, img, w, h, args["spp"], args["params"], mom=mom,
                                min_history=args["min_history"])
    same_report(got, want, f"{w}x{h} {kind}")
    assert (got_words == words).all(), "tile_active differs from the reference"


@gpu
def test_samples_are_summed_in_64_bits(rt, pipe):
    w, h = 16, 8
    img = np.zeros((h, w, 4), F32)
    img[..., :3] = 0.25
    img[..., 3] = 2.0 ** 33
    err = np.zeros((h, w), F32)
    got, _ = run_report(pipe, img, w, h, 20, MIXED, err=err)
    same_report(got, report_ref(img, 20, MIXED, err=err)[0], "saturated counts")
    assert got["samples"] == 128 * 0xFFFFFFFF and got["max_count"] == 0xFFFFFFFF
    assert got["min_count"] == 0xFFFFFFFF and got["capped"] == 128
    img[3, 5, 3], img[6, 11, 3] = np.nan, -2.0
    got, _ = run_report(pipe, img, w, h, 20, MIXED, err=err)
    same_report(got, report_ref(img, 20, MIXED, err=err)[0], "with a NaN and a negative count")
    assert got["min_count"] == 0 and got["samples"] == 126 * 0xFFFFFFFF
    assert got["below_min"] == 2 == got["active"]


@gpu
@pytest.mark.parametrize("kind", ["mixed", "low_spp"])
def test_tile_active_is_the_mask_update_adaptive_writes(rt, pipe, kind):
    import torch
    w, h = 193, 131
    c = ta.case(w, h, 1, True, kind)
    spp = ta.SPP_OF[kind]
    a, e, out = to_dev(pipe, c.img), to_dev(pipe, c.err), pipe.new_image(w, h)
    sampled = pipe.update_adaptive(a, out, w, h, c.cam, c.sc, e, tile_mask=True, **MIXED)
    rep, active = pipe.progress_report(a, w, h, spp, error=e, tile_active=True, **MIXED)
    torch.cuda.synchronize()
    assert torch.equal(sampled, active), "tile_active is not the sampler's tile_mask"
    assert rep["active"] == int(c.sampled.sum()) > 0


@gpu
def test_tile_active_is_the_mask_one_converge_frame_writes(rt, pipe):
    import torch
    c = tc.case(48, 32, 1, True)
    a, m = to_dev(pipe, c.img), to_dev(pipe, c.mom)
    rep, active = pipe.progress_report(a, c.w, c.h, tc.SPP, moments=m,
                                       min_history=tc.MIN_HISTORY, tile_active=True, **tc.PARAMS)
    _, sampled, _ = pipe.converge(a, m, c.w, c.h, c.cam, c.sc, c.seeds[:1],
                                  min_history=tc.MIN_HISTORY, tile_mask=True, **tc.PARAMS)
    torch.cuda.synchronize()
    assert torch.equal(sampled, active), "tile_active is not the fused round's tile_mask"
    assert rep["active"] == int(c.frames[0].sampled.sum()) > 0


@gpu
@pytest.mark.parametrize("form", ["error", "moments"])
def test_band_sets(rt, pipe, form):
    """48 x 35: five bands, the last one of three rows.  The band sets (0, 2, 3) and (1, 2, 2)
    partition it: their reports combine into the whole image's and their masks are its rows.
    The rows of the local buffers below the image hold values that would count."""
    w, h = 48, 35
    if form == "error":
        img, plane = mixed_planes(w, h)
        kw = dict(spp=20, params=MIXED)
    else:
        img, plane = moment_planes(w, h, "error_inputs")
        kw = dict(spp=ERRIN["spp"], params=ERRIN["params"], min_history=ERRIN["min_history"])
    key = "err" if form == "error" else "mom"
    whole, whole_words, _ = report_ref(img, **kw, **{key: plane})
    got_whole, _ = run_report(pipe, img, w, h, kw["spp"], kw["params"],
                              min_history=kw.get("min_history", 4), **{key: plane})
    same_report(got_whole, whole, "the whole image")
    parts = []
    for bands in ((0, 2, 3), (1, 2, 2)):
        gb = [bands[0] + j * bands[1] for j in range(bands[2])]
        rows = np.concatenate([np.arange(8 * b, 8 * b + 8) for b in gb])
        on = rows < h
        local_img = np.full((rows.size, w, 4), 3.0, F32)         # off the image: counts of 3
        local_plane = np.full((rows.size,) + plane.shape[1:], np.inf, F32)
        local_img[on], local_plane[on] = img[rows[on]], plane[rows[on]]
        want, want_words, _ = report_ref(img[rows[on]], **kw, **{key: plane[rows[on]]})
        got, got_words = run_report(pipe, local_img, w, h, kw["spp"], kw["params"],
                                    min_history=kw.get("min_history", 4), bands=bands,
                                    **{key: local_plane})
        same_report(got, want, f"band set {bands}")
        assert (got_words == whole_words[gb]).all(), f"band set {bands}: the mask rows differ"
        assert (got_words == want_words).all()
        parts.append(got)
    assert sum(p["pixels"] for p in parts) == w * h
    same_report(combined(parts), whole, "the band sets combined")
    # an empty band set: the report of no pixels, nothing written
    words = guarded_words(pipe, 6)
    rep, _ = pipe.progress_report(to_dev(pipe, img[:8]), w, h, 20,
                                  error=to_dev(pipe, img[:8, :, 0]), tile_active=words,
                                  bands=(0, 1, 0), **MIXED)
    assert (words.cpu().numpy() == np.int64(SENT_WORD)).all()
    assert all(rep[f] == 0 for f in COUNTS + ("max_count",))
    assert rep["min_count"] == 0xFFFFFFFF and rep["max_error"] == -np.inf


@gpu
def test_repeated_and_side_stream_calls_give_the_same_bytes(rt, pipe):
    import torch
    L = rt._lib
    w, h = 193, 131
    img, mom = moment_planes(w, h, "error_inputs")
    a, m = to_dev(pipe, img), to_dev(pipe, mom)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    params = L.AdaptiveParamsC(*(ERRIN["params"][k] for k in ("min_samples", "abs_tolerance2",
                                                              "rel_tolerance2")))

    def once():
        words = guarded_words(pipe, tiles)
        rep = L.ProgressReportC()
        L.call("rt_progress_stats", pipe._ctx, a.data_ptr(), m.data_ptr(), None,
               words.data_ptr(), w, h, ERRIN["spp"], ctypes.byref(params), ERRIN["min_history"],
               pipe._stream(), ctypes.byref(rep))
        return bytes(rep), tail_intact(words, tiles, "tile_active").tobytes()

    first, second = once(), once()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = once()
    side.synchronize()
    assert first == second == third
    assert first[0][84:] == bytes(12), "the reserved words are not 0"
    want = report_ref(img, ERRIN["spp"], ERRIN["params"], mom=mom,
                      min_history=ERRIN["min_history"])[0]
    same_report(pipe._report_dict(L.ProgressReportC.from_buffer_copy(first[0])), want, "raw call")


@gpu
def test_following_calls_are_undisturbed(rt, oracle):
    """A report and a zero-frame run between two rt_update_frames calls: the second call's
    image is the oracle's chain over all the seeds, and rt_last_launch_info stays."""
    import torch
    w, h, depth = 24, 16, 3
    still = ta.make_camera(rt, w, h, depth, True, 500)
    seeds = np.array(rt.frame_seeds(3, 6), F32)
    start = ta.planes(w, h, "converged")[0]
    simg, smom = settled_planes(w, h)
    p = rt.ComputeShaderPipeline(0)
    try:
        bufs = [to_dev(p, start), p.new_image(w, h)]
        newest = p.update_frames(bufs[0], bufs[1], w, h, still, ta.scene(), seeds[:3])
        info = p.last_launch_info()
        rep, _ = p.progress_report(bufs[newest], w, h, 500, moments=to_dev(p, smom),
                                   min_history=2, tile_active=True, **tc.CAP_PARAMS)
        assert rep["pixels"] == w * h
        a, m = to_dev(p, simg), to_dev(p, smom)
        done, rep, _ = p.render_to_tolerance(a, m, w, h, still, ta.scene(), seeds,
                                             min_history=2, **tc.CAP_PARAMS)
        assert done == 0 and rep["active"] == 0
        assert p.last_launch_info() == info
        again = p.update_frames(bufs[newest], bufs[1 - newest], w, h, still, ta.scene(),
                                seeds[3:])
        torch.cuda.synchronize()
        chain = fd.oracle_chain(oracle, start, still, ta.scene().spheres, seeds)
        got = bufs[newest if again == 0 else 1 - newest].cpu().numpy()
        assert bits_equal(got, chain[-1])[0], "a following rt_update_frames differs"
    finally:
        p.close()


def run_to_tolerance(p, img, mom, w, h, cam, sc, seeds, params, min_history, **goal):
    """render_to_tolerance on copies of host planes: frames_run, report, numpy image, moments
    and mask words, the device tensors."""
    tiles_y, tiles_x = (h + 7) // 8, (w + 7) // 8
    a, m = guarded(p, 4 * w * h, img), guarded(p, 4 * w * h, mom)
    words = guarded_words(p, tiles_y * tiles_x)
    done, rep, res = p.render_to_tolerance(a, m, w, h, cam, sc, seeds, min_history=min_history,
                                           tile_active=words, **goal, **params)
    assert res is words
    return SimpleNamespace(
        frames=done, report=rep, a=a, m=m,
        img=tail_intact(a, 4 * w * h, "image").reshape(h, w, 4),
        mom=tail_intact(m, 4 * w * h, "moments").reshape(h, w, 4),
        words=tail_intact(words, tiles_y * tiles_x, "tile_active").view(np.uint64).reshape(
            tiles_y, tiles_x))


def check_run(got, ref, what):
    assert got.frames == ref.frames, f"{what}: frames_run {got.frames}, reference {ref.frames}"
    same, bad = bits_equal(got.img, ref.img)
    assert same, f"{what}: {bad} values of the image differ from the reference"
    same, bad = bits_equal(got.mom, ref.mom)
    assert same, f"{what}: {bad} values of the moments differ from the reference"
    same_report(got.report, ref.report, what)
    assert (got.words == ref.words).all(), f"{what}: tile_active differs"


@gpu
def test_run_stops_when_nothing_is_active(rt, pipe):
    import torch
    c = stop_case()
    got = run_to_tolerance(pipe, c.img, c.mom, c.w, c.h, c.cam, c.sc, c.seeds, tc.PARAMS,
                           tc.MIN_HISTORY, max_active=STOP["max_active"],
                           check_every=STOP["check_every"])
    check_run(got, c.ref, "the stopping case")
    assert 0 < got.frames < STOP["max_frames"]
    # one rt_converge_frames call of frames_run frames
    a, m = to_dev(pipe, c.img), to_dev(pipe, c.mom)
    pipe.converge(a, m, c.w, c.h, c.cam, c.sc, c.seeds[:got.frames], min_history=tc.MIN_HISTORY,
                  **tc.PARAMS)
    torch.cuda.synchronize()
    assert bits_equal(a.cpu().numpy(), got.img)[0], "the image differs from one converge call"
    assert bits_equal(m.cpu().numpy(), got.mom)[0], "the moments differ from one converge call"
    # the last report is a fresh one of the result
    fresh, words = pipe.progress_report(a, c.w, c.h, tc.SPP, moments=m,
                                        min_history=tc.MIN_HISTORY, tile_active=True, **tc.PARAMS)
    same_report(fresh, got.report, "a fresh report of the result")
    assert (words.cpu().numpy().view(np.uint64).reshape(got.words.shape) == got.words).all()


@gpu
def test_run_ends_at_its_budget(rt, pipe):
    """samples_per_pixel 500 and cap_case's tolerances: 3 + 3 + 1 frames, then the budget."""
    c = tc.cap_case()
    seeds = c.seeds[:7]
    from oracle import oracle
    ref = run_ref(oracle, c.img, c.mom, c.cam, c.sc.spheres, seeds, c.params, c.min_history, 0, 3)
    assert ref.frames == 7 and len(ref.seen) == 4 and min(ref.seen) > 0
    assert bits_equal(ref.img, c.frames[6].img)[0] and bits_equal(ref.mom, c.frames[6].mom)[0]
    got = run_to_tolerance(pipe, c.img, c.mom, c.w, c.h, c.cam, c.sc, seeds, c.params,
                           c.min_history, max_active=0, check_every=3)
    check_run(got, ref, "budget first")
    assert got.frames == 7 and got.report["active"] > 0
    # a goal the first report already meets by max_active alone
    loose = run_to_tolerance(pipe, c.img, c.mom, c.w, c.h, c.cam, c.sc, seeds, c.params,
                             c.min_history, max_active=c.w * c.h, check_every=3)
    assert loose.frames == 0 and bits_equal(loose.img, c.img)[0]


@gpu
def test_run_of_a_settled_image_runs_nothing(rt, pipe):
    w, h = 24, 16
    img, mom = settled_planes(w, h)
    cam = ta.make_camera(rt, w, h, 1, True, 500)
    seeds = np.array(rt.frame_seeds(5, 8), F32)
    got = run_to_tolerance(pipe, img, mom, w, h, cam, ta.scene(), seeds, tc.CAP_PARAMS, 2,
                           max_active=0, check_every=4)
    assert got.frames == 0
    assert bits_equal(got.img, img)[0] and bits_equal(got.mom, mom)[0], "a buffer was written"
    want, words, _ = report_ref(img, 500, tc.CAP_PARAMS, mom=mom, min_history=2)
    same_report(got.report, want, "already settled")
    assert not got.words.any() and (got.words == words).all()


@gpu
def test_run_with_a_moved_camera_runs_its_first_batch(rt, pipe, oracle):
    """The settled planes with camera_has_moved: no first report, frame 0 resets the image."""
    w, h = 24, 16
    img, mom = settled_planes(w, h)
    cam = ta.make_camera(rt, w, h, 1, True, 500, moved=True)
    seeds = np.array(rt.frame_seeds(5, 4), F32)
    ref = run_ref(oracle, img, mom, cam, ta.scene().spheres, seeds, tc.CAP_PARAMS, 2, 0, 2)
    assert ref.frames >= 2 and len(ref.seen) == ref.frames // 2     # no report before frame 0
    assert ref.img[..., 3].max() == ref.frames                      # the reset took the counts
    got = run_to_tolerance(pipe, img, mom, w, h, cam, ta.scene(), seeds, tc.CAP_PARAMS, 2,
                           max_active=0, check_every=2)
    check_run(got, ref, "a moved camera")


@gpu
def test_refused_calls_launch_nothing(rt, pipe):
    import torch
    w, h = 24, 16
    image, moments = guarded(pipe, 4 * w * h), guarded(pipe, 4 * w * h)
    plane, words = guarded(pipe, w * h), guarded_words(pipe, 6)
    px = dict(image=image.data_ptr(), moments=moments.data_ptr(), error=plane.data_ptr(),
              mask=words.data_ptr())
    rows, keep, calls = refusals(rt, pipe._ctx, px)
    for what, (status, call) in rows.items():
        assert call() == status, what
    outputs_untouched(keep)
    torch.cuda.synchronize()
    for t, what in ((image, "image"), (moments, "moments"), (plane, "error")):
        assert (t.cpu().numpy() == F32(SENT)).all(), f"a refused call wrote {what}"
    assert (words.cpu().numpy() == np.int64(SENT_WORD)).all(), "a refused call wrote tile_active"
    with pytest.raises(ValueError):
        pipe.progress_report(image, w, h, 20)
    with pytest.raises(ValueError):
        pipe.progress_report(image, w, h, 20, moments=moments, error=plane)
    with pytest.raises(ValueError):
        pipe.progress_report(image.cpu(), w, h, 20, error=plane)
    with pytest.raises(ValueError):
        pipe.render_to_tolerance(image, moments[:8], w, h, None, None, [0.5])
    # the ends of the ranges are accepted, and the context still works
    img, mom = settled_planes(w, h)
    image[:4 * w * h] = to_dev(pipe, img).reshape(-1)
    moments[:4 * w * h] = to_dev(pipe, mom).reshape(-1)
    assert calls.stats(params=(1 << 24, 0.0, 0.0), min_history=1 << 24) == 0
    assert calls.stats(form="error", min_history=0) == 0            # not read with an error plane
    assert keep["report"].pixels == w * h
    assert calls.run(goal=(w * h, 65536, 65536)) == 0 and keep["done"].value == 0
