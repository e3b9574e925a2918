"""Variance-driven adaptive sampling (include/rt_adaptive.h): rt_adaptive_error,
rt_update_adaptive, rt_update_adaptive_bands, rt_adaptive_params_default.

The reference is in this file: `adaptive_ref`, a NumPy float32 restatement of the header's rule
built on the CPU oracle's `update` — once with the camera as given (the sampled texels) and once
with samples_per_pixel 0 (the texels that pass through) — which also tallies the rule every pixel
falls under and forms the tile mask.  The error plane's reference is tests/test_variance.py's
`initial_variance` with +inf as the fallback.  Every GPU output is compared bit for bit
(NaN == NaN), and a sentinel tail follows every buffer the library writes.

A *case* is an input that mixes every rule (`mixed`: samples_per_pixel at the largest count;
`low_spp`: samples_per_pixel below many counts) at one of the three shapes; the CPU tests count
from the reference alone that each case reaches every rule and every kind of tile (printed with
-s).  The other inputs are extremes that by their nature reach one rule: a reset and `active`
(every pixel sampled), `converged` (none), and `mixed` without spheres.
"""
import ctypes
import functools
import math
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import test_fast_domains as fd
import test_variance as tv
from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_adaptive.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
SENT = -12345.0
SENT_WORD = 0x5A5A5A5A5A5A5A5A     # the tile mask's sentinel (int64)
TAIL = 16                          # elements of sentinel after every buffer the library writes
DEFAULTS = (16, 1e-5, 2.5e-4)      # min_samples, abs_tolerance2, rel_tolerance2
RULES = ("below_min", "by_error", "nan_error", "inf_error", "converged", "capped")
SAMPLED_RULES = RULES[:4]
# the parity inputs' parameters: thresholds the planted error values sit on and next to
MIN_SAMPLES, ABS2, REL2 = 4, 1e-4, 1e-2
SHAPES = [(24, 16), (21, 13), (193, 131)]   # whole tiles; ragged; 25 tile columns (4 k + 1)
INPUTS = ("mixed", "low_spp", "reset", "no_spheres", "converged", "active")
CASE_INPUTS = ("mixed", "low_spp")


# ---- the reference ---------------------------------------------------------------------------------
def f2u(a):
    """WGSL u32(f32): truncate, saturate, NaN and negatives -> 0 (as uint64 values)."""
    a = np.asarray(a, F32)
    out = np.zeros(a.shape, np.uint64)
    with np.errstate(all="ignore"):
        pos = a > 0
        big = a >= F32(4294967296.0)
        out[pos & ~big] = a[pos & ~big].astype(np.uint64)
    out[big] = 0xFFFFFFFF
    return out


def tile_words(sampled):
    """The tile mask of an (H, W) bool array: (tile rows, tile columns) uint64, bit
    (y & 7) * 8 + (x & 7); lanes off the image are 0."""
    h, w = sampled.shape
    ty, tx = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((ty * 8, tx * 8), bool)
    pad[:h, :w] = sampled
    bits = pad.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)
    return (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def adaptive_ref(oracle, inp, cam, spheres, error, min_samples, abs2, rel2, counts=None):
    """rt_update_adaptive's text over an (H, W, 4) float32 image: (out, tile mask words, the
    sampled pixels).  With `counts` (a dict) it tallies the pixels under each rule."""
    I = np.ascontiguousarray(inp, F32)
    err = np.ascontiguousarray(error, F32)
    spheres = np.ascontiguousarray(spheres, F32).reshape(-1, 8)
    full, _ = oracle.update(I, cam.blob, spheres)
    passed, _ = oracle.update(I, cam.with_fields(samples_per_pixel=0.0).blob, spheres)
    spp = int(f2u(F32(cam.samples_per_pixel)))
    rule = np.empty(I.shape[:2], "U9")
    if cam.camera_has_moved > 0.5:
        rule[:] = "below_min" if 0 < spp else "capped"
    else:
        n = f2u(I[..., 3])
        with np.errstate(all="ignore"):
            lm = tv.lum(I)
            thr = F32(abs2) + F32(rel2) * (lm * lm)
            assert thr.dtype == F32
            le = err <= thr
        unordered = np.isnan(err) | np.isnan(thr)
        rule[:] = "by_error"
        rule[le] = "converged"
        rule[unordered] = "nan_error"
        rule[~unordered & ~le & np.isposinf(err)] = "inf_error"
        rule[n < min_samples] = "below_min"
        rule[n >= spp] = "capped"
    sampled = np.isin(rule, SAMPLED_RULES)
    out = np.where(sampled[..., None], full, passed)
    assert out.dtype == F32
    if counts is not None:
        counts.update({k: int((rule == k).sum()) for k in RULES})
    return out, tile_words(sampled), sampled


def tile_kinds(words, w, h):
    """(tiles without a sampled pixel, tiles with all 64, partial tiles) of a mask."""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    return int((words == 0).sum()), int((words == full).sum()), \
        int(((words != 0) & (words != full)).sum())


# ---- inputs ----------------------------------------------------------------------------------------
def make_camera(rt, w, h, depth, defocus, spp, moved=False, seed=0.375, **kw):
    s = rt.CameraSettings(max_depth=depth, samples_per_pixel=spp, camera_has_moved=moved,
                          defocus_angle=0.6 if defocus else 0.0, **kw)
    return rt.SceneCamera.from_settings(s, w, h, seed)


@functools.lru_cache(None)
def scene():
    import gpu_ray_tracing as rt
    return rt.create_default_spheres(seed=1)


@functools.lru_cache(None)
def planes(w, h, kind):
    """(accumulator, error plane) of an input kind.  `mixed`: colours in [0, 1.5), counts 0..20
    by position, and error values placed on the pixel's own threshold: 0, four times it, NaN,
    +inf, exactly it (converged: <=), the next float above it (not converged) and half of it.
    Tile (0, 0) holds count 0 (all 64 sampled), tile (1, 0) count 20 and error 0 (none), and a
    few texels of tile (0, 1) hold the counts and colours u32() and the comparison treat
    specially."""
    rng = np.random.default_rng(1000 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 4), F32)
    img[..., :3] = (rng.random((h, w, 3)) * 1.5).astype(F32)
    img[..., 3] = (5 * xx + 3 * yy) % 21
    if kind == "converged":
        img[..., 3] = 16 + (xx + yy) % 5
        err = np.zeros((h, w), F32)
    elif kind == "active":
        err = np.full((h, w), np.inf, F32)
    else:
        img[0:8, 0:8, 3] = 0.0
        img[0:8, 8:16, 3] = 20.0
        lm = tv.lum(img)
        thr = F32(ABS2) + F32(REL2) * (lm * lm)
        sel = (xx + 3 * yy) % 7
        err = np.select([sel == 0, sel == 1, sel == 2, sel == 3, sel == 4, sel == 5],
                        [np.zeros_like(thr), F32(4.0) * thr, F32(np.nan), F32(np.inf), thr,
                         np.nextafter(thr, F32(np.inf))], F32(0.5) * thr).astype(F32)
        err[0:8, 8:16] = 0.0
        img[9, 3, 3] = np.nan              # u32(NaN) = 0: a first sample
        img[9, 4, 3], err[9, 4] = 7.5, 0   # converged: passes through as 7
        img[9, 5, 3] = -3.0                # u32(-3) = 0
        img[9, 6, 1], img[9, 6, 3], err[9, 6] = np.nan, 5.0, 0   # a NaN threshold: not converged
        img[10, 3, 3] = 3e9                # above every cap
        img[10, 4, 3] = 2.0 ** 33          # saturates: passes through as 2^32
        img[10, 5, :3], err[10, 5] = (0.0, 0.0, 0.0), ABS2   # thr = abs_tolerance2 itself
    img.setflags(write=False)
    err.setflags(write=False)
    return img, err


PLANES_OF = {"mixed": "mixed", "low_spp": "mixed", "reset": "mixed", "no_spheres": "mixed",
             "converged": "converged", "active": "active"}
SPP_OF = {"mixed": 20, "low_spp": 10, "reset": 500, "no_spheres": 20, "converged": 500,
          "active": 500}


def camera_kw(domain):
    """`domain` False: test_fast_domains' camera below the proven ray length (no lens, focus
    distance 2^-7), which the camera-ray-only instance refuses."""
    return {} if domain else {"focus_distance": 2.0 ** -7}


@functools.lru_cache(None)
def case(w, h, depth, defocus, kind, domain=True):
    """One parity input and its reference (computed once, read-only)."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    img, err = planes(w, h, PLANES_OF[kind])
    cam = make_camera(rt, w, h, depth, defocus and domain, SPP_OF[kind], moved=kind == "reset",
                      **camera_kw(domain))
    sc = scene() if kind != "no_spheres" else rt.SphereCollection(np.zeros((0, 8), F32))
    tally = {}
    out, words, sampled = adaptive_ref(oracle, img, cam, sc.spheres, err, MIN_SAMPLES, ABS2, REL2,
                                       tally)
    for a in (out, words, sampled):
        a.setflags(write=False)
    return SimpleNamespace(w=w, h=h, cam=cam, sc=sc, img=img, err=err, out=out, words=words,
                           sampled=sampled, tally=tally, kind=kind)


# ---- CPU tests -------------------------------------------------------------------------------------
def test_library_exports_the_adaptive_entry_points(rt):
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", HEADER.read_text(), flags=re.M)
    assert declared == ["rt_adaptive_params_default", "rt_adaptive_error", "rt_update_adaptive",
                        "rt_update_adaptive_bands"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert {s for s in exported if "adaptive" in s} == set(declared)
    for s in declared:
        assert not any(k in s for k in ("variance", "moments", "denoise", "reproject"))
    L = rt._lib
    assert L.adaptive_symbols() == declared
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.selftest_roots_symbols(), L.denoise_symbols(), L.reproject_symbols(),
                  L.variance_symbols()):
        assert not set(declared) & set(other)
    assert L.lib().rt_abi_version() == 7
    assert ctypes.sizeof(L.AdaptiveParamsC) == 12
    assert [f for f, _ in L.AdaptiveParamsC._fields_] == ["min_samples", "abs_tolerance2",
                                                         "rel_tolerance2"]
    p = L.AdaptiveParamsC(99, -1.0, -1.0)
    L.lib().rt_adaptive_params_default(ctypes.byref(p))
    assert (p.min_samples, p.abs_tolerance2, p.rel_tolerance2) == (16, F32(1e-5), F32(2.5e-4))
    L.lib().rt_adaptive_params_default(None)                    # a no-op, not a crash
    d = rt.ADAPTIVE_DEFAULTS
    assert (d["min_samples"], d["abs_tolerance2"], d["rel_tolerance2"]) == DEFAULTS
    assert callable(rt.ComputeShaderPipeline.adaptive_error)
    assert callable(rt.ComputeShaderPipeline.update_adaptive)
    assert "rt_abi.h" in HEADER.read_text() and "adaptive" not in \
        (ROOT / "include" / "rt_abi.h").read_text()


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "rt_adaptive.h"\n'
                   "typedef char params_are_12_bytes[sizeof(rt_adaptive_params) == 12 ? 1 : -1];\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("kind", CASE_INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cases_reach_their_rules_and_tiles(shape, kind):
    w, h = shape
    c = case(w, h, 1, False, kind)
    none, full, part = tile_kinds(c.words, w, h)
    print(f"{w}x{h} {kind}: " + ", ".join(f"{k} {c.tally[k]}" for k in RULES)
          + f"; tiles: {none} idle, {full} full, {part} partial")
    assert sum(c.tally.values()) == w * h
    for k in RULES:
        assert c.tally[k] >= 1, f"never reaches {k}"
    assert none >= 1 and full >= 1 and part >= 1
    assert int(c.sampled.sum()) == sum(c.tally[k] for k in SAMPLED_RULES)
    assert sum(bin(int(v)).count("1") for v in c.words.ravel()) == int(c.sampled.sum())
    # the planted texels: what passes through is rt_update's own rewrite of the count
    assert c.out[9, 4, 3] == 7.0 and not c.sampled[9, 4]
    assert c.out[10, 4, 3] == 2.0 ** 32 and not c.sampled[10, 4]
    assert c.sampled[9, 3] and c.out[9, 3, 3] == 1.0 and c.sampled[9, 5] and c.sampled[9, 6]
    assert not c.sampled[10, 5]                                  # error == threshold
    assert bits_equal(c.out[~c.sampled][:, :3], c.img[~c.sampled][:, :3])[0]
    n_in = f2u(c.img[..., 3])[c.sampled]
    assert (c.out[c.sampled][:, 3] == (n_in + 1).astype(F32)).all()


def test_ragged_shape_has_off_image_lanes_with_zero_bits():
    w, h = 21, 13
    for kind in INPUTS:
        c = case(w, h, 1, False, kind)
        assert c.words.shape == (2, 3)
        yy, xx = np.mgrid[0:16, 0:24]
        off = (xx >= w) | (yy >= h)
        bits = off.reshape(2, 8, 3, 8).transpose(0, 2, 1, 3).reshape(2, 3, 64)
        off_words = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(
            -1, dtype=np.uint64)
        assert off_words[:, 2].all() and off_words[1].all()      # the ragged column and row
        assert not (c.words & off_words).any(), kind
    # every pixel sampled: the mask is exactly the on-image lanes
    assert (case(w, h, 1, False, "active").words == ~off_words).all()


def test_extreme_inputs_reach_what_they_are_for():
    for w, h in SHAPES:
        assert case(w, h, 1, False, "reset").sampled.all()
        assert case(w, h, 1, False, "active").sampled.all()
        assert not case(w, h, 1, False, "converged").sampled.any()
        c = case(w, h, 1, False, "converged")
        assert bits_equal(c.out, c.img)[0]                       # integral counts: I itself
        c = case(w, h, 3, False, "no_spheres")
        assert c.sc.count == 0 and c.sampled.any() and not c.sampled.all()
    for depth in (1, 3):
        c = case(24, 16, depth, False, "mixed", False)
        assert not fd.camera_rays_bounded(c.cam, 24, 16, c.sc.spheres)[0]
        assert fd.camera_rays_bounded(case(24, 16, depth, True, "mixed").cam, 24, 16,
                                      scene().spheres)[0]


def _rmse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


QW, QH, QDEPTH, QROUNDS = 96, 64, 8, 96


@functools.lru_cache(None)
def quality_reference():
    import gpu_ray_tracing as rt
    from oracle import oracle
    cam = make_camera(rt, QW, QH, QDEPTH, True, 100000)
    ref, _ = oracle.render(np.zeros((QH, QW, 4), F32), cam.blob, scene().spheres,
                           rt.frame_seeds(1024, 1024))
    return ref


@pytest.mark.slow
@pytest.mark.parametrize("seed_set", [7, 5])
def test_adaptive_beats_uniform_at_equal_samples(rt, oracle, seed_set):
    """96 rounds of adaptive_ref + moments_ref + the error plane with the default parameters,
    against ceil(mean spp) uniform frames of the same seeds: RMSE over rgb against 1024 spp."""
    ref = quality_reference()
    sph = scene().spheres
    cam = make_camera(rt, QW, QH, QDEPTH, True, 100000)
    seeds = rt.frame_seeds(seed_set, QROUNDS)
    frames = [cam.with_fields(random_seed=float(s), camera_has_moved=1.0 if k == 0 else 0.0)
              for k, s in enumerate(seeds)]
    acc = mom = np.zeros((QH, QW, 4), F32)
    err = np.full((QH, QW), np.inf, F32)
    for c in frames:
        new, _, _ = adaptive_ref(oracle, acc, c, sph, err, *DEFAULTS)
        mom, acc = tv.moments_ref(acc, new, mom), new
        err = tv.initial_variance(acc, mom, 4, np.inf)[0]
    mean_spp = float(acc[..., 3].mean())
    uni = np.zeros((QH, QW, 4), F32)
    for c in frames[:math.ceil(mean_spp)]:
        uni, _ = oracle.update(uni, c.blob, sph)
    a, u = _rmse(acc, ref), _rmse(uni, ref)
    print(f"frame_seeds({seed_set}, .): mean spp {mean_spp:.1f} (min {acc[..., 3].min():.0f}, "
          f"max {acc[..., 3].max():.0f}), adaptive RMSE {a:.4f}, uniform RMSE {u:.4f} at "
          f"{math.ceil(mean_spp)} spp")
    assert mean_spp < QROUNDS
    assert a < u


# ---- GPU side --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


@pytest.fixture
def scan(request, pipe):
    pipe.set_scan_mode(request.param)
    yield request.param
    pipe.set_scan_mode("culled")


SCANS = ["culled", "exhaustive"]


def guarded(p, n, fill=None):
    """n floats (a copy of `fill`, or sentinels) followed by TAIL sentinels, on the device."""
    import torch
    t = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=p.torch_device)
    if fill is not None:
        t[:n] = torch.from_numpy(np.array(fill, F32).reshape(-1)).to(p.torch_device)
    return t


def guarded_words(p, n):
    import torch
    return torch.full((n + TAIL,), SENT_WORD, dtype=torch.int64, device=p.torch_device)


def tail_intact(t, n, what):
    got = t.cpu().numpy()
    sent = F32(SENT) if got.dtype == F32 else np.int64(SENT_WORD)
    assert (got[n:] == sent).all(), f"the tail after {what} was written"
    return got[:n]


def to_dev(p, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(p.torch_device)


def run_adaptive(p, c, mask=True, bands=None, rows=None):
    """update_adaptive on a case's planes (or the rows `rows` of them, for a band set): (out,
    mask words or None) as numpy, after the checks every call must pass."""
    import torch
    img = c.img if rows is None else c.img[rows]
    err = c.err if rows is None else c.err[rows]
    h = img.shape[0]
    px = c.w * h
    tiles = ((c.w + 7) // 8) * ((h + 7) // 8)
    inp, e = to_dev(p, img), to_dev(p, err)
    out = guarded(p, 4 * px)
    words = guarded_words(p, tiles) if mask else False
    res = p.update_adaptive(inp, out, c.w, c.h, c.cam, c.sc, e, min_samples=MIN_SAMPLES,
                            abs_tolerance2=ABS2, rel_tolerance2=REL2, tile_mask=words,
                            bands=bands)
    torch.cuda.current_stream().synchronize()
    assert (res is words) if mask else (res is None)
    assert bits_equal(inp.cpu().numpy(), img)[0], "in was written"
    assert bits_equal(e.cpu().numpy(), err)[0], "error was written"
    got = tail_intact(out, 4 * px, "out").reshape(h, c.w, 4)
    got_words = None
    if mask:
        got_words = tail_intact(words, tiles, "tile_mask").view(np.uint64).reshape(
            (h + 7) // 8, (c.w + 7) // 8)
    return got, got_words


def check(got, got_words, c, what=""):
    same, bad = bits_equal(got, c.out)
    assert same, f"{what}: {bad} values of out differ from the reference"
    if got_words is not None:
        assert (got_words == c.words).all(), f"{what}: the tile mask differs from the reference"


@gpu
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("defocus", [True, False], ids=["lens", "pinhole"])
@pytest.mark.parametrize("scan", SCANS, indirect=True)
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_and_mask_match_reference(rt, pipe, shape, depth, scan, defocus, kind):
    import torch
    c = case(shape[0], shape[1], depth, defocus, kind)
    got, words = run_adaptive(pipe, c)
    check(got, words, c, kind)
    if kind == "active":
        # every pixel sampled: rt_update's own output
        a, b = to_dev(pipe, c.img), pipe.new_image(c.w, c.h)
        pipe.update(a, b, c.w, c.h, c.cam, c.sc)
        torch.cuda.synchronize()
        assert bits_equal(got, b.cpu().numpy())[0], "all-active differs from rt_update"
    if kind == "mixed":
        got2, none = run_adaptive(pipe, c, mask=False)            # the mask is optional
        assert none is None and bits_equal(got2, c.out)[0]


@gpu
@pytest.mark.parametrize("kind", ["mixed", "reset", "active"])
@pytest.mark.parametrize("depth", [1, 3])
def test_camera_outside_the_proven_domain(rt, pipe, depth, kind):
    """Culled mode at depth 1 with a camera the camera-ray-only instance refuses: the culled
    instance runs (rt_update on the same camera reports it)."""
    import torch
    c = case(24, 16, depth, False, kind, False)
    got, words = run_adaptive(pipe, c)
    check(got, words, c, kind)
    a, b = to_dev(pipe, c.img), pipe.new_image(c.w, c.h)
    pipe.update(a, b, c.w, c.h, c.cam, c.sc)
    torch.cuda.synchronize()
    if depth == 1:
        assert pipe.last_launch_info()["kernel_name"] == fd.CULLED
    if kind == "active":
        assert bits_equal(got, b.cpu().numpy())[0]


def error_inputs(w, h):
    """An accumulator and a moments image that reach every branch of rt_adaptive_error."""
    rng = np.random.default_rng(w + 7 * h)
    img = (rng.random((h, w, 4)) * 2).astype(F32)
    mom = np.zeros((h, w, 4), F32)
    mom[..., 0] = rng.random((h, w))
    mom[..., 1] = mom[..., 0] ** 2 + (rng.random((h, w)) - 0.3).astype(F32) * F32(0.1)
    i = np.arange(w * h).reshape(h, w)
    img[..., 3] = i % 23                                        # n = 0 and n = 1 among them
    mom[..., 3] = (i // 3) % 9                                  # below and above min_history
    flat_i, flat_m = img.reshape(-1, 4), mom.reshape(-1, 4)
    step = max(1, (w * h) // 13)
    flat_i[0::step, 3] = 1.0
    for k, rec in enumerate([(np.nan, 1.0, 0.0, 6.0), (0.5, np.inf, 0.0, 6.0),
                             (0.5, 1.0, 0.0, np.nan), (0.5, np.nan, 0.0, 6.0)]):
        flat_m[(k + 1) % (w * h)] = rec
    flat_i[5 % (w * h), 3] = np.nan
    flat_i[6 % (w * h), 3] = 0.0
    flat_m[6 % (w * h)] = (0.25, 0.5, 0.0, 8.0)
    return img, mom


@gpu
@pytest.mark.parametrize("min_history", [1, 4])
@pytest.mark.parametrize("shape", SHAPES + [(65536, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_error_plane_matches_initial_variance(rt, pipe, shape, min_history):
    import torch
    w, h = shape
    img, mom = error_inputs(w, h)
    want, measured = tv.initial_variance(img, mom, min_history, np.inf)
    assert measured.any() and not measured.all() and np.isposinf(want).any()
    assert (img[..., 3] == 1).any() and (img[..., 3] == 0).any() and np.isnan(mom[..., 3]).any()
    a, m = to_dev(pipe, img), to_dev(pipe, mom)
    e = guarded(pipe, w * h)
    res = pipe.adaptive_error(a, m, w, h, min_history=min_history, out=e)
    assert res is e
    torch.cuda.synchronize()
    assert bits_equal(tail_intact(e, w * h, "error").reshape(h, w), want)[0]
    assert bits_equal(a.cpu().numpy(), img)[0] and bits_equal(m.cpu().numpy(), mom)[0]
    if shape == SHAPES[0]:
        fresh = pipe.adaptive_error(a, m, w, h, min_history=min_history)
        torch.cuda.synchronize()
        assert fresh.shape == (h, w) and bits_equal(fresh.cpu().numpy(), want)[0]


@gpu
def test_loop_matches_the_chain_of_references(rt, oracle, pipe):
    """Six rounds of update_adaptive, moments_update and adaptive_error at 48 x 32 and depth 3
    against adaptive_ref, moments_ref and initial_variance chained the same way."""
    import torch
    w, h, rounds = 48, 32, 6
    params = dict(min_samples=2, abs_tolerance2=1e-3, rel_tolerance2=2e-2)
    cam = make_camera(rt, w, h, 3, True, 500)
    seeds = rt.frame_seeds(11, rounds)
    frames = [cam.with_fields(random_seed=float(s), camera_has_moved=1.0 if k == 0 else 0.0)
              for k, s in enumerate(seeds)]
    acc = mom = np.zeros((h, w, 4), F32)
    err = np.full((h, w), np.inf, F32)
    want = []
    for c in frames:
        new, words, sampled = adaptive_ref(oracle, acc, c, scene().spheres, err,
                                           params["min_samples"], params["abs_tolerance2"],
                                           params["rel_tolerance2"])
        mom, acc = tv.moments_ref(acc, new, mom), new
        err = tv.initial_variance(acc, mom, 2, np.inf)[0]
        want.append((acc, mom, err, words, sampled))
    last = want[-1][4]
    assert last.any() and not last.all(), "the last round is neither all sampled nor all idle"
    a, b, m = pipe.new_image(w, h), pipe.new_image(w, h), pipe.new_image(w, h)
    e = torch.full((h, w), float("inf"), dtype=torch.float32, device=pipe.torch_device)
    for k, c in enumerate(frames):
        words = pipe.update_adaptive(a, b, w, h, c, scene(), e, tile_mask=True, **params)
        pipe.moments_update(a, b, m, w, h)
        pipe.adaptive_error(b, m, w, h, min_history=2, out=e)
        torch.cuda.synchronize()
        acc, mom, err, ref_words, _ = want[k]
        assert bits_equal(b.cpu().numpy(), acc)[0], f"round {k}: the accumulator differs"
        assert bits_equal(m.cpu().numpy(), mom)[0], f"round {k}: the moments differ"
        assert bits_equal(e.cpu().numpy(), err)[0], f"round {k}: the error plane differs"
        assert (words.cpu().numpy().view(np.uint64).reshape(ref_words.shape)
                == ref_words).all(), f"round {k}: the tile mask differs"
        a, b = b, a


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_band_sets(rt, pipe, depth):
    """rt_update_adaptive_bands over ranks 0 and 2 of three ranks' band sets at 24 x 40: the
    rows of the whole image's reference.  An empty band set launches nothing."""
    import torch
    w, h = 24, 40
    c = case(w, h, depth, True, "mixed")
    for rank in (0, 2):
        bands = rt.stripe_band_set(h, rank, 3)
        assert bands[2] == (2 if rank == 0 else 1)
        gb = [bands[0] + j * bands[1] for j in range(bands[2])]
        rows = np.concatenate([np.arange(8 * b, 8 * b + 8) for b in gb])
        got, words = run_adaptive(pipe, c, bands=bands, rows=rows)
        assert bits_equal(got, c.out[rows])[0], f"rank {rank}"
        assert (words == c.words[gb]).all(), f"rank {rank}"
    out = guarded(pipe, 4 * w * 8)
    pipe.update_adaptive(to_dev(pipe, c.img[:8]), out, w, h, c.cam, c.sc, to_dev(pipe, c.err[:8]),
                         bands=(0, 1, 0))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == F32(SENT)).all(), "an empty band set wrote out"


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_following_calls_are_undisturbed(rt, oracle, depth):
    """A following rt_update and a following rt_update_frames on the adaptive output match the
    oracle, and rt_last_launch_info is what it was before the adaptive call."""
    import torch
    w, h = 24, 16
    c = case(w, h, depth, True, "mixed")
    still = make_camera(rt, w, h, depth, True, 500)
    seeds = np.array(rt.frame_seeds(3, 3), F32)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, out = to_dev(p, c.img), p.new_image(w, h)
        p.init_image(out, w, h)                    # the context now knows a uniform count of out
        warm = p.new_image(w, h)
        p.update(a, warm, w, h, still, c.sc)
        info = p.last_launch_info()
        p.update_adaptive(a, out, w, h, c.cam, c.sc, to_dev(p, c.err), min_samples=MIN_SAMPLES,
                          abs_tolerance2=ABS2, rel_tolerance2=REL2)
        assert p.last_launch_info() == info
        nxt = p.new_image(w, h)
        p.update(out, nxt, w, h, still.with_fields(random_seed=float(seeds[0])), c.sc)
        torch.cuda.synchronize()
        assert bits_equal(out.cpu().numpy(), c.out)[0]
        want, _ = oracle.update(c.out, still.with_fields(random_seed=float(seeds[0])).blob,
                                c.sc.spheres)
        assert bits_equal(nxt.cpu().numpy(), want)[0], "a following rt_update differs"
        other = p.new_image(w, h)
        newest = p.update_frames(out, other, w, h, still, c.sc, seeds)
        torch.cuda.synchronize()
        chain = fd.oracle_chain(oracle, c.out, still, c.sc.spheres, seeds)
        got = (out if newest == 0 else other).cpu().numpy()
        assert bits_equal(got, chain[-1])[0], "a following rt_update_frames differs"
    finally:
        p.close()


@gpu
def test_side_stream_gives_the_same_bits(rt, pipe):
    import torch
    c = case(24, 16, 3, True, "mixed")
    img, mom = error_inputs(24, 16)
    a, e, out = to_dev(pipe, c.img), to_dev(pipe, c.err), pipe.new_image(24, 16)
    ia, im = to_dev(pipe, img), to_dev(pipe, mom)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        words = pipe.update_adaptive(a, out, 24, 16, c.cam, c.sc, e, min_samples=MIN_SAMPLES,
                                     abs_tolerance2=ABS2, rel_tolerance2=REL2, tile_mask=True)
        plane = pipe.adaptive_error(ia, im, 24, 16)
    side.synchronize()
    check(out.cpu().numpy(), words.cpu().numpy().view(np.uint64).reshape(c.words.shape), c)
    assert bits_equal(plane.cpu().numpy(), tv.initial_variance(img, mom, 4, np.inf)[0])[0]


@gpu
def test_refused_calls_launch_nothing(rt, pipe):
    import torch
    L = rt._lib
    c = case(24, 16, 1, True, "mixed")
    w, h = c.w, c.h
    px, tiles = w * h, 6
    a, e = to_dev(pipe, c.img), to_dev(pipe, c.err)
    mom = to_dev(pipe, error_inputs(w, h)[1])
    out, plane, words = guarded(pipe, 4 * px), guarded(pipe, px), guarded_words(pipe, tiles)
    cam = c.cam.to_c()
    sp, n = pipe._spheres(c.sc)
    ctx = pipe._ctx
    A, Z = RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE
    I, O, E, M, T = a.data_ptr(), out.data_ptr(), e.data_ptr(), mom.data_ptr(), words.data_ptr()
    PL = plane.data_ptr()
    band = L.band_sets([(0, 1, 2)])

    def update(params=(MIN_SAMPLES, ABS2, REL2), bands=None, **kw):
        v = dict(ctx=ctx, inp=I, out=O, err=E, mask=T, w=w, h=h, cam=ctypes.byref(cam))
        v.update(kw)
        pc = L.AdaptiveParamsC(*params) if params is not None else None
        head = (v["ctx"], v["inp"], v["out"], v["err"], v["mask"], v["w"], v["h"])
        tail = (v["cam"], sp, n, ctypes.byref(pc) if pc is not None else None, pipe._stream())
        if bands is None:
            L.call("rt_update_adaptive", *head, *tail)
        else:
            L.call("rt_update_adaptive_bands", *head, bands[0], *tail)

    rows = {"ctx NULL": (RT_ERR_INVALID_CONTEXT, dict(ctx=None)),
            "in NULL": (A, dict(inp=None)), "out NULL": (A, dict(out=None)),
            "error NULL": (A, dict(err=None)), "camera NULL": (A, dict(cam=None)),
            "params NULL": (A, dict(params=None)),
            "out == in": (A, dict(inp=O)), "out == error": (A, dict(err=O)),
            "out == tile_mask": (A, dict(mask=O)),
            "min_samples 2^24 + 1": (A, dict(params=((1 << 24) + 1, ABS2, REL2))),
            "width 0": (Z, dict(w=0)), "height 0": (Z, dict(h=0)),
            "width 65537": (Z, dict(w=65537)), "height 65537": (Z, dict(h=65537)),
            "bands NULL": (A, dict(bands=(None,))),
            "bands: ctx NULL": (RT_ERR_INVALID_CONTEXT, dict(bands=(band,), ctx=None)),
            "bands past the image": (A, dict(bands=(L.band_sets([(1, 1, 2)]),))),
            "bands: step 0": (A, dict(bands=(L.band_sets([(0, 0, 1)]),)))}
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf")),
                      ("-inf", float("-inf"))]:
        rows[f"abs_tolerance2 {what}"] = (A, dict(params=(MIN_SAMPLES, bad, REL2)))
        rows[f"rel_tolerance2 {what}"] = (A, dict(params=(MIN_SAMPLES, ABS2, bad)))
    for what, (status, kw) in rows.items():
        with pytest.raises(rt.RtError) as err:
            update(**kw)
        assert err.value.status == status, what

    def error(ctx=ctx, image=I, moments=M, plane=PL, w=w, h=h, min_history=4):
        L.call("rt_adaptive_error", ctx, image, moments, plane, w, h, min_history, pipe._stream())

    erows = {"ctx NULL": (RT_ERR_INVALID_CONTEXT, dict(ctx=None)),
             "image NULL": (A, dict(image=None)), "moments NULL": (A, dict(moments=None)),
             "error NULL": (A, dict(plane=None)), "error == image": (A, dict(image=PL)),
             "error == moments": (A, dict(moments=PL)),
             "min_history 0": (A, dict(min_history=0)),
             "min_history 2^24 + 1": (A, dict(min_history=(1 << 24) + 1)),
             "width 0": (Z, dict(w=0)), "height 0": (Z, dict(h=0)),
             "width 65537": (Z, dict(w=65537)), "height 65537": (Z, dict(h=65537))}
    for what, (status, kw) in erows.items():
        with pytest.raises(rt.RtError) as err:
            error(**kw)
        assert err.value.status == status, what
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == F32(SENT)).all(), "a refused call wrote out"
    assert (plane.cpu().numpy() == F32(SENT)).all(), "a refused call wrote the error plane"
    assert (words.cpu().numpy() == np.int64(SENT_WORD)).all(), "a refused call wrote tile_mask"
    with pytest.raises(ValueError):
        pipe.update_adaptive(a.cpu(), out, w, h, c.cam, c.sc, e)
    with pytest.raises(ValueError):
        pipe.update_adaptive(a, out, w, h, c.cam, c.sc, e[:1])
    with pytest.raises(ValueError):
        pipe.adaptive_error(a, mom.cpu(), w, h)
    # the ends of the ranges are accepted, and the context still works
    update(params=(1 << 24, 0.0, 0.0))
    error(min_history=1 << 24)
    update()
    torch.cuda.synchronize()
    check(tail_intact(out, 4 * px, "out").reshape(h, w, 4),
          tail_intact(words, tiles, "tile_mask").view(np.uint64).reshape(2, 3), c)
