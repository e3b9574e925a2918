"""The a-trous denoiser (include/rt_denoise.h): rt_denoise, rt_denoise_params_default.

The reference is in this file: `denoise_ref`, a vectorised NumPy float32 restatement of the
header's normative text (np.fmax for the normal weight, the taps in the stated order, np.where
for the conditional accumulation).  Its guide planes come from the oracle's exported sphere_hit
and libm's fmaf, the construction of tests/test_aov.py restated here; its input colours from
the CPU oracle's update, which the GPU tests first check against the image the GPU renders.
Every GPU output is compared bit for bit (NaN == NaN).

The CPU tests check the boundary, count from the reference alone how often each case reaches
each skip rule (printed with -s), and check that the filter denoises: a cap on the error
against a 512-sample render, not a tolerance.
"""
import ctypes
import ctypes.util
import functools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_denoise.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
W, H = 37, 21                 # a partial 64x4 tile both ways; lower than the reach of step 16's taps
#                               (tests/test_post_shapes.py has the shapes beyond one workgroup)
MISS = -1
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
SENT = -12345.0
TAIL = 16                     # 64 bytes of sentinel after dst and scratch
DEFAULTS = (5, 5, 1.0, 4.0)   # iterations, normal_power_log2, inv_sigma_color2, inv_sigma_position2
H5 = (F32(1 / 16), F32(1 / 4), F32(3 / 8), F32(1 / 4), F32(1 / 16))
ROUTES = [None, "direct"]      # RT_DENOISE_ROUTE: the library's choice, or every step direct


# ---- the reference filter -------------------------------------------------------------------------
def _shifted(a, oy, ox):
    """a[y + oy, x + ox] where that is on the image (zeros elsewhere), and the on-image mask."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def _dist2(a, b):
    e = a - b
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def denoise_ref(src, hit, normal, ids, iterations, npow, ic0, ip, counts=None):
    """rt_denoise.h's text over (H, W, 4) float32 arrays (ids: (H, W) int32 or None).  With
    `counts` (a dict) it also tallies the taps each skip rule drops and the pass-through
    pixels, over all iterations."""
    c = np.ascontiguousarray(src, F32)
    hit = np.ascontiguousarray(hit, F32)
    normal = np.ascontiguousarray(normal, F32)
    one, zero, ip = F32(1.0), F32(0.0), F32(ip)
    miss_p = ~(hit[..., 3] < np.inf)
    tally = dict(off_image=0, miss_mismatch=0, id_mismatch=0, weight=0, pass_through=0, taps=0)
    with np.errstate(all="ignore"):
        ic = F32(ic0)
        for i in range(iterations):
            s = 1 << i
            ic_i = np.minimum(ic, FLT_MAX)
            sw = np.zeros(c.shape[:2], F32)
            acc = np.zeros(c.shape[:2] + (3,), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = H5[dy + 2] * H5[dx + 2]
                    cq, inside = _shifted(c, dy * s, dx * s)
                    hq, _ = _shifted(hit, dy * s, dx * s)
                    nq, _ = _shifted(normal, dy * s, dx * s)
                    miss_q = ~(hq[..., 3] < np.inf)
                    same_miss = miss_p == miss_q
                    if ids is not None:
                        iq, _ = _shifted(ids, dy * s, dx * s)
                        same_id = ids == iq
                    else:
                        same_id = np.ones_like(inside)
                    dc = _dist2(c, cq)
                    dp = np.where(miss_p, zero, _dist2(hit, hq))
                    dn = (normal[..., 0] * nq[..., 0] + normal[..., 1] * nq[..., 1]) \
                        + normal[..., 2] * nq[..., 2]
                    wn = np.fmax(dn, zero)
                    for _ in range(npow):
                        wn = wn * wn
                    wn = np.where(miss_p, one, wn)
                    wgt = (k * wn) / ((one + dp * ip) * (one + dc * ic_i))
                    assert wgt.dtype == F32
                    positive = wgt > 0
                    keep = inside & same_miss & same_id & positive
                    sw = np.where(keep, sw + wgt, sw)
                    acc = np.where(keep[..., None], acc + wgt[..., None] * cq[..., :3], acc)
                    tally["taps"] += inside.size
                    tally["off_image"] += int((~inside).sum())
                    tally["miss_mismatch"] += int((inside & ~same_miss).sum())
                    tally["id_mismatch"] += int((inside & same_miss & ~same_id).sum())
                    tally["weight"] += int((inside & same_miss & same_id & ~positive).sum())
            ok = sw > 0
            out = c.copy()
            out[..., :3] = np.where(ok[..., None], acc / sw[..., None], c[..., :3])
            assert out.dtype == F32
            tally["pass_through"] += int((~ok).sum())
            c = out
            ic = ic * F32(4.0)
    if counts is not None:
        counts.update(tally)
    return c


# ---- the guide planes: the oracle's sphere_hit along each pixel's centre ray ---------------------
@functools.lru_cache(None)
def _fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return m.fmaf


def centre_ray(blob, x, y):
    fmaf = _fmaf()
    b = np.asarray(blob, F32)
    o, vul, pdu, pdv = b[0:3], b[4:7], b[8:11], b[12:15]
    sx, sy = F32(x) + F32(0.5), F32(y) + F32(0.5)
    ray = np.empty(6, F32)
    ray[0:3] = o
    for k in range(3):
        pc = F32(fmaf(sy, pdv[k], fmaf(sx, pdu[k], vul[k])))
        ray[3 + k] = pc - o[k]
    return ray


def guide_planes(blob, spheres, w, h):
    """sphere_id, hit and normal of a w x h image, as rt_trace_aov defines them."""
    from oracle import oracle
    hit_fn = oracle.lib().oracle_sphere_hit
    sph = np.ascontiguousarray(spheres, F32).reshape(-1, 8)
    base = sph.ctypes.data
    recs = [ctypes.c_void_p(base + 32 * i) for i in range(sph.shape[0])]
    ray = np.zeros(6, F32)
    out = np.zeros(8, F32)
    pray, pout = ctypes.c_void_p(ray.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    tmin = ctypes.c_float(0.001)
    ids = np.full((h, w), MISS, np.int32)
    hit = np.zeros((h, w, 4), F32)
    hit[..., 3] = np.inf
    normal = np.zeros((h, w, 4), F32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                ray[:] = centre_ray(blob, x, y)
                tmax = ctypes.c_float(3.4e35)
                for i, rec in enumerate(recs):
                    if hit_fn(rec, pray, tmin, tmax, pout):
                        tmax = ctypes.c_float(out[0])
                        ids[y, x] = i
                        hit[y, x, :3], hit[y, x, 3] = out[1:4], out[0]
                        normal[y, x] = out[4:8]
    return {"sphere_id": ids, "hit": hit, "normal": normal}


# ---- cases ------------------------------------------------------------------------------------------
def default_camera(rt, w, h, **settings):
    settings.setdefault("max_depth", 4)
    return rt.SceneCamera.from_settings(rt.CameraSettings(**settings), w, h, 0.25)


def variant(iterations=5, use_ids=True, npow=5, ic=1.0, ip=4.0):
    return (iterations, use_ids, npow, ic, ip)


# name -> (width, height, scene, camera settings, variants, the skip rules it must reach)
_INSIDE = dict(look_from=(0.25, 1.0, 0.5), look_at=(4.0, 1.0, 0.0), field_of_view=60.0)
CASES = {
    "n40": (W, H, "n40", {}, [variant(n, ids) for n in (1, 2, 5) for ids in (True, False)],
            ("off_image", "miss_mismatch", "id_mismatch")),
    "1x1": (1, 1, "three", {}, [variant()], ("off_image",)),
    "8x8": (8, 8, "three", {}, [variant()], ("off_image",)),
    "5x40": (5, 40, "three", {}, [variant()], ("off_image",)),
    "70x3": (70, 3, "three", {}, [variant()], ("off_image",)),
    # exactly one 64 x 4 tile of the kernel, and one pixel more both ways
    "64x4": (64, 4, "three", {}, [variant()], ("off_image",)),
    "65x5": (65, 5, "three", {}, [variant()], ("off_image",)),
    "halo": (100, 52, "n40", {}, [variant()], ("off_image", "miss_mismatch", "id_mismatch")),
    "inside": (W, H, "n40", _INSIDE, [variant()], ("off_image",)),
    "zero": (W, H, "zero", {}, [variant()], ("off_image",)),
    "nonfinite": (W, H, "n40", {}, [variant(), variant(2, False)],
                  ("off_image", "weight", "pass_through")),
    "params": (W, H, "n40", {}, [variant(ic=0.0, ip=0.0), variant(ic=3e38), variant(npow=0),
                                 variant(npow=10), variant(8)], ("off_image", "id_mismatch")),
    "seeded": (W, H, "n40", {}, [variant(), variant(3, False)], ("off_image", "id_mismatch")),
    "undisturbed": (64, 40, "n40", {}, [variant()], ("off_image",)),
}
PLANTED = {(3, 5): np.nan, (10, 20): np.inf, (17, 30): -np.inf}   # (y, x): the colour planted
NAN_NORMAL = (12, 14)


def _scene(rt, kind):
    if kind == "three":
        return rt.three_spheres().spheres
    if kind == "zero":
        return np.zeros((0, 8), F32)
    return rt.synthetic_scene(40).spheres


@functools.lru_cache(None)
def case(name):
    """A case's inputs (read-only arrays), computed once and shared."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    w, h, kind, settings, variants, rules = CASES[name]
    cam = default_camera(rt, w, h, **settings)
    spheres = np.ascontiguousarray(_scene(rt, kind), F32).reshape(-1, 8)
    g = guide_planes(cam.blob, spheres, w, h)
    # the 1-spp accumulator pipe.update writes for this camera and scene
    rendered, _ = oracle.update(np.zeros((h, w, 4), F32), cam.blob, spheres)
    src = rendered.copy()
    if name == "seeded":
        src[..., :3] = (np.random.default_rng(20240).random((h, w, 3)) * 4.0).astype(F32)
    if name == "nonfinite":
        for (y, x), v in PLANTED.items():
            src[y, x, 1] = v
        g["normal"][NAN_NORMAL][0] = np.nan
    for a in (src, rendered, spheres, *g.values()):
        a.setflags(write=False)
    return SimpleNamespace(name=name, w=w, h=h, cam=cam, spheres=spheres, variants=variants,
                           rules=rules, sc=rt.SphereCollection(spheres), src=src,
                           rendered=rendered, **g)


@functools.lru_cache(None)
def expected(name, var):
    """(reference output, its skip tallies) of one variant of a case."""
    c = case(name)
    n, use_ids, npow, ic, ip = var
    counts = {}
    out = denoise_ref(c.src, c.hit, c.normal, c.sphere_id if use_ids else None, n, npow, ic, ip,
                      counts)
    out.setflags(write=False)
    return out, counts


ALL = [(name, var) for name in CASES for var in CASES[name][4]]


def _id(v):
    name, (n, use_ids, npow, ic, ip) = v
    return f"{name}-i{n}-{'ids' if use_ids else 'noids'}-p{npow}-c{ic:g}-s{ip:g}"


# ---- CPU tests --------------------------------------------------------------------------------------
def test_library_exports_the_denoise_entry_points(rt):
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", HEADER.read_text(), flags=re.M)
    assert declared == ["rt_denoise_params_default", "rt_denoise"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(declared) <= exported
    assert {s for s in exported if "denoise" in s} == set(declared)
    L = rt._lib
    assert set(L.denoise_symbols()) == set(declared)
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.selftest_roots_symbols()):
        assert not set(declared) & set(other)
    assert L.lib().rt_abi_version() == 7
    assert ctypes.sizeof(L.DenoiseParamsC) == 16
    assert [f for f, _ in L.DenoiseParamsC._fields_] == [
        "iterations", "normal_power_log2", "inv_sigma_color2", "inv_sigma_position2"]
    p = L.DenoiseParamsC(99, 99, -1.0, -1.0)
    L.lib().rt_denoise_params_default(ctypes.byref(p))
    assert (p.iterations, p.normal_power_log2, p.inv_sigma_color2,
            p.inv_sigma_position2) == DEFAULTS
    L.lib().rt_denoise_params_default(None)                     # a no-op, not a crash
    assert rt.RT_DENOISE_MAX_ITERATIONS == 8
    d = rt.DENOISE_DEFAULTS
    assert (d["iterations"], d["normal_power_log2"]) == DEFAULTS[:2]
    from gpu_ray_tracing.compute_shader import inv_sigma2
    assert (inv_sigma2(d["sigma_color"]), inv_sigma2(d["sigma_position"])) == DEFAULTS[2:]
    assert inv_sigma2(0.1) == float(F32(1.0) / (F32(0.1) * F32(0.1)))


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "rt_denoise.h"\n'
                   "typedef char params_are_16_bytes[sizeof(rt_denoise_params) == 16 ? 1 : -1];\n"
                   "typedef char max_is_8[RT_DENOISE_MAX_ITERATIONS == 8u ? 1 : -1];\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_rules(name):
    c = case(name)
    reached = dict.fromkeys(("off_image", "miss_mismatch", "id_mismatch", "weight",
                             "pass_through"), 0)
    for var in c.variants:
        out, n = expected(name, var)
        print(f"{_id((name, var))}: {c.w}x{c.h}, taps {n['taps']}: off-image {n['off_image']}, "
              f"hit/miss mismatch {n['miss_mismatch']}, id mismatch {n['id_mismatch']}, "
              f"!(w > 0) {n['weight']}, pass-through pixels {n['pass_through']}, "
              f"{int((out[..., :3] != c.src[..., :3]).any(-1).sum())} of {c.w * c.h} pixels changed")
        assert bits_equal(out[..., 3], c.src[..., 3])[0]
        for k in reached:
            reached[k] += n[k]
        if not var[1]:
            assert n["id_mismatch"] == 0
    for rule in c.rules:
        assert reached[rule] >= 1, f"{name} never reaches {rule}"
    miss = ~(c.hit[..., 3] < np.inf)
    if name in ("n40", "halo", "nonfinite", "params", "seeded"):
        assert miss.any() and not miss.all()
    if name == "inside":
        assert not miss.any() and reached["miss_mismatch"] == 0
    if name == "zero":
        assert miss.all() and reached["miss_mismatch"] == 0 and reached["id_mismatch"] == 0
    if name == "1x1":
        # every tap but the centre is off the image, in all five iterations
        assert reached["off_image"] == 5 * 24 and reached["pass_through"] == 0
    if name in ("5x40", "70x3"):
        # narrower (shorter) than every step >= 8: no tap along that axis but the centre's
        assert min(c.w, c.h) < 8
    if name == "n40":
        out, _ = expected(name, variant(5, True))
        changed = (out[..., :3] != c.src[..., :3]).any(-1).mean()
        assert changed >= 0.9, changed


def test_nonfinite_pixels_pass_through_and_reach_no_neighbour():
    c = case("nonfinite")
    for var in c.variants:
        out, n = expected("nonfinite", var)
        planted = np.zeros((c.h, c.w), bool)
        for (y, x) in PLANTED:
            planted[y, x] = True
            assert bits_equal(out[y, x], c.src[y, x])[0], (y, x)
        assert np.isfinite(out[~planted]).all()
        assert n["pass_through"] >= 3 * var[0]
    assert np.isnan(c.normal[NAN_NORMAL][0])


def test_clamp_and_zero_sigmas_are_well_defined():
    c = case("params")
    for var in c.variants:
        out, _ = expected("params", var)
        assert np.isfinite(out).all(), var
    with np.errstate(over="ignore"):
        assert np.isinf(F32(3e38) * F32(4.0)) and np.minimum(F32(3e38) * F32(4.0), FLT_MAX) == FLT_MAX


@pytest.mark.slow
def test_it_denoises(oracle):
    """1 spp filtered with the defaults is nearer the 512-spp image than 1 spp is: RMSE over
    rgb at most 0.8 of the input's."""
    from oracle import host_ref
    w, h = 96, 64
    spheres = host_ref.generate_scene(1, seed=1)
    blob = host_ref.scene_camera_from(width=w, height=h, max_depth=8, random_seed=0.25)
    seeds = host_ref.frame_seeds(7, 512)
    zero = np.zeros((h, w, 4), F32)
    noisy, _ = oracle.render(zero, blob, spheres, seeds[:1])
    target, _ = oracle.render(zero, blob, spheres, seeds)
    g = guide_planes(blob, spheres, w, h)
    n, npow, ic, ip = DEFAULTS
    out = denoise_ref(noisy, g["hit"], g["normal"], g["sphere_id"], n, npow, ic, ip)

    def rmse(a):
        return float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - target[..., :3]) ** 2)))
    before, after = rmse(noisy), rmse(out)
    print(f"RMSE against 512 spp: input {before:.4f}, denoised {after:.4f}, "
          f"ratio {after / before:.3f}")
    assert after <= 0.8 * before


# ---- GPU side ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


@pytest.fixture
def route(request, monkeypatch):
    monkeypatch.delenv("RT_DENOISE_ROUTE", raising=False)
    if getattr(request, "param", None):
        monkeypatch.setenv("RT_DENOISE_ROUTE", request.param)
    return getattr(request, "param", None)


def guarded(p, n):
    import torch
    return torch.full((n + TAIL,), SENT, dtype=torch.float32, device=p.torch_device)


def device_inputs(p, c):
    import torch
    dev = p.torch_device
    return SimpleNamespace(src=torch.from_numpy(c.src.copy()).to(dev),
                           hit=torch.from_numpy(c.hit.copy()).to(dev),
                           normal=torch.from_numpy(c.normal.copy()).to(dev),
                           ids=torch.from_numpy(c.sphere_id.copy()).to(dev))


def raw_call(rt, p, ctx, src, dst, scratch, w, h, hit, normal, ids, params):
    """rt_denoise through the C boundary (data pointers or None); raises RtError."""
    L = rt._lib
    pc = L.DenoiseParamsC(*params) if params is not None else None
    L.call("rt_denoise", ctx, src, dst, scratch, w, h, hit, normal, ids,
           ctypes.byref(pc) if pc is not None else None, p._stream())


def run(rt, p, c, var, d=None):
    """dst of one variant (numpy), after the checks every call must pass: the tails of dst
    and scratch intact, src and the guide planes unchanged."""
    import torch
    n, use_ids, npow, ic, ip = var
    d = d or device_inputs(p, c)
    px = c.w * c.h * 4
    dst, scratch = guarded(p, px), guarded(p, px)
    raw_call(rt, p, p._ctx, d.src.data_ptr(), dst.data_ptr(), scratch.data_ptr(), c.w, c.h,
             d.hit.data_ptr(), d.normal.data_ptr(), d.ids.data_ptr() if use_ids else None,
             (n, npow, ic, ip))
    torch.cuda.current_stream().synchronize()
    got, scr = dst.cpu().numpy(), scratch.cpu().numpy()
    assert (got[px:] == F32(SENT)).all(), "the 64 bytes after dst were written"
    assert (scr[px:] == F32(SENT)).all(), "the 64 bytes after scratch were written"
    if n == 1:
        assert (scr == F32(SENT)).all(), "one iteration wrote scratch"
    assert bits_equal(d.src.cpu().numpy(), c.src)[0], "src was written"
    assert bits_equal(d.hit.cpu().numpy(), c.hit)[0], "hit was written"
    assert bits_equal(d.normal.cpu().numpy(), c.normal)[0], "normal was written"
    assert (d.ids.cpu().numpy() == c.sphere_id).all(), "sphere_id was written"
    return got[:px].reshape(c.h, c.w, 4)


def check(got, c, name, var):
    want, _ = expected(name, var)
    same, bad = bits_equal(got, want)
    assert same, f"{_id((name, var))}: {bad} values differ from the reference"
    assert bits_equal(got[..., 3], c.src[..., 3])[0], "alpha is not the input's"


@gpu
@pytest.mark.parametrize("v", ALL, ids=_id)
def test_matches_reference(rt, pipe, route, v):
    name, var = v
    c = case(name)
    check(run(rt, pipe, c, var), c, name, var)


@gpu
@pytest.mark.parametrize("route", ROUTES[1:], indirect=True)
@pytest.mark.parametrize("name", ["halo", "n40", "70x3", "nonfinite"])
def test_every_route_matches_reference(rt, pipe, route, name):
    c = case(name)
    var = c.variants[0]
    check(run(rt, pipe, c, var), c, name, var)


@gpu
def test_input_is_the_image_the_gpu_renders(rt, pipe, route):
    """The cases' colours are the CPU oracle's 1-spp update; pipe.update writes the same bits,
    and filtering the GPU's own image and trace_aov's own planes gives the reference too."""
    import torch
    for name in ("n40", "inside"):
        c = case(name)
        a, b = pipe.new_image(c.w, c.h), pipe.new_image(c.w, c.h)
        pipe.update(a, b, c.w, c.h, c.cam, c.sc)
        guides = pipe.trace_aov(c.w, c.h, c.cam, c.sc, planes=("sphere_id", "hit", "normal"))
        out = pipe.denoise(b, c.w, c.h, guides)
        assert out.shape == (c.h, c.w, 4)
        noids = pipe.denoise(b, c.w, c.h, {k: guides[k] for k in ("hit", "normal")},
                             iterations=1, use_ids=False)
        torch.cuda.synchronize()
        assert bits_equal(b.cpu().numpy(), c.rendered)[0]
        if name == "n40":
            check(out.cpu().numpy(), c, name, variant())
            check(noids.cpu().numpy(), c, name, variant(1, False))
        else:
            check(out.cpu().numpy(), c, name, c.variants[0])
        with pytest.raises(ValueError):
            pipe.denoise(b, c.w, c.h, {"hit": guides["hit"], "normal": guides["normal"]})
        with pytest.raises(ValueError):
            pipe.denoise(b.cpu(), c.w, c.h, guides)


@gpu
def test_python_sigmas(rt, pipe, route):
    """sigma -> float32 1 / sigma^2 on the Python side; out and scratch given by the caller."""
    import torch
    from gpu_ray_tracing.compute_shader import inv_sigma2
    c = case("seeded")
    d = device_inputs(pipe, c)
    guides = {"hit": d.hit, "normal": d.normal, "sphere_id": d.ids}
    out = torch.empty((c.h, c.w, 4), dtype=torch.float32, device=pipe.torch_device)
    scratch = torch.empty_like(out)
    res = pipe.denoise(d.src, c.w, c.h, guides, iterations=3, normal_power_log2=2,
                       sigma_color=0.7, sigma_position=0.3, out=out, scratch=scratch)
    assert res is out
    torch.cuda.synchronize()
    want = denoise_ref(c.src, c.hit, c.normal, c.sphere_id, 3, 2, inv_sigma2(0.7), inv_sigma2(0.3))
    assert bits_equal(out.cpu().numpy(), want)[0]
    with pytest.raises(rt.RtError) as e:
        pipe.denoise(d.src, c.w, c.h, guides, sigma_color=0.0)      # 1 / 0 = inf
    assert e.value.status == RT_ERR_INVALID_ARGUMENT


@gpu
def test_errors_launch_nothing(rt, pipe, route):
    import torch
    c = case("n40")
    d = device_inputs(pipe, c)
    px = c.w * c.h * 4
    dst, scratch = guarded(pipe, px), guarded(pipe, px)
    S, D, X = d.src.data_ptr(), dst.data_ptr(), scratch.data_ptr()
    Hh, N, I = d.hit.data_ptr(), d.normal.data_ptr(), d.ids.data_ptr()
    ctx, w, h = pipe._ctx, c.w, c.h
    ok = (5, 5, 1.0, 4.0)
    rows = {
        "ctx NULL": (RT_ERR_INVALID_CONTEXT, (None, S, D, X, w, h, Hh, N, I, ok)),
        "src NULL": (RT_ERR_INVALID_ARGUMENT, (ctx, None, D, X, w, h, Hh, N, I, ok)),
        "dst NULL": (RT_ERR_INVALID_ARGUMENT, (ctx, S, None, X, w, h, Hh, N, I, ok)),
        "hit NULL": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, X, w, h, None, N, I, ok)),
        "normal NULL": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, X, w, h, Hh, None, I, ok)),
        "params NULL": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, X, w, h, Hh, N, I, None)),
        "dst == src": (RT_ERR_INVALID_ARGUMENT, (ctx, D, D, X, w, h, Hh, N, I, ok)),
        "dst == src, one iteration": (RT_ERR_INVALID_ARGUMENT,
                                      (ctx, D, D, None, w, h, Hh, N, I, (1, 5, 1.0, 4.0))),
        "scratch NULL": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, None, w, h, Hh, N, I, ok)),
        "scratch NULL, two iterations": (RT_ERR_INVALID_ARGUMENT,
                                         (ctx, S, D, None, w, h, Hh, N, I, (2, 5, 1.0, 4.0))),
        "scratch == src": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, S, w, h, Hh, N, I, ok)),
        "scratch == dst": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, D, w, h, Hh, N, I, ok)),
        "iterations 0": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, X, w, h, Hh, N, I, (0, 5, 1.0, 4.0))),
        "iterations 9": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, X, w, h, Hh, N, I, (9, 5, 1.0, 4.0))),
        "power 11": (RT_ERR_INVALID_ARGUMENT, (ctx, S, D, X, w, h, Hh, N, I, (5, 11, 1.0, 4.0))),
        "width 0": (RT_ERR_INVALID_SIZE, (ctx, S, D, X, 0, h, Hh, N, I, ok)),
        "height 0": (RT_ERR_INVALID_SIZE, (ctx, S, D, X, w, 0, Hh, N, I, ok)),
        "width 65537": (RT_ERR_INVALID_SIZE, (ctx, S, D, X, 65537, h, Hh, N, I, ok)),
        "height 65537": (RT_ERR_INVALID_SIZE, (ctx, S, D, X, w, 65537, Hh, N, I, ok)),
    }
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf")),
                      ("-inf", float("-inf"))]:
        rows[f"colour term {what}"] = (RT_ERR_INVALID_ARGUMENT,
                                       (ctx, S, D, X, w, h, Hh, N, I, (5, 5, bad, 4.0)))
        rows[f"position term {what}"] = (RT_ERR_INVALID_ARGUMENT,
                                         (ctx, S, D, X, w, h, Hh, N, I, (5, 5, 1.0, bad)))
    for what, (status, args) in rows.items():
        with pytest.raises(rt.RtError) as e:
            raw_call(rt, pipe, *args)
        assert e.value.status == status, what
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == F32(SENT)).all(), "a refused call wrote dst"
    assert (scratch.cpu().numpy() == F32(SENT)).all(), "a refused call wrote scratch"
    # one iteration needs no scratch, and the context still works
    var = variant(1, True)
    raw_call(rt, pipe, ctx, S, D, None, w, h, Hh, N, I, (1, 5, 1.0, 4.0))
    torch.cuda.synchronize()
    check(dst.cpu().numpy()[:px].reshape(h, w, 4), c, "n40", var)


@gpu
def test_side_stream_gives_the_same_bits(rt, pipe, route):
    import torch
    c = case("halo")
    d = device_inputs(pipe, c)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = pipe.denoise(d.src, c.w, c.h, {"hit": d.hit, "normal": d.normal,
                                             "sphere_id": d.ids})
    side.synchronize()
    check(out.cpu().numpy(), c, "halo", c.variants[0])


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_render_is_undisturbed(rt, oracle, route, depth):
    """4 frames of update_frames, against 2 frames + denoise + 2 frames on the same context:
    the same two images, the oracle's, and no trace of the denoiser in the launch info or the
    candidate lists."""
    import torch
    c = case("undisturbed")
    w, h = c.w, c.h
    cam = rt.SceneCamera.from_settings(rt.CameraSettings(max_depth=depth), w, h, 0.5)
    still = cam.with_fields(camera_has_moved=0.0)
    seeds = np.array(rt.frame_seeds(5, 4), F32)
    want, cur = [], np.zeros((h, w, 4), F32)
    for k, s in enumerate(seeds):
        cur, _ = oracle.update(cur, (cam if k == 0 else still).with_fields(
            random_seed=float(s)).blob, c.spheres)
        want.append(cur)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, b = p.new_image(w, h), p.new_image(w, h)
        p.update_frames(a, b, w, h, cam, c.sc, seeds)
        torch.cuda.synchronize()
        seq_a = (a.cpu().numpy(), b.cpu().numpy())
        a2, b2 = p.new_image(w, h), p.new_image(w, h)
        p.update_frames(a2, b2, w, h, cam, c.sc, seeds[:2])
        info, stats = p.last_launch_info(), p.candidate_stats()
        d = device_inputs(p, c)
        out = p.denoise(a2, w, h, {"hit": d.hit, "normal": d.normal, "sphere_id": d.ids})
        assert p.last_launch_info() == info
        assert p.candidate_stats() == stats
        torch.cuda.synchronize()
        mid = a2.cpu().numpy()
        got = out.cpu().numpy()
        p.update_frames(a2, b2, w, h, still, c.sc, seeds[2:])
        torch.cuda.synchronize()
        seq_b = (a2.cpu().numpy(), b2.cpu().numpy())
    finally:
        p.close()
    n, npow, ic, ip = DEFAULTS
    assert bits_equal(got, denoise_ref(mid, c.hit, c.normal, c.sphere_id, n, npow, ic, ip))[0]
    for i, name in enumerate("ab"):
        assert bits_equal(seq_b[i], seq_a[i])[0], f"image_{name} differs between the sequences"
    # frame f writes image_b for even f: image_a holds frame 3, image_b frame 2
    assert bits_equal(seq_a[0], want[3])[0] and bits_equal(seq_a[1], want[2])[0]
    assert bits_equal(seq_b[0], want[3])[0] and bits_equal(seq_b[1], want[2])[0]
