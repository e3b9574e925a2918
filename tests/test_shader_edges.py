"""The shader's own input space at its edges: materials, depth and sphere count.

The shading of a hit exists four times (rt_kernels.hip: shade_hit of the one-frame and chain
kernels, the tile-pair kernel's path, scatter_path of the bounce instances; rt_trace_device.h:
ray_color<kScan> of the exhaustive, culled and list instances), so every case here runs through every route of its
depth and the kernel name of each launch is asserted (a silent re-routing would show):

  depth <= 1   `update` under the four modes of test_gpu_parity's `pipe` fixture;
               update_frames of 5 frames from a reset under rt_set_frame_pairs off / on / quad /
               on2 / quad2 (rt_trace_kernel<2|3|4>, rt_tpair_kernel<2|4>)
  depth >= 2   update_frames of 5 frames from a reset under rt_set_path_compaction per_wave /
               compact / pair / split (rt_bounce_kernel<0..3>); `update` and a 3-frame `render`
               in exhaustive scan mode (rt_trace_kernel<0>, ray_color<kTraceExhaustive>)

Every GPU case is compared bit for bit with the CPU oracle (NaN == NaN), both ping-pong buffers
of update_frames.  Every case has a CPU twin that asserts, from the oracle or from a float64
mirror of the pixel-centre camera rays, that the case reaches the edge it names; the twins
print the count behind each bound (run with -s).

A  material and scatter edges: the decode thresholds w < -1 and w <= 1 (wgsl:272-284) from both
   sides, fuzz 1 and -1, refraction indices that give total internal reflection (wgsl:119),
   zero, negative, huge, tiny, infinite and NaN ratios, and the degenerate Lambertian direction
   (wgsl:87) aimed at from the frame's own random unit vector.
B  depth edges: 15..65 bounces inside an enclosing sphere (no path ends early), across the
   three bounds DESIGN.md §4.4 lists: the device table of scatter random numbers (depth <= 16),
   the inline table (64 / depth hinted frames: 2 at 32, 1 at 33..64, 0 above); and u32(f32) of
   max_depth and samples_per_pixel (wgsl:264, 343) for fractions, negatives, -0 and NaN.
C  sphere counts 0, 1, 2, around 32 (the cone culling's kCullMinSpheres), around 64 (the grid's
   kGridMinSpheres and the 64-record padding) and 128 (the capacity doubling), each on a fresh
   context and as one growing and shrinking sequence per context; 4095, 4096 and 4097 spheres
   around kLdsMaxRecords, where the compact bounce instance asks for 64 KiB of dynamic LDS.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import bits_equal
from test_fast_domains import default_scene, differing_pixels, make_camera, scene_bound
from test_gpu_parity import assert_same, host, pipe  # noqa: F401  (pipe: the fixture)

gpu = pytest.mark.gpu

W, H = 64, 48
NPIX = W * H
SEED0 = 21
CAM_SEED = 0.375
FRAMES = 5
F32 = np.float32
NAN, INF = float("nan"), float("inf")


def below(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


def above(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


# ---- routes and their kernels ---------------------------------------------------------------
PAIR_KERNEL = {"off": "rt_trace_kernel<2>", "on": "rt_trace_kernel<3>",
               "quad": "rt_trace_kernel<4>", "on2": "rt_tpair_kernel<2>",
               "quad2": "rt_tpair_kernel<4>"}
PATH_KERNEL = {"per_wave": "rt_bounce_kernel<0>", "compact": "rt_bounce_kernel<1>",
               "pair": "rt_bounce_kernel<2>", "split": "rt_bounce_kernel<3>"}
EXHAUSTIVE = "rt_trace_kernel<0>"
PIPE_MODES = ["culled", "culled_one", "culled_general", "exhaustive"]


def update_kernel(mode, depth):
    """The instance one `update` runs under a mode of the `pipe` fixture: at these 48 tiles the
    camera-ray-only case runs one tile per wave unless rt_set_single_kernel is off."""
    if mode == "exhaustive":
        return EXHAUSTIVE
    if depth >= 2:
        return "rt_bounce_kernel<0>"
    return "rt_trace_kernel<2>" if mode == "culled_general" else "rt_single_kernel<1>"


def configure(p, mode):
    """A fresh context as the `pipe` fixture sets its own up."""
    p.set_scan_mode(mode.split("_")[0])
    if mode == "culled_general":
        p.set_single_kernel("off")
    elif mode == "culled_one":
        p.set_single_kernel("one")


def f2u(x):
    """WGSL u32(f32) as the oracle and the host convert it: truncate, saturate, NaN -> 0."""
    x = float(F32(x))
    if not x > 0.0:
        return 0
    return min(int(x), 0xFFFFFFFF)


# ---- cases: a camera, a scene, five seeds and the oracle's five frames from a reset --------
def frame_seeds(rt, first=CAM_SEED, n=FRAMES):
    s = np.array(rt.frame_seeds(SEED0, n), np.float32)
    s[0] = first
    return s


def oracle_frames(oracle, cam, spheres, seeds):
    """(image after each frame, segments traced per frame) of a chain from a reset."""
    imgs, segs, cur = [], [], np.zeros((H, W, 4), np.float32)
    for k, s in enumerate(seeds):
        c = cam.with_fields(random_seed=float(s))
        if k:
            c = c.with_fields(camera_has_moved=0.0)
        cur, n = oracle.update(cur, c.blob, spheres)
        cur.setflags(write=False)
        imgs.append(cur)
        segs.append(n)
    return imgs, segs


CASES = {}


def case_builder(name):
    def register(fn):
        CASES[name] = fn
        return fn
    return register


@functools.lru_cache(None)
def case(name):
    """The case's camera and scene and the oracle's chain, computed once and shared by the CPU
    twin and every GPU test of the case (read-only)."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    cam, spheres = CASES[name](rt, oracle)
    spheres = np.ascontiguousarray(spheres, np.float32).reshape(-1, 8)
    spheres.setflags(write=False)
    seeds = frame_seeds(rt, float(cam.random_seed))
    chain, segs = oracle_frames(oracle, cam, spheres, seeds)
    depth = f2u(cam.max_depth)
    return SimpleNamespace(name=name, cam=cam, spheres=spheres, seeds=seeds, chain=chain,
                           segs=segs, depth=depth, sc=rt.SphereCollection(spheres))


def nan_pixels(img):
    return int(np.isnan(np.asarray(img)[..., :3]).any(axis=-1).sum())


# ---- GPU runners: every one returns the list of what went wrong -----------------------------
def mismatch(got, want, what):
    ok, bad = bits_equal(got, want)
    return [] if ok else [f"{what}: {bad} channels differ from the oracle"]


def run_update(p, c, want_kernel):
    a, b = p.new_image(W, H), p.new_image(W, H)
    p.update(a, b, W, H, c.cam, c.sc)
    name = p.last_launch_info()["kernel_name"]
    wrong = mismatch(host(b), c.chain[0], f"update {name}")
    if name != want_kernel:
        wrong.append(f"update ran {name}, not {want_kernel}")
    return wrong


def run_render(p, c, frames=3):
    a, b = p.new_image(W, H), p.new_image(W, H)
    p.render(a, b, W, H, c.cam, c.sc, c.seeds[:frames])
    info = p.last_launch_info()
    wrong = mismatch(host(b), c.chain[frames - 1], f"render of {frames}")
    if info["kernel_name"] != EXHAUSTIVE or info["launches"] != 1:
        wrong.append(f"render ran {info}, not one launch of {EXHAUSTIVE}")
    return wrong


def run_frames(p, c, want_kernel, frames=FRAMES):
    a, b = p.new_image(W, H), p.new_image(W, H)
    newest = p.update_frames(a, b, W, H, c.cam, c.sc, c.seeds[:frames], 0, 1)
    info = p.last_launch_info()
    new, prev = (host(b), host(a)) if newest == 1 else (host(a), host(b))
    what = f"{frames} frames {info['kernel_name']}"
    wrong = mismatch(new, c.chain[frames - 1], what + " newest")
    wrong += mismatch(prev, c.chain[frames - 2], what + " previous")
    if info["kernel_name"] != want_kernel or info["frames"] != frames:
        wrong.append(f"update_frames ran {info}, not {frames} frames of {want_kernel}")
    return wrong


def frame_routes(depth):
    """(setter, mode, kernel) of the update_frames routes of a depth."""
    if depth >= 2:
        return [("set_path_compaction", m, k) for m, k in PATH_KERNEL.items()]
    return [("set_frame_pairs", m, k) for m, k in PAIR_KERNEL.items()]


def check_frames(rt, c, frames=FRAMES, routes=None):
    """update_frames on a fresh context per route; at depth >= 2 also `update` and a 3-frame
    `render` in exhaustive scan mode."""
    wrong = []
    for setter, mode, kernel in routes or frame_routes(c.depth):
        p = rt.ComputeShaderPipeline(0)
        try:
            getattr(p, setter)(mode)
            wrong += run_frames(p, c, kernel, frames)
        finally:
            p.close()
    if c.depth >= 2 and routes is None:
        p = rt.ComputeShaderPipeline(0)
        try:
            p.set_scan_mode("exhaustive")
            wrong += run_update(p, c, EXHAUSTIVE)
            wrong += run_render(p, c)
        finally:
            p.close()
    assert not wrong, (c.name, wrong)


def check_update(pipe, request, c):
    mode = request.node.callspec.params["pipe"]
    wrong = run_update(pipe, c, update_kernel(mode, c.depth))
    assert not wrong, (c.name, mode, wrong)


# ---- the float64 mirror of the camera rays and of the first hit -----------------------------
def vec(v):
    return np.array(list(v), np.float64)


def camera_rays(cam, dx=0.5, dy=0.5, lens=None):
    """Origin (3,) and directions (H, W, 3) of the rays through pixel position (x + dx, y + dy)
    (wgsl:305-325 without the jitter); lens = angle on the defocus circle, None = the centre."""
    c = cam.to_c()
    yy, xx = np.mgrid[0:H, 0:W]
    o = vec(c.center)
    if lens is not None:
        o = o + math.cos(lens) * vec(c.defocus_disk_u) + math.sin(lens) * vec(c.defocus_disk_v)
    d = (vec(c.viewport_upper_left) + (xx[..., None] + dx) * vec(c.pixel_delta_u) +
         (yy[..., None] + dy) * vec(c.pixel_delta_v) - o)
    return o, d


def first_hit(spheres, o, d):
    """sphere_list_hit (wgsl:164-221) in double for rays o + t d, d of shape (H, W, 3): hit
    mask, sphere index, face normal, front face."""
    s = np.asarray(spheres, np.float64).reshape(-1, 8)
    if not len(s):
        z = np.zeros(d.shape[:2])
        return z.astype(bool), z.astype(int), np.zeros(d.shape), z.astype(bool)
    cen, rad = s[:, :3], s[:, 3]
    oc = cen[None, None] - o                                   # (1, 1, N, 3)
    a = (d * d).sum(-1)[..., None]
    h = (oc * d[:, :, None, :]).sum(-1)
    cc = (oc * oc).sum(-1) - rad * rad
    disc = h * h - a * cc
    sq = np.sqrt(np.maximum(disc, 0.0))
    t1, t2 = (h - sq) / a, (h + sq) / a
    t = np.where(t1 > 1e-3, t1, np.where(t2 > 1e-3, t2, np.inf))
    t = np.where(disc < 0.0, np.inf, t)
    idx = t.argmin(-1)
    tt = np.take_along_axis(t, idx[..., None], -1)[..., 0]
    hit = np.isfinite(tt)
    pt = o + np.where(hit, tt, 0.0)[..., None] * d
    out = (pt - cen[idx]) / rad[idx][..., None]
    front = (d * out).sum(-1) < 0.0
    return hit, idx, np.where(front[..., None], out, -out), front


def is_dielectric(w):
    w = np.asarray(w, np.float64)
    return ~(w < -1.0) & ~(w <= 1.0)                           # wgsl:272-284, NaN included


def total_reflections(spheres, cam, lens_angles=(None,)):
    """(primary hits on dielectric spheres, those with ratio * sin_theta > 1 (wgsl:119)) by the
    mirror; with several lens angles a pixel counts when it does for every one of them."""
    s = np.asarray(spheres, np.float64).reshape(-1, 8)
    hits, tir = np.ones((H, W), bool), np.ones((H, W), bool)
    for ang in lens_angles:
        o, d = camera_rays(cam, lens=ang)
        hit, idx, n, front = first_hit(s, o, d)
        glass = hit & is_dielectric(s[idx, 7])
        ir = s[idx, 4]
        with np.errstate(all="ignore"):
            ratio = np.where(front, 1.0 / ir, ir)
            u = d / np.sqrt((d * d).sum(-1))[..., None]
            cos_t = np.minimum(-(u * n).sum(-1), 1.0)
            sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
            cannot = ratio * sin_t > 1.0
        hits &= glass
        tir &= glass & cannot
    return int(hits.sum()), int(tir.sum())


# =============================================================================================
# A. material and scatter edges
# =============================================================================================
A_DEPTHS = [1, 3]
A1_W = [-1.0, below(-1.0), 1.0, above(1.0), NAN, -0.5, 0.75, -0.0, INF, -INF]
A1_UNIFORM = {"m1": -1.0, "m1_below": below(-1.0), "p1": 1.0, "p1_above": above(1.0)}
A3_INDEX = {"0.5": 0.5, "2_3": 2.0 / 3.0, "1": 1.0, "0": 0.0, "m1.5": -1.5, "1e30": 1e30,
            "1e-30": 1e-30, "inf": INF, "nan": NAN}
A4_SEEDS = {"s0": 0.375, "s1": 0.8125}
A4_CENTER = (0.0, 1.0, 0.0)
A_SCENES = {}


def a_scene(name):
    def register(fn):
        A_SCENES[name] = fn
        for depth in A_DEPTHS:
            CASES[f"a_{name}_d{depth}"] = functools.partial(a_case, fn, depth)
        return fn
    return register


def a_case(fn, depth, rt, oracle):
    spheres, cam_kw = fn(rt, oracle)
    return make_camera(rt, depth, **cam_kw), spheres


@a_scene("w_round_robin")
def _(rt, oracle):
    s = default_scene(rt)
    s[:, 7] = [A1_W[i % len(A1_W)] for i in range(len(s))]
    return s, {}


for _name, _w in A1_UNIFORM.items():
    @a_scene("w_all_" + _name)
    def _(rt, oracle, w=_w):
        s = default_scene(rt)
        s[:, 7] = w
        return s, {}


for _name, _fuzz in (("fuzz_p1", 1.0), ("fuzz_m1", -1.0)):
    @a_scene(_name)
    def _(rt, oracle, fuzz=_fuzz):
        s = default_scene(rt)
        s[-3:, 7] = fuzz                                       # the three large spheres: metal
        s[-3:, 4:7] = [[0.9, 0.8, 0.7], [0.4, 0.2, 0.1], [0.7, 0.6, 0.5]]
        return s, {}


for _name, _ir in A3_INDEX.items():
    @a_scene("index_" + _name)
    def _(rt, oracle, ir=_ir):
        s = default_scene(rt)
        s[is_dielectric(s[:, 7]), 4] = ir
        return s, {}


@a_scene("large_index_0.5")
def _(rt, oracle):
    s = default_scene(rt)
    s[-3:, 4:] = [0.5, 0.0, 0.0, 2.0]
    return s, {}


def inside_glass(rt, ir):
    s = default_scene(rt)
    lf = rt.CameraSettings().look_from
    return np.concatenate([s, np.array([[lf[0], lf[1], lf[2], 0.5, ir, 0.0, 0.0, 2.0]],
                                       np.float32)])


@a_scene("inside_glass_1.5")
def _(rt, oracle):
    return inside_glass(rt, 1.5), {}


@a_scene("inside_glass_16")
def _(rt, oracle):
    """Rays leave the centre of the sphere around the camera almost along its normals
    (sin_theta is the lens radius over 0.5, about 0.1), so glass of index 1.5 never reflects
    them totally at that first exit; index 16 does for every ray."""
    return inside_glass(rt, 16.0), {}


def frame_ruv(oracle, seed):
    """random_unit_vector(hash(B + 2)) (wgsl:234-243, 268, 353): the scatter direction's random
    part at bounce 0 of a reset frame with this random_seed, the same for every pixel."""
    b = f2u(F32(seed) * F32(4294967296.0))
    sb = oracle.hash_u32((b + 2) & 0xFFFFFFFF)
    z = F32(2.0 * oracle.random_float(sb) - 1.0)
    ang = F32(np.float64(oracle.random_float(sb + 1)) * np.float64(F32(6.283185307)))
    r = F32(math.sqrt(float(F32(1.0 - float(z) * float(z)))))
    sa, ca = oracle.sincos(float(ang))
    return np.array([F32(r * F32(ca)), F32(r * F32(sa)), z], np.float64)


def a4_geometry(oracle, seed):
    ruv = frame_ruv(oracle, seed)
    p = np.array(A4_CENTER, np.float64) - ruv                  # R = 1: the normal there is -ruv
    return ruv, p


for _name, _seed in A4_SEEDS.items():
    @a_scene("degenerate_" + _name)
    def _(rt, oracle, seed=_seed):
        """One Lambertian sphere seen through a lens-less 0.02-degree camera aimed along ruv
        at the point whose normal is -ruv: the image straddles the cap |n + ruv|^2 < 1e-6."""
        ruv, p = a4_geometry(oracle, seed)
        s = np.array([[*A4_CENTER, 1.0, 0.8, 0.6, 0.4, -2.0]], np.float32)
        return s, dict(seed=seed, look_from=tuple(p - 10.0 * ruv), look_at=tuple(p),
                       field_of_view=0.02, defocus_angle=0.0, focus_distance=10.0)


A_CASES = [f"a_{n}_d{d}" for n in A_SCENES for d in A_DEPTHS]


# ---- A: CPU twins ---------------------------------------------------------------------------
@pytest.mark.parametrize("depth", A_DEPTHS)
def test_a1_each_threshold_changes_the_image(rt, oracle, depth):
    """The two sides of w = -1 (Lambertian below, metal at and above) and of w = 1 (metal at and
    below, dielectric above) give images that differ in at least 1000 of the 3072 pixels, and
    the scene that mixes all ten values of w holds no NaN pixel."""
    for lo, hi in (("m1_below", "m1"), ("p1", "p1_above")):
        a, b = case(f"a_w_all_{lo}_d{depth}"), case(f"a_w_all_{hi}_d{depth}")
        wa, wb = F32(a.spheres[0, 7]), F32(b.spheres[0, 7])
        assert np.nextafter(wa, F32(np.inf)) == wb and 1.0 in (abs(float(wa)), abs(float(wb)))
        changed = differing_pixels(a.chain[0], b.chain[0])
        print(f"depth {depth}: w {float(wa)!r} against {float(wb)!r}: {changed} changed pixels")
        assert changed >= 1000
    mixed = case(f"a_w_round_robin_d{depth}")
    assert len(set(np.asarray(mixed.spheres[:10, 7]).view(np.uint32).tolist())) == 10
    nans = [nan_pixels(img) for img in mixed.chain]
    print(f"depth {depth}: round-robin scene NaN pixels per frame {nans}")
    assert nans == [0] * FRAMES


@pytest.mark.parametrize("fuzz", ["fuzz_p1", "fuzz_m1"])
def test_a2_fuzz_extremes_absorb_and_reflect(rt, oracle, fuzz):
    """Depth 1, pixels whose centre ray hits one of the three large metal spheres first: at
    least 50 exactly black (the scatter pointed into the sphere, wgsl:99, 277-279) and at least
    50 not."""
    c = case(f"a_{fuzz}_d1")
    assert abs(float(c.spheres[-1, 7])) == 1.0 and c.depth == 1
    o, d = camera_rays(c.cam)
    hit, idx, _, _ = first_hit(c.spheres, o, d)
    on = hit & (idx >= len(c.spheres) - 3)
    black = (np.asarray(c.chain[0])[..., :3] == 0.0).all(-1)
    print(f"{fuzz}: {int(on.sum())} pixels on the spheres, {int((on & black).sum())} black, "
          f"{int((on & ~black).sum())} not")
    assert int((on & black).sum()) >= 50 and int((on & ~black).sum()) >= 50


def test_a3_total_internal_reflection_is_reached(rt, oracle):
    """At least 200 primary hits with ratio * sin_theta > 1 on the three large spheres at index
    0.5, and at the first exit of the rays that start inside the index-16 sphere (for every
    point of the lens circle); inside the index-1.5 sphere every ray's first hit is a back
    face and none reflects totally."""
    c = case("a_large_index_0.5_d3")
    hits, tir = total_reflections(c.spheres, c.cam)
    print(f"large spheres at index 0.5: {tir} of {hits} primary hits cannot refract")
    assert tir >= 200
    hits, tir = total_reflections(case("a_index_0.5_d3").spheres, c.cam)
    print(f"default scene's dielectrics at index 0.5: {tir} of {hits}")
    assert tir >= 1
    lens = [2.0 * math.pi * k / 16 for k in range(16)]
    for name, least, most in (("a_inside_glass_16_d3", 200, NPIX), ("a_inside_glass_1.5_d3", 0, 0)):
        c = case(name)
        o, d = camera_rays(c.cam)
        hit, idx, _, front = first_hit(c.spheres, o, d)
        assert hit.all() and (idx == len(c.spheres) - 1).all() and not front.any()
        hits, tir = total_reflections(c.spheres, c.cam, lens)
        print(f"{name}: {tir} of {hits} first exits cannot refract")
        assert hits == NPIX and least <= tir <= most


@pytest.mark.parametrize("depth", A_DEPTHS)
def test_a3_nan_pixels_per_index(rt, oracle, depth):
    """No NaN pixel for any finite or infinite index; under a quarter of the image for the NaN
    index (a NaN ray is accepted by every sphere in turn, wgsl:196, so the last one, the large
    metal sphere, absorbs it)."""
    for name in A3_INDEX:
        c = case(f"a_index_{name}_d{depth}")
        glass = is_dielectric(c.spheres[:, 7])
        assert glass.sum() >= 5 and np.array_equal(
            np.asarray(c.spheres[glass, 4]).view(np.uint32),
            np.full(int(glass.sum()), F32(A3_INDEX[name])).view(np.uint32))
        nans = max(nan_pixels(img) for img in c.chain)
        print(f"depth {depth} index {name}: at most {nans} NaN pixels in a frame")
        assert nans == 0 if name != "nan" else nans < NPIX // 4
    for name in ("large_index_0.5", "inside_glass_1.5", "inside_glass_16"):
        assert max(nan_pixels(img) for img in case(f"a_{name}_d{depth}").chain) == 0


@pytest.mark.parametrize("seed", list(A4_SEEDS))
def test_a4_image_straddles_the_degenerate_cap(rt, oracle, seed):
    """By the mirror, at the pixel's centre and four corners (the jitter stays within them): at
    least 200 pixels wholly inside the cap |n + ruv|^2 < 1e-6 and at least 200 wholly outside.
    The oracle's depth-1 image agrees: inside, the scattered ray is the normal, -ruv but for
    1e-3, so every such pixel shows albedo x sky(-ruv); outside, it is the short sum n + ruv,
    which points anywhere."""
    c = case(f"a_degenerate_{seed}_d1")
    ruv, p = a4_geometry(oracle, A4_SEEDS[seed])
    assert abs(float((ruv * ruv).sum()) - 1.0) < 1e-6 and abs(ruv[1]) < 0.95
    inside, outside = np.ones((H, W), bool), np.ones((H, W), bool)
    for dx, dy in ((0.5, 0.5), (0, 0), (0, 1), (1, 0), (1, 1)):
        o, d = camera_rays(c.cam, dx, dy)
        hit, _, n, front = first_hit(c.spheres, o, d)
        g = ((n + ruv) ** 2).sum(-1)
        inside &= hit & front & (g < 0.98e-6)
        outside &= ~hit | (g > 1.02e-6)
    print(f"{seed}: ruv {ruv}, {int(inside.sum())} pixels inside the cap, "
          f"{int(outside.sum())} outside, {NPIX - int(inside.sum()) - int(outside.sum())} across")
    assert int(inside.sum()) >= 200 and int(outside.sum()) >= 200
    a = 0.5 * (-ruv[1] + 1.0)
    sky = (1.0 - a) + a * np.array([0.5, 0.7, 1.0])
    want = np.asarray(c.spheres[0, 4:7], np.float64) * sky
    err = np.abs(np.asarray(c.chain[0])[..., :3] - want).max(-1)
    print(f"{seed}: |colour - albedo x sky(-ruv)| inside at most {err[inside].max():.2e}, "
          f"outside above 1e-2 in {int((err[outside] > 1e-2).sum())} pixels")
    assert err[inside].max() < 2e-3
    assert int((err[outside] > 1e-2).sum()) >= 200


# ---- A: GPU -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", A_CASES)
def test_a_update(rt, oracle, pipe, request, name):
    check_update(pipe, request, case(name))


@gpu
@pytest.mark.parametrize("name", A_CASES)
def test_a_frames(rt, oracle, name):
    check_frames(rt, case(name))


# =============================================================================================
# B. depth edges
# =============================================================================================
B_DEPTHS = [15, 16, 17, 30, 32, 33, 64, 65]
ENCLOSURE = [0.0, 0.0, 0.0, 30.0, 0.9, 0.9, 0.9, -2.0]


def b_scene(rt, which):
    """Inside a sphere of radius 30 around the origin: the camera at (13, 2, 3) is inside, no
    ray sees the sky.

    "literal" is the default scene as it is, in a Lambertian enclosure.  Some of its paths
    still end early: a fuzzed metal reflection that points into its sphere is absorbed
    (wgsl:99), and a path that leaves the ground where ground and enclosure cross can find the
    enclosure's root under the 0.001 of wgsl:196 and leave (81 of 46 080 segments short at
    depth 15; colours go down to 2e-32 between dark spheres).
    "grid" lets the twin require that every path reaches the last bounce and every colour
    stays above 2^-60: the default scene without its ground, every metal sphere's fuzz at 0,
    every opaque albedo raised to 0.7 + 0.3 x; the glass spheres stay.  "small" is its three
    large spheres only.
    A Lambertian enclosure merges the paths, though.  The scatter's random vector is the same
    for every pixel (wgsl:268, 353), and from any point p of a sphere (C, R) seen from inside,
    the ray along n + ruv = (C - p) / R + ruv meets the sphere again at t = R in C + R ruv: after
    its first bounce off the enclosure every pixel follows one path (191 distinct colours in a
    frame; in "literal" that one path is absorbed by a fuzzed metal sphere at bounce 33 of one
    frame, and 3057 pixels with it).  "mirror" is "grid" inside a mirror of the same size: its
    paths stay apart (3054 distinct colours) and never end either."""
    s = default_scene(rt)
    if which != "literal":
        opaque = ~is_dielectric(s[:, 7])
        s[opaque, 4:7] = 0.7 + 0.3 * s[opaque, 4:7]
        s[~(s[:, 7] < -1.0) & opaque, 7] = 0.0
        s = s[-3:] if which == "small" else s[1:]
    s = np.concatenate([s, np.array([ENCLOSURE], np.float32)])
    if which == "mirror":
        s[-1, 7] = 0.0
    return s


B_SCENES = ("grid", "small", "literal", "mirror")
for _which in B_SCENES:
    for _depth in B_DEPTHS:
        @case_builder(f"b_{_which}_d{_depth}")
        def _(rt, oracle, which=_which, depth=_depth):
            return make_camera(rt, depth), b_scene(rt, which)

B_CASES = [f"b_{w}_d{d}" for w in B_SCENES for d in B_DEPTHS]

# u32(f32) of max_depth and samples_per_pixel on the default scene: (field values, the integer
# settings that must give the same image)
B_CONV = {
    "depth_under_2": (dict(max_depth=below(2.0)), dict(max_depth=1.0)),
    "depth_2.5": (dict(max_depth=2.5), dict(max_depth=2.0)),
    "depth_m3": (dict(max_depth=-3.0), dict(max_depth=0.0)),
    "depth_m0": (dict(max_depth=-0.0), dict(max_depth=0.0)),
    "depth_nan": (dict(max_depth=NAN), dict(max_depth=0.0)),
    "spp_3.7_d1": (dict(max_depth=1.0, samples_per_pixel=3.7), dict(samples_per_pixel=3.0)),
    "spp_3.7_d3": (dict(max_depth=3.0, samples_per_pixel=3.7), dict(samples_per_pixel=3.0)),
    "spp_m1_d1": (dict(max_depth=1.0, samples_per_pixel=-1.0), dict(samples_per_pixel=0.0)),
    "spp_m1_d3": (dict(max_depth=3.0, samples_per_pixel=-1.0), dict(samples_per_pixel=0.0)),
    "spp_nan_d1": (dict(max_depth=1.0, samples_per_pixel=NAN), dict(samples_per_pixel=0.0)),
    "spp_nan_d3": (dict(max_depth=3.0, samples_per_pixel=NAN), dict(samples_per_pixel=0.0)),
}
for _name, (_fields, _) in B_CONV.items():
    @case_builder("b_conv_" + _name)
    def _(rt, oracle, fields=_fields):
        return make_camera(rt, 3).with_fields(**fields), default_scene(rt)

B_CONV_CASES = ["b_conv_" + n for n in B_CONV]


# ---- B: CPU twins ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", B_SCENES)
def test_b_every_path_lives_to_the_last_bounce(rt, oracle, which):
    """Inside the enclosure the oracle traces exactly W x H x depth segments in every frame,
    neighbouring depths of the list differ in all 3072 pixels, no NaN appears and every colour
    stays above 2^-60 (so no guard of the accumulator's fast cores hides the depth).
    "literal" (b_scene): at least 14 segments per pixel in every frame (no other test runs
    more than 8 bounces), no NaN, and all but 16 pixels differ."""
    count = len(b_scene(rt, which))
    assert (count >= 64) == (which != "small")                 # kGridMinSpheres
    prev = None
    for depth in B_DEPTHS:
        c = case(f"b_{which}_d{depth}")
        assert c.depth == depth
        if which == "literal":
            assert all(14 * NPIX <= s <= NPIX * depth for s in c.segs), c.segs
        else:
            assert c.segs == [NPIX * depth] * FRAMES, (depth, c.segs)
        rgb = np.concatenate([np.asarray(img)[..., :3] for img in c.chain])
        lit = rgb[rgb > 0.0]
        assert nan_pixels(rgb) == 0
        assert which == "literal" or float(rgb.min()) > 2.0 ** -60
        colours = len(np.unique(np.asarray(c.chain[0])[..., :3].reshape(-1, 3), axis=0))
        assert which != "mirror" or colours >= 2000
        changed = NPIX if prev is None else differing_pixels(prev.chain[0], c.chain[0])
        print(f"{which} depth {depth}: {c.segs[0] / NPIX:.4f} segments per pixel, minimum "
              f"colour {float(lit.min()):.3g}, 0 NaN pixels, {colours} distinct colours, "
              f"{changed} pixels differ from the depth before")
        assert changed == NPIX or which == "literal" and changed >= NPIX - 16
        prev = c
    # the hint tables' bounds fall inside the list (rt_kernels.h)
    assert [64 // d for d in (32, 33, 64, 65)] == [2, 1, 1, 0] and {16, 17} <= set(B_DEPTHS)


def test_b_conversions_truncate_saturate_and_drop_nan(rt, oracle):
    """u32(f32) (wgsl:264, 343): every case's chain equals the chain of the integer it must
    convert to; samples_per_pixel 3.7 stops at count 3, and -1 and NaN never sample."""
    for name, (fields, same_as) in B_CONV.items():
        c = case("b_conv_" + name)
        other = c.cam.with_fields(**same_as)
        want, segs = oracle_frames(oracle, other, c.spheres, c.seeds)
        for got, ref in zip(c.chain, want):
            assert_same(got, ref)
        counts = [float(np.asarray(img)[..., 3].max()) for img in c.chain]
        assert all((np.asarray(img)[..., 3] == n).all() for img, n in zip(c.chain, counts))
        print(f"{name}: depth {c.depth}, counts per frame {counts}, segments per pixel "
              f"{[s / NPIX for s in c.segs]}")
        assert c.segs == segs
        if name.startswith("spp_3.7"):
            assert counts == [1.0, 2.0, 3.0, 3.0, 3.0] and c.segs[3:] == [0, 0]
        elif name.startswith("spp"):
            assert counts == [0.0] * FRAMES and not np.asarray(c.chain[-1]).any()
        else:
            assert counts == [1.0, 2.0, 3.0, 4.0, 5.0]
            assert c.depth == {"depth_under_2": 1, "depth_2.5": 2}.get(name, 0)
            assert all(NPIX * min(c.depth, 1) <= s <= NPIX * c.depth for s in c.segs)
    one, two = case("b_conv_depth_under_2"), case("b_conv_depth_2.5")
    assert differing_pixels(one.chain[0], two.chain[0]) >= 500     # (every pixel that hits)


# ---- B: GPU -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", B_CASES)
def test_b_depth_frames(rt, oracle, name):
    """The four bounce routes (5 frames; from depth 17 on without the device table, which the
    launch itself refuses beyond kHintRsDepth) and the exhaustive instance's `update` and
    3-frame `render` (hinted and unhinted frames in one launch at 32 and 33)."""
    check_frames(rt, case(name))


@gpu
@pytest.mark.parametrize("name", B_CASES[:len(B_DEPTHS)])
def test_b_depth_update(rt, oracle, pipe, request, name):
    check_update(pipe, request, case(name))


@gpu
@pytest.mark.parametrize("name", B_CONV_CASES)
def test_b_conversion_update(rt, oracle, pipe, request, name):
    check_update(pipe, request, case(name))


@gpu
@pytest.mark.parametrize("name", B_CONV_CASES)
def test_b_conversion_frames(rt, oracle, name):
    """(max_depth just under 2 must run the depth-1 instances: the routes' kernel names.)"""
    check_frames(rt, case(name))


# =============================================================================================
# C. sphere counts
# =============================================================================================
C_COUNTS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 128, 129]
C_BACK = [33, 2, 0]                       # the one-context sequence shrinks again
C_DEPTHS = [3, 1]
C_LARGE = [4095, 4096, 4097]
K_GRID_MIN_SPHERES = 64                   # rt_scene.cpp
K_CULL_MIN_SPHERES = 32                   # rt_trace_device.h: shorter lists are scanned whole
K_LDS_MAX_RECORDS = 4096                  # rt_kernels.h


def c_permutation(rt):
    """The default scene in a fixed order: the ground, the three large spheres, then the small
    ones shuffled (a prefix in generation order would fill one corner of the field only)."""
    s = default_scene(rt)
    small = np.random.default_rng(5).permutation(np.arange(1, len(s) - 3))
    return s[np.concatenate([[0], np.arange(len(s) - 3, len(s)), small])]


def grid_rule(spheres):
    """build_grid's rule (rt_scene.cpp): (a grid is built, the small spheres counted) — at least
    kGridMinSpheres spheres within the scene bound, of which at least half that many have a
    radius of at most four times the median."""
    s = np.asarray(spheres, np.float64).reshape(-1, 8)
    if not len(s):
        return False, 0
    radii = np.abs(s[:, 3])
    small = int((radii <= 4.0 * np.sort(radii)[len(s) // 2]).sum())
    built = (len(s) >= K_GRID_MIN_SPHERES and scene_bound(spheres) <= 2.0 ** 40 and
             small >= K_GRID_MIN_SPHERES // 2)
    return built, small


for _n in C_COUNTS:
    for _depth in C_DEPTHS:
        @case_builder(f"c_n{_n}_d{_depth}")
        def _(rt, oracle, n=_n, depth=_depth):
            return make_camera(rt, depth), c_permutation(rt)[:n]

for _n in C_LARGE:
    for _depth in C_DEPTHS:
        @case_builder(f"c_n{_n}_d{_depth}")
        def _(rt, oracle, n=_n, depth=_depth):
            return make_camera(rt, depth), np.array(rt.synthetic_scene(n).spheres, np.float32)


# ---- C: CPU twins ---------------------------------------------------------------------------
def test_c_sphere_collection_holds_zero_rows(rt, oracle):
    sc = rt.SphereCollection(np.zeros((0, 8), np.float32))
    assert sc.count == 0 and sc.as_bytes() == b""
    c = case("c_n0_d3")
    assert c.sc.count == 0 and c.segs == [NPIX] * FRAMES       # one miss per pixel, then the sky
    assert differing_pixels(c.chain[0], case("c_n1_d3").chain[0]) >= 1000


def test_c_small_counts_cross_their_thresholds(rt, oracle):
    """The prefixes by the mirror of build_grid's rule: no grid up to 63 spheres, one from 64
    on; the rule's second condition (32 small spheres) is met by every prefix of 64 or more —
    more than half of any finite radii are at most their median — and the prefixes cross 32
    small spheres on their own below that.  31 / 32 / 33 straddle kCullMinSpheres, 63 / 64 /
    65 the 64-record padding and a fresh context's first capacity, 128 / 129 the next one.
    From 63 spheres on the image differs from the ground's in at least 1000 pixels."""
    perm = c_permutation(rt)
    assert len(perm) == len(default_scene(rt)) >= max(C_COUNTS) and perm[0, 3] == 1000.0
    rule = {n: grid_rule(perm[:n]) for n in range(len(perm) + 1)}
    first_grid = min(n for n, (built, _) in rule.items() if built)
    first_small = min(n for n, (_, small) in rule.items() if small >= K_GRID_MIN_SPHERES // 2)
    print(f"grid from {first_grid} spheres on; 32 small spheres from {first_small} on")
    assert first_grid == K_GRID_MIN_SPHERES and first_small < first_grid
    assert all(rule[n][0] == (n >= first_grid) for n in rule)
    assert {first_grid - 1, first_grid, first_grid + 1} <= set(C_COUNTS)
    assert {K_CULL_MIN_SPHERES - 1, K_CULL_MIN_SPHERES, K_CULL_MIN_SPHERES + 1} <= set(C_COUNTS)
    assert any(rule[n][1] < 32 for n in C_COUNTS if n) and any(rule[n][1] > 32 for n in C_COUNTS)
    pad = lambda n: (n + 63) & ~63
    cap = lambda n: max(64, 1 << (n - 1).bit_length()) if n else 64
    assert [pad(n) for n in (63, 64, 65, 128, 129)] == [64, 64, 128, 128, 192]
    assert [cap(n) for n in (0, 64, 65, 128, 129)] == [64, 64, 128, 128, 256]
    for depth in C_DEPTHS:
        ground = case(f"c_n1_d{depth}")
        for n in C_COUNTS:
            c = case(f"c_n{n}_d{depth}")
            assert len(c.spheres) == n and nan_pixels(c.chain[-1]) == 0
            changed = differing_pixels(c.chain[0], ground.chain[0])
            print(f"depth {depth}, {n} spheres: grid {rule[n][0]}, {rule[n][1]} small, "
                  f"{changed} pixels differ from the ground's image")
            if n >= 63:
                assert changed >= 1000


def test_c_large_counts_straddle_the_lds_bound(rt, oracle):
    """4095 and 4096 records pad to kLdsMaxRecords (the compact instance stages them in LDS:
    64 KiB of dynamic LDS beside its 16 KiB of path slots), 4097 to more (no copy)."""
    for n in C_LARGE:
        c = case(f"c_n{n}_d3")
        padded = (len(c.spheres) + 63) & ~63
        print(f"{n} spheres pad to {padded} records, {padded * 16} bytes")
        assert len(c.spheres) == n and (padded <= K_LDS_MAX_RECORDS) == (n <= 4096)
        assert padded == (4096 if n <= 4096 else 4160) and grid_rule(c.spheres)[0]


# ---- C: GPU -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("depth", C_DEPTHS)
@pytest.mark.parametrize("n", C_COUNTS)
def test_c_small_count_on_fresh_contexts(rt, oracle, n, depth):
    """Every route of the depth, each on a context that has seen no other scene."""
    c = case(f"c_n{n}_d{depth}")
    wrong = []
    for mode in PIPE_MODES:
        p = rt.ComputeShaderPipeline(0)
        try:
            configure(p, mode)
            wrong += run_update(p, c, update_kernel(mode, depth))
        finally:
            p.close()
    assert not wrong, (c.name, wrong)
    check_frames(rt, c)


def c_sequence_routes():
    out = []
    for depth in C_DEPTHS:
        out += [(depth, "frames", r) for r in frame_routes(depth)]
        out += [(depth, "update", m) for m in PIPE_MODES]
    return out


@gpu
@pytest.mark.parametrize("depth,kind,route", c_sequence_routes(),
                         ids=lambda v: v if isinstance(v, str) else
                         str(v) if isinstance(v, int) else v[1])
def test_c_counts_grow_and_shrink_on_one_context(rt, oracle, depth, kind, route):
    """The counts in ascending order and back down on one context: every step uploads another
    scene, the capacity doubles twice on the way up, and on the way down the buffers keep the
    longer scene's records beyond the count."""
    p = rt.ComputeShaderPipeline(0)
    wrong = []
    try:
        if kind == "frames":
            getattr(p, route[0])(route[1])
        else:
            configure(p, route)
        for n in C_COUNTS + C_BACK:
            c = case(f"c_n{n}_d{depth}")
            if kind == "frames":
                wrong += [f"{n} spheres: {w}" for w in run_frames(p, c, route[2])]
            else:
                wrong += [f"{n} spheres: {w}" for w in run_update(p, c, update_kernel(route, depth))]
    finally:
        p.close()
    assert not wrong, wrong


@gpu
@pytest.mark.parametrize("n", C_LARGE)
def test_c_large_counts(rt, oracle, n):
    """Depth 3, 3 frames: the compact instance with its LDS copy of the records at 4095 and
    4096 spheres and without it at 4097, and the per-wave instance; one `update` at depth 1."""
    routes = [r for r in frame_routes(3) if r[1] in ("compact", "per_wave")]
    check_frames(rt, case(f"c_n{n}_d3"), frames=3, routes=routes)
    c = case(f"c_n{n}_d1")
    p = rt.ComputeShaderPipeline(0)
    try:
        wrong = run_update(p, c, update_kernel("culled", 1))
    finally:
        p.close()
    assert not wrong, (c.name, wrong)
