"""The exact fast cores on both sides of every guard that admits them.

Each guard is a hard threshold: the scene bound max(|C| + |R|) <= 2^40, every radius in
[2^-20, 2^20], camera rays with |d|^2 in [2^-11, 2^20], bounce rays per wave (a in
[2^-11, 2^20], origin components below 2^39), accumulator counts n + 1 < 2^22 and numerators
of at least 2^-102.  Every parity case here is a pair of inputs, one just inside a guard and
one just outside it, compared bit for bit with the CPU oracle; where the kernel name reveals
the selection (depth 1: list instance against culled instance) the pair must land on opposite
sides.  The CPU tests assert from the oracle and a double-precision mirror of the host's guards
that no case is vacuous.  The device self-test of the root selection (rt_selftest_roots) and
its header's export test are here too."""
import functools
import math

import numpy as np
import pytest

from conftest import bits_equal
from test_gpu_parity import assert_same, host, to_dev

gpu = pytest.mark.gpu

W, H = 64, 48
SEED0 = 21
CULLED = "rt_trace_kernel<1>"
LOOK_FROM = (13.0, 2.0, 3.0)
SKY_AT = (0.0, 9.0, 0.0)              # from LOOK_FROM this looks over the scene at the sky
F32 = np.float32


def below(x):
    return float(np.nextafter(F32(x), F32(0)))


def above(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


# ---- the host's guards, mirrored in double (rt_scene.cpp) ----------------------------------
def scene_bound(spheres):
    s = np.asarray(spheres, np.float32).reshape(-1, 8).astype(np.float64)
    if not len(s):
        return 0.0
    return float(np.max(np.sqrt((s[:, :3] ** 2).sum(1)) + np.abs(s[:, 3])))


def radii_ok(spheres):
    r = np.abs(np.asarray(spheres, np.float32).reshape(-1, 8)[:, 3].astype(np.float64))
    return bool(np.all((r >= 2.0 ** -20) & (r <= 2.0 ** 20)))


def camera_rays_bounded(cam, w, h, spheres):
    """camera_rays_bounded of rt_scene.cpp from the camera blob: (bounded, dmin^2, dmax^2)."""
    c = cam.to_c()
    f = lambda v: np.array(list(v), np.float64)
    center, vul = f(c.center), f(c.viewport_upper_left)
    pdu, pdv = f(c.pixel_delta_u), f(c.pixel_delta_v)
    defocus = c.defocus_angle > 0.0
    du = f(c.defocus_disk_u) if defocus else np.zeros(3)
    dv = f(c.defocus_disk_v) if defocus else np.zeros(3)
    norm = lambda v: float(np.sqrt((v * v).sum()))
    e = vul - center
    nrm = np.cross(pdu, pdv)
    nn = norm(nrm)
    if not (nn > 0.0 and math.isfinite(nn)):
        return False, 0.0, math.inf
    along = lambda v: abs(float((v * nrm).sum())) / nn
    lens = norm(du) + norm(dv)
    span = (w + 8.0) * norm(pdu) + (h + 8.0) * norm(pdv)
    mag = norm(vul) + norm(center) + span + lens
    dmax = norm(e) + span + lens + 1e-5 * mag
    dmin = along(e) - along(du) - along(dv) - 1e-5 * mag
    ok = (radii_ok(spheres) and dmin > 0.0 and dmin * dmin >= 2.0 ** -11 and
          dmax * dmax <= 2.0 ** 20 and
          norm(center) + lens * (1.0 + 1e-5) + scene_bound(spheres) <= 2.0 ** 40)
    return ok, dmin * dmin, dmax * dmax


# ---- running a case ------------------------------------------------------------------------
def make_camera(rt, depth, w=W, h=H, spp=500, moved=True, seed=0.375, **kw):
    s = rt.CameraSettings(max_depth=depth, samples_per_pixel=spp, camera_has_moved=moved, **kw)
    return rt.SceneCamera.from_settings(s, w, h, seed)


def oracle_chain(oracle, state, cam, spheres, seeds):
    """The oracle's image after each frame of an update_frames call: frame 0 honours the
    camera's camera_has_moved, the later ones continue."""
    out, cur = [], np.ascontiguousarray(state, np.float32)
    for k, s in enumerate(seeds):
        c = cam.with_fields(random_seed=float(s))
        if k:
            c = c.with_fields(camera_has_moved=0.0)
        cur, _ = oracle.update(cur, c.blob, spheres)
        out.append(cur)
    return out


def differing_pixels(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    return int((a != b).any(axis=-1).sum())


def run_frames(rt, p, cam, sc, seeds, w=W, h=H, state=None):
    """len(seeds) frames on pipeline p from `state` (zeros): (newest, previous, launch info);
    one frame through `update`, more through update_frames."""
    a = p.new_image(w, h) if state is None else to_dev(np.array(state))
    b = p.new_image(w, h)
    if len(seeds) == 1:
        p.update(a, b, w, h, cam.with_fields(random_seed=float(seeds[0])), sc)
        return host(b), host(a), p.last_launch_info()
    newest = p.update_frames(a, b, w, h, cam, sc, seeds, 0, 1)
    info = p.last_launch_info()
    return (host(b), host(a), info) if newest == 1 else (host(a), host(b), info)


def check_case(rt, oracle, cam, spheres, frames=2, side=None):
    """`frames` frames from a reset against the oracle, both buffers; side: "list" / "culled"
    is the depth-1 instance the launch must have selected."""
    sc = rt.SphereCollection(np.ascontiguousarray(spheres, np.float32))
    seeds = rt.frame_seeds(SEED0, frames)
    p = rt.ComputeShaderPipeline(0)
    try:
        newest, prev, info = run_frames(rt, p, cam, sc, seeds)
    finally:
        p.close()
    want = oracle_chain(oracle, np.zeros((H, W, 4), np.float32), cam, sc.spheres, seeds)
    name = info["kernel_name"]
    wrong = []                         # (selection and parity reported together)
    if side == "culled" and name != CULLED:
        wrong.append(f"ran {name}, not the culled instance")
    if side == "list" and (name in (CULLED, "rt_trace_kernel<0>") or "bounce" in name):
        wrong.append(f"ran {name}, not a list instance")
    if side == "bounce" and not name.startswith("rt_bounce_kernel"):
        wrong.append(f"ran {name}, not the bounce instance")
    for got, ref in ((newest, want[-1]), (prev, want[-2]))[:min(frames, 2)]:
        ok, bad = bits_equal(got, ref)
        if not ok:
            wrong.append(f"{bad} channels differ from the oracle")
    assert not wrong, wrong


def depth_side(depth, inside):
    return "bounce" if depth >= 2 else "list" if inside else "culled"


# ---- the scenes ------------------------------------------------------------------------------
def default_scene(rt):
    return np.array(rt.create_default_spheres(3).spheres, np.float32).reshape(-1, 8)


def small_scene(rt):
    return np.array(rt.three_spheres().spheres, np.float32).reshape(-1, 8)


def on_axis(dist, look_at=SKY_AT):
    """The f32 point `dist` from LOOK_FROM along the view axis (computed in double)."""
    lf, la = np.array(LOOK_FROM, np.float64), np.array(look_at, np.float64)
    axis = (la - lf) / np.sqrt(((la - lf) ** 2).sum())
    return (lf + dist * axis).astype(np.float32)


def far_sphere(center, radius):
    return np.array([[center[0], center[1], center[2], radius, 0.8, 0.3, 0.2, -2.0]], np.float32)


# B1: a sphere of R = 2^20 on the view axis of a 0.001-degree camera, depth 1.  The guard of
# the list instance is |center| + bound <= 2^40 (camera_rays_bounded; no lens).
B1_R = 2.0 ** 20
B1_CAMERA = dict(look_from=LOOK_FROM, look_at=SKY_AT, field_of_view=1e-3, defocus_angle=0.0)


def b1_guard(center):
    c = np.asarray(center, np.float32).astype(np.float64)
    return float(np.sqrt((np.array(LOOK_FROM) ** 2).sum()) + np.sqrt((c * c).sum()) + B1_R)


@functools.lru_cache(None)
def b1_edge_centers():
    """The f32 centres on the view axis nearest the guard: the last one at or under 2^40 and
    the first one over, one ulp of the largest coordinate (x) apart."""
    c = on_axis(2.0 ** 40 - B1_R)
    step = lambda v, to: np.array([np.nextafter(v[0], F32(to)), v[1], v[2]], np.float32)
    while b1_guard(c) > 2.0 ** 40:
        c = step(c, 0.0)
    while b1_guard(step(c, -np.inf)) <= 2.0 ** 40:          # (x is negative: away from zero)
        c = step(c, -np.inf)
    return tuple(c), tuple(step(c, -np.inf))


def b1_center(place):
    if place == "in":
        return on_axis(2.0 ** 39.5)
    if place == "out":
        return on_axis(2.0 ** 40.2)
    return np.array(b1_edge_centers()[0 if place == "in_edge" else 1], np.float32)


B1_PLACES = {"in": True, "out": False, "in_edge": True, "out_edge": False}

# B2: bounce instance (depth 3), default camera turned to SKY_AT; (radius, distance)
B2_CAMERA = dict(look_from=LOOK_FROM, look_at=SKY_AT, field_of_view=20.0, defocus_angle=0.6)
B2_PLACES = {"in_2p39.5": (2.0 ** 37, 2.0 ** 39.5, True),
             "in_2p39.9": (2.0 ** 36, 2.0 ** 39.9, True),
             "out_2p40.5": (2.0 ** 38, 2.0 ** 40.5, False)}
B2_BASES = {"grid": default_scene, "four": small_scene}

# B3: the radius ends.  small: three spheres of radius R seen from 2^-5 away through a
# 0.02-degree camera; large: a ground sphere of radius R under the default spheres.
B3_RADII = {"small_in": 2.0 ** -20, "small_out": below(2.0 ** -20),
            "large_in": 2.0 ** 20, "large_out": above(2.0 ** 20)}
B3_SMALL_CAMERA = dict(look_from=(0.0, 0.0, 2.0 ** -5), look_at=(0.0, 0.0, 0.0),
                       focus_distance=2.0 ** -5, field_of_view=0.02, defocus_angle=0.0)


def b3_scene(rt, which):
    r = B3_RADII[which]
    if which.startswith("small"):
        return np.array([[-3 * r, 0, 0, r, 1.5, 0, 0, 2.0],
                         [0, 0, 0, r, 0.4, 0.2, 0.1, -2.0],
                         [3 * r, 0, 0, r, 0.7, 0.6, 0.5, 0.0]], np.float32), {}
    base = default_scene(rt)
    base[0, 1], base[0, 3] = -r, r
    return base, {}


def b3_camera(rt, which, depth):
    return make_camera(rt, depth, **(B3_SMALL_CAMERA if which.startswith("small") else {}))


def b3_without(rt, which):
    if which.startswith("small"):
        return np.zeros((0, 8), np.float32)
    return default_scene(rt)[1:]


# B4: the camera-ray length ends.  Without a lens the focus distance only scales the rays
# (the view stays), so the default scene is seen through every rung.  camera_rays_bounded is
# conservative (it bounds |d| over the padded image and widens by 1e-5 of the magnitudes), so
# each ladder takes two rungs from the guard's own switch (bisected on the mirror above) and
# the rest around the power of two, where roots_fast_wave's exact test of a = |d|^2 switches
# inside the image at depth 3.
def b4_camera(rt, f, depth):
    return make_camera(rt, depth, focus_distance=float(f), defocus_angle=0.0)


@functools.lru_cache(None)
def b4_switch(low):
    import gpu_ray_tracing as rt
    sc = default_scene(rt)
    inside, outside = (1.0, 2.0 ** -7) if low else (1.0, 2.0 ** 11)
    for _ in range(60):
        mid = math.sqrt(inside * outside)
        if camera_rays_bounded(b4_camera(rt, mid, 1), W, H, sc)[0]:
            inside = mid
        else:
            outside = mid
    return inside


def b4_ladder(low):
    s = b4_switch(low)
    if low:
        return [s * 1.5, s * (1 + 1e-3), s * (1 - 1e-3), 2.0 ** -5.5 * 1.005, 2.0 ** -5.5 * 0.99,
                2.0 ** -5.5 / 1.5]
    return [s / 1.5, s * (1 - 1e-3), s * (1 + 1e-3), 2.0 ** 10 * 0.99, 2.0 ** 10 * 1.01,
            2.0 ** 10 * 1.5]


# B5: counts around 2^22 (kAccRnMax) and 2^24 (where f32(n + 1) stops being exact)
B5_COUNTS = ([2 ** 22 + k for k in range(-3, 2)] + [2 ** 24 + k for k in range(-2, 2)])
B5_SHAPE = (40, 24)
B5_SPP = 2 ** 25

# B6: albedos whose products with the sky fall under 2^-102 (acc_ok's bound)
B6_ALBEDOS = [2.0 ** -101, 2.0 ** -102, 2.0 ** -103, 2.0 ** -140]


def b6_scene(albedo):
    return np.array([[0, -1000, 0, 1000, 0.5, 0.5, 0.5, -2.0],
                     [0, 1, 0, 1, 1.5, 0, 0, 2.0],
                     [-4, 1, 0, 1, albedo, albedo, albedo, -2.0],
                     [4, 1, 0, 1, albedo, albedo, albedo, 0.0]], np.float32)


def tiny_channels(img):
    c = np.asarray(img)[..., :3]
    return int(((c > 0) & (c < 2.0 ** -102)).sum())


# ---- CPU preconditions: no case is vacuous ----------------------------------------------------
def oracle_two_frames(oracle, rt, cam, spheres):
    return oracle_chain(oracle, np.zeros((H, W, 4), np.float32), cam, spheres,
                        rt.frame_seeds(SEED0, 2))[-1]


@pytest.mark.parametrize("place", list(B1_PLACES))
def test_b1_far_sphere_is_seen_and_on_its_side(rt, oracle, place):
    inside = B1_PLACES[place]
    c = b1_center(place)
    sc = np.concatenate([default_scene(rt), far_sphere(c, B1_R)])
    bound = scene_bound(sc)
    assert (bound <= 2.0 ** 40) == inside and (b1_guard(c) <= 2.0 ** 40) == inside
    assert radii_ok(sc)
    cam = make_camera(rt, 1, **B1_CAMERA)
    assert camera_rays_bounded(cam, W, H, sc)[0] == inside
    assert camera_rays_bounded(cam, W, H, default_scene(rt))[0]
    if place.endswith("edge"):
        lo, hi = b1_edge_centers()
        assert lo[1:] == hi[1:] and np.nextafter(F32(lo[0]), F32(-np.inf)) == F32(hi[0])
        assert abs(bound - 2.0 ** 40) < 2.0 ** 17     # within an ulp of the coordinate (2^16)
    changed = differing_pixels(oracle_two_frames(oracle, rt, cam, sc),
                               oracle_two_frames(oracle, rt, cam, default_scene(rt)))
    print(place, "bound / 2^40 =", bound / 2.0 ** 40, "changed pixels:", changed)
    assert changed >= 100


@pytest.mark.parametrize("base", list(B2_BASES))
@pytest.mark.parametrize("place", list(B2_PLACES))
def test_b2_far_sphere_is_seen_and_on_its_side(rt, oracle, place, base):
    radius, dist, inside = B2_PLACES[place]
    c = on_axis(dist)
    without = B2_BASES[base](rt)
    sc = np.concatenate([without, far_sphere(c, radius)])
    assert (scene_bound(sc) <= 2.0 ** 40) == inside
    assert (len(sc) >= 64) == (base == "grid")         # kGridMinSpheres
    if inside:
        # hit points on the far sphere lie beyond 2^39 in x (roots_fast_wave's origin test);
        # those on the near spheres do not
        near = float(np.abs(c.astype(np.float64)[0]) * (dist - radius) / dist)
        assert near > 2.0 ** 39 and scene_bound(without) < 2.0 ** 39
    cam = make_camera(rt, 3, **B2_CAMERA)
    changed = differing_pixels(oracle_two_frames(oracle, rt, cam, sc),
                               oracle_two_frames(oracle, rt, cam, without))
    print(place, base, "bound / 2^40 =", scene_bound(sc) / 2.0 ** 40, "changed pixels:", changed)
    assert changed >= 100


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("which", list(B3_RADII))
def test_b3_end_radius_is_seen_and_on_its_side(rt, oracle, which, depth):
    sc, _ = b3_scene(rt, which)
    inside = which.endswith("_in")
    assert radii_ok(sc) == inside and scene_bound(sc) <= 2.0 ** 40
    r = F32(B3_RADII[which])
    edge = F32(2.0 ** -20 if which.startswith("small") else 2.0 ** 20)
    away = F32(0) if which.startswith("small") else F32(np.inf)
    assert r == edge if inside else r == np.nextafter(edge, away)
    cam = b3_camera(rt, which, depth)
    assert camera_rays_bounded(cam, W, H, sc)[0] == inside
    changed = differing_pixels(oracle_two_frames(oracle, rt, cam, sc),
                               oracle_two_frames(oracle, rt, cam, b3_without(rt, which)))
    print(which, depth, "changed pixels:", changed)
    assert changed >= 100


@pytest.mark.parametrize("low", [True, False])
def test_b4_ladders_straddle_the_guard_and_the_power_of_two(rt, low):
    sc = default_scene(rt)
    sides = [camera_rays_bounded(b4_camera(rt, f, 1), W, H, sc)[0] for f in b4_ladder(low)]
    assert sides[:3] == [True, True, False] and not any(sides[3:]), sides
    # the rays' own a = |d|^2 (pixel centres): entirely inside the range on the first rung,
    # on both sides of the power of two within the ladder's last three
    def a_range(f):
        c = b4_camera(rt, f, 1).to_c()
        g = lambda v: np.array(list(v), np.float64)
        yy, xx = np.mgrid[0:H, 0:W]
        d = (g(c.viewport_upper_left) - g(c.center))[None, None, :] + \
            (xx[..., None] + 0.5) * g(c.pixel_delta_u) + (yy[..., None] + 0.5) * g(c.pixel_delta_v)
        a = (d * d).sum(-1)
        return float(a.min()), float(a.max())
    edge = 2.0 ** -11 if low else 2.0 ** 20
    lo, hi = a_range(b4_ladder(low)[0])
    assert 2.0 ** -11 < lo and hi < 2.0 ** 20
    spans = [a_range(f) for f in b4_ladder(low)[3:]]
    assert any(lo < edge for lo, _ in spans) and any(hi > edge for _, hi in spans)
    assert any(lo < edge < hi for lo, hi in spans)    # the switch inside one image
    print("low" if low else "high", "switch at focus_distance", b4_switch(low), spans)


def test_b5_counts_are_exact_and_cross_their_power_of_two():
    """Every count up to 2^24 is an f32 integer; 2^24 + 1 is not (it is stored as 2^24, where
    the reference's own count sticks: f32(2^24) + 1 rounds back).  The one-frame call and the
    four-frame call from each count reach across 2^22 (n + 1 < 2^22 ends at n = 2^22 - 2) and
    2^24 within the set."""
    for n in B5_COUNTS:
        assert (float(F32(n)) == n) == (n <= 2 ** 24)
    assert float(F32(2 ** 24 + 1)) == 2.0 ** 24 and F32(2 ** 24) + F32(1) == F32(2 ** 24)
    for edge, guard in ((2 ** 22, 2 ** 22 - 1), (2 ** 24, 2 ** 24)):
        near = [n for n in B5_COUNTS if abs(n - edge) <= 3]
        assert min(near) < guard - 1 and max(near) >= guard       # one-frame calls, both sides
        assert any(n < guard <= n + 4 for n in near)              # a four-frame call crosses
    assert B5_SPP > max(B5_COUNTS) + 8


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("albedo", B6_ALBEDOS)
def test_b6_first_frame_holds_numerators_under_the_bound(rt, oracle, albedo, depth):
    """At least 500 channels of the reset frame (numerator = colour) lie in (0, 2^-102).  One
    case cannot: at depth 1 a sphere's colour is albedo x sky with every sky channel in
    [0.5, 1], so albedo 2^-101 gives numerators in [2^-102, 2^-101] — the binade just inside
    the bound, which is asserted instead (its continuing frames, colour minus accumulator, do
    fall under 2^-102)."""
    cam = make_camera(rt, depth)
    first = oracle_chain(oracle, np.zeros((H, W, 4), np.float32), cam, b6_scene(albedo),
                         rt.frame_seeds(SEED0, 1))[0]
    zeros = int((first[..., :3] == 0).sum())
    print("albedo 2^%d depth %d: %d channels in (0, 2^-102), %d zero"
          % (round(math.log2(albedo)), depth, tiny_channels(first), zeros))
    if depth == 1 and albedo == 2.0 ** -101:
        c = first[..., :3]
        assert tiny_channels(first) == 0
        assert int(((c >= 2.0 ** -102) & (c <= 2.0 ** -101)).sum()) >= 500
        chain = oracle_chain(oracle, np.zeros((H, W, 4), np.float32), cam, b6_scene(albedo),
                             rt.frame_seeds(SEED0, 2))
        num = chain[1][..., :3].astype(np.float64) - chain[0][..., :3]   # (col - c) / 2
        assert int(((num != 0) & (np.abs(num) < 2.0 ** -103)).sum()) >= 500
    else:
        assert tiny_channels(first) >= 500


def test_selftest_roots_header_is_exported_and_bound(rt):
    """include/rt_selftest_roots.h: the library exports what it declares and the ctypes
    binding covers exactly that."""
    import re
    import subprocess
    from conftest import PKG_DIR, ROOT
    text = (ROOT / "include" / "rt_selftest_roots.h").read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_selftest_roots"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG_DIR / "build" / "librt_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    assert set(declared) <= set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(rt._lib.selftest_roots_symbols()) == set(declared)
    assert not set(declared) & set(rt._lib.exported_symbols())
    assert not set(declared) & set(rt._lib.chain_parts_symbols())
    # the struct's mirror and the table's size
    assert [f for f, _ in rt._lib.RootsTallyC._fields_] == ["mismatches", "drawn", "compared",
                                                            "rooted"]
    assert rt._lib.ctypes.sizeof(rt._lib.RootsTallyC) == 32
    sizes = dict(re.findall(r"^#define (RT_ROOTS_\w+) (\d+)u$", text, flags=re.M))
    assert int(sizes["RT_ROOTS_FAMILIES"]) == rt._lib.RT_ROOTS_FAMILIES == \
        len(rt.ComputeShaderPipeline.ROOT_FAMILIES)
    assert int(sizes["RT_ROOTS_STRATA"]) == rt._lib.RT_ROOTS_STRATA == \
        len(rt.ComputeShaderPipeline.ROOT_STRATA)
    assert rt._lib.lib().rt_selftest_roots(None, 0, None) == 6


# ---- GPU ------------------------------------------------------------------------------------
@gpu
def test_root_selection_selftest(rt):
    """rt_selftest_roots on 2^26 cases: per family (consider_fast, consider_any_fast) and
    stratum no mismatch, at least half of the cases drawn really compared, and the sum over the
    strata as rt_selftest_fastmath's out[3] counts it (the same cases).  The far strata (|O| or
    |C| in [2^38, 2^40]) and the edge strata (a within a binade of an end) each hold half of
    the cases, so each is at least a quarter of what was compared.  Of the compared cases at
    least a quarter had a non-negative discriminant: half the spheres are placed with their
    centre within R of the ray (D >= 0 but for rounding) and the grazing half falls on either
    side of D = 0 evenly, three quarters in exact arithmetic; where R is far below an ulp of
    the coordinates the sign of D is rounding noise, even odds."""
    n = 1 << 26
    p = rt.ComputeShaderPipeline(0)
    try:
        tally = p.selftest_roots(n)
        few = p.selftest_fastmath(1 << 16)
    finally:
        p.close()
    for key, t in tally.items():
        print(key, t)
    total = {f: 0 for f in p.ROOT_FAMILIES}
    for (fam, st), t in tally.items():
        assert t["drawn"] == n // 4, (fam, st, t)
        assert t["mismatches"] == 0, (fam, st, t)
        assert 2 * t["compared"] >= t["drawn"], (fam, st, t)
        assert 4 * t["rooted"] >= t["compared"] and t["rooted"] <= t["compared"], (fam, st, t)
        total[fam] += t["compared"]
    for fam in p.ROOT_FAMILIES:
        far = tally[(fam, "far")]["compared"] + tally[(fam, "far_edge")]["compared"]
        edge = tally[(fam, "edge")]["compared"] + tally[(fam, "far_edge")]["compared"]
        assert 4 * far >= total[fam] and 4 * edge >= total[fam]
    assert few[3] == 0 and few[4] == (1 << 32) + (1 << 16)


@gpu
@pytest.mark.parametrize("place", list(B1_PLACES))
def test_b1_scene_bound_depth1(rt, oracle, place):
    sc = np.concatenate([default_scene(rt), far_sphere(b1_center(place), B1_R)])
    check_case(rt, oracle, make_camera(rt, 1, **B1_CAMERA), sc,
               side=depth_side(1, B1_PLACES[place]))


@gpu
@pytest.mark.parametrize("base", list(B2_BASES))
@pytest.mark.parametrize("place", list(B2_PLACES))
def test_b2_scene_bound_depth3(rt, oracle, place, base):
    radius, dist, _ = B2_PLACES[place]
    sc = np.concatenate([B2_BASES[base](rt), far_sphere(on_axis(dist), radius)])
    check_case(rt, oracle, make_camera(rt, 3, **B2_CAMERA), sc, side="bounce")


@gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("which", list(B3_RADII))
def test_b3_radius_ends(rt, oracle, which, depth):
    sc, _ = b3_scene(rt, which)
    check_case(rt, oracle, b3_camera(rt, which, depth), sc,
               side=depth_side(depth, which.endswith("_in")))


@gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("low", [True, False])
def test_b4_camera_ray_length_ends(rt, oracle, low, depth):
    sc = default_scene(rt)
    seen = set()
    for f in b4_ladder(low):
        cam = b4_camera(rt, f, depth)
        inside = camera_rays_bounded(cam, W, H, sc)[0]
        check_case(rt, oracle, cam, sc, side=depth_side(depth, inside))
        seen.add(inside)
    assert seen == {True, False}


@functools.lru_cache(None)
def b5_reference(depth, n):
    """The B5 input for count n and the oracle's chain of eight frames from it, and its one
    frame (computed once for the three pair modes)."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    w, h = B5_SHAPE
    rng = np.random.default_rng(n % 1000 + depth)
    state = np.concatenate([rng.random((h, w, 3), np.float32),
                            np.full((h, w, 1), n, np.float32)], axis=2)
    cam = make_camera(rt, depth, w, h, spp=B5_SPP, moved=False)
    seeds = rt.frame_seeds(SEED0, 9)
    one = oracle_chain(oracle, state, cam, default_scene(rt), seeds[8:])[0]
    chain = oracle_chain(oracle, state, cam, default_scene(rt), seeds[:8])
    for a in [state, one] + chain:
        a.setflags(write=False)
    return state, cam, seeds, one, chain


@gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("pairs", ["off", "on2", "quad"])
def test_b5_count_ends(rt, oracle, pairs, depth):
    """Images of one uniform count n around 2^22 and 2^24: a one-frame update, and a
    four-frame update_frames followed by a second one on its own output, both buffers each.
    (The library hints only counts it recorded itself, and records none for the output of a
    call whose input count it did not know: every call here accumulates by the per-pixel
    IEEE division, with f32(n + 1) on both sides of 2^22 and 2^24.  The Markstein step's own
    bound, kAccRnMax, is reached only by a context that has itself accumulated 2^22 frames —
    2.7 to 7.5 s per case on a 2x1 image, left out of the suite — and rt_selftest_fastmath's
    out[1] checks that step on random k below the bound.)"""
    w, h = B5_SHAPE
    sc = rt.SphereCollection(default_scene(rt))
    p = rt.ComputeShaderPipeline(0)
    p.set_frame_pairs(pairs)
    try:
        for n in B5_COUNTS:
            state, cam, seeds, one, chain = b5_reference(depth, n)
            got, _, _ = run_frames(rt, p, cam, sc, seeds[8:], w, h, state)
            assert_same(got, one)
            a, b = to_dev(np.array(state)), p.new_image(w, h)
            for call in (0, 1):
                newest = p.update_frames(a, b, w, h, cam, sc, seeds[4 * call:4 * call + 4], 0, 1)
                if newest == 1:
                    a, b = b, a
                assert_same(host(a), chain[4 * call + 3])
                assert_same(host(b), chain[4 * call + 2])
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("albedo", B6_ALBEDOS)
def test_b6_numerator_end(rt, oracle, albedo, depth):
    """A reset frame (the one-frame kernel at depth 1, the bounce instance above), then a
    continuing call of three frames from the count the library recorded (frame groups at
    depth 1)."""
    sc = rt.SphereCollection(b6_scene(albedo))
    cam = make_camera(rt, depth)
    seeds = rt.frame_seeds(SEED0, 4)
    want = oracle_chain(oracle, np.zeros((H, W, 4), np.float32), cam, sc.spheres, seeds)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, b = p.new_image(W, H), p.new_image(W, H)
        p.update(a, b, W, H, cam.with_fields(random_seed=float(seeds[0])), sc)
        first = p.last_launch_info()["kernel_name"]
        assert_same(host(b), want[0])
        still = cam.with_fields(camera_has_moved=0.0)
        newest = p.update_frames(b, a, W, H, still, sc, seeds[1:], 0, 1)
        later = p.last_launch_info()
        assert newest == 1 and later["frames"] == 3
        assert_same(host(a), want[3])
        assert_same(host(b), want[2])
    finally:
        p.close()
    if depth == 1:
        assert first.startswith("rt_single_kernel") and later["launches"] == 1
        assert later["kernel_name"] not in (CULLED, "rt_trace_kernel<0>", first)
    else:
        assert first.startswith("rt_bounce_kernel")
        assert later["kernel_name"].startswith("rt_bounce_kernel")
