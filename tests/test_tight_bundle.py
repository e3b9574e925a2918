"""The list build's ray bundle (rt_set_tight_bundle, rt_tile_lists): the two-slope
beam between the lens disk and a tile's footprint on the focus plane, with the lens radius the
largest singular value of (defocus_disk_u, defocus_disk_v).

Every case renders a 64 x 48 (8 x 6 tiles) or 24 x 16 image of at most eight spheres as a chain
of three frames through rt_tpair_kernel<2>, with the beam and with the single cone it replaces,
culling on and off: all of it equals the oracle bit for bit (NaN == NaN).  The lists themselves
are then read back (rt_tile_lists) and checked against reference rays traced on the CPU in
float64 from the camera blob: through the 9 x 9 pixel-corner grid of each tile (the jitter's
extremes) from 16 points on the lens rim (the centre alone without a lens).  These rays are a
subset of the rays the tile can trace, so a sphere one of them hits and the list lacks is a
hole in the list.

  superset   culling off: every sphere a reference ray hits with a root above 0.001 is listed;
             culling on: every reference ray's first hit is listed;
             a tile flagged certain: every reference ray's first hit is the list's one sphere,
             at its near root (the front face), and its radius is positive.
  tightness  on the cases with a sphere nearer than the focus plane the lists hold fewer entries
             than the single cone's rule gives — replayed here in Python from its formulas, and
             as the device builds them with the beam switched off — and no fewer certain tiles.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_chain_pair_edges import KERNELS
from test_gpu_parity import assert_same, host
from test_occlusion_cull import GLASS, LAMB, METAL, make_camera, sphere

gpu = pytest.mark.gpu

FRAMES = 3
LOOK_FROM = np.array([13.0, 2.0, 3.0])
FORWARD = -LOOK_FROM / np.linalg.norm(LOOK_FROM)        # look_at is the origin
RIGHT = np.cross(FORWARD, [0.0, 1.0, 0.0])
RIGHT /= np.linalg.norm(RIGHT)
UP = np.cross(RIGHT, FORWARD)
FOCUS = 10.0
LENSES = {"pinhole": {"defocus_angle": 0.0}, "lens": {"defocus_angle": 0.6},
          "wide": {"defocus_angle": 8.0, "field_of_view": 5.0}}
NONE = 0xFFFFFFFF


def at_depth(z, side=0.0, up=0.0, origin=LOOK_FROM):
    """The point z along the view axis from the camera, `side` to the right and `up` above it."""
    return tuple(origin + z * FORWARD + side * RIGHT + up * UP)


def backdrop():
    """A sphere that fills every view used here from depth 60 on, and the ground behind it."""
    return [sphere((0, -1030, 0), 1000, LAMB, (0.5, 0.5, 0.5)),
            sphere(at_depth(100.0), 40.0, METAL)]


def depth_scene(frac, fov, side=None):
    """One sphere at frac x the focus distance, an eighth of the view's height in radius, a
    little off the axis (or `side` off it), before the backdrop."""
    z = frac * FOCUS
    r = z * np.tan(np.radians(fov) / 8.0)
    return backdrop() + [sphere(at_depth(z, 0.3 * r if side is None else side, -0.2 * r), r,
                                GLASS)]


# name: (width, height, camera settings, blob fields written after from_settings, spheres,
#        near: a sphere lies between the lens and the focus plane where the beam is narrower
#        than the cone by more than the sphere's margin, so the lists must get shorter)
CASES = {}
for _l, _lens in LENSES.items():
    _fov = _lens.get("field_of_view", 20.0)
    for _n, _f in (("half", 0.5), ("fifth", 0.2), ("on", 1.0), ("twice", 2.0), ("five", 5.0)):
        # (under the wide lens a sphere before the focus plane is blurred over the whole 5
        # degree view by either bundle: it stands 0.6 to the side, where the beam of the
        # tiles on the other side does not reach it and their cone does)
        _side = 0.6 if _l == "wide" and _f < 1.0 else None
        CASES[f"depth_{_n}_{_l}"] = (64, 48, _lens, {}, depth_scene(_f, _fov, _side), _f < 1.0)
CASES.update({
    # a sphere through the focus plane, from 0.8 to 1.1 of the focus distance
    "straddles_focus": (64, 48, {}, {}, backdrop() + [sphere(at_depth(9.5, 0.4), 1.5)], True),
    "straddles_focus_wide": (64, 48, LENSES["wide"], {},
                             backdrop() + [sphere(at_depth(9.8, 0.1), 0.4)], True),
    # a sphere that touches the plane of the lens from the front, beside the lens disk, and one
    # wholly behind the camera
    "lens_plane": (64, 48, {}, {}, backdrop() + [sphere(at_depth(0.3, 0.25), 0.3, GLASS),
                                                 sphere(at_depth(-1.0), 0.8, METAL)], False),
    # ... one about a centre behind the camera that holds the lens: every ray starts inside it
    "around_camera": (24, 16, {}, {}, backdrop() + [sphere(at_depth(-0.2), 0.5)], False),
    # the silhouette of a sphere centred on the ray through the pixel corner (32, 24), on the
    # focus plane, runs through the tile corner (40, 24) (its radius is filled in below)
    "tile_corner": (64, 48, LENSES["pinhole"], {}, None, False),
    "tile_corner_lens": (64, 48, {}, {}, None, False),
    # defocus_disk_u / _v neither orthogonal nor of one length nor across the axis (filled in
    # below from the camera's own vectors)
    "skew_lens": (64, 48, {"defocus_angle": 3.0}, "skew", depth_scene(0.5, 20.0), True),
    "skew_lens_small": (24, 16, {"defocus_angle": 3.0}, "skew", depth_scene(2.0, 20.0), False),
    # the camera 0.59 above a ground of radius 1000: inside sqrt(R^2 + m^2) of its centre
    "camera_in_ground_margin": (64, 48, {"look_from": (13.0, 0.5, 3.0)}, {},
                                [sphere((0, -1000, 0), 1000, LAMB, (0.5, 0.5, 0.5)),
                                 sphere(at_depth(5.0, 0.0, 0.3, np.array([13.0, 0.5, 3.0])),
                                        0.4, METAL)], True),
    # a negative radius before the focus plane
    "negative_radius": (64, 48, {}, {}, backdrop() + [sphere(at_depth(5.0, 0.2), -0.6, GLASS)],
                        True),
    "negative_radius_small": (24, 16, {}, {},
                              backdrop() + [sphere(at_depth(5.0, 0.2), -0.3, GLASS)], True),
})


def camera_of(rt, name):
    w, h, settings, fields, _, _ = CASES[name]
    cam = make_camera(rt, w, h, settings)
    if fields == "skew":
        u, v = np.array(cam.defocus_disk_u, np.float64), np.array(cam.defocus_disk_v, np.float64)
        axis = np.cross(u, v)
        axis *= np.linalg.norm(u) / np.linalg.norm(axis)
        cam = cam.with_fields(
            defocus_disk_u=tuple(float(c) for c in 1.5 * u + 0.5 * v + 0.3 * axis),
            defocus_disk_v=tuple(float(c) for c in 0.3 * u + 0.4 * v - 0.2 * axis))
    return cam


def spheres_of(rt, name):
    rows = CASES[name][4]
    if rows is None:                                   # tile_corner: from the camera's vectors
        cam = camera_of(rt, name)
        vul, pdu = np.array(cam.viewport_upper_left), np.array(cam.pixel_delta_u)
        pdv = np.array(cam.pixel_delta_v)
        c = vul + 32.0 * pdu + 24.0 * pdv
        rows = backdrop() + [sphere(tuple(c), float(np.linalg.norm(8.0 * pdu)))]
    assert len(rows) <= 8
    return np.array(rows, np.float32).reshape(-1, 8)


# ---- reference rays ------------------------------------------------------------------------

def tile_rays(cam, tx, ty):
    """(origins (L, 1, 3), directions (L, 81, 3)) of the tile's reference rays, float64."""
    f = lambda v: np.array(v, np.float64)
    sx, sy = np.meshgrid(8.0 * tx + np.arange(9.0), 8.0 * ty + np.arange(9.0))
    pc = (f(cam.viewport_upper_left) + sx.reshape(-1, 1) * f(cam.pixel_delta_u) +
          sy.reshape(-1, 1) * f(cam.pixel_delta_v))
    o = f(cam.center)[None, :]
    if cam.defocus_angle > 0.0:
        a = 2.0 * np.pi * np.arange(16) / 16.0
        o = o + np.cos(a)[:, None] * f(cam.defocus_disk_u) + np.sin(a)[:, None] * f(cam.defocus_disk_v)
    o = o[:, None, :]
    return o, pc[None, :, :] - o


def roots(sph, o, d):
    """Per sphere and ray the accepted root (inf: none) and whether it is the near root."""
    acc, near = [], []
    a = (d * d).sum(-1)
    for row in sph.astype(np.float64):
        oc = row[:3] - o
        h = (d * oc).sum(-1)
        disc = h * h - a * ((oc * oc).sum(-1) - row[3] * row[3])
        q = np.sqrt(np.maximum(disc, 0.0))
        r1, r2 = (h - q) / a, (h + q) / a
        ok1, ok2 = (disc >= 0.0) & (r1 > 0.001), (disc >= 0.0) & (r2 > 0.001)
        acc.append(np.where(ok1, r1, np.where(ok2, r2, np.inf)))
        near.append(ok1)
    return np.array(acc), np.array(near)


def listed(lists, t, sph):
    """Which spheres' scan records (centre, radius squared in f32) tile t's list holds."""
    recs = lists["records"][t, :lists["count"][t]]
    want = np.concatenate([sph[:, :3], (sph[:, 3] * sph[:, 3])[:, None]], axis=1)
    return np.array([(recs.view(np.uint32) == w.view(np.uint32)).all(axis=1).any() for w in want])


# ---- the single cone's rule, replayed (footprint_beam's `parent` form and beam_misses) -------

def parent_entries(cam, sph, w, h):
    """Entries over the image by the single cone's rule, in f32 as the kernel evaluates it."""
    f = np.float32
    v = lambda a: np.array(a, f)
    vul, pdu, pdv, ctr = (v(cam.viewport_upper_left), v(cam.pixel_delta_u), v(cam.pixel_delta_v),
                          v(cam.center))
    ln = lambda a: np.sqrt((a * a).sum(dtype=f), dtype=f)
    rl0 = f(0)
    if cam.defocus_angle > 0.0:
        du, dv = v(cam.defocus_disk_u), v(cam.defocus_disk_v)
        rl0 = np.sqrt((du * du).sum(dtype=f) + (dv * dv).sum(dtype=f), dtype=f)
    total = 0
    for ty in range((h + 7) // 8):
        for tx in range((w + 7) // 8):
            x0, x1, y0, y1 = f(8 * tx), f(8 * tx + 8), f(8 * ty), f(8 * ty + 8)
            pc = vul + f(0.5) * (x0 + x1) * pdu + f(0.5) * (y0 + y1) * pdv
            rq = max(ln(vul + x * pdu + y * pdv - pc) for x in (x0, x1) for y in (y0, y1))
            mag = np.abs(pc).sum(dtype=f) + np.abs(ctr).sum(dtype=f)
            rq = rq * f(1.001) + f(1e-5) * mag
            rl = rl0 * f(1.001) + f(1e-5) * mag
            L, delta = ln(pc - ctr), rq + rl
            assert L > f(4) * delta
            axis = (pc - ctr) / L
            sin_t = delta / (L - delta) * f(1.01)
            cos_t = np.sqrt(f(1) - sin_t * sin_t, dtype=f) * f(0.999)
            d_max = (L + delta) * f(1.001)
            for row in sph:
                g = row[:3] - pc
                t = (g * axis).sum(dtype=f)
                p = np.sqrt(max((g * g).sum(dtype=f) - t * t, f(0)), dtype=f)
                at, R = abs(t), abs(row[3]) * f(1.0001)
                mag2 = at + p + rq
                lhs = p * cos_t - at * sin_t - rq - f(1e-5) * mag2
                m = f(2.5e-3) * (mag2 + d_max + R)
                total += not (lhs > R and lhs * lhs > (R * R + m * m) * f(1.0001))
    return total


# ---- the device -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipe(rt):
    p = rt.ComputeShaderPipeline(0)
    p.set_frame_images("every")
    yield p
    p.close()


def build(rt, pipe, oracle_images, w, h, cam, sph, tight, cull):
    """Renders the chain with the given bundle and culling, compares the last two frames with
    the oracle's, and returns (the lists, the certain-tile statistics)."""
    scene = rt.SphereCollection(sph)
    pipe.set_tight_bundle(tight)
    pipe.set_occlusion_cull(cull)
    pipe.set_frame_pairs("on2")
    try:
        a, b = pipe.new_image(w, h), pipe.new_image(w, h)
        if pipe.update_frames(a, b, w, h, cam, scene, rt.frame_seeds(33, FRAMES)) == 1:
            a, b = b, a
        info, lists, stats = pipe.last_launch_info(), pipe.tile_lists(), pipe.certain_tiles_stats()
    finally:
        pipe.set_frame_pairs("auto")
        pipe.set_occlusion_cull(True)
        pipe.set_tight_bundle(True)
    assert info["kernel_name"] == KERNELS["on2"], info
    assert_same(host(a), oracle_images[0])
    assert_same(host(b), oracle_images[1])
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert len(lists["count"]) == tiles and lists["records"].shape == (tiles, 19, 4)
    assert not (lists["count"] == NONE).any(), "every tile of these cases has a list"
    assert (lists["count"] <= 19).all()
    assert int((lists["flags"] & 1).sum()) == stats["certain_tiles"]
    return lists, stats


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_lists_hold_every_hit_and_are_tighter(rt, oracle, pipe, name):
    w, h, _, _, _, near_case = CASES[name]
    cam, sph = camera_of(rt, name), spheres_of(rt, name)
    zero = np.zeros((h, w, 4), np.float32)
    seeds = rt.frame_seeds(33, FRAMES)
    want = (oracle.render(zero, cam.blob, sph, seeds)[0],
            oracle.render(zero, cam.blob, sph, seeds[:FRAMES - 1])[0])
    got = {(tight, cull): build(rt, pipe, want, w, h, cam, sph, tight, cull)
           for tight in (True, False) for cull in (False, True)}
    tiles_x = (w + 7) // 8
    for tight in (True, False):
        plain, culled = got[tight, False][0], got[tight, True][0]
        assert (plain["removed"] == 0).all() and (plain["flags"] == 0).all()
        assert (culled["count"] + culled["removed"] == plain["count"]).all()
        for t in range(len(plain["count"])):
            o, d = tile_rays(cam, t % tiles_x, t // tiles_x)
            root, near = roots(sph, o, d)
            hit = np.isfinite(root)
            in_plain, in_culled = listed(plain, t, sph), listed(culled, t, sph)
            # culling off: every sphere a reference ray hits
            missing = hit.any(axis=(1, 2)) & ~in_plain
            assert not missing.any(), (name, tight, t, np.flatnonzero(missing))
            # culling on: every reference ray's first hit
            first = root.argmin(axis=0)
            firsts = np.unique(first[hit.any(axis=0)])
            assert in_culled[firsts].all(), (name, tight, t, firsts, in_culled)
            if culled["flags"][t] & 1:
                assert culled["count"][t] == 1 and hit.any(axis=0).all(), (name, tight, t)
                assert len(firsts) == 1 and in_culled[firsts[0]], (name, tight, t, firsts)
                j = int(firsts[0])
                assert near[j].all() and sph[j, 3] > 0.0, (name, tight, t, j)
    beam, cone = got[True, False][0], got[False, False][0]
    n_beam, n_cone = int(beam["count"].sum()), int(cone["count"].sum())
    n_replay = parent_entries(cam, sph, w, h)
    c_beam, c_cone = got[True, True][1]["certain_tiles"], got[False, True][1]["certain_tiles"]
    print(f"{name}: entries beam {n_beam}, cone {n_cone}, cone replayed {n_replay}; "
          f"culled beam {int(got[True, True][0]['count'].sum())}, "
          f"cone {int(got[False, True][0]['count'].sum())}; certain beam {c_beam}, cone {c_cone}")
    # the beam lies inside the cone: never more entries, never fewer certain tiles
    assert (beam["count"] <= cone["count"]).all()
    assert n_cone <= n_replay                # (the device also applies the block's cone)
    assert c_beam >= c_cone
    if near_case:
        assert n_beam < n_cone and n_beam < n_replay, (n_beam, n_cone, n_replay)


@gpu
def test_setting_rebuilds_the_lists(rt, oracle, pipe):
    """rt_set_tight_bundle is part of the lists' key: the next call with the same camera and
    scene rebuilds them."""
    name = "depth_half_lens"
    w, h = CASES[name][:2]
    cam, sph = camera_of(rt, name), spheres_of(rt, name)
    zero = np.zeros((h, w, 4), np.float32)
    seeds = rt.frame_seeds(33, FRAMES)
    want = (oracle.render(zero, cam.blob, sph, seeds)[0],
            oracle.render(zero, cam.blob, sph, seeds[:FRAMES - 1])[0])
    seen = [int(build(rt, pipe, want, w, h, cam, sph, tight, True)[0]["count"].sum())
            for tight in (True, False, True)]
    assert seen[0] == seen[2] < seen[1], seen


@gpu
def test_no_lists_before_a_trace_and_in_exhaustive_mode(rt, oracle):
    p = rt.ComputeShaderPipeline(0)
    try:
        assert len(p.tile_lists()["count"]) == 0
        name = "depth_on_lens"
        w, h = CASES[name][:2]
        cam, sph = camera_of(rt, name), spheres_of(rt, name)
        a, b = p.new_image(w, h), p.new_image(w, h)
        p.update(a, b, w, h, cam, rt.SphereCollection(sph))
        assert len(p.tile_lists()["count"]) == 48
        p.set_scan_mode("exhaustive")
        assert len(p.tile_lists()["count"]) == 0
        # a capacity below the number of tiles: that many are written, the number is reported
        p.set_scan_mode("culled")
        buf = (rt._lib.TileListC * 2)()
        n = ctypes.c_uint64(0)
        rt._lib.call("rt_tile_lists", p._ctx, buf, 2, ctypes.byref(n))
        assert n.value == 48 and buf[0].count <= 19 and buf[0].reserved == 0
    finally:
        p.close()


def test_cases_are_well_formed(rt):
    """Without a GPU: every case has a finite camera and one to eight spheres, and the skewed
    lens vectors are neither orthogonal nor of one length."""
    for name in CASES:
        sph = spheres_of(rt, name)
        assert sph.shape[1] == 8 and 1 <= len(sph) <= 8, name
        cam = camera_of(rt, name)
        assert np.isfinite(cam.blob).all(), name
    u = np.array(camera_of(rt, "skew_lens").defocus_disk_u)
    v = np.array(camera_of(rt, "skew_lens").defocus_disk_v)
    assert abs(u @ v) > 0.1 * np.linalg.norm(u) * np.linalg.norm(v)
    assert np.linalg.norm(u) > 2.0 * np.linalg.norm(v)


def test_tile_lists_header_is_exported_and_bound(rt):
    """include/rt_tile_lists.h: the library exports what it declares, the ctypes binding binds
    it, and ABI 7's own list does not change."""
    text = (ROOT / "include" / "rt_tile_lists.h").read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_tile_lists", "rt_set_tight_bundle"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG_DIR / "build" / "librt_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(declared) <= exported
    assert rt._lib.tile_lists_symbols() == declared
    assert not set(declared) & set(rt._lib.exported_symbols())
    abi = (ROOT / "include" / "rt_abi.h").read_text()
    assert "rt_tile_lists" not in abi and "rt_set_tight_bundle" not in abi
    assert rt._lib.lib().rt_abi_version() == 7
    assert ctypes.sizeof(rt._lib.TileListC) == 320


def test_null_context_and_bad_value(rt):
    L = rt._lib.lib()
    assert L.rt_set_tight_bundle(None, 1) == 6
    assert L.rt_tile_lists(None, None, 0, None) == 6
