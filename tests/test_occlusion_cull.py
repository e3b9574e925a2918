"""Occlusion culling of the per-tile candidate lists (rt_set_occlusion_cull): a
sphere that another sphere of the same list hides from every camera ray of the tile is dropped
at list build.  Every case renders a small image with at most eight spheres as a chain of four
frames (every frame's image written: the last two are compared) and as a one-frame update,
with culling on and off.  All of it equals the oracle bit for bit (NaN == NaN), and a case
built to cull asserts through the statistics that the lists got shorter, a case built not to
cull that they did not."""
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_gpu_parity import assert_same, host

gpu = pytest.mark.gpu

FRAMES = 4
LOOK_FROM = np.array([13.0, 2.0, 3.0])
TO_CAMERA = LOOK_FROM / np.linalg.norm(LOOK_FROM)   # from the origin towards the camera
LAMB, METAL, GLASS = -2.0, 0.0, 2.0


def sphere(center, radius, mat=LAMB, color=(0.6, 0.5, 0.4)):
    c = (1.5, 0.0, 0.0) if mat > 1.0 else color        # a dielectric's first channel is its ir
    return [*center, radius, *c, mat]


def behind(dist, side=0.0, up=0.0):
    """A point `dist` behind the origin as the default camera sees it."""
    right = np.cross([0.0, 1.0, 0.0], TO_CAMERA)
    right /= np.linalg.norm(right)
    return tuple(-dist * TO_CAMERA + side * right + np.array([0.0, up, 0.0]))


def filled_view(mat=LAMB, radius=6.0):
    """One sphere fills the view; two small spheres and the ground lie behind it."""
    return [sphere((0, -1007, 0), 1000, LAMB, (0.5, 0.5, 0.5)),
            sphere(behind(9.0, 1.0, 0.5), 0.5, METAL),
            sphere((0, 0, 0), radius, mat),
            sphere(behind(8.0, -1.5, -0.5), 0.4, GLASS)]


# name: (width, height, camera settings, spheres, what the statistics must show)
#   "cull": culling on removes entries; "keep": it removes none although some list holds two
#   entries or more; "off": it removes none because it switched itself off
CASES = {
    "filled_view": (32, 16, {}, filled_view(), "cull"),
    "filled_view_depth4": (32, 16, {"max_depth": 4}, filled_view(), "cull"),
    "glass_occluder": (32, 16, {}, filled_view(GLASS), "cull"),
    "metal_occluder": (32, 16, {}, filled_view(METAL), "cull"),
    "negative_radius": (32, 16, {}, filled_view(LAMB, -6.0)[:3] +
                        [sphere(behind(8.0, -1.5, -0.5), -0.4, GLASS)], "cull"),
    "no_lens": (32, 16, {"defocus_angle": 0.0}, filled_view(), "cull"),
    "wide_lens": (32, 16, {"defocus_angle": 8.0}, filled_view(), "cull"),
    # the silhouette of the only large sphere crosses every tile it touches
    "silhouette_crosses": (32, 16, {}, [sphere((0, -1001, 0), 1000),
                                        sphere((0, 0, 0), 1.0),
                                        sphere(behind(3.0), 0.5, METAL)], "keep"),
    # ... and here it covers the middle tiles and crosses the ones around them
    "silhouette_mixed": (64, 32, {}, [sphere((0, -1004, 0), 1000),
                                      sphere((0, 0, 0), 2.5),
                                      sphere(behind(4.0), 0.5, METAL),
                                      sphere(behind(4.0, 3.5), 0.5, GLASS)], "cull"),
    # ties: the same sphere at two indices with another between them, and concentric ones
    "identical_twins": (32, 16, {}, [sphere((0, 0, 0), 6.0, LAMB, (0.9, 0.1, 0.1)),
                                     sphere(behind(9.0, 1.0), 0.5, METAL),
                                     sphere((0, 0, 0), 6.0, LAMB, (0.1, 0.1, 0.9))], "cull"),
    "twins_alone": (32, 16, {}, [sphere((0, 0, 0), 6.0, LAMB, (0.9, 0.1, 0.1)),
                                 sphere((0, 0, 0), 6.0, GLASS)], "keep"),
    "concentric": (32, 16, {}, [sphere((0, 0, 0), 5.0, METAL),
                                sphere((0, 0, 0), 6.0, GLASS),
                                sphere((0, 0, 0), 5.5, LAMB)], "cull"),
    # a small sphere sunk halfway into the occluder's near side, one that overlaps it in depth
    "intersecting": (32, 16, {}, [sphere((0, 0, 0), 6.0),
                                  sphere(tuple(6.0 * TO_CAMERA), 0.5, METAL),
                                  sphere(tuple(5.0 * TO_CAMERA + np.array([0.0, 3.4, 0.0])), 0.5,
                                         GLASS)], "keep"),
    # the camera inside a sphere that holds the whole scene
    "camera_inside": (64, 32, {}, [sphere((0, 0, 0), 20.0, LAMB, (0.7, 0.8, 0.9)),
                                   sphere((0, 0, 0), 3.0, METAL),
                                   sphere(behind(5.0), 0.5)], "cull"),
    # a sphere whose surface is 0.01 from the pinhole: its root is about 0.001
    "root_at_0001": (32, 16, {"defocus_angle": 0.0},
                     [sphere(tuple(LOOK_FROM - 0.06 * TO_CAMERA), 0.05, GLASS),
                      sphere((0, 0, 0), 1.0),
                      sphere(behind(3.0), 0.5, METAL)], "keep"),
    # ... and with the lens, whose disk reaches into that sphere
    "lens_in_sphere": (32, 16, {}, [sphere(tuple(LOOK_FROM - 0.06 * TO_CAMERA), 0.05, GLASS),
                                    sphere((0, 0, 0), 1.0),
                                    sphere(behind(3.0), 0.5, METAL)], "keep"),
    # a level camera: the horizon runs through the middle rows, the ground grazes behind the
    # sphere in the rows just below it
    "grazing_ground": (64, 32, {"look_at": (0.0, 2.0, 0.0)},
                       [sphere((0, -1000, 0), 1000, LAMB, (0.5, 0.5, 0.5)),
                        sphere((0, 2.5, 0), 2.5, METAL),
                        sphere(behind(5.0, 0.0, 2.5), 0.5)], "cull"),
    # one coordinate outside the bounded domain of the root test (2^40)
    "unbounded_scene": (32, 16, {}, filled_view() + [sphere((0, 3e12, 0), 1.0)], "off"),
}


def random_scene(k):
    """Up to eight spheres about the view axis of a 16 x 16 image: large ones that cover
    tiles, small ones before and behind them, sometimes the ground."""
    rng = np.random.default_rng(1000 + k)
    rows = []
    if rng.random() < 0.5:
        rows.append(sphere((0, -1000 - rng.uniform(1, 8), 0), 1000))
    for _ in range(int(rng.integers(2, 8 - len(rows) + 1))):
        big = rng.random() < 0.4
        r = rng.uniform(1.5, 6.0) if big else rng.uniform(0.1, 0.8)
        if rng.random() < 0.15:
            r = -r
        along = rng.uniform(-10.0, 9.0)                      # towards the camera is negative
        c = behind(along, rng.normal(0, 1.0), rng.normal(0, 1.0))
        rows.append(sphere(c, r, (LAMB, METAL, 0.4, GLASS)[int(rng.integers(4))],
                           tuple(rng.uniform(0.1, 0.9, 3))))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


RANDOM_SCENES = 24


def make_camera(rt, w, h, settings):
    kw = dict(max_depth=1, samples_per_pixel=500, camera_has_moved=True)
    kw.update(settings)
    return rt.SceneCamera.from_settings(rt.CameraSettings(**kw), w, h, 0.5)


@pytest.fixture(scope="module")
def pipe(rt):
    p = rt.ComputeShaderPipeline(0)
    p.set_frame_images("every")
    yield p
    p.close()


def render(rt, pipe, on, w, h, cam, rows):
    """(frame 4, frame 3, the one-frame update, the lists' statistics) with culling on / off."""
    scene = rt.SphereCollection(np.array(rows, np.float32).reshape(-1, 8))
    pipe.set_occlusion_cull(on)
    a, b = pipe.new_image(w, h), pipe.new_image(w, h)
    newest = pipe.update_frames(a, b, w, h, cam, scene, rt.frame_seeds(33, FRAMES))
    if newest == 1:
        a, b = b, a
    stats = pipe.candidate_stats()
    one_in, one_out = pipe.new_image(w, h), pipe.new_image(w, h)
    pipe.update(one_in, one_out, w, h, cam, scene)
    assert pipe.candidate_stats() == stats            # the same lists serve both
    return host(a).copy(), host(b).copy(), host(one_out).copy(), stats


def check(rt, oracle, pipe, w, h, settings, rows):
    """Both settings against the oracle and each other; returns (stats on, stats off)."""
    cam = make_camera(rt, w, h, settings)
    sph = np.array(rows, np.float32).reshape(-1, 8)
    zero = np.zeros((h, w, 4), np.float32)
    want4, _ = oracle.render(zero, cam.blob, sph, rt.frame_seeds(33, FRAMES))
    want3, _ = oracle.render(zero, cam.blob, sph, rt.frame_seeds(33, FRAMES)[:FRAMES - 1])
    want1, _ = oracle.update(zero, cam.blob, sph)
    got = {on: render(rt, pipe, on, w, h, cam, rows) for on in (True, False)}
    for on in (True, False):
        assert_same(got[on][0], want4)
        assert_same(got[on][1], want3)
        assert_same(got[on][2], want1)
    for k in range(3):
        assert_same(got[True][k], got[False][k])
    return got[True][3], got[False][3]


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_culled_lists_render_the_same_bits(rt, oracle, pipe, name):
    w, h, settings, rows, expect = CASES[name]
    assert len(rows) <= 8
    on, off = check(rt, oracle, pipe, w, h, settings, rows)
    assert off["occlusion_removed"] == 0 and off["occlusion_tiles"] == 0
    assert on["tiles"] == off["tiles"] == ((w + 7) // 8) * ((h + 7) // 8)
    assert on["tiles_without_list"] == off["tiles_without_list"] == 0
    assert off["max_entries"] >= 2, off                # some list could have lost an entry
    assert on["entries"] + on["occlusion_removed"] == off["entries"]
    if expect == "cull":
        assert on["occlusion_removed"] > 0 and on["occlusion_tiles"] > 0, on
        assert on["entries"] < off["entries"] and on["mean_entries"] < off["mean_entries"]
    else:
        assert on["occlusion_removed"] == 0, on
        assert on == off


def test_unbounded_scene_culls_once_it_is_bounded():
    """The "off" case's scene without its far sphere is the "cull" case: what switched the
    rule off there was the domain, not the geometry."""
    w, h, settings, rows, expect = CASES["unbounded_scene"]
    assert expect == "off" and rows[:-1] == CASES["filled_view"][3]


@gpu
def test_random_small_scenes(rt, oracle, pipe):
    removed = culled_scenes = 0
    for k in range(RANDOM_SCENES):
        rows = random_scene(k)
        assert 2 <= len(rows) <= 8
        settings = {"defocus_angle": (0.6, 0.0, 3.0)[k % 3], "max_depth": 1 if k % 4 else 3}
        on, off = check(rt, oracle, pipe, 16, 16, settings, rows)
        assert off["occlusion_removed"] == 0
        assert on["entries"] + on["occlusion_removed"] == off["entries"], (k, on, off)
        removed += on["occlusion_removed"]
        culled_scenes += on["occlusion_removed"] > 0
    # the batch exercises the rule: several scenes lose entries, several lose none
    assert removed > 0 and 3 <= culled_scenes <= RANDOM_SCENES - 3, (removed, culled_scenes)


@gpu
def test_setting_rebuilds_the_lists(rt, pipe):
    """rt_set_occlusion_cull is part of the lists' key: the next call with the same camera and
    scene rebuilds them."""
    w, h, settings, rows, _ = CASES["filled_view"]
    cam = make_camera(rt, w, h, settings)
    seen = []
    for on in (True, False, True):
        seen.append(render(rt, pipe, on, w, h, cam, rows)[3])
    assert seen[0] == seen[2] and seen[0]["entries"] < seen[1]["entries"]


def test_occlusion_header_is_exported_and_bound(rt):
    """include/rt_occlusion_cull.h: the library exports what it declares, the ctypes binding
    binds it, and ABI 7's own list does not change."""
    text = (ROOT / "include" / "rt_occlusion_cull.h").read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_set_occlusion_cull", "rt_occlusion_cull_stats"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG_DIR / "build" / "librt_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(declared) <= exported
    assert rt._lib.occlusion_symbols() == declared
    assert not set(declared) & set(rt._lib.exported_symbols())
    assert "rt_occlusion" not in (ROOT / "include" / "rt_abi.h").read_text()
    assert rt._lib.lib().rt_abi_version() == 7


def test_null_context_and_bad_value(rt):
    L = rt._lib.lib()
    assert L.rt_set_occlusion_cull(None, 1) == 6
    assert L.rt_occlusion_cull_stats(None, None) == 6
