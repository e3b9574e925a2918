"""Certain tiles (rt_set_certain_tiles): a tile whose culled candidate list is
one sphere that every camera ray of the tile certainly hits — from outside, on the front face,
near root accepted — is flagged at list build, and the tile-pair frame loops (rt_tpair_kernel<2>
/ <4>) trace a pair of two such tiles with a straight-line sample.  Every case renders a small
image with at most eight spheres as a chain of four frames (every frame's image written: the
last two are compared) in both frame-group modes test_chain_pair_edges forces, and as a
one-frame update, with the path on and off.  All of it equals the oracle bit for bit
(NaN == NaN), and every case asserts through rt_certain_tiles_stats what it was built for:
certain tiles (and, where the geometry gives them, certain pairs) above 0, or exactly 0.

Two of the geometries one might ask for cannot exist.  Two horizontally adjacent tiles share
the rays through their common pixel edge, and a certain tile needs every one of its rays to hit
its sphere first by a margin.  So the two tiles of one pair are never certain for two
different spheres, and a certain tile never has an empty neighbour: between two certain regions
of different spheres, or a certain region and the empty sky, lies at least one general tile.
`two_spheres` therefore covers whole pairs by two different spheres (of different classes) in
one image, and `silhouette` has certain tiles beside general ones and general ones beside
empty ones; a certain tile whose partner holds no list entry is the three-tile-wide image,
whose last tile's partner lies outside."""
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_chain_pair_edges import KERNELS
from test_gpu_parity import assert_same, host, to_dev
from test_occlusion_cull import (CASES as CULL_CASES, GLASS, LAMB, METAL, behind, filled_view,
                                 make_camera, random_scene, sphere)

gpu = pytest.mark.gpu

FRAMES = 4
MODES = ("on2", "quad2")
FUZZY = 0.3                                              # metal with fuzz
MATS = {"lambertian": LAMB, "metal": FUZZY, "glass": GLASS}
# (a tile's cone is degenerate, and the tile without a list, once the lens disk and the tile's
# footprint on the focus plane together exceed a quarter of the focus distance: the wide lens
# takes a narrow field of view, whose tiles are small there)
LENSES = {"lens": {}, "pinhole": {"defocus_angle": 0.0},
          "wide_lens": {"defocus_angle": 8.0, "field_of_view": 5.0}}
GROUND = sphere((0, -1000, 0), 1000, LAMB, (0.5, 0.5, 0.5))


def fill(mat=LAMB, radius=6.0):
    """filled_view with the ground 20 below the origin instead of 7: the ground's near root is
    bounded from below with an error of sqrt(E), about 2 for its radius, and under a wide lens
    the nearer ground is not provably behind the covering sphere.  (At the default 20 degree
    field of view a tile of a 32 x 16 image spans 10 degrees and the bundle bounds are loose:
    the sphere is certain in the tiles of one row, four of eight — enough for two pairs.)"""
    return [sphere((0, -1020, 0), 1000, LAMB, (0.5, 0.5, 0.5))] + filled_view(mat, radius)[1:]


# name: (width, height, camera settings, spheres, what the statistics must show with the path
# on).  "pairs": certain tiles and certain pairs; "tiles": certain tiles; "none": exactly 0.
CASES = {}
for _m, _mat in MATS.items():
    for _l, _lens in LENSES.items():
        CASES[f"fill_{_m}_{_l}"] = (32, 16, _lens, fill(_mat), "pairs")
CASES.update({
    # a narrow view of the ground 8.5 degrees below the horizontal.  (The bundle's bound on a
    # ray's distance from the centre grows with the tile's angle times the distance along the
    # axis: at the default 20 degrees a tile of these small images spans 10, and the bound
    # leaves the ground's 1000 radius.)
    "ground_only": (32, 16, {"field_of_view": 4.0}, [GROUND], "pairs"),
    # a metal sphere over the left pairs, a glass one over the right pairs, general tiles between
    "two_spheres": (64, 32, {}, [sphere(behind(0.0, -5.0), 4.0, FUZZY),
                                 sphere(behind(0.0, 5.0), 4.0, GLASS)], "pairs"),
    # a negative radius flips the normal: the covering sphere is the list's only entry, and
    # the tile stays general
    "negative_radius": (32, 16, {}, CULL_CASES["negative_radius"][3], "none"),
    "camera_inside": (64, 32, {}, [sphere((0, 0, 0), 20.0, LAMB, (0.7, 0.8, 0.9))], "none"),
    # a sphere whose surface is 0.01 from the pinhole: its root is about 0.001 in every tile
    "root_at_0001": (32, 16, {"defocus_angle": 0.0}, CULL_CASES["root_at_0001"][3], "none"),
    # a shell half a thousandth in front of the covering sphere: inside the f32 error of the
    # two roots, so the cull keeps both entries in every tile
    "occluder_kept": (32, 16, {}, [sphere((0, 0, 0), 6.0),
                                   sphere((0, 0, 0), 6.0005, GLASS)], "none"),
    # one coordinate outside the bounded domain of the root test (2^40): the rule is off
    "unbounded_scene": (32, 16, {}, fill() + [sphere((0, 3e12, 0), 1.0)], "none"),
    # the silhouette of the only sphere runs through the image: certain tiles in the middle,
    # general ones around them, empty ones outside
    "silhouette": (64, 32, {}, [sphere((0, 0, 0), 2.5, FUZZY)], "tiles"),
    # three tiles a row: the last tile's partner lies outside the image
    "three_tiles_wide": (24, 16, {}, fill(), "pairs"),
    # partial tiles on both edges
    "partial_tiles": (36, 20, {}, fill(GLASS), "pairs"),
    # the horizon (3.6 degrees down from a camera 2 above the ground) runs through the second
    # tile row of a view from 0.1 to 10.1 degrees down; the bottom row sees the ground alone
    "horizon": (64, 32, {"look_at": (0.0, 0.8, 0.0), "field_of_view": 10.0},
                [GROUND, sphere((0, 0.5, 0), 0.5, METAL)], "tiles"),
})
RANDOM_SCENES = 16


@pytest.fixture(scope="module")
def pipe(rt):
    p = rt.ComputeShaderPipeline(0)
    p.set_frame_images("every")
    yield p
    p.close()


def render(rt, pipe, on, pairs, w, h, cam, rows, scan="culled"):
    """(frame 4, frame 3, the one-frame update, the statistics after the chain, its launch)
    with the path on / off in one frame-group mode."""
    scene = rt.SphereCollection(np.array(rows, np.float32).reshape(-1, 8))
    pipe.set_certain_tiles(on)
    pipe.set_scan_mode(scan)
    pipe.set_frame_pairs(pairs)
    try:
        a, b = pipe.new_image(w, h), pipe.new_image(w, h)
        newest = pipe.update_frames(a, b, w, h, cam, scene, rt.frame_seeds(33, FRAMES))
        if newest == 1:
            a, b = b, a
        stats, info = pipe.certain_tiles_stats(), pipe.last_launch_info()
        one_in, one_out = pipe.new_image(w, h), pipe.new_image(w, h)
        pipe.update(one_in, one_out, w, h, cam, scene)
        assert pipe.certain_tiles_stats()["certain_tiles"] == stats["certain_tiles"]
    finally:
        pipe.set_frame_pairs("auto")
        pipe.set_scan_mode("culled")
        pipe.set_certain_tiles(True)
    return host(a).copy(), host(b).copy(), host(one_out).copy(), stats, info


def check(rt, oracle, pipe, w, h, settings, rows, scan="culled"):
    """Both settings in both modes against the oracle; returns the statistics with the path on
    (one per mode, equal) after checking that off reports none."""
    cam = make_camera(rt, w, h, settings)
    sph = np.array(rows, np.float32).reshape(-1, 8)
    zero = np.zeros((h, w, 4), np.float32)
    want4, _ = oracle.render(zero, cam.blob, sph, rt.frame_seeds(33, FRAMES))
    want3, _ = oracle.render(zero, cam.blob, sph, rt.frame_seeds(33, FRAMES)[:FRAMES - 1])
    want1, _ = oracle.update(zero, cam.blob, sph)
    seen = []
    for pairs in MODES:
        for on in (True, False):
            got4, got3, got1, stats, info = render(rt, pipe, on, pairs, w, h, cam, rows, scan)
            # (outside the bounded domain the library runs no frame-group kernel at all)
            if scan == "culled" and not any(abs(v) > 2.0 ** 40 for row in rows for v in row):
                assert info["kernel_name"] == KERNELS[pairs], info
            assert_same(got4, want4)
            assert_same(got3, want3)
            assert_same(got1, want1)
            if on:
                seen.append(stats)
            else:
                assert stats == {"certain_tiles": 0, "certain_pairs": 0}, stats
    assert seen[0] == seen[1], seen
    return seen[0]


def assert_expected(stats, expect, tiles):
    print(stats, "of", tiles, "tiles")
    if expect == "none":
        assert stats == {"certain_tiles": 0, "certain_pairs": 0}, stats
    else:
        assert 0 < stats["certain_tiles"] <= tiles, stats
        assert 2 * stats["certain_pairs"] <= stats["certain_tiles"], stats
        if expect == "pairs":
            assert stats["certain_pairs"] > 0, stats


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_certain_tiles_render_the_same_bits(rt, oracle, pipe, name):
    w, h, settings, rows, expect = CASES[name]
    assert len(rows) <= 8
    stats = check(rt, oracle, pipe, w, h, settings, rows)
    assert_expected(stats, expect, ((w + 7) // 8) * ((h + 7) // 8))
    if name in ("silhouette", "three_tiles_wide"):
        # Every certain pair holds two certain tiles, so more certain tiles than twice the
        # certain pairs means a certain tile whose own pair is not a certain pair: its partner
        # (every tile of the 64-wide image has one; in the 24-wide image the third tile of a
        # row has none) is a general tile, and that pair takes the general sample.
        assert 2 * stats["certain_pairs"] < stats["certain_tiles"], stats


@gpu
def test_exhaustive_scan_has_no_certain_tiles(rt, oracle, pipe):
    """The exhaustive scan reads no lists: nothing is certain, whatever an earlier build left."""
    w, h, settings, rows, _ = CASES["fill_lambertian_lens"]
    assert_expected(check(rt, oracle, pipe, w, h, settings, rows), "pairs", 8)
    assert_expected(check(rt, oracle, pipe, w, h, settings, rows, scan="exhaustive"), "none", 8)


@gpu
@pytest.mark.parametrize("pairs", MODES)
def test_foreign_counts_take_the_fallback(rt, oracle, pipe, pairs):
    """After a first call the library expects every pixel at four samples; the image it is then
    given holds another count in its upper half (whole tiles, certain pairs among them): those
    workgroups of the pair launch take the per-tile fallback, the others the frame groups."""
    w, h, settings, rows, _ = CASES["fill_metal_lens"]
    cam = make_camera(rt, w, h, settings)
    still = make_camera(rt, w, h, dict(settings, camera_has_moved=False))
    scene = rt.SphereCollection(np.array(rows, np.float32).reshape(-1, 8))
    seeds = rt.frame_seeds(9, 2 * FRAMES)
    state, _ = oracle.render(np.zeros((h, w, 4), np.float32), cam.blob, scene.spheres,
                             seeds[:FRAMES])
    state = state.copy()
    state[0:8, :, 3] = 1.0
    ref, prev = state, None
    for s_ in seeds[FRAMES:]:
        prev = ref
        ref, _ = oracle.update(ref, still.with_fields(random_seed=float(s_)).blob, scene.spheres)
    for on in (True, False):
        a, b = pipe.new_image(w, h), pipe.new_image(w, h)
        pipe.set_certain_tiles(on)
        pipe.set_frame_pairs(pairs)
        try:
            if pipe.update_frames(a, b, w, h, cam, scene, seeds[:FRAMES]) == 1:
                a, b = b, a
            a.copy_(to_dev(state))                # behind the library's back
            newest = pipe.update_frames(a, b, w, h, still, scene, seeds[FRAMES:])
            stats, info = pipe.certain_tiles_stats(), pipe.last_launch_info()
        finally:
            pipe.set_frame_pairs("auto")
            pipe.set_certain_tiles(True)
        assert newest == 0
        assert_same(host(a), ref)
        assert_same(host(b), prev)
        assert info["kernel_name"] == KERNELS[pairs], info
        assert (stats["certain_pairs"] > 0) == on, stats


@gpu
def test_random_small_scenes(rt, oracle, pipe):
    certain_scenes = 0
    for k in range(RANDOM_SCENES):
        rows = random_scene(k)
        assert 2 <= len(rows) <= 8
        settings = {"defocus_angle": (0.6, 0.0, 3.0)[k % 3]}
        stats = check(rt, oracle, pipe, 32, 16, settings, rows)
        assert 2 * stats["certain_pairs"] <= stats["certain_tiles"] <= 8, (k, stats)
        certain_scenes += stats["certain_tiles"] > 0
    print("scenes with certain tiles:", certain_scenes, "of", RANDOM_SCENES)
    # the batch enters the path (a large sphere is drawn with probability 0.4 per sphere) and
    # also holds scenes without a certain tile
    assert 0 < certain_scenes < RANDOM_SCENES, certain_scenes


@gpu
def test_setting_rebuilds_the_lists(rt, pipe):
    """rt_set_certain_tiles is part of the lists' key: the next call with the same camera and
    scene rebuilds them."""
    w, h, settings, rows, _ = CASES["fill_lambertian_lens"]
    cam = make_camera(rt, w, h, settings)
    seen = [render(rt, pipe, on, "on2", w, h, cam, rows)[3] for on in (True, False, True)]
    assert seen[0] == seen[2] and seen[0]["certain_pairs"] > 0, seen
    assert seen[1] == {"certain_tiles": 0, "certain_pairs": 0}, seen


def test_certain_tiles_header_is_exported_and_bound(rt):
    """include/rt_certain_tiles.h: the library exports what it declares, the ctypes binding
    binds it, and ABI 7's own list does not change."""
    text = (ROOT / "include" / "rt_certain_tiles.h").read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_set_certain_tiles", "rt_certain_tiles_stats"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG_DIR / "build" / "librt_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(declared) <= exported
    assert rt._lib.certain_symbols() == declared
    assert not set(declared) & set(rt._lib.exported_symbols())
    assert "rt_certain" not in (ROOT / "include" / "rt_abi.h").read_text()
    assert rt._lib.lib().rt_abi_version() == 7


def test_null_context_and_bad_value(rt):
    L = rt._lib.lib()
    assert L.rt_set_certain_tiles(None, 1) == 6
    assert L.rt_certain_tiles_stats(None, None) == 6
