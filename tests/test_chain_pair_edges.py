"""The tile-pair frame-group kernels (rt_tpair_kernel<2> / <4>, set_frame_pairs "on2" / "quad2")
at the edges of what their frame loop keeps per unit: a unit without a partner tile, a lone
tile, partial tiles, several bands, groups short of a frame, both wave-uniform flags off and on
(max_depth 0 / 1, the one-step normal division), lens and pinhole cameras, and pairs whose
tiles hold a fallback (no candidate list), a short list and an empty list.  update_frames
against the oracle's chained updates, both ping-pong buffers, bit for bit (NaN == NaN).  (A
call of one frame is the one-frame kernel's in every mode; it is kept as a case of the same
entry point.)"""
import numpy as np
import pytest

from test_gpu_parity import assert_same, host

gpu = pytest.mark.gpu

KERNELS = {"on2": "rt_tpair_kernel<2>", "quad2": "rt_tpair_kernel<4>"}
SHAPES = [(72, 16),    # nine tiles a row: the last unit has no partner tile
          (8, 8),      # a lone tile
          (67, 45),    # partial tiles on both edges
          (136, 24)]   # several bands
FRAMES = [1, 2, 3, 7]  # groups of 2 and of 4 frames, some short of a frame
LOOK_FROM = np.array([13.0, 2.0, 3.0])
CLUSTER_AT = np.array([0.0, 1.0, 0.0])


def _rows(rows):
    return np.array(rows, np.float32).reshape(-1, 8)


def scene_mix():
    """14 spheres of the three materials with radii 0.2, 1 and 1000 (every one passes the
    upload's one-step normal check): no tile's list can overflow."""
    rows = [[0, -1000, 0, 1000, 0.5, 0.5, 0.5, -2.0],
            [0, 1, 0, 1, 1.5, 0, 0, 2.0],               # dielectric, ir 1.5
            [-4, 1, 0, 1, 0.4, 0.2, 0.1, -2.0],         # lambertian
            [4, 1, 0, 1, 0.7, 0.6, 0.5, 0.0]]           # metal, no fuzz
    for k in range(10):
        mat = (-2.0, 0.3, 2.0)[k % 3]                   # lambertian, fuzzy metal, dielectric
        rows.append([-3.0 + 0.9 * k, 0.2, 2.0 - 0.7 * (k % 4), 0.2,
                     1.5 if mat > 1 else 0.2 + 0.07 * k, 0.5, 0.9 - 0.06 * k, mat])
    return _rows(rows)


def scene_radii17():
    """17 spheres, 17 distinct radii: some radius fails the one-step check (normal_rn 0)."""
    rows = [[0, -1000, 0, 1000, 0.5, 0.5, 0.5, -2.0]]
    for k in range(16):
        r = 0.17 + 0.043 * k
        mat = (-2.0, 0.3, 2.0)[k % 3]
        rows.append([-4.0 + 0.55 * k, r, 1.5 - 0.8 * (k % 4), r,
                     1.5 if mat > 1 else 0.3 + 0.04 * k, 0.6, 0.4, mat])
    return _rows(rows)


def scene_classes(sigma=0.3):
    """60 small spheres around CLUSTER_AT (the camera of `classes` cases looks at it: the
    tiles at the image centre, the left tiles of their pairs, see more than a list holds),
    three more about a tile to the right (a short list in the pair's other tile) and nothing
    else: the outer tiles' lists are empty."""
    rng = np.random.default_rng(7)
    n = 60
    s = np.zeros((n + 3, 8), np.float32)
    s[:n, 0:3] = rng.normal(0.0, sigma, (n, 3)) + CLUSTER_AT
    s[:n, 3] = 0.1
    # the image's x axis in the world (vup x (look_from - look_at), normalised)
    w = LOOK_FROM - CLUSTER_AT
    u = np.cross([0.0, 1.0, 0.0], w)
    u /= np.linalg.norm(u)
    for k in range(3):
        s[n + k, 0:3] = CLUSTER_AT + (2.2 + 0.15 * k) * u + [0.0, 0.1 * k - 0.1, 0.0]
        s[n + k, 3] = 0.125                              # (a power of two)
    s[:, 4:7] = 0.5
    s[:, 7] = -2.0
    s[1::3, 7] = 0.25                                    # metal
    s[2::3, 7] = 2.0                                     # dielectric
    s[2::3, 4] = 1.5
    return s


SCENES = {"mix": scene_mix, "radii17": scene_radii17, "classes": scene_classes}
NORMAL_RN = {"mix": 1, "radii17": 0}


def make_camera(rt, w, h, depth, defocus, scene):
    look_at = tuple(CLUSTER_AT) if scene == "classes" else (0.0, 0.0, 0.0)
    s = rt.CameraSettings(max_depth=depth, samples_per_pixel=500, camera_has_moved=True,
                          defocus_angle=defocus, field_of_view=20.0, look_at=look_at)
    return rt.SceneCamera.from_settings(s, w, h, 0.5)


_oracle_cache = {}


def oracle_frames(rt, oracle, scene, w, h, depth, defocus, frames):
    """The oracle's image after `frames` chained updates from a reset (computed once)."""
    key = (scene, w, h, depth, defocus, frames)
    if key not in _oracle_cache:
        cam = make_camera(rt, w, h, depth, defocus, scene)
        img, _ = oracle.render(np.zeros((h, w, 4), np.float32), cam.blob, SCENES[scene](),
                               rt.frame_seeds(33, frames))
        img.setflags(write=False)
        _oracle_cache[key] = img
    return _oracle_cache[key]


def run(rt, scene, w, h, depth, defocus, frames, pairs, images, rank=0, nranks=1):
    """update_frames from a reset: (newest image, the other one, launch info, list stats)."""
    p = rt.ComputeShaderPipeline(0)
    try:
        p.set_frame_pairs(pairs)
        p.set_frame_images(images)
        rows = rt.stripe_local_rows(h, rank, nranks) if nranks > 1 else h
        a, b = p.new_image(w, rows), p.new_image(w, rows)
        newest = p.update_frames(a, b, w, h, make_camera(rt, w, h, depth, defocus, scene),
                                 rt.SphereCollection(SCENES[scene]()),
                                 rt.frame_seeds(33, frames), rank, nranks)
        if newest == 1:
            a, b = b, a
        return host(a).copy(), host(b).copy(), p.last_launch_info(), p.candidate_stats()
    finally:
        p.close()


def check(rt, oracle, scene, w, h, depth, defocus, frames, pairs, images):
    new, prev, info, stats = run(rt, scene, w, h, depth, defocus, frames, pairs, images)
    assert info["frames"] == frames
    # (a launch of one frame is the one-frame kernel's in every mode: rt_frames.cpp, nf == 1)
    assert info["kernel_name"] == KERNELS[pairs] or frames == 1, info
    assert_same(new, oracle_frames(rt, oracle, scene, w, h, depth, defocus, frames))
    if frames >= 2:
        assert_same(prev, oracle_frames(rt, oracle, scene, w, h, depth, defocus, frames - 1))
    return info, stats


@gpu
@pytest.mark.parametrize("images", ["every", "last_two"])
@pytest.mark.parametrize("pairs", ["on2", "quad2"])
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_and_short_groups(rt, oracle, w, h, frames, pairs, images):
    """Every shape with every frame count: units without a partner, partial tiles, bands, and
    frame groups with fewer frames than waves."""
    check(rt, oracle, "mix", w, h, 1, 0.6, frames, pairs, images)


@gpu
@pytest.mark.parametrize("pairs", ["on2", "quad2"])
@pytest.mark.parametrize("defocus", [0.6, 0.0])
@pytest.mark.parametrize("depth", [0, 1])
@pytest.mark.parametrize("scene", ["mix", "radii17"])
@pytest.mark.parametrize("w,h", [(72, 16), (67, 45)])
def test_uniform_flags_and_cameras(rt, oracle, w, h, scene, depth, defocus, pairs):
    """max_depth 0 and 1 (the scan's flag), radii that pass the one-step normal check and
    radii that do not (the shader's flag), lens and pinhole camera."""
    info, _ = check(rt, oracle, scene, w, h, depth, defocus, 3, pairs, "every")
    assert info["normal_rn"] == NORMAL_RN[scene]


@gpu
@pytest.mark.parametrize("images", ["every", "last_two"])
@pytest.mark.parametrize("pairs", ["on2", "quad2"])
@pytest.mark.parametrize("w,h,frames", [(72, 16, 3), (72, 16, 7), (136, 24, 2)])
def test_count_classes_across_pairs(rt, oracle, w, h, frames, pairs, images):
    """A tile without a list beside a tile with a short one, and pairs of empty lists."""
    _, st = check(rt, oracle, "classes", w, h, 1, 0.6, frames, pairs, images)
    assert st["tiles"] == ((w + 7) // 8) * ((h + 7) // 8) and st["capacity"] == 19
    assert 0 < st["tiles_without_list"] < st["tiles"], st      # a fallback tile
    assert st["max_entries"] >= 1, st                          # a listed tile that is not empty
    # fewer entries than listed tiles: some listed tile is empty
    assert st["mean_entries"] < 1.0, st


@gpu
@pytest.mark.parametrize("pairs", ["on2", "quad2"])
def test_rank_share(rt, oracle, pairs):
    """Rank 1 of 2 of the three-band image: band 1 alone."""
    w, h, frames = 136, 24, 3
    new, prev, info, _ = run(rt, "mix", w, h, 1, 0.6, frames, pairs, "every", rank=1, nranks=2)
    assert info["kernel_name"] == KERNELS[pairs]
    assert new.shape[0] == 8
    assert_same(new, oracle_frames(rt, oracle, "mix", w, h, 1, 0.6, frames)[8:16])
    assert_same(prev, oracle_frames(rt, oracle, "mix", w, h, 1, 0.6, frames - 1)[8:16])
