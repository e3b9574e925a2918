"""Chain parts (rt_set_chain_parts): an update_frames call of several fused frame-group
launches as two staggered chains over halves of the scheduling units.  The split call against
the unsplit one, bit for bit on both ping-pong buffers (NaN == NaN), and against the CPU
oracle; what last_launch_info reports; and the schedule function on the host."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, camera, host, to_dev

gpu = pytest.mark.gpu

CAP = 4            # frames per launch: 13 frames need several launches per part
SHAPES = [(72, 40),   # nine tiles per row: the last pair unit has one tile; 25 pair units (odd)
          (70, 37)]   # partial tiles on both edges
KERNELS = {"on": "rt_trace_kernel<3>", "quad": "rt_trace_kernel<4>",
           "on2": "rt_tpair_kernel<2>", "quad2": "rt_tpair_kernel<4>",
           "auto": "rt_trace_kernel<4>"}       # (AUTO at these sizes: four waves per tile)


def scene_of(rt, name):
    return rt.three_spheres() if name == "three" else rt.synthetic_scene(20)


_oracle_cache = {}


def oracle_frames(rt, oracle, scene, w, h, frames, seed0=33):
    """The oracle's image after `frames` frames from a reset (computed once per key)."""
    key = (scene, w, h, frames, seed0)
    if key not in _oracle_cache:
        yy, xx = np.mgrid[0:h, 0:w]
        cam = camera(rt, w, h, depth=1, spp=500)
        st, _ = oracle.render_pixels(np.zeros((h * w, 4), np.float32), xx.ravel(), yy.ravel(),
                                     cam.blob, scene_of(rt, scene).spheres,
                                     rt.frame_seeds(seed0, frames))
        st = st.reshape(h, w, 4)
        st.setflags(write=False)
        _oracle_cache[key] = st
    return _oracle_cache[key]


def run_calls(rt, parts, w, h, scene, pairs, images, calls, rank=0, nranks=1, spp=500,
              timing=False, edit=None):
    """A pipeline with chain parts `parts` runs `calls` = [(moved, frames), ...] on one pair
    of images, each call reading the image the one before left newest; returns per call
    (newest image, other image, last_launch_info).  edit(image): applied in place to the newest
    image before the last call."""
    sc = scene_of(rt, scene)
    p = rt.ComputeShaderPipeline(0)
    p.set_frames_per_launch(CAP)
    p.set_frame_pairs(pairs)
    p.set_frame_images(images)
    p.set_chain_parts(parts)
    p.set_launch_timing(timing)
    rows = rt.stripe_local_rows(h, rank, nranks) if nranks > 1 else h
    out = []
    try:
        a, b = p.new_image(w, rows), p.new_image(w, rows)
        used = 0
        for i, (moved, frames) in enumerate(calls):
            if edit is not None and i == len(calls) - 1:
                edit(a)
            seeds = rt.frame_seeds(33, used + frames)[used:]
            used += frames
            cam = camera(rt, w, h, depth=1, spp=spp, moved=moved)
            newest = p.update_frames(a, b, w, h, cam, sc, seeds, rank, nranks)
            if newest == 1:
                a, b = b, a
            out.append((host(a).copy(), host(b).copy(), p.last_launch_info()))
    finally:
        p.close()
    return out


def assert_calls_equal(one, two):
    assert len(one) == len(two)
    for (n1, o1, _), (n2, o2, _) in zip(one, two):
        assert_same(n2, n1)
        assert_same(o2, o1)


def two_part_launches(rt, frames):
    s = rt.chain_schedule(frames, CAP)
    assert {part for part, _, _ in s} == {0, 1}
    return len(s)


@gpu
@pytest.mark.parametrize("images", ["every", "last_two"])
@pytest.mark.parametrize("pairs", ["auto", "on", "quad", "on2", "quad2"])
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("scene", ["three", "n20"])
def test_split_call_matches_unsplit_and_oracle(rt, oracle, scene, w, h, pairs, images):
    """A reset call of 13 frames (odd; raster units, costs recorded), a continuing call of 13
    (the cost-ordered unit table) and a continuing call of 12 (even): both buffers after every
    call equal the unsplit call's, and the first call's equal the oracle's frames 13 and 12."""
    calls = [(True, 13), (False, 13), (False, 12)]
    one = run_calls(rt, 1, w, h, scene, pairs, images, calls)
    two = run_calls(rt, 2, w, h, scene, pairs, images, calls)
    assert_calls_equal(one, two)
    assert_same(two[0][0], oracle_frames(rt, oracle, scene, w, h, 13))
    assert_same(two[0][1], oracle_frames(rt, oracle, scene, w, h, 12))
    for (_, _, i1), (_, _, i2), (_, frames) in zip(one, two, calls):
        assert i2["kernel_name"] == KERNELS[pairs]
        assert i1["chain_parts"] == 1 and i1["launches"] == -(-frames // CAP)
        assert i2["chain_parts"] == 2 and i2["launches"] == two_part_launches(rt, frames)
        assert i2["queues"] == i1["queues"] and i2["frames"] == i1["frames"] == frames
        assert i2["max_frames_per_launch"] == CAP


@gpu
@pytest.mark.parametrize("pairs", ["on2", "quad"])
def test_count_cap_reached_mid_part(rt, oracle, pairs):
    """samples_per_pixel = 5 with 13 frames: the count cap is reached inside a launch of each
    part (frames 5.. no longer accumulate)."""
    w, h = SHAPES[0]
    calls = [(True, 13), (False, 13)]
    one = run_calls(rt, 1, w, h, "n20", pairs, "every", calls, spp=5)
    two = run_calls(rt, 2, w, h, "n20", pairs, "every", calls, spp=5)
    assert_calls_equal(one, two)
    assert two[1][2]["chain_parts"] == 2
    assert np.all(two[1][0][..., 3] == 5)
    # five accumulated frames, whatever follows
    assert_same(two[1][0][..., :3], oracle_frames(rt, oracle, "n20", w, h, 5)[..., :3])


@gpu
@pytest.mark.parametrize("pairs", ["on2", "quad2", "on"])
def test_foreign_count_inside_a_split_call(rt, oracle, pairs):
    """One tile of the input holds another sample count than the context expects: its
    workgroup takes the per-tile fallback in every launch of its part; the rest of the image
    runs the frame groups."""
    w, h = SHAPES[0]

    def edit(img):
        img[8:16, 16:24, 3] = 1.0

    calls = [(True, 4), (False, 13)]
    one = run_calls(rt, 1, w, h, "three", pairs, "last_two", calls, edit=edit)
    two = run_calls(rt, 2, w, h, "three", pairs, "last_two", calls, edit=edit)
    assert_calls_equal(one, two)
    assert one[0][2]["launches"] == two[0][2]["launches"] == 1
    assert two[0][2]["chain_parts"] == 1 and two[1][2]["chain_parts"] == 2
    state = two[0][0].copy()
    edit(state)
    yy, xx = np.mgrid[0:h, 0:w]
    cam = camera(rt, w, h, depth=1, spp=500, moved=False)
    want, _ = oracle.render_pixels(state.reshape(-1, 4), xx.ravel(), yy.ravel(), cam.blob,
                                   scene_of(rt, "three").spheres, rt.frame_seeds(33, 17)[4:])
    assert_same(two[1][0], want.reshape(h, w, 4))


@gpu
@pytest.mark.parametrize("pairs", ["on2", "auto"])
def test_rank_share(rt, oracle, pairs):
    """Rank 1 of 3: two of the five stripe bands."""
    w, h = SHAPES[0]
    calls = [(True, 13), (False, 13)]
    one = run_calls(rt, 1, w, h, "n20", pairs, "every", calls, rank=1, nranks=3)
    two = run_calls(rt, 2, w, h, "n20", pairs, "every", calls, rank=1, nranks=3)
    assert_calls_equal(one, two)
    assert two[1][2]["chain_parts"] == 2
    want = oracle_frames(rt, oracle, "n20", w, h, 13)
    got = two[0][0]
    for j, band in enumerate((1, 4)):
        assert_same(got[8 * j:8 * j + 8], want[8 * band:8 * band + 8])


@gpu
def test_launch_info_and_modes(rt):
    """A call within the cap is one launch and one chain part in every mode; AUTO keeps small
    launches in one chain; with launch timing armed the call stays unsplit; more than two
    parts is an error."""
    w, h = SHAPES[0]
    for parts in (0, 1, 2):
        (_, _, info), = run_calls(rt, parts, w, h, "three", "on2", "every", [(True, CAP)])
        assert info["launches"] == 1 and info["chain_parts"] == 1
    (_, _, info), = run_calls(rt, 0, w, h, "three", "on2", "every", [(True, 13)])
    assert info["launches"] == 4 and info["chain_parts"] == 1
    plain = run_calls(rt, 2, w, h, "three", "on2", "every", [(True, 13)])
    timed = run_calls(rt, 2, w, h, "three", "on2", "every", [(True, 13)], timing=True)
    assert plain[0][2]["chain_parts"] == 2
    assert timed[0][2]["chain_parts"] == 1 and timed[0][2]["launches"] == 4
    assert_calls_equal(plain, timed)
    p = rt.ComputeShaderPipeline(0)
    try:
        with pytest.raises(rt._lib.RtError):
            p.set_chain_parts(3)
    finally:
        p.close()


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("cap", [1, 4, 64])
def test_schedule_on_the_host(rt, cap, variant):
    """rt_chain_schedule for 1..300 frames: every part covers every frame once, in order; no
    launch above the cap; no interior boundary shared by the parts; a count within the cap is
    one unsplit launch; above it (cap >= 4) there are two parts, no launch of one frame."""
    for frames in range(1, 301):
        s = rt.chain_schedule(frames, cap, variant)
        parts = sorted({part for part, _, _ in s})
        if frames <= cap:
            assert s == [(0, 0, frames)]
            continue
        assert parts == ([0, 1] if cap >= 4 else [0]), (frames, cap)
        cuts = {}
        for k in parts:
            at = 0
            for part, first, n in s:
                if part != k:
                    continue
                assert first == at and 1 <= n <= cap, (frames, cap, s)
                assert len(parts) == 1 or n >= 2, (frames, cap, s)
                at += n
            assert at == frames, (frames, cap, s)
            cuts[k] = {first for part, first, _ in s if part == k and first}
        if len(parts) == 2:
            assert not (cuts[0] & cuts[1]), (frames, cap, s)
        # issue order: by first frame
        assert [first for _, first, _ in s] == sorted(first for _, first, _ in s)
    assert rt.chain_schedule(200, 64, 1) == [
        (0, 0, 64), (1, 0, 32), (1, 32, 64), (0, 64, 64), (1, 96, 64), (0, 128, 56),
        (1, 160, 32), (0, 184, 16), (1, 192, 8)]
    assert rt.chain_schedule(200, 64, 2) == [
        (0, 0, 64), (1, 0, 32), (1, 32, 64), (0, 64, 64), (1, 96, 64), (0, 128, 64),
        (1, 160, 40), (0, 192, 8)]


def test_chain_parts_header_is_exported_and_bound(rt):
    """include/rt_chain_parts.h: the library exports what it declares and the ctypes binding
    covers exactly that."""
    import re
    import subprocess
    from conftest import PKG_DIR, ROOT
    text = (ROOT / "include" / "rt_chain_parts.h").read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_set_chain_parts", "rt_chain_schedule"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG_DIR / "build" / "librt_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    assert set(declared) <= set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(rt._lib.chain_parts_symbols()) == set(declared)
    assert not set(declared) & set(rt._lib.exported_symbols())
    # the struct's mirror
    assert [f for f, _ in rt._lib.ChainLaunchC._fields_] == ["part", "first", "frames"]
    assert rt._lib.ctypes.sizeof(rt._lib.ChainLaunchC) == 12


def test_setter_errors_without_device(rt):
    L = rt._lib.lib()
    assert L.rt_set_chain_parts(None, 1) == 6
    n = rt._lib.U32(0)
    assert L.rt_chain_schedule(0, 4, 0, None, 0, n) == 1
    assert L.rt_chain_schedule(13, 4, 5, None, 0, n) == 1
    assert L.rt_chain_schedule(13, 4, 0, None, 0, n) == 2 and n.value == 8
