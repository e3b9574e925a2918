"""The adaptive round as one multi-frame launch (include/rt_converge.h): rt_converge_frames,
rt_converge_frames_bands.

The reference is the chain the header names, built from the restatements the repository already
has: per frame tests/test_variance.py's `initial_variance` with +inf as the fallback (the error
plane), tests/test_adaptive.py's `adaptive_ref` (the update) and tests/test_variance.py's
`moments_ref` (`chain_ref` below).  Every GPU output is compared bit for bit (NaN == NaN), and a
sentinel tail follows every buffer the library writes.

The parity input is test_adaptive's accumulator (colours in [0, 1.5), counts 0..20 by position)
with moments of zero, except that tile (1, 0) holds counts of 20 and moments (0.5, 0.25, 0, 20),
whose error is 0, and that the texel (x 10, y 3) of that tile holds the count 7.5: it is idle in
frame 0, passes through as 7, loses its moments to rt_moments_update's rule 4 and is sampled in
frames 1 and 2 — the tile a kernel that stops at "no lane sampled" gets wrong.  It runs at 48 x 32,
at 21 x 13 with a reset on frame 0 (ragged tiles, and the only full ones: at samples_per_pixel 12
every tile of the input holds counts that are capped from the start) and at 193 x 131.  The CPU
tests count from the reference alone what the inputs reach (printed with -s).
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
import test_fast_domains as fd
import test_variance as tv
from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_converge.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
SENT, SENT_WORD, TAIL = ta.SENT, ta.SENT_WORD, ta.TAIL
SENT_U32 = 0x5A5A5A5A              # tile_samples' sentinel (int32)
# the parity input's parameters (tile (1, 0)'s error 0 is below every threshold)
SPP, MIN_SAMPLES, MIN_HISTORY, ABS2, REL2 = 12, 4, 2, 1e-3, 2e-2
PARAMS = dict(min_samples=MIN_SAMPLES, abs_tolerance2=ABS2, rel_tolerance2=REL2)
FRAMES, SEED_SET = 8, 11
PLANT_X, PLANT_Y = 10, 3
MOMENT_RULES = ("first", "consecutive", "capped", "broken")     # rt_moments_update's rules 1-4


# ---- the reference ---------------------------------------------------------------------------------
def popcounts(words):
    """Set bits of each uint64 word."""
    b = np.ascontiguousarray(words, np.uint64).view(np.uint8).reshape(words.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(-1).astype(np.uint32)


def chain_ref(oracle, img, mom, cam, spheres, seeds, params, min_history):
    """The header's loop: one record per frame (image, moments, the frame's tile mask words and
    sampled pixels, the frame's tally of rt_moments_update's rules)."""
    img, mom = np.ascontiguousarray(img, F32), np.ascontiguousarray(mom, F32)
    frames = []
    for f, s in enumerate(seeds):
        cam_f = cam.with_fields(random_seed=float(s),
                                camera_has_moved=cam.camera_has_moved if f == 0 else 0.0)
        err = tv.initial_variance(img, mom, min_history, np.inf)[0]
        new, words, sampled = ta.adaptive_ref(oracle, img, cam_f, spheres, err,
                                              params["min_samples"], params["abs_tolerance2"],
                                              params["rel_tolerance2"])
        tally = {}
        mom, img = tv.moments_ref(img, new, mom, tally), new
        for a in (img, mom, words, sampled):
            a.setflags(write=False)
        frames.append(SimpleNamespace(img=img, mom=mom, words=words, sampled=sampled,
                                      tally=tally))
    return frames


def want(c, k=None):
    """What a call of the first k frames of case c leaves: image, moments, error plane, the last
    frame's tile mask and the samples per tile."""
    k = len(c.frames) if k is None else k
    last = c.frames[k - 1]
    err = tv.initial_variance(last.img, last.mom, c.min_history, np.inf)[0]
    samples = sum(popcounts(fr.words) for fr in c.frames[:k])
    return SimpleNamespace(img=last.img, mom=last.mom, err=err, words=last.words, samples=samples)


def parity_planes(w, h):
    """The parity input (see the module's text)."""
    img = ta.planes(w, h, "active")[0].copy()      # colours in [0, 1.5), counts (5 x + 3 y) % 21
    mom = np.zeros((h, w, 4), F32)
    img[0:8, 8:16, 3] = 20.0
    mom[0:8, 8:16] = (0.5, 0.25, 0.0, 20.0)
    img[PLANT_Y, PLANT_X, 3] = 7.5
    img.setflags(write=False)
    mom.setflags(write=False)
    return img, mom


def make_case(w, h, cam, sc, img, mom, seeds, params, min_history):
    from oracle import oracle
    frames = chain_ref(oracle, img, mom, cam, sc.spheres, seeds, params, min_history)
    return SimpleNamespace(w=w, h=h, cam=cam, sc=sc, img=img, mom=mom,
                           seeds=np.array(seeds, F32), params=params, min_history=min_history,
                           frames=frames)


@functools.lru_cache(None)
def case(w, h, depth, defocus, moved=False, domain=True, frames=FRAMES):
    """The parity input at one shape and camera, and its reference (computed once, read-only)."""
    import gpu_ray_tracing as rt
    cam = ta.make_camera(rt, w, h, depth, defocus and domain, SPP, moved=moved,
                         **ta.camera_kw(domain))
    img, mom = parity_planes(w, h)
    return make_case(w, h, cam, ta.scene(), img, mom, rt.frame_seeds(SEED_SET, frames), PARAMS,
                     MIN_HISTORY)


CAP_FRAMES = (64, 65, 130)
CAP_PARAMS = dict(min_samples=4, abs_tolerance2=0.0, rel_tolerance2=1e-7)


@functools.lru_cache(None)
def cap_case():
    """24 x 16 at depth 1 over 130 frames: samples_per_pixel 500 and tolerances so small that
    some tiles sample in every frame, across the 64-frame launches of one call."""
    import gpu_ray_tracing as rt
    w, h = 24, 16
    cam = ta.make_camera(rt, w, h, 1, True, 500)
    img, mom = parity_planes(w, h)
    return make_case(w, h, cam, ta.scene(), img, mom, rt.frame_seeds(5, max(CAP_FRAMES)),
                     CAP_PARAMS, MIN_HISTORY)


# ---- CPU tests -------------------------------------------------------------------------------------
def test_library_exports_the_converge_entry_points(rt):
    text = HEADER.read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_converge_frames", "rt_converge_frames_bands"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert {s for s in exported if "converge" in s} == set(declared)
    for s in declared:
        assert not any(k in s for k in ("adaptive", "variance", "moments", "denoise",
                                        "reproject"))
    L = rt._lib
    assert L.converge_symbols() == declared
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.selftest_roots_symbols(), L.denoise_symbols(), L.reproject_symbols(),
                  L.variance_symbols(), L.adaptive_symbols()):
        assert not set(declared) & set(other)
    assert L.lib().rt_abi_version() == 7
    assert re.search(r"#define RT_CONVERGE_MAX_FRAMES_PER_LAUNCH 64u\b", text)
    assert L.RT_CONVERGE_MAX_FRAMES_PER_LAUNCH == 64
    assert '#include "rt_adaptive.h"' in text
    assert "converge" not in (ROOT / "include" / "rt_abi.h").read_text()
    assert "rt_converge" not in (ROOT / "include" / "rt_adaptive.h").read_text()
    assert callable(rt.ComputeShaderPipeline.converge)


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "rt_converge.h"\n'
                   "typedef char cap_is_64[RT_CONVERGE_MAX_FRAMES_PER_LAUNCH == 64u ? 1 : -1];\n"
                   "typedef char params_are_12_bytes[sizeof(rt_adaptive_params) == 12 ? 1 : -1];\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def tile_counts(c):
    """Sampled lanes per (frame, tile row, tile column)."""
    return np.stack([popcounts(fr.words) for fr in c.frames])


@pytest.mark.parametrize("depth", [1, 3])
def test_parity_input_reaches_what_it_is_for(depth):
    w, h = 48, 32
    c = case(w, h, depth, True)
    T = tile_counts(c)
    per_frame = [int(fr.sampled.sum()) for fr in c.frames]
    rules = {k: sum(fr.tally[k] for fr in c.frames) for k in MOMENT_RULES}
    active = T.reshape(FRAMES, -1) > 0
    settled = active.any(0) & ~active[-1]            # was active, idle from some frame to the end
    last = ta.tile_kinds(c.frames[-1].words, w, h)
    full_somewhere = max(ta.tile_kinds(fr.words, w, h)[1] for fr in c.frames)
    counts = np.stack([ta.f2u(fr.img[..., 3]) for fr in c.frames])
    before = np.concatenate([ta.f2u(c.img[..., 3])[None], counts[:-1]])
    reached_cap = int(((before < SPP) & (counts == SPP)).any(0).sum())
    print(f"depth {depth}: sampled pixels per frame {per_frame}; tile (1, 0) per frame "
          f"{T[:, 0, 1].tolist()}; {int(settled.sum())} tiles settle; last frame: {last[0]} idle, "
          f"{last[1]} full, {last[2]} partial tiles; {full_somewhere} full tiles in some frame; "
          f"{reached_cap} pixels reach the cap; rules 1-4: "
          + " / ".join(str(rules[k]) for k in MOMENT_RULES))
    # tile (1, 0): idle in frame 0, then exactly the planted texel in frames 1 and 2
    assert T[:, 0, 1].tolist() == [0, 1, 1, 0, 0, 0, 0, 0]
    assert c.frames[1].sampled[PLANT_Y, PLANT_X] and c.frames[2].sampled[PLANT_Y, PLANT_X]
    assert c.frames[0].img[PLANT_Y, PLANT_X, 3] == 7.0            # 7.5 passes through as 7
    assert not c.frames[0].mom[PLANT_Y, PLANT_X].any()            # and rule 4 zeroes its moments
    assert c.frames[0].tally["broken"] >= 1
    assert settled.sum() == {1: 17, 3: 7}[depth]
    assert last[0] >= 1 and last[2] >= 1
    # No tile of this input is ever full: counts of 12..20 sit in every tile and are capped from
    # the start (samples_per_pixel 12).  Full tiles are the reset input's: the test below.
    assert full_somewhere == 0
    assert reached_cap >= 1
    assert per_frame[:2] == [844, 774]
    if depth == 1:
        assert per_frame[2] == 149
        assert [rules[k] for k in MOMENT_RULES] == [71, 1822, 10394, 1]
    assert per_frame[0] > per_frame[-1] > 0
    for k in MOMENT_RULES:
        assert rules[k] >= 1, f"rt_moments_update's rule {k} is never reached"
    assert sum(rules.values()) == FRAMES * w * h


@pytest.mark.parametrize("depth", [1, 3])
def test_reset_input_has_full_and_ragged_tiles(depth):
    """21 x 13 with a reset on frame 0: every pixel is sampled in frame 0, so the tiles inside
    the image are full and the ragged ones hold exactly their on-image lanes."""
    w, h = 21, 13
    c = case(w, h, depth, True, True)
    assert c.cam.camera_has_moved > 0.5 and c.frames[0].sampled.all()
    none, full, part = ta.tile_kinds(c.frames[0].words, w, h)
    print(f"depth {depth}, 21x13 reset: frame 0 has {full} full and {part} ragged tiles; sampled "
          f"pixels per frame {[int(fr.sampled.sum()) for fr in c.frames]}")
    assert (none, full, part) == (0, 2, 4)
    assert c.frames[0].tally["first"] == w * h                   # rule 1 everywhere
    assert popcounts(c.frames[0].words).sum() == w * h
    assert c.frames[-1].sampled.any() and not c.frames[-1].sampled.all()


@pytest.mark.parametrize("depth", [1, 3])
def test_a_settled_tile_stays_settled_on_the_reference(depth):
    """The early exit's rule, on the reference: after a frame that is not a reset, sampled no
    pixel of a tile and left the tile's texels bit-identical, every later frame does the same.
    And a frame without a sample alone does not settle a tile: tile (1, 0)'s frame 0."""
    w, h = 48, 32
    c = case(w, h, depth, True)
    T = tile_counts(c)

    def tile_of(a, ty, tx):
        return a[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]

    fixed = 0
    for ty in range(h // 8):
        for tx in range(w // 8):
            prev = (c.img, c.mom)
            settled_at = None
            for f, fr in enumerate(c.frames):
                same = all(bits_equal(tile_of(a, ty, tx), tile_of(b, ty, tx))[0]
                           for a, b in zip(prev, (fr.img, fr.mom)))
                if settled_at is not None:
                    assert T[f, ty, tx] == 0 and same, (ty, tx, settled_at, f)
                elif T[f, ty, tx] == 0 and same:
                    settled_at = f
                    fixed += 1
                prev = (fr.img, fr.mom)
    print(f"depth {depth}: {fixed} of {T[0].size} tiles reach a fixed point within {FRAMES} frames")
    assert fixed >= 1
    assert T[0, 0, 1] == 0 and T[1, 0, 1] == 1                    # idle, changed, sampled again


def test_cap_case_samples_in_every_frame():
    c = cap_case()
    T = tile_counts(c)
    always = (T.reshape(len(c.frames), -1) > 0).all(0)
    print(f"24x16 over {len(c.frames)} frames: {int(always.sum())} of {always.size} tiles sample "
          f"in every frame; sampled pixels in frames 0, 63, 64, 129: "
          f"{[int(c.frames[f].sampled.sum()) for f in (0, 63, 64, 129)]}")
    assert always.any(), "no tile samples in every frame"
    assert max(CAP_FRAMES) > 2 * 64 and 64 in CAP_FRAMES and 65 in CAP_FRAMES


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


guarded, guarded_words, to_dev = ta.guarded, ta.guarded_words, ta.to_dev


def guarded_u32(p, n):
    import torch
    return torch.full((n + TAIL,), SENT_U32, dtype=torch.int32, device=p.torch_device)


def tail_intact(t, n, what):
    got = t.cpu().numpy()
    sent = {np.dtype(F32): F32(SENT), np.dtype(np.int64): np.int64(SENT_WORD),
            np.dtype(np.int32): np.int32(SENT_U32)}[got.dtype]
    assert (got[n:] == sent).all(), f"the tail after {what} was written"
    return got[:n]


def run_converge(p, c, k=None, first=0, error=True, mask=True, samples=True, bands=None,
                 rows=None, state=None, moved=None):
    """converge over frames [first, first + k) of a case (on its planes, the rows `rows` of them
    for a band set, or `state` = (image, moments) device tensors of an earlier call): a
    namespace of numpy results (None for an output not asked for) and the device tensors."""
    import torch
    k = len(c.frames) - first if k is None else k
    img = c.img if rows is None else c.img[rows]
    mom = c.mom if rows is None else c.mom[rows]
    h = img.shape[0]
    px = c.w * h
    ty, tx = (h + 7) // 8, (c.w + 7) // 8
    a, m = state if state is not None else (guarded(p, 4 * px, img), guarded(p, 4 * px, mom))
    e = guarded(p, px) if error else None
    words = guarded_words(p, ty * tx) if mask else False
    taken = guarded_u32(p, ty * tx) if samples else False
    cam = c.cam if moved is None else c.cam.with_fields(camera_has_moved=1.0 if moved else 0.0)
    res = p.converge(a, m, c.w, c.h, cam, c.sc, c.seeds[first:first + k],
                     min_history=c.min_history, error=e, tile_mask=words, tile_samples=taken,
                     bands=bands, **c.params)
    torch.cuda.current_stream().synchronize()
    assert res[0] is e and res[1] is (words if mask else None)
    assert res[2] is (taken if samples else None)
    out = SimpleNamespace(a=a, m=m, err=None, words=None, samples=None)
    out.img = tail_intact(a, 4 * px, "image").reshape(h, c.w, 4)
    out.mom = tail_intact(m, 4 * px, "moments").reshape(h, c.w, 4)
    if error:
        out.err = tail_intact(e, px, "error").reshape(h, c.w)
    if mask:
        out.words = tail_intact(words, ty * tx, "tile_mask").view(np.uint64).reshape(ty, tx)
    if samples:
        out.samples = tail_intact(taken, ty * tx, "tile_samples").view(np.uint32).reshape(ty, tx)
    return out


def check(got, ref, what="", rows=None, bands=None):
    sel = (lambda a: a) if rows is None else (lambda a: a[rows])
    tsel = (lambda a: a) if bands is None else (lambda a: a[bands])
    for name in ("img", "mom", "err"):
        if getattr(got, name) is not None:
            same, bad = bits_equal(getattr(got, name), sel(getattr(ref, name)))
            assert same, f"{what}: {bad} values of {name} differ from the reference"
    if got.words is not None:
        assert (got.words == tsel(ref.words)).all(), f"{what}: the tile mask differs"
    if got.samples is not None:
        assert (got.samples == tsel(ref.samples)).all(), f"{what}: tile_samples differs"


# (shape, a reset on frame 0, the depths it runs at)
PARITY = [((48, 32), False, (1, 3)), ((21, 13), True, (1, 3)), ((193, 131), False, (1,))]
PARITY_CASES = [pytest.param(s, moved, d, id=f"{s[0]}x{s[1]}-depth{d}")
                for s, moved, depths in PARITY for d in depths]


@gpu
@pytest.mark.parametrize("defocus", [True, False], ids=["lens", "pinhole"])
@pytest.mark.parametrize("scan", ta.SCANS, indirect=True)
@pytest.mark.parametrize("shape,moved,depth", PARITY_CASES)
def test_outputs_match_the_chain_of_references(rt, pipe, shape, moved, depth, scan, defocus):
    c = case(shape[0], shape[1], depth, defocus, moved)
    ref = want(c)
    check(run_converge(pipe, c), ref, "all outputs")
    if shape == (48, 32):
        # each optional output is optional
        for off in ("error", "mask", "samples"):
            got = run_converge(pipe, c, **{off: False})
            assert getattr(got, {"error": "err", "mask": "words"}.get(off, off)) is None
            check(got, ref, f"without {off}")


@gpu
def test_matches_the_three_call_loop(rt, pipe):
    """Six frames at 193 x 131 and depth 3 against update_adaptive, moments_update and
    adaptive_error called in turn on the same input."""
    import torch
    w, h, frames = 193, 131, 6
    cam = ta.make_camera(rt, w, h, 3, True, SPP)
    img, mom = parity_planes(w, h)
    seeds = rt.frame_seeds(SEED_SET, frames)
    a, b, m = to_dev(pipe, img), pipe.new_image(w, h), to_dev(pipe, mom)
    e = pipe.adaptive_error(a, m, w, h, min_history=MIN_HISTORY)
    for s in seeds:
        pipe.update_adaptive(a, b, w, h, cam.with_fields(random_seed=float(s)), ta.scene(), e,
                             **PARAMS)
        pipe.moments_update(a, b, m, w, h)
        pipe.adaptive_error(b, m, w, h, min_history=MIN_HISTORY, out=e)
        a, b = b, a
    ca, cm = to_dev(pipe, img), to_dev(pipe, mom)
    ce, _, _ = pipe.converge(ca, cm, w, h, cam, ta.scene(), seeds, min_history=MIN_HISTORY,
                             error=True, **PARAMS)
    torch.cuda.synchronize()
    assert not bits_equal(ca.cpu().numpy(), img)[0], "nothing was sampled"
    assert bits_equal(ca.cpu().numpy(), a.cpu().numpy())[0], "the image differs"
    assert bits_equal(cm.cpu().numpy(), m.cpu().numpy())[0], "the moments differ"
    assert bits_equal(ce.cpu().numpy(), e.cpu().numpy())[0], "the error plane differs"


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_splitting_a_call(rt, pipe, depth):
    """8 frames in one call, and 3 + 5 frames in two calls with the seeds split and the reset
    only in the first: the same image and moments, and tile_samples that sum."""
    c = case(21, 13, depth, True, True)
    one = run_converge(pipe, c)
    check(one, want(c), "one call")
    head = run_converge(pipe, c, k=3)
    check(head, want(c, 3), "the first three frames")
    rest = run_converge(pipe, c, k=5, first=3, state=(head.a, head.m), moved=False)
    assert bits_equal(rest.img, one.img)[0] and bits_equal(rest.mom, one.mom)[0]
    assert bits_equal(rest.err, one.err)[0] and (rest.words == one.words).all()
    assert (head.samples + rest.samples == one.samples).all()


@gpu
@pytest.mark.parametrize("frames", CAP_FRAMES)
def test_crossing_the_launch_cap(rt, pipe, frames):
    c = cap_case()
    check(run_converge(pipe, c, k=frames), want(c, frames), f"{frames} frames")


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_camera_outside_the_proven_domain(rt, pipe, depth):
    c = case(24, 16, depth, False, False, False, 6)
    assert not fd.camera_rays_bounded(c.cam, 24, 16, c.sc.spheres)[0]
    check(run_converge(pipe, c), want(c), "outside the domain")


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_band_sets(rt, pipe, depth):
    """rt_converge_frames_bands over ranks 0 and 2 of three ranks' band sets at 24 x 40: the
    rows of the whole image's reference.  An empty band set writes nothing."""
    import torch
    w, h = 24, 40
    c = case(w, h, depth, True, False, True, 6)
    ref = want(c)
    for rank in (0, 2):
        bands = rt.stripe_band_set(h, rank, 3)
        assert bands[2] == (2 if rank == 0 else 1)
        gb = [bands[0] + j * bands[1] for j in range(bands[2])]
        rows = np.concatenate([np.arange(8 * b, 8 * b + 8) for b in gb])
        check(run_converge(pipe, c, bands=bands, rows=rows), ref, f"rank {rank}", rows, gb)
    bufs = [guarded(pipe, 4 * w * 8), guarded(pipe, 4 * w * 8), guarded(pipe, w * 8)]
    words, taken = guarded_words(pipe, 3), guarded_u32(pipe, 3)
    pipe.converge(bufs[0], bufs[1], w, h, c.cam, c.sc, c.seeds, error=bufs[2], tile_mask=words,
                  tile_samples=taken, bands=(0, 1, 0), **PARAMS)
    torch.cuda.synchronize()
    for t in bufs:
        assert (t.cpu().numpy() == F32(SENT)).all(), "an empty band set wrote a buffer"
    assert (words.cpu().numpy() == np.int64(SENT_WORD)).all()
    assert (taken.cpu().numpy() == np.int32(SENT_U32)).all()


@gpu
def test_side_stream_gives_the_same_bits(rt, pipe):
    import torch
    c = case(48, 32, 3, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run_converge(pipe, c)
    side.synchronize()
    check(got, want(c), "on a side stream")


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_following_calls_are_undisturbed(rt, oracle, depth):
    """A following rt_update and a following rt_update_frames on the output match the oracle,
    and rt_last_launch_info is what it was before the call."""
    import torch
    w, h = 24, 16
    c = case(w, h, depth, True, False, True, 6)
    ref = want(c)
    still = ta.make_camera(rt, w, h, depth, True, 500)
    seeds = np.array(rt.frame_seeds(3, 3), F32)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, m = to_dev(p, c.img), to_dev(p, c.mom)
        scratch = p.new_image(w, h)
        p.init_image(scratch, w, h)
        p.update(scratch, a.clone(), w, h, still, c.sc)
        # the context now knows a uniform count of the image the call rewrites
        p.init_image(a, w, h)
        a.copy_(torch.from_numpy(c.img.copy()))
        info = p.last_launch_info()
        p.converge(a, m, w, h, c.cam, c.sc, c.seeds, min_history=c.min_history, **c.params)
        assert p.last_launch_info() == info
        nxt = p.new_image(w, h)
        cam0 = still.with_fields(random_seed=float(seeds[0]))
        p.update(a, nxt, w, h, cam0, c.sc)
        torch.cuda.synchronize()
        assert bits_equal(a.cpu().numpy(), ref.img)[0] and bits_equal(m.cpu().numpy(), ref.mom)[0]
        expect, _ = oracle.update(ref.img, cam0.blob, c.sc.spheres)
        assert bits_equal(nxt.cpu().numpy(), expect)[0], "a following rt_update differs"
        other = p.new_image(w, h)
        newest = p.update_frames(a, other, w, h, still, c.sc, seeds)
        torch.cuda.synchronize()
        chain = fd.oracle_chain(oracle, ref.img, still, c.sc.spheres, seeds)
        got = (a if newest == 0 else other).cpu().numpy()
        assert bits_equal(got, chain[-1])[0], "a following rt_update_frames differs"
    finally:
        p.close()


@gpu
def test_refused_calls_launch_nothing(rt, pipe):
    import torch
    L = rt._lib
    c = case(24, 16, 1, True, False, True, 6)
    w, h = c.w, c.h
    px, tiles = w * h, 6
    image, moments = guarded(pipe, 4 * px), guarded(pipe, 4 * px)
    plane, words, taken = guarded(pipe, px), guarded_words(pipe, tiles), guarded_u32(pipe, tiles)
    cam = c.cam.to_c()
    sp, n = pipe._spheres(c.sc)
    seeds = np.ascontiguousarray(c.seeds, F32)
    SP = ctypes.c_void_p(seeds.ctypes.data)
    A, Z = RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE
    I, M, E, T, S = (t.data_ptr() for t in (image, moments, plane, words, taken))
    band = L.band_sets([(0, 1, 2)])

    def converge(params=(MIN_SAMPLES, ABS2, REL2), bands=None, **kw):
        v = dict(ctx=pipe._ctx, image=I, moments=M, error=E, mask=T, samples=S, w=w, h=h,
                 cam=ctypes.byref(cam), frames=len(seeds), seeds=SP, min_history=MIN_HISTORY)
        v.update(kw)
        pc = L.AdaptiveParamsC(*params) if params is not None else None
        head = (v["ctx"], v["image"], v["moments"], v["error"], v["mask"], v["samples"], v["w"],
                v["h"])
        tail = (v["cam"], sp, n, v["frames"], v["seeds"],
                ctypes.byref(pc) if pc is not None else None, v["min_history"], pipe._stream())
        if bands is None:
            L.call("rt_converge_frames", *head, *tail)
        else:
            L.call("rt_converge_frames_bands", *head, bands[0], *tail)

    rows = {"ctx NULL": (RT_ERR_INVALID_CONTEXT, dict(ctx=None)),
            "image NULL": (A, dict(image=None)), "moments NULL": (A, dict(moments=None)),
            "camera NULL": (A, dict(cam=None)), "params NULL": (A, dict(params=None)),
            "random_seeds NULL": (A, dict(seeds=None)),
            "frames 0": (A, dict(frames=0)), "frames 65537": (A, dict(frames=65537)),
            "min_history 0": (A, dict(min_history=0)),
            "min_history 2^24 + 1": (A, dict(min_history=(1 << 24) + 1)),
            "min_samples 2^24 + 1": (A, dict(params=((1 << 24) + 1, ABS2, REL2))),
            "width 0": (Z, dict(w=0)), "height 0": (Z, dict(h=0)),
            "width 65537": (Z, dict(w=65537)), "height 65537": (Z, dict(h=65537)),
            "bands NULL": (A, dict(bands=(None,))),
            "bands: ctx NULL": (RT_ERR_INVALID_CONTEXT, dict(bands=(band,), ctx=None)),
            "bands past the image": (A, dict(bands=(L.band_sets([(1, 1, 2)]),))),
            "bands: step 0": (A, dict(bands=(L.band_sets([(0, 0, 1)]),)))}
    names = ("image", "moments", "error", "mask", "samples")
    ptrs = dict(zip(names, (I, M, E, T, S)))
    for i, x in enumerate(names):                   # any two of the buffers equal
        for y in names[i + 1:]:
            rows[f"{y} == {x}"] = (A, {y: ptrs[x]})
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf")),
                      ("-inf", float("-inf"))]:
        rows[f"abs_tolerance2 {what}"] = (A, dict(params=(MIN_SAMPLES, bad, REL2)))
        rows[f"rel_tolerance2 {what}"] = (A, dict(params=(MIN_SAMPLES, ABS2, bad)))
    for what, (status, kw) in rows.items():
        with pytest.raises(rt.RtError) as err:
            converge(**kw)
        assert err.value.status == status, what
    torch.cuda.synchronize()
    for t, what in ((image, "image"), (moments, "moments"), (plane, "error")):
        assert (t.cpu().numpy() == F32(SENT)).all(), f"a refused call wrote {what}"
    assert (words.cpu().numpy() == np.int64(SENT_WORD)).all(), "a refused call wrote tile_mask"
    assert (taken.cpu().numpy() == np.int32(SENT_U32)).all(), "a refused call wrote tile_samples"
    with pytest.raises(ValueError):
        pipe.converge(image.cpu(), moments, w, h, c.cam, c.sc, c.seeds)
    with pytest.raises(ValueError):
        pipe.converge(image, moments[:8], w, h, c.cam, c.sc, c.seeds)
    with pytest.raises(ValueError):
        pipe.converge(image, moments, w, h, c.cam, c.sc, c.seeds, error=plane[:1])
    # the ends of the ranges are accepted, and the context still works
    image[:4 * px] = to_dev(pipe, c.img).reshape(-1)
    moments[:4 * px] = to_dev(pipe, c.mom).reshape(-1)
    converge(params=(1 << 24, 0.0, 0.0), min_history=1 << 24, frames=1)
    check(run_converge(pipe, c), want(c), "after the refused calls")
