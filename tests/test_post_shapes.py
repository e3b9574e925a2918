"""The post-processing kernels beyond one workgroup: rt_trace_aov, rt_denoise, rt_reproject,
rt_moments_update and rt_variance_filter at the shapes where their index arithmetic first
matters: interior workgroups in both directions, several tiles per class of rows in the LDS
("rows") route, every tap of steps 32 to 128 on the image in the direct route, and the largest
width and height the headers allow.

Nothing is restated here that another file defines: the references are test_denoise's
`guide_planes` and `denoise_ref`, test_reproject's `reproject_ref` and test_variance's
`moments_ref` and `denoise_guided_ref`, unchanged, and the inputs are made the way those files'
`case` functions make them (the shapes are entered into test_denoise.CASES for that; its own
parametrised lists are fixed when it is imported and do not see them).  Every GPU output is
compared bit for bit (NaN == NaN).

The CPU tests make the GPU tests mean something.  From arithmetic alone they pin the rows
route's launch geometry at each shape, and from the references' inputs they count the kept taps
that cross a workgroup's border, the kept taps 2 * 32, 2 * 64 and 2 * 128 pixels away, and the
reprojection's footprints that lie in another workgroup (printed with -s).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import test_aov as ta
import test_denoise as td
import test_reproject as tr
import test_variance as tv
from conftest import bits_equal

gpu = pytest.mark.gpu

F32 = np.float32
MISS = -1
STEPS = (1, 2, 4, 8, 16)       # the steps of the rows route
LONG = (5, 6, 7)               # the iterations of steps 32, 64 and 128: the direct route
TILE_W, TILE_ROWS = 64, 4      # a filter workgroup: 64 pixels of 4 rows of one class y mod S
REP_W, REP_H = 32, 8           # a reprojection workgroup

# name -> (width, height): why these are the smallest that reach the code is in
# test_launch_geometry and the tests after it
SHAPES = {"grid": (193, 131), "wide": (515, 6), "tall": (6, 515), "maxw": (65536, 1),
          "maxh": (1, 65536)}
# the camera settings of each shape's view, over test_denoise.default_camera's.  `tall` looks
# beside the three large spheres: under the default view they fill the middle of its column and
# no surface is 256 rows high, so step 128 would keep no tap at dy = +-2 (test_long_reach); here
# the ground is rows 109 to 514.
# The extents need views whose pan stays on an image one pixel thick.  `maxw`: the default 20
# degrees of one row are 3.5 units a pixel and 13 pixels of 65536 hit anything; 0.5 degrees give
# 509 hit pixels and, at two silhouettes, footprints that restart.  `maxh`: a camera in the plane
# z = 0 of both look_at points, so the pan is a tilt in that plane and moves the single column
# along itself; it looks down from (8, 10, 0) through 110 degrees, with sky above the far limb of
# the ground and, at the edge the tilt brings in, ground: 937 hit pixels out of range.
CAMERAS = {name: {} for name in SHAPES}
CAMERAS["tall"] = dict(look_at=(0.0, 0.0, 3.0))
CAMERAS["maxw"] = dict(field_of_view=0.5)
CAMERAS["maxh"] = dict(look_from=(8.0, 10.0, 0.0), field_of_view=110.0)
NS = {"grid": (1, 2, 3, 4, 5, 8), "wide": (6, 7, 8), "tall": (6, 7, 8), "maxw": (5, 8),
      "maxh": (5, 8)}          # iterations: each rows step as the last one written, both
#                                parities of the ping-pong after the switch of routes
DENOISE = {name: [td.variant(n, ids) for n in NS[name]
                  for ids in ((True, False) if name == "grid" else (True,))] for name in SHAPES}
GUIDED = {name: [tv.variant(n, ids) for n in NS[name]
                 for ids in ((True, False) if name == "grid" else (True,))] for name in SHAPES}
for _name, (_w, _h) in SHAPES.items():
    td.CASES[_name] = (_w, _h, "n40", CAMERAS[_name], DENOISE[_name],
                       ("off_image", "miss_mismatch", "id_mismatch"))
EXTENTS = ["maxw", "maxh"]
REPROJECTED = ["grid", "maxw", "maxh"]
TWO_MODES = ["grid", "maxw", "maxh"]


def pan(name):
    """test_reproject's PAN from the shape's own view, as a key of test_reproject.view."""
    return tuple(sorted({**CAMERAS[name], **dict(tr.PAN)}.items()))


def material_of(spheres, ids):
    """The material plane of rt_trace_aov from the id plane, as test_reproject.view makes it."""
    material = np.zeros(ids.shape + (4,), F32)
    hit = ids != MISS
    material[hit] = spheres[ids[hit], 4:8]
    material.setflags(write=False)
    return material


@functools.lru_cache(None)
def base_view(name):
    """test_denoise.case(name)'s view in the form of test_reproject.view."""
    c = td.case(name)
    return SimpleNamespace(cam=c.cam, spheres=c.spheres, sphere_id=c.sphere_id, hit=c.hit,
                           normal=c.normal, material=material_of(c.spheres, c.sphere_id))


@functools.lru_cache(None)
def moved(name, what="accumulator"):
    """A reprojection case in test_reproject.case's form: the shape's view, the same view after
    test_reproject's PAN, and as the previous image the accumulator of test_variance.chain's
    FRAMES frames or its moments image."""
    w, h = SHAPES[name]
    acc, mom = tv.chain(name)
    cur = tr.view(w, h, pan(name))
    return SimpleNamespace(name=name, w=w, h=h, prev=base_view(name), cur=cur,
                           sc=td.case(name).sc, normal=cur.normal,
                           prev_rgba=acc[-1] if what == "accumulator" else mom[-1])


@functools.lru_cache(None)
def moved_expected(name, what, var):
    """(reference output, tallies, detail) of one variant of moved(name, what)."""
    c = moved(name, what)
    max_history, lamb, tol2 = var
    counts, detail = {}, {}
    out = tr.reproject_ref(c.prev_rgba, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit,
                           c.normal, c.cur.material, c.prev.cam.blob, max_history, lamb, tol2,
                           counts, detail)
    out.setflags(write=False)
    return out, counts, detail


# ---- launch geometry -------------------------------------------------------------------------------
def rows_grid(w, h, s):
    """The rows route's grid as atrous::launch (csrc/rt_atrous.h) computes it, and per block of
    its y axis the class, the tile and whether the workgroup leaves at once (y0 >= h)."""
    gx = (w + TILE_W - 1) // TILE_W
    gy = s * (((h + s - 1) // s + TILE_ROWS - 1) // TILE_ROWS)
    blocks = []
    for b in range(gy):
        cls, tile = b & (s - 1), b // s
        y0 = cls + s * TILE_ROWS * tile
        blocks.append((cls, tile, y0 >= h))
    return gx, gy, blocks


# step -> (grid.y, {live tiles of a class: classes with that many}, workgroups that exit per
# column block), worked out by hand from rt_denoise_kernel's y0 for 131 rows
GRID_ROWS = {1: (33, {33: 1}, 0), 2: (34, {17: 2}, 0), 4: (36, {9: 3, 8: 1}, 1),
             8: (40, {5: 3, 4: 5}, 5), 16: (48, {3: 3, 2: 13}, 13)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_launch_geometry(name):
    w, h = SHAPES[name]
    seen = {}
    for s in STEPS:
        gx, gy, blocks = rows_grid(w, h, s)
        live = {}
        for cls, tile, exits in blocks:
            live[cls] = live.get(cls, 0) + (not exits)
        hist = {}
        for n in live.values():
            hist[n] = hist.get(n, 0) + 1
        exits = sum(e for _, _, e in blocks)
        both_sides = max(0, gx - 2)
        print(f"{name} {w}x{h} step {s}: grid {gx} x {gy}, live tiles per class "
              f"{dict(sorted(hist.items(), reverse=True))}, exiting workgroups per column block "
              f"{exits}, highest tile {max(t for _, t, e in blocks if not e)}, column blocks "
              f"with a block on both sides {both_sides}")
        assert gx < 65536 and gy < 65536
        # every row is some live workgroup's, once
        rows = sorted(cls + s * (TILE_ROWS * tile + j) for cls, tile, e in blocks if not e
                      for j in range(TILE_ROWS) if cls + s * (TILE_ROWS * tile + j) < h)
        assert rows == list(range(h))
        seen[s] = (gx, gy, hist, exits, blocks)
    direct = ((w + TILE_W - 1) // TILE_W, (h + TILE_ROWS - 1) // TILE_ROWS)
    aov = ((w + 7) // 8, (h + 7) // 8)
    rep = ((w + REP_W - 1) // REP_W, (h + REP_H - 1) // REP_H)
    print(f"{name}: direct route grid {direct}, G-buffer tile columns x bands {aov}, "
          f"reprojection grid {rep}")
    if name == "grid":
        for s in STEPS:
            gx, gy, hist, exits, blocks = seen[s]
            assert (gy, hist, exits) == GRID_ROWS[s], s
            assert gx == 4 and w - TILE_W * (gx - 1) == 1      # blocks 1, 2 interior; 3: one pixel
        assert any(t == 2 and not e for _, t, e in seen[16][4])
        assert {c for c, t, e in seen[16][4] if t == 1 and not e} >= {0, 1, 2}
        assert all(seen[s][3] >= 1 for s in (4, 8, 16))
        assert rep[0] >= 3 and rep[1] >= 3 and aov[0] > 8 and aov[1] >= 3
    if name == "wide":
        assert w >= 4 * 128 + 1 and direct[0] == 9
    if name == "tall":
        assert h >= 4 * 128 + 1 and direct[1] == 129
        assert seen[4][2] == {33: 3, 32: 1}
    if name == "maxw":
        assert seen[16][0] == 1024 and aov[0] == 8192 and rep[0] == 2048
    if name == "maxh":
        assert seen[16][1] == 16384 and direct[1] == 16384 and aov[1] == 8192 and rep[1] == 8192


# ---- the kept taps, from the references' inputs ----------------------------------------------------
def same_surface(c, use_ids, oy, ox):
    """hit[Q] and the mask of the taps Q = P + (ox, oy) no skip rule before the weight's drops."""
    hq, inside = td._shifted(c.hit, oy, ox)
    miss_p = ~(c.hit[..., 3] < np.inf)
    keep = inside & (miss_p == ~(hq[..., 3] < np.inf))
    if use_ids:
        keep = keep & (c.sphere_id == td._shifted(c.sphere_id, oy, ox)[0])
    return hq, keep


def geometry_weight(c, hq, oy, ox, k, npow, ip):
    """(k * wn, 1 + dp * ip) of the headers' weight for the taps at (ox, oy)."""
    one, zero = F32(1.0), F32(0.0)
    miss_p = ~(c.hit[..., 3] < np.inf)
    nq, _ = td._shifted(c.normal, oy, ox)
    dp = np.where(miss_p, zero, td._dist2(c.hit, hq))
    dn = (c.normal[..., 0] * nq[..., 0] + c.normal[..., 1] * nq[..., 1]) \
        + c.normal[..., 2] * nq[..., 2]
    wn = np.fmax(dn, zero)
    for _ in range(npow):
        wn = wn * wn
    wn = np.where(miss_p, one, wn)
    return k * wn, one + dp * F32(ip)


def denoise_kept(name, i, use_ids=True):
    """[(dy, dx, mask of the kept taps)] of iteration i of rt_denoise's default variant on a
    shape: the input of iteration i is the reference's output after i iterations."""
    c = td.case(name)
    _, _, npow, ic0, ip = td.variant()
    col = c.src if i == 0 else td.expected(name, td.variant(i, use_ids))[0]
    s = 1 << i
    taps = []
    with np.errstate(all="ignore"):
        ic = F32(ic0)
        for _ in range(i):
            ic = ic * F32(4.0)
        ic = np.minimum(ic, td.FLT_MAX)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                hq, surface = same_surface(c, use_ids, dy * s, dx * s)
                cq, _ = td._shifted(col, dy * s, dx * s)
                num, den = geometry_weight(c, hq, dy * s, dx * s, td.H5[dy + 2] * td.H5[dx + 2],
                                           npow, ip)
                wgt = num / (den * (F32(1.0) + td._dist2(col, cq) * ic))
                assert wgt.dtype == F32
                taps.append((dy, dx, surface & (wgt > 0)))
    return taps


def guided_kept(name, i, use_ids=True):
    """The same for rt_variance_filter's default variant: image and variance after i iterations."""
    c = tv.case(name)
    _, _, npow, il, ip, mh, fb = tv.variant()
    if i == 0:
        col, v = c.src, tv.initial_variance(c.src, c.moments, mh, fb)[0]
    else:
        col, v, _ = tv.expected(name, tv.variant(i, use_ids))
    s = 1 << i
    taps = []
    with np.errstate(all="ignore"):
        sg = np.zeros(col.shape[:2], F32)
        sgv = np.zeros(col.shape[:2], F32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                g = tv.H3[dy + 1] * tv.H3[dx + 1]
                _, surface = same_surface(c, use_ids, dy * s, dx * s)
                vq, _ = td._shifted(v, dy * s, dx * s)
                sg = np.where(surface, sg + g, sg)
                sgv = np.where(surface, sgv + g * vq, sgv)
        ve = sgv / sg + F32(1e-8)
        lp = tv.lum(col)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                hq, surface = same_surface(c, use_ids, dy * s, dx * s)
                cq, _ = td._shifted(col, dy * s, dx * s)
                num, den = geometry_weight(c, hq, dy * s, dx * s, td.H5[dy + 2] * td.H5[dx + 2],
                                           npow, ip)
                dl = lp - tv.lum(cq)
                wgt = ((num * cq[..., 3]) * ve) / (den * (ve + (dl * dl) * F32(il)))
                assert wgt.dtype == F32
                taps.append((dy, dx, surface & (wgt > 0)))
    return taps


FILTERS = {"rt_denoise": (denoise_kept, td, td.variant), "rt_variance_filter": (guided_kept, tv,
                                                                                tv.variant)}


def kept_of_reference(mod, variant, name, i):
    """The kept taps of iteration i by the reference's own tallies: those of i + 1 iterations
    less those of i."""
    def kept(n):
        if n == 0:
            return 0
        t = mod.expected(name, variant(n))[-1]
        return t["taps"] - t["off_image"] - t["miss_mismatch"] - t["id_mismatch"] - t["weight"]
    return kept(i + 1) - kept(i)


@pytest.mark.parametrize("which", list(FILTERS))
def test_kept_taps_cross_workgroup_borders(which):
    """On `grid`, in every iteration of the rows route: kept taps whose Q is in another 64-column
    block than P, kept taps whose Q is in another tile of P's class of rows, and at step 16
    pixels of the two interior column blocks that keep a tap 32 pixels away on each side."""
    kept_fn, mod, variant = FILTERS[which]
    w, h = SHAPES["grid"]
    yy, xx = np.mgrid[0:h, 0:w]
    for i, s in enumerate(STEPS):
        taps = kept_fn("grid", i)
        total = sum(int(k.sum()) for _, _, k in taps)
        assert total == kept_of_reference(mod, variant, "grid", i), \
            "this file's count of the kept taps is not the reference's"
        other_block = other_tile = 0
        far = {-2: np.zeros((h, w), bool), 2: np.zeros((h, w), bool)}
        for dy, dx, keep in taps:
            other_block += int((keep & ((xx + dx * s) // TILE_W != xx // TILE_W)).sum())
            other_tile += int((keep & ((yy + dy * s) // (TILE_ROWS * s)
                                       != yy // (TILE_ROWS * s))).sum())
            if dx in far:
                far[dx] |= keep
        interior = (xx // TILE_W >= 1) & (xx // TILE_W <= 2)
        both = int((interior & far[-2] & far[2]).sum())
        print(f"{which} grid step {s}: {total} kept taps, {other_block} into another column "
              f"block, {other_tile} into another tile of the class, {both} pixels of blocks 1-2 "
              f"with a kept tap at dx = -2 and at dx = +2")
        assert other_block >= 1 and other_tile >= 1
        if s == 16:
            assert both >= 1


@pytest.mark.parametrize("which", list(FILTERS))
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_long_reach(name, which):
    """Steps 32, 64 and 128 (iterations 5 to 7, the direct route) keep taps 2 steps away on
    each side along the shape's long axis."""
    kept_fn, mod, variant = FILTERS[which]
    for i in LONG:
        taps = kept_fn(name, i)
        assert sum(int(k.sum()) for _, _, k in taps) == kept_of_reference(mod, variant, name, i)
        side = {-2: 0, 2: 0}
        for dy, dx, keep in taps:
            d = dx if name == "wide" else dy
            if d in side:
                side[d] += int(keep.sum())
        axis = "dx" if name == "wide" else "dy"
        print(f"{which} {name} step {1 << i}: kept taps at {axis} = -2: {side[-2]}, "
              f"at {axis} = +2: {side[2]}")
        assert side[-2] >= 1 and side[2] >= 1


@pytest.mark.parametrize("name", EXTENTS)
def test_extents_have_something_to_filter(name):
    c = td.case(name)
    w, h = SHAPES[name]
    miss = c.sphere_id == MISS
    print(f"{name}: {int((~miss).sum())} hit pixels, {int(miss.sum())} miss")
    assert miss.any() and not miss.all()
    for which, (kept_fn, mod, variant) in FILTERS.items():
        src = (td.case(name) if mod is td else tv.case(name)).src
        res = mod.expected(name, variant())
        out, n = res[0], res[-1]
        changed = int((out[..., :3] != src[..., :3]).any(-1).sum())
        print(f"{which} {name}: off-image {n['off_image']}, hit/miss mismatch "
              f"{n['miss_mismatch']}, id mismatch {n['id_mismatch']}, {changed} pixels changed")
        assert n["off_image"] >= 1 and n["miss_mismatch"] + n["id_mismatch"] >= 1
        assert changed >= 1
        end = [(dy, dx) for dy, dx, keep in kept_fn(name, 0)
               if (dy, dx) != (0, 0) and keep[h - 1, w - 1]]
        print(f"{which} {name}: pixel ({w - 1}, {h - 1}) keeps the taps (dy, dx) {end}")
        assert end


def previous_footprint(c):
    """(x0, y0) of each pixel's 2 x 2 footprint in the previous view: rt_reproject.h's projection
    with reproject_ref's operations (meaningful where the reference kept a tap)."""
    basis, ok = tr.reproject_basis_ref(c.prev.cam.blob)
    assert ok
    with np.errstate(all="ignore"):
        q = c.cur.hit[..., :3] - np.asarray(c.prev.cam.blob, F32)[0:3]
        a, b, d = (tr._dot3(basis[3 * k:3 * k + 3], q) for k in range(3))
        px, py = a / d - F32(0.5), b / d - F32(0.5)
        assert px.dtype == F32
        return np.floor(px), np.floor(py)


@pytest.mark.parametrize("name", REPROJECTED)
def test_reprojection_reaches_its_rules(name):
    """Per shape: pixels that keep every tap that can be on the image (four; two on an image one
    pixel thick, where the other two are off it), taps off the image, restarted pixels; on `grid`
    a four-tap footprint wholly in another workgroup than its pixel, for a pixel of an interior
    workgroup."""
    c = moved(name)
    w, h = SHAPES[name]
    for var in tr.BOTH:
        out, n, detail = moved_expected(name, "accumulator", var)
        hits = c.cur.sphere_id != MISS
        restarted = int((hits & (out[..., 3] == 0)).sum())
        most = 4 if min(w, h) > 1 else 2
        full = detail["kept"] == most
        print(f"{tr._id((name, var))}: " + ", ".join(f"{k} {n[k]}" for k in tr.TALLIES)
              + f"; {int(full.sum())} pixels keep {most} taps, {restarted} hit pixels restart")
        assert int(detail["kept"].max()) == most and full.any()
        assert n["off_image"] >= 1
        # a miss restarts too, and with lambertian_only every specular pixel: ask for a pixel
        # that hits a sphere and restarts for what the previous view holds
        if not var[1]:
            assert restarted == n["none"] + n["behind"] + n["out_of_range"] and restarted >= 1
        assert (out[..., 3] > 0).sum() == n["four"] + n["some"]
        if name != "grid":
            continue
        fx, fy = previous_footprint(c)
        yy, xx = np.mgrid[0:h, 0:w]
        gx, gy = (w + REP_W - 1) // REP_W, (h + REP_H - 1) // REP_H
        bx, by = xx // REP_W, yy // REP_H
        interior = (bx > 0) & (bx < gx - 1) & (by > 0) & (by < gy - 1)
        elsewhere = np.ones((h, w), bool)
        for j in (0, 1):
            for i in (0, 1):
                elsewhere &= ((fx + i) // REP_W != bx) | ((fy + j) // REP_H != by)
        far = int((full & interior & elsewhere).sum())
        print(f"{tr._id((name, var))}: {far} four-tap pixels of interior workgroups whose "
              f"footprint is in other workgroups")
        assert far >= 1
    mom, n, _ = moved_expected(name, "moments", tr.BOTH[0])
    assert n["four" if most == 4 else "some"] >= 1 and (mom[..., 3] > 0).any()


# ---- GPU side --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


@pytest.fixture(params=tv.ROUTES, ids=["rows", "direct"])
def route(request, monkeypatch):
    monkeypatch.delenv("RT_DENOISE_ROUTE", raising=False)
    if request.param:
        monkeypatch.setenv("RT_DENOISE_ROUTE", request.param)
    return request.param


def _did(v):
    return td._id(v).split("-p")[0]


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_gbuffer_matches_reference(rt, pipe, name):
    """All four planes from guarded buffers; both scan modes on `grid` and the extents; on
    `maxh` the round-robin bands of rank 1 of 3 against the whole image's rows."""
    c = td.case(name)
    want = {"sphere_id": c.sphere_id, "hit": c.hit, "normal": c.normal,
            "material": base_view(name).material}
    try:
        for mode in ta.MODES if name in TWO_MODES else ta.MODES[:1]:
            pipe.set_scan_mode(mode)
            assert not ta.differences(ta.trace(pipe, c), want, f"{mode} ")
            if name != "maxh":
                continue
            first, step, count = rt.stripe_band_set(c.h, 1, 3)
            assert (first, step, count) == (1, 3, 2731)
            got = ta.trace(pipe, c, bands=(first, step, count), rows=8 * count)
            rows = {k: v.reshape((c.h // 8, 8) + v.shape[1:])[first::step]
                    for k, v in want.items()}
            local = {k: v.reshape(rows[k].shape) for k, v in got.items()}
            assert not ta.differences(local, rows, f"{mode}, bands of rank 1 of 3 ")
    finally:
        pipe.set_scan_mode(ta.MODES[0])


@gpu
@pytest.mark.parametrize("v", [(name, var) for name in SHAPES for var in DENOISE[name]], ids=_did)
def test_denoise_matches_reference(rt, pipe, route, v):
    name, var = v
    c = td.case(name)
    td.check(td.run(rt, pipe, c, var), c, name, var)


@gpu
@pytest.mark.parametrize("v", [(name, var) for name in SHAPES for var in GUIDED[name]],
                         ids=lambda v: tv._id(v).split("-p")[0])
def test_variance_filter_matches_reference(rt, pipe, route, v):
    """Image and variance; tv.run also checks the buffer tails and that no input is written."""
    name, var = v
    got, variance = tv.run(rt, pipe, tv.case(name), var)
    tv.check(got, variance, name, var)


@gpu
@pytest.mark.parametrize("name", ["grid", "maxh"])
def test_moments_match_reference(rt, pipe, name):
    """test_variance's chain of FRAMES in-place updates, each compared, at these shapes."""
    import torch
    acc, mom = tv.chain(name)
    w, h = SHAPES[name]
    px = 4 * w * h
    m = tv.guarded(pipe, px, np.zeros(px, F32))
    for k in range(1, len(acc)):
        a, b = tv.guarded(pipe, px, acc[k - 1]), tv.guarded(pipe, px, acc[k])
        tv.raw_moments(rt, pipe, pipe._ctx, a.data_ptr(), b.data_ptr(), m.data_ptr(), w, h)
        torch.cuda.synchronize()
        got = tv.tail_intact(m, px, "moments").reshape(h, w, 4)
        assert bits_equal(got, mom[k])[0], f"frame {k}"
        assert bits_equal(tv.tail_intact(a, px, "in"), acc[k - 1].reshape(-1))[0], "in was written"
        assert bits_equal(tv.tail_intact(b, px, "out"), acc[k].reshape(-1))[0], "out was written"


@gpu
@pytest.mark.parametrize("var", tr.BOTH, ids=["all", "lambertian"])
@pytest.mark.parametrize("what", ["accumulator", "moments"])
@pytest.mark.parametrize("name", REPROJECTED)
def test_reproject_matches_reference(rt, pipe, name, what, var):
    """tr.run also checks dst's tail and that the previous image and the planes are not written."""
    want, _, _ = moved_expected(name, what, var)
    same, bad = bits_equal(tr.run(rt, pipe, moved(name, what), var), want)
    assert same, f"{name} {what} {var}: {bad} values differ from the reference"


@gpu
def test_pipeline_matches_the_chain_of_references_on_grid(rt, oracle, pipe, route):
    """test_variance's chained run at `grid`, with the planes the GPU traces for both views: 4
    frames of update + moments_update, reproject of the accumulator and of the moments after the
    pan, one more update + moments_update, denoise_guided; against the oracle's update,
    moments_ref, reproject_ref and denoise_guided_ref chained the same way."""
    import torch
    c = moved("grid")
    w, h = c.w, c.h
    seeds = rt.frame_seeds(21, 5)
    cams = tv._frame_cams(c.prev.cam, seeds[:4])
    after = c.cur.cam.with_fields(random_seed=float(seeds[4]), camera_has_moved=0.0)
    # the CPU chain
    acc = mom = np.zeros((h, w, 4), F32)
    for cam in cams:
        new, _ = oracle.update(acc, cam.blob, c.prev.spheres)
        mom, acc = tv.moments_ref(acc, new, mom), new
    planes = (c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit, c.normal, c.cur.material,
              c.prev.cam.blob, 64, 1, 1e-5)
    rep, rep_m = tr.reproject_ref(acc, *planes), tr.reproject_ref(mom, *planes)
    want_acc, _ = oracle.update(rep, after.blob, c.cur.spheres)
    tally = {}
    want_m = tv.moments_ref(rep, want_acc, rep_m, tally)
    assert tally["first"] >= 1 and tally["consecutive"] >= 1
    n, npow, il, ip, mh, fb = tv.DEFAULTS
    want, want_v = tv.denoise_guided_ref(want_acc, want_m, c.cur.hit, c.normal, c.cur.sphere_id,
                                         n, npow, il, ip, mh, fb)
    # the GPU chain
    prev_guides = pipe.trace_aov(w, h, c.prev.cam, c.sc, planes=("sphere_id", "hit"))
    guides = pipe.trace_aov(w, h, c.cur.cam, c.sc)
    a, b, m = pipe.new_image(w, h), pipe.new_image(w, h), pipe.new_image(w, h)
    for cam in cams:
        pipe.update(a, b, w, h, cam, c.sc)
        pipe.moments_update(a, b, m, w, h)
        a, b = b, a
    rep_g = pipe.reproject(a, w, h, c.prev.cam, prev_guides, guides)
    rep_mg = pipe.reproject(m, w, h, c.prev.cam, prev_guides, guides)
    pipe.update(rep_g, b, w, h, after, c.sc)
    pipe.moments_update(rep_g, b, rep_mg, w, h)
    out, variance = pipe.denoise_guided(b, w, h, guides, rep_mg)
    torch.cuda.synchronize()
    assert (guides["sphere_id"].cpu().numpy() == c.cur.sphere_id).all()
    assert bits_equal(rep_g.cpu().numpy(), rep)[0], "the reprojected accumulator differs"
    assert bits_equal(b.cpu().numpy(), want_acc)[0], "the accumulator differs"
    assert bits_equal(rep_mg.cpu().numpy(), want_m)[0], "the moments differ"
    assert bits_equal(out.cpu().numpy(), want)[0], "the filtered image differs"
    assert bits_equal(variance.cpu().numpy(), want_v)[0], "the variance differs"
