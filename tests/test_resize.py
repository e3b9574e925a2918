"""Carrying the accumulator across image sizes (include/rt_resize.h): rt_resize_carry,
rt_resize_params_default.

The reference is in this file: `resize_ref`, a vectorised NumPy float32 restatement of the
header's per-pixel text that also tallies how often each rule fires.  Views, accumulators, the
basis and the equal-size reference come from tests/test_reproject.py by import (`tr.view` takes
its own size, so a 19 x 11 and a 37 x 21 view of one pose differ slightly in aspect ratio: the
ratio between the sizes is not an integer, which is wanted); the miss directions are
test_denoise's centre ray.  Every GPU output is compared bit for bit (NaN == NaN).

The CPU tests check the boundary, the equal-size identity with test_reproject's reference, count
from the reference alone that every case reaches the rules it is there for (printed with -s),
and check two strict inequalities against a 512-sample render: carrying up beats copying texels,
and carrying down beats the native accumulator of the same sample count.
"""
import ctypes
import functools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import test_denoise as td
import test_post_shapes as tps
import test_reproject as tr
from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_resize.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
W, H = 37, 21                  # the current size of the named cases (test_reproject's)
MISS = -1
NONE, NEAREST = 0, 1           # RT_RESIZE_FILL_*
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
SENT = tr.SENT
TAIL = tr.TAIL                 # 64 bytes of sentinel after each dst
DECLARED = ["rt_resize_params_default", "rt_resize_carry"]
TALLIES = ("miss", "zeroed", "not_projected", "sky_kept", "surface_kept", "four", "partial",
           "hole", "filled", "filled_ineligible", "capped")


# ---- the reference ---------------------------------------------------------------------------------
def miss_offsets(blob, w, h):
    """q of rule 3 for a miss, for every pixel: test_denoise.centre_ray's direction (its two
    fmaf per component, libm's, and the subtraction of the centre), vectorised."""
    fmaf = np.frompyfunc(td._fmaf(), 3, 1)
    b = np.asarray(blob, F32)
    o, vul, pdu, pdv = b[0:3], b[4:7], b[8:11], b[12:15]
    sx = (np.arange(w, dtype=F32) + F32(0.5))[None, :]
    sy = (np.arange(h, dtype=F32) + F32(0.5))[:, None]
    q = np.empty((h, w, 3), F32)
    for k in range(3):
        inner = fmaf(sx, pdu[k], vul[k]).astype(F32)
        pc = fmaf(sy, pdv[k], inner).astype(F32)
        q[..., k] = pc - o[k]
    return q


def resize_ref(prev, prev_ids, prev_hit, ids, hit, normal, material, prev_blob, blob, max_history,
               lambertian_only, tol2, sky, fill, counts=None, detail=None):
    """rt_resize.h's per-pixel text.  prev, prev_ids and prev_hit are (ph, pw, .) arrays, the
    others (h, w, .); blob is the current camera (used for a miss).  `counts` receives TALLIES;
    `detail` receives "used" (previous texels some kept tap read), "kept" (kept taps per pixel),
    "filled" (the pixels rule 6 filled) and "source" (the (Y, X) each pixel's fill would read)."""
    prev = np.ascontiguousarray(prev, F32)
    prev_hit = np.ascontiguousarray(prev_hit, F32)
    hit = np.ascontiguousarray(hit, F32)
    normal = np.ascontiguousarray(normal, F32)
    h, w = ids.shape
    ph, pw = prev_ids.shape
    basis, ok = tr.reproject_basis_ref(prev_blob)
    assert ok
    r0, r1, r2 = basis[0:3], basis[3:6], basis[6:9]
    o = np.asarray(prev_blob, F32)[0:3]
    one, half = F32(1.0), F32(0.5)
    tally = dict.fromkeys(TALLIES, 0)
    with np.errstate(all="ignore"):
        surface = ids != MISS
        if lambertian_only:
            lamb = np.ascontiguousarray(material, F32)[..., 3] < F32(-1.0)
        else:
            lamb = np.ones((h, w), bool)
        eligible = np.where(surface, lamb, bool(sky))                   # rule 1
        want = eligible | bool(fill)                                    # rule 2
        tally["miss"] = int((~surface).sum())
        tally["zeroed"] = int((~want).sum())
        p, nP = hit[..., :3], normal[..., :3]
        q = p - o                                                       # rule 3
        if (want & ~surface).any():
            q = np.where(surface[..., None], q, miss_offsets(blob, w, h))
        a, b, c = tr._dot3(r0, q), tr._dot3(r1, q), tr._dot3(r2, q)     # rule 4
        px, py = a / c - half, b / c - half
        assert px.dtype == F32 and c.dtype == F32
        projected = (c > 0) & (px >= -1) & (px < F32(pw)) & (py >= -1) & (py < F32(ph))
        tally["not_projected"] = int((want & ~projected).sum())
        live = eligible & projected
        seen = want & projected
        fx, fy = np.floor(px), np.floor(py)
        tx, ty = px - fx, py - fy
        x0 = np.where(seen, fx, 0).astype(np.int64)
        y0 = np.where(seen, fy, 0).astype(np.int64)
        r2q = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        lim = F32(tol2) * r2q
        sw = np.zeros((h, w), F32)
        acc = np.zeros((h, w, 3), F32)
        n = np.full((h, w), np.inf, F32)
        kept = np.zeros((h, w), np.int64)
        used = np.zeros((ph, pw), bool)
        for j in (0, 1):                                                # rule 5
            for i in (0, 1):
                X, Y = x0 + i, y0 + j
                bw = (ty if j else one - ty) * (tx if i else one - tx)
                on = (X >= 0) & (X < pw) & (Y >= 0) & (Y < ph)
                Xc, Yc = np.clip(X, 0, pw - 1), np.clip(Y, 0, ph - 1)
                e = p - prev_hit[Yc, Xc, :3]
                dl = tr._dot3(nP.transpose(2, 0, 1), e)
                match = np.where(surface, (prev_ids[Yc, Xc] == ids) & (dl * dl <= lim),
                                 prev_ids[Yc, Xc] == MISS)
                pc = prev[Yc, Xc]
                assert bw.dtype == F32 and dl.dtype == F32 and lim.dtype == F32
                keep = live & on & match & (pc[..., 3] > 0) & (bw > 0)
                sw = np.where(keep, sw + bw, sw)
                acc = np.where(keep[..., None], acc + bw[..., None] * pc[..., :3], acc)
                n = np.where(keep, np.minimum(n, pc[..., 3]), n)
                kept += keep
                used[Yc[keep], Xc[keep]] = True
        got = kept > 0
        hole = seen & ~got                                              # rule 6
        filled = hole if fill else np.zeros((h, w), bool)
        NX = np.clip(np.where(seen, np.floor(px + half), 0).astype(np.int64), 0, pw - 1)
        NY = np.clip(np.where(seen, np.floor(py + half), 0).astype(np.int64), 0, ph - 1)
        out = np.zeros((h, w, 4), F32)
        out[..., :3] = np.where(got[..., None], acc / sw[..., None],
                                np.where(filled[..., None], prev[NY, NX, :3], F32(0.0)))
        out[..., 3] = np.where(got, np.minimum(n, F32(max_history)), F32(0.0))
        assert sw.dtype == F32 and acc.dtype == F32 and n.dtype == F32
        tally["sky_kept"] = int((got & ~surface).sum())
        tally["surface_kept"] = int((got & surface).sum())
        tally["four"] = int((kept == 4).sum())
        tally["partial"] = int(((kept >= 1) & (kept <= 3)).sum())
        tally["hole"] = int(hole.sum())
        tally["filled"] = int(filled.sum())
        tally["filled_ineligible"] = int((filled & ~eligible).sum())
        tally["capped"] = int((got & (n > F32(max_history))).sum())
    if counts is not None:
        counts.update(tally)
    if detail is not None:
        detail.update(used=used, kept=kept, filled=filled, source=(NY, NX), surface=surface)
    return out


# ---- cases -----------------------------------------------------------------------------------------
def variant(max_history=64, lamb=0, tol2=1e-5, sky=1, fill=NONE):
    return (max_history, lamb, tol2, sky, fill)


def both(**kw):
    return [variant(lamb=0, **kw), variant(lamb=1, **kw)]


SMALL = (19, 11)
# name -> (previous size, previous move, current size, current move, variants)
CASES = {
    "up2": (SMALL, tr.BASE, (W, H), tr.BASE, both()),
    "up2_fill": (SMALL, tr.BASE, (W, H), tr.BASE, both(fill=NEAREST)),
    "turn": (SMALL, tr.BASE, (W, H), tr.TURN, both(fill=NEAREST)),
    "behind": (SMALL, tr.AWAY, (W, H), tr.BASE, both() + both(fill=NEAREST)),
    "from1x1": ((1, 1), tr.BASE, (W, H), tr.BASE, both(fill=NEAREST)),
    "down2": ((74, 42), tr.BASE, (W, H), tr.BASE, both()),
    "cap": (SMALL, tr.BASE, (W, H), tr.BASE, both(max_history=8)),
    "sky0": (SMALL, tr.BASE, (W, H), tr.BASE, both(sky=0)),
    "specular": (SMALL, tr.BASE, (W, H), tr.BASE, [variant(lamb=1, fill=NEAREST),
                                                  variant(lamb=1, sky=0, fill=NEAREST)]),
    "nonfinite": (SMALL, tr.BASE, (W, H), tr.BASE, both(fill=NEAREST)),
}
# Sizes around the kernel's 32 x 8 workgroup of 2 x 2 waves of 16 x 4: test_reproject's, each
# from half its size (rounded up), two of them also from twice their size, and one shape whose
# footprints lie beyond a workgroup's reach (test_post_shapes' `grid`).
SIZE_VARIANTS = both(fill=NEAREST)
SHAPE_CASES = []
for _w, _h in tr.SIZES:
    SHAPE_CASES.append((((_w + 1) // 2, (_h + 1) // 2), (_w, _h)))
for _w, _h in ((33, 9), (65, 5)):
    SHAPE_CASES.append(((2 * _w, 2 * _h), (_w, _h)))
for _prev, _cur in SHAPE_CASES:
    CASES["%dx%d<-%dx%d" % (_cur + _prev)] = (_prev, tr.BASE, _cur, tr.PAN, SIZE_VARIANTS)
GRID = "193x131<-97x66"
STRIPS = {"65536x1<-32768x1": "maxw", "1x65536<-1x32768": "maxh"}


def _key(settings):
    return tuple(sorted(settings.items()))


@functools.lru_cache(None)
def views(name):
    """(previous view, current view, previous accumulator) of a case, read-only and shared."""
    if name == GRID:
        cur = tps.moved("grid").cur                        # tr.view(193, 131, the pan)
        return tr.view(97, 66, tr.BASE), cur, tr.accumulator(97, 66, tr.BASE)
    if name in STRIPS:
        shape = STRIPS[name]
        w, h = tps.SHAPES[shape]
        pw, ph = (w + 1) // 2, (h + 1) // 2
        base = _key(tps.CAMERAS[shape])
        return (tr.view(pw, ph, base), tr.view(w, h, tps.pan(shape)),
                tr.accumulator(pw, ph, base))
    (pw, ph), pmove, (w, h), cmove, _ = CASES[name]
    return tr.view(pw, ph, pmove), tr.view(w, h, cmove), tr.accumulator(pw, ph, pmove)


def variants_of(name):
    return SIZE_VARIANTS if name == GRID or name in STRIPS else CASES[name][4]


def _planted(pv, cv, prev):
    """nonfinite: NaN, +inf and -inf in the green of three previous texels that kept taps read,
    a NaN in the green of another texel that a fill reads, and a NaN in the normal of a
    Lambertian pixel that keeps four taps; chosen from the unmodified case so that both
    lambertian_only values reach them (a hole with lambertian_only 0 is filled with 1 too, and
    a tap kept with 1 is kept with 0 too)."""
    holes, detail = {}, {}
    for lamb, into in ((0, holes), (1, detail)):
        resize_ref(prev, pv.sphere_id, pv.hit, cv.sphere_id, cv.hit, cv.normal, cv.material,
                   pv.cam.blob, cv.cam.blob, 64, lamb, 1e-5, 1, NEAREST, detail=into)
    fy, fx = np.nonzero(holes["filled"])
    assert fy.size >= 1
    NY, NX = holes["source"]
    k = fy.size // 2
    fill_spot = (int(NY[fy[k], fx[k]]), int(NX[fy[k], fx[k]]))
    ys, xs = np.nonzero(detail["used"])
    spots = [(int(y), int(x)) for y, x in zip(ys, xs) if (int(y), int(x)) != fill_spot]
    assert len(spots) >= 30
    spots = [spots[len(spots) // 4], spots[len(spots) // 2], spots[3 * len(spots) // 4]]
    qy, qx = np.nonzero((detail["kept"] == 4) & detail["surface"])
    assert qy.size >= 1
    planted = dict(zip(spots, (np.nan, np.inf, -np.inf)))
    planted[fill_spot] = np.nan
    return planted, fill_spot, (int(qy[qy.size // 2]), int(qx[qx.size // 2]))


@functools.lru_cache(None)
def case(name):
    """A case's inputs (read-only arrays), computed once and shared."""
    import gpu_ray_tracing as rt
    pv, cv, prev = views(name)
    ph, pw = pv.sphere_id.shape
    h, w = cv.sphere_id.shape
    c = SimpleNamespace(name=name, pw=pw, ph=ph, w=w, h=h, prev=pv, cur=cv, normal=cv.normal,
                        sc=rt.SphereCollection(cv.spheres), planted=None, fill_spot=None,
                        nan_normal=None)
    if name == "nonfinite":
        c.planted, c.fill_spot, c.nan_normal = _planted(pv, cv, prev)
        prev = prev.copy()
        for (y, x), v in c.planted.items():
            prev[y, x, 1] = v
        c.normal = cv.normal.copy()
        c.normal[c.nan_normal][0] = np.nan
    for a in (prev, c.normal):
        a.setflags(write=False)
    c.prev_rgba = prev
    return c


def reference(c, image, var, counts=None, detail=None):
    max_history, lamb, tol2, sky, fill = var
    return resize_ref(image, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit, c.normal,
                      c.cur.material, c.prev.cam.blob, c.cur.cam.blob, max_history, lamb, tol2,
                      sky, fill, counts, detail)


@functools.lru_cache(None)
def expected(name, var):
    """(reference output, its tallies) of one variant of a case."""
    counts = {}
    out = reference(case(name), case(name).prev_rgba, var, counts)
    out.setflags(write=False)
    return out, counts


def second_image(c):
    """A second previous image (a moments image, say) whose alphas differ from the first's:
    zeros, counts above every max_history used here, and the first's count elsewhere."""
    second = (c.prev_rgba * F32(0.5) + F32(0.125)).astype(F32)
    second[..., 3] = c.prev_rgba[..., 3]
    second[::3, ::2, 3] = 0.0
    second[1::3, 1::2, 3] = 100.0
    second.setflags(write=False)
    return second


ALL = [(name, var) for name in CASES for var in CASES[name][4]]
LARGE = [(name, var) for name in (GRID, *STRIPS) for var in SIZE_VARIANTS]


def _id(v):
    name, (max_history, lamb, tol2, sky, fill) = v
    return (f"{name}-h{max_history}-{'lambertian' if lamb else 'all'}-sky{sky}-"
            f"{'nearest' if fill else 'nofill'}")


def _line(name, var, n):
    return f"{_id((name, var))}: " + ", ".join(f"{k} {n[k]}" for k in TALLIES)


# ---- CPU tests -------------------------------------------------------------------------------------
def test_library_exports_the_resize_entry_points(rt):
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", HEADER.read_text(), flags=re.M)
    assert declared == DECLARED
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert {s for s in exported if s.startswith("rt_resize_")} == set(declared)
    L = rt._lib
    assert L.resize_symbols() == declared
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.occlusion_symbols(), L.certain_symbols(), L.tile_lists_symbols(),
                  L.selftest_roots_symbols(), L.denoise_symbols(), L.reproject_symbols(),
                  L.variance_symbols(), L.adaptive_symbols(), L.converge_symbols(),
                  L.progress_symbols(), L.edit_symbols(), L.matte_symbols(), L.query_symbols()):
        assert not set(declared) & set(other)
    # no name trips the filters the other boundaries' tests apply to the exported names
    for s in declared:
        assert not any(k in s for k in ("reproject", "aov", "denoise", "variance", "moments",
                                        "adaptive", "converge", "progress"))
        assert not s.startswith(("rt_edit_", "rt_matte_"))
    assert L.lib().rt_abi_version() == 7
    assert ctypes.sizeof(L.ResizeParamsC) == 32 and ctypes.sizeof(L.ResizeImagesC) == 32
    assert [f for f, _ in L.ResizeParamsC._fields_] == [
        "max_history", "lambertian_only", "position_tolerance2", "sky", "fill", "_reserved"]
    assert [f for f, _ in L.ResizeImagesC._fields_] == [
        "prev_rgba", "dst_rgba", "prev_second", "dst_second"]
    p = L.ResizeParamsC(99, 99, -1.0, 99, 99, (9, 9, 9))
    L.lib().rt_resize_params_default(ctypes.byref(p))
    assert (p.max_history, p.lambertian_only, p.sky, p.fill) == (64, 1, 0, NONE)
    assert list(p._reserved) == [0, 0, 0] and F32(p.position_tolerance2) == F32(1e-5)
    L.lib().rt_resize_params_default(None)                      # a no-op, not a crash
    assert (rt.RESIZE_FILL_NONE, rt.RESIZE_FILL_NEAREST) == (NONE, NEAREST)
    text = HEADER.read_text()
    assert re.search(r"#define RT_RESIZE_FILL_NONE\s+0u", text)
    assert re.search(r"#define RT_RESIZE_FILL_NEAREST\s+1u", text)


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "rt_resize.h"\n'
                   "typedef char params_are_32_bytes[sizeof(rt_resize_params) == 32 ? 1 : -1];\n"
                   "typedef char images_are_32_bytes[sizeof(rt_resize_images) == 32 ? 1 : -1];\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_miss_offsets_are_the_centre_rays():
    for move in (tr.BASE, tr.TURN):
        blob = tr.view(W, H, move).cam.blob
        q = miss_offsets(blob, W, H)
        want = np.array([[td.centre_ray(blob, x, y)[3:6] for x in range(W)] for y in range(H)])
        assert bits_equal(q, want)[0]


@pytest.mark.parametrize("name", ["pan", "nonfinite"])
@pytest.mark.parametrize("lamb", [0, 1])
def test_equal_sizes_give_the_reprojection_reference(name, lamb):
    """prev size == size, sky 0, fill NONE: rt_reproject.h's text, bit for bit."""
    c = tr.case(name)
    args = (c.prev_rgba, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit, c.normal,
            c.cur.material, c.prev.cam.blob)
    want = tr.reproject_ref(*args, 64, lamb, 1e-5)
    got = resize_ref(*args, c.cur.cam.blob, 64, lamb, 1e-5, 0, NONE)
    assert (want[..., 3] > 0).sum() >= 50
    assert bits_equal(got, want)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_rules(name):
    c = case(name)
    per = {}
    for var in CASES[name][4]:
        out, n = expected(name, var)
        per[var] = n
        print(_line(name, var, n))
        max_history, lamb, tol2, sky, fill = var
        pixels = c.w * c.h
        assert n["four"] + n["partial"] == n["sky_kept"] + n["surface_kept"]
        assert n["zeroed"] + n["not_projected"] + n["hole"] + n["four"] + n["partial"] == pixels
        assert int((out[..., 3] > 0).sum()) == n["four"] + n["partial"]
        assert n["filled"] == (n["hole"] if fill else 0)
        if not fill:
            assert not out[out[..., 3] == 0].any()
    every, lambertian = (per[v] for v in CASES[name][4][:2])
    if name == "up2":
        for k in ("sky_kept", "surface_kept", "four", "partial", "hole"):
            assert every[k] > 0, k
        assert every["zeroed"] == 0 and lambertian["zeroed"] > 0
    if name == "up2_fill":
        assert every["filled"] > 0 and lambertian["filled_ineligible"] > 0
    if name == "turn":
        assert every["not_projected"] > 0 and every["filled"] > 0
        assert every["sky_kept"] > 0 and every["surface_kept"] > 0
    if name == "behind":
        for var, n in per.items():
            assert n["not_projected"] + n["zeroed"] == c.w * c.h
            assert not expected(name, var)[0].any()
        assert every["not_projected"] == c.w * c.h
    if name == "from1x1":
        assert every["filled"] > 700
    if name == "down2":
        assert every["four"] > 0
    if name == "cap":
        assert every["capped"] > 0 and lambertian["capped"] > 0
        assert expected(name, CASES[name][4][0])[0][..., 3].max() == 8.0
    if name == "sky0":
        out, n = expected(name, CASES[name][4][0])
        assert n["miss"] > 0 and n["zeroed"] == n["miss"] and n["sky_kept"] == 0
        assert not out[c.cur.sphere_id == MISS].any()
    if name == "specular":
        lamb_sky, lamb_nosky = per[CASES[name][4][0]], per[CASES[name][4][1]]
        spec = int(((c.cur.sphere_id != MISS) & ~(c.cur.material[..., 3] < -1)).sum())
        assert spec > 0 and lamb_sky["filled_ineligible"] >= 1
        # without sky the misses are filled too: they are ineligible, not zeroed
        assert lamb_nosky["zeroed"] == 0
        assert lamb_nosky["filled_ineligible"] > lamb_sky["filled_ineligible"]
        out, _ = expected(name, CASES[name][4][0])
        detail = {}
        reference(c, c.prev_rgba, CASES[name][4][0], detail=detail)
        shown = detail["filled"] & (c.cur.sphere_id != MISS) & ~(c.cur.material[..., 3] < -1)
        assert shown.any() and out[shown][:, :3].any() and not out[shown][:, 3].any()
    if "<-" in name:
        assert every["four"] + every["partial"] > 0 or c.pw * c.ph == 1


def test_nonfinite_colours_propagate_fill_and_a_nan_normal_makes_a_hole():
    c = case("nonfinite")
    plain = case("up2_fill")
    for var in CASES["nonfinite"][4]:
        out, _ = expected("nonfinite", var)
        clean, _ = expected("up2_fill", var)
        assert np.isnan(out[..., 1]).any() and np.isinf(out[..., 1]).any()
        assert np.isfinite(out[..., (0, 2, 3)]).all()           # only green is planted
        detail = {}
        reference(plain, plain.prev_rgba, var, detail=detail)
        NY, NX = detail["source"]
        reads = detail["filled"] & (NY == c.fill_spot[0]) & (NX == c.fill_spot[1])
        assert reads.any() and np.isnan(out[reads][:, 1]).all()
        y, x = c.nan_normal
        # the pixel kept four taps; with a NaN normal it keeps none and is filled
        assert clean[y, x, 3] > 0 and out[y, x, 3] == 0 and out[y, x, :3].any()
        same = np.isfinite(out).all(-1)
        same[y, x] = False
        assert bits_equal(out[same], clean[same])[0]


@functools.lru_cache(None)
def target():
    """512 samples of the 37 x 21 BASE view."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    v = tr.view(W, H, tr.BASE)
    out, _ = oracle.render(np.zeros((H, W, 4), F32), v.cam.blob, v.spheres,
                           np.array(rt.frame_seeds(7, 512), F32))
    return out


def _mse(a, mask=None):
    d = (a[..., :3].astype(np.float64) - target()[..., :3]) ** 2
    return float(np.mean(d if mask is None else d[mask]))


def test_carrying_up_beats_copying_texels():
    """(a): up2 with fill NEAREST against the nearest-texel copy a DISPLAY_FACTOR host shows."""
    c = case("up2_fill")
    carried, _ = expected("up2_fill", variant(fill=NEAREST))
    ys = ((np.arange(H) * 2 + 1) * c.ph) // (2 * H)         # floor((y + 0.5) * ph / H)
    xs = ((np.arange(W) * 2 + 1) * c.pw) // (2 * W)
    copied = c.prev_rgba[ys[:, None], xs[None, :]]
    ours, theirs = _mse(carried), _mse(copied)
    print(f"up2, fill NEAREST: MSE against 512 spp {ours:.5f}, nearest-texel copy {theirs:.5f}")
    assert ours < theirs


def test_carrying_down_beats_the_native_accumulator():
    """(b): down2 against the 16-sample accumulator rendered at 37 x 21, over interior pixels:
    those where every fine pixel in rows 2y - 2 .. 2y + 3, columns 2x - 2 .. 2x + 3 (clipped)
    has the pixel's id."""
    c = case("down2")
    carried, _ = expected("down2", variant())
    native = tr.accumulator(W, H, tr.BASE)
    fine, ids = c.prev.sphere_id, c.cur.sphere_id
    interior = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            block = fine[max(2 * y - 2, 0):min(2 * y + 4, c.ph), max(2 * x - 2, 0):min(2 * x + 4, c.pw)]
            interior[y, x] = bool((block == ids[y, x]).all())
    ours, theirs = _mse(carried, interior), _mse(native, interior)
    print(f"down2: {int(interior.sum())} interior pixels, MSE against 512 spp {ours:.6f}, "
          f"native 16-sample accumulator {theirs:.6f}")
    assert interior.sum() >= 400
    assert (carried[interior][:, 3] > 0).all()
    assert ours < theirs


# ---- GPU side --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


def guarded(p, n):
    return tr.guarded(p, n)


def host_inputs(c):
    return dict(prev_rgba=c.prev_rgba, prev_ids=c.prev.sphere_id, prev_hit=c.prev.hit,
                ids=c.cur.sphere_id, hit=c.cur.hit, normal=c.normal, material=c.cur.material)


def device_inputs(p, c):
    import torch
    return SimpleNamespace(**{k: torch.from_numpy(v.copy()).to(p.torch_device)
                              for k, v in host_inputs(c).items()})


def tail_intact(t, n, what):
    got = t.cpu().numpy()
    assert (got[n:] == F32(SENT)).all(), f"the 64 bytes after {what} were written"
    return got[:n]


def run(rt, p, c, var, second=None, d=None):
    """dst (and dst_second) of one variant through pipe.resize_carry, after the checks every call
    must pass: the tails intact, the previous images and the six planes unchanged."""
    import torch
    max_history, lamb, tol2, sky, fill = var
    d = d or device_inputs(p, c)
    px = c.w * c.h * 4
    dst = guarded(p, px)
    prev_guides, guides = tr.guides_of(d, lamb)
    kw = dict(max_history=max_history, position_tolerance2=tol2, lambertian_only=bool(lamb),
              sky=bool(sky), fill=fill, out=dst)
    dst2 = sec = None
    if second is not None:
        sec = torch.from_numpy(second.copy()).to(p.torch_device)
        dst2 = guarded(p, px)
        kw.update(prev_second=sec, out_second=dst2)
    res = p.resize_carry(d.prev_rgba, (c.pw, c.ph), (c.w, c.h), c.prev.cam, c.cur.cam,
                         prev_guides, guides, **kw)
    torch.cuda.current_stream().synchronize()
    got = tail_intact(dst, px, "dst").reshape(c.h, c.w, 4)
    for k, v in host_inputs(c).items():
        now = getattr(d, k).cpu().numpy()
        if v.dtype == np.int32:
            assert (now == v).all(), f"{k} was written"
        else:
            assert bits_equal(now, v)[0], f"{k} was written"
    if second is None:
        assert res is dst
        return got
    assert res[0] is dst and res[1] is dst2
    assert bits_equal(sec.cpu().numpy(), second)[0], "prev_second was written"
    return got, tail_intact(dst2, px, "dst_second").reshape(c.h, c.w, 4)


def check(got, name, var):
    want, _ = expected(name, var)
    same, bad = bits_equal(got, want)
    assert same, f"{_id((name, var))}: {bad} values differ from the reference"


@gpu
@pytest.mark.parametrize("v", ALL, ids=_id)
def test_matches_reference(rt, pipe, v):
    name, var = v
    check(run(rt, pipe, case(name), var), name, var)


@gpu
@pytest.mark.parametrize("v", LARGE, ids=_id)
def test_matches_reference_beyond_a_workgroup_and_at_the_extents(rt, pipe, v):
    name, var = v
    _, n = expected(name, var)
    print(_line(name, var, n))
    assert n["sky_kept"] > 0 and n["surface_kept"] > 0 and n["not_projected"] > 0
    if var[1]:
        assert n["filled"] > 0      # (the tall strip has no hole with lambertian_only 0)
    check(run(rt, pipe, case(name), var), name, var)


def raw_call(rt, p, ctx, images, pw, ph, w, h, prev_cam, cam, planes, params):
    """rt_resize_carry through the C boundary (data pointers or None); raises RtError."""
    L = rt._lib
    im = L.ResizeImagesC(*images) if images is not None else None
    pl = L.ReprojectPlanesC(*planes) if planes is not None else None
    pc = None
    if params is not None:
        pc = L.ResizeParamsC(*params[:5], tuple(params[5:]) if len(params) > 5 else (0, 0, 0))

    def ref(s):
        return ctypes.byref(s) if s is not None else None
    L.call("rt_resize_carry", ctx, ref(im), pw, ph, w, h, ref(prev_cam), ref(cam), ref(pl),
           ref(pc), p._stream())


@gpu
@pytest.mark.parametrize("name", ["pan", "nonfinite", "counts"])
@pytest.mark.parametrize("lamb", [0, 1])
def test_equal_sizes_give_rt_reproject_bits(rt, pipe, name, lamb):
    """The same device inputs through rt_reproject and through rt_resize_carry (sky 0, fill
    NONE, camera NULL)."""
    import torch
    c = tr.case(name)
    d = tr.device_inputs(pipe, c)
    px = c.w * c.h * 4
    a, b = guarded(pipe, px), guarded(pipe, px)
    planes = (d.prev_ids.data_ptr(), d.prev_hit.data_ptr(), d.ids.data_ptr(), d.hit.data_ptr(),
              d.normal.data_ptr(), d.material.data_ptr() if lamb else None)
    cam = c.prev.cam.to_c()
    tr.raw_call(rt, pipe, pipe._ctx, d.prev_rgba.data_ptr(), a.data_ptr(), c.w, c.h, cam, planes,
                (32, lamb, 1e-5, 0))
    raw_call(rt, pipe, pipe._ctx, (d.prev_rgba.data_ptr(), b.data_ptr(), None, None), c.w, c.h,
             c.w, c.h, cam, None, planes, (32, lamb, 1e-5, 0, NONE))
    torch.cuda.synchronize()
    one, two = tail_intact(a, px, "rt_reproject's dst"), tail_intact(b, px, "dst")
    assert (one.reshape(c.h, c.w, 4)[..., 3] > 0).sum() >= 50
    assert bits_equal(one, two)[0]
    want, _ = tr.expected(name, tr.variant(32, lamb))
    assert bits_equal(two.reshape(c.h, c.w, 4), want)[0]


@gpu
@pytest.mark.parametrize("v", [("up2_fill", variant(max_history=8, fill=NEAREST)),
                               ("up2", variant(max_history=8, lamb=1)),
                               ("down2", variant(max_history=8)),
                               ("33x9<-17x5", variant(max_history=8, lamb=1, fill=NEAREST))],
                         ids=_id)
def test_second_pair_equals_two_calls(rt, pipe, v):
    """A fused call against two single calls and against the reference, for a second image whose
    alphas differ from the first's: zeros, and counts above max_history."""
    name, var = v
    c = case(name)
    second = second_image(c)
    assert (second[..., 3] == 0).any() and (second[..., 3] > var[0]).any()
    assert (second[..., 3] != c.prev_rgba[..., 3]).any()
    d = device_inputs(pipe, c)
    first, fused = run(rt, pipe, c, var, second, d)
    alone = run(rt, pipe, c, var, None, d)
    import torch
    d2 = device_inputs(pipe, c)
    d2.prev_rgba = torch.from_numpy(second.copy()).to(pipe.torch_device)
    c2 = SimpleNamespace(**{**vars(c), "prev_rgba": second})
    second_alone = run(rt, pipe, c2, var, None, d2)
    assert bits_equal(first, alone)[0] and bits_equal(fused, second_alone)[0]
    assert bits_equal(first, reference(c, c.prev_rgba, var))[0]
    n, kept, kept_first = {}, {}, {}
    want = reference(c, second, var, n, kept)
    reference(c, c.prev_rgba, var, detail=kept_first)
    # the second pair's own alpha test: it keeps other taps than the first pair, and is capped
    assert n["capped"] > 0 and (kept["kept"] != kept_first["kept"]).any()
    assert bits_equal(fused, want)[0]


@gpu
@pytest.mark.parametrize("lamb", [0, 1])
def test_the_tracer_takes_the_carried_image(rt, oracle, pipe, lamb):
    """up2's output (mixed counts; zeros with colour where filled) through rt_update with
    camera_has_moved = 0."""
    import torch
    for name, var in (("up2", variant(lamb=lamb)), ("up2_fill", variant(lamb=lamb, fill=NEAREST))):
        c = case(name)
        want, _ = expected(name, var)
        assert len(np.unique(want[..., 3])) >= 2
        still = c.cur.cam.with_fields(camera_has_moved=0.0)
        got = run(rt, pipe, c, var)
        check(got, name, var)
        rep = torch.from_numpy(got.copy()).to(pipe.torch_device)
        out = pipe.new_image(c.w, c.h)
        pipe.update(rep, out, c.w, c.h, still, c.sc)
        torch.cuda.synchronize()
        one, _ = oracle.update(want, still.blob, c.cur.spheres)
        assert bits_equal(out.cpu().numpy(), one)[0]


@gpu
def test_errors_launch_nothing(rt, pipe):
    import torch
    c = case("up2")
    d = device_inputs(pipe, c)
    px = c.w * c.h * 4
    dst, dst2 = guarded(pipe, px), guarded(pipe, px)
    sec = torch.from_numpy(second_image(c).copy()).to(pipe.torch_device)
    S, D, S2, D2 = d.prev_rgba.data_ptr(), dst.data_ptr(), sec.data_ptr(), dst2.data_ptr()
    one, two = (S, D, None, None), (S, D, S2, D2)
    planes = (d.prev_ids.data_ptr(), d.prev_hit.data_ptr(), d.ids.data_ptr(), d.hit.data_ptr(),
              d.normal.data_ptr(), d.material.data_ptr())
    ctx, pw, ph, w, h = pipe._ctx, c.pw, c.ph, c.w, c.h
    pcam, cam = c.prev.cam.to_c(), c.cur.cam.to_c()
    flat = c.prev.cam.blob.copy()
    flat[8:11] = 0.0
    degenerate = rt.SceneCamera(flat).to_c()
    ok = (64, 1, 1e-5, 1, NEAREST)
    A, Z = RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE

    def row(images=two, sizes=(pw, ph, w, h), prev_cam=pcam, camera=cam, pl=planes, params=ok,
            context=ctx):
        return (context, images, *sizes, prev_cam, camera, pl, params)

    rows = {
        "ctx NULL": (RT_ERR_INVALID_CONTEXT, row(context=None)),
        "images NULL": (A, row(images=None)),
        "prev_rgba NULL": (A, row(images=(None, D, S2, D2))),
        "dst_rgba NULL": (A, row(images=(S, None, S2, D2))),
        "prev_second alone": (A, row(images=(S, D, S2, None))),
        "dst_second alone": (A, row(images=(S, D, None, D2))),
        "dst == prev": (A, row(images=(D, D, None, None))),
        "dst == prev_second": (A, row(images=(S, D, D, D2))),
        "dst_second == prev": (A, row(images=(D2, D, S2, D2))),
        "dst_second == prev_second": (A, row(images=(S, D, D2, D2))),
        "dst_second == dst": (A, row(images=(S, D, S2, D))),
        "prev_camera NULL": (A, row(prev_cam=None)),
        "planes NULL": (A, row(pl=None)),
        "params NULL": (A, row(params=None)),
        "camera NULL with sky": (A, row(camera=None, params=(64, 1, 1e-5, 1, NONE))),
        "camera NULL with fill": (A, row(camera=None, params=(64, 1, 1e-5, 0, NEAREST))),
        "max_history 0": (A, row(params=(0, 1, 1e-5, 1, NEAREST))),
        "max_history 2^24 + 1": (A, row(params=((1 << 24) + 1, 1, 1e-5, 1, NEAREST))),
        "lambertian_only 2": (A, row(params=(64, 2, 1e-5, 1, NEAREST))),
        "sky 2": (A, row(params=(64, 1, 1e-5, 2, NEAREST))),
        "fill 2": (A, row(params=(64, 1, 1e-5, 1, 2))),
        "degenerate prev_camera": (A, row(prev_cam=degenerate)),
    }
    for k in range(3):
        word = [0, 0, 0]
        word[k] = 1
        rows[f"_reserved[{k}] 1"] = (A, row(params=ok + tuple(word)))
    for k, what in enumerate(("prev_width", "prev_height", "width", "height")):
        for bad in (0, 65537):
            sizes = [pw, ph, w, h]
            sizes[k] = bad
            rows[f"{what} {bad}"] = (Z, row(sizes=tuple(sizes)))
    fields = [f for f, _ in rt._lib.ReprojectPlanesC._fields_]
    for i, f in enumerate(fields):
        rows[f"{f} NULL"] = (A, row(pl=planes[:i] + (None,) + planes[i + 1:]))
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf")),
                      ("-inf", float("-inf"))]:
        rows[f"tolerance {what}"] = (A, row(params=(64, 1, bad, 1, NEAREST)))
    for what, (status, args) in rows.items():
        with pytest.raises(rt.RtError) as e:
            raw_call(rt, pipe, *args)
        assert e.value.status == status, what
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == F32(SENT)).all(), "a refused call wrote dst_rgba"
    assert (dst2.cpu().numpy() == F32(SENT)).all(), "a refused call wrote dst_second"
    # camera NULL is accepted with sky 0 and fill NONE; without lambertian_only the material
    # plane is not required; and the context still works
    raw_call(rt, pipe, *row(images=one, camera=None, pl=planes[:5] + (None,),
                            params=(64, 0, 1e-5, 0, NONE)))
    torch.cuda.synchronize()
    check(tail_intact(dst, px, "dst").reshape(h, w, 4), "sky0", variant(sky=0))
    assert (dst2.cpu().numpy() == F32(SENT)).all()


@gpu
def test_a_call_leaves_the_render_state_alone(rt, oracle):
    """After 4 rendered frames: rt_last_launch_info and the candidate statistics are what they
    were, the destinations' uniform counts are forgotten, and the next frames equal the
    oracle's."""
    import torch
    c = case("up2_fill")
    var = variant(fill=NEAREST)
    w, h = c.w, c.h
    seeds = np.array(rt.frame_seeds(3, 4), F32)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, b = p.new_image(w, h), p.new_image(w, h)
        images = (a, b)
        newest = p.update_frames(a, b, w, h, c.cur.cam, c.sc, seeds)
        info, stats = p.last_launch_info(), p.candidate_stats()
        d = device_inputs(p, c)
        prev_guides, guides = tr.guides_of(d, False)
        p.resize_carry(d.prev_rgba, (c.pw, c.ph), (w, h), c.prev.cam, c.cur.cam, prev_guides,
                       guides, lambertian_only=False, sky=True, fill=NEAREST,
                       out=images[newest])
        assert p.last_launch_info() == info
        assert p.candidate_stats() == stats
        torch.cuda.synchronize()
        rep = images[newest].cpu().numpy()
        still = c.cur.cam.with_fields(camera_has_moved=0.0)
        more = np.array(rt.frame_seeds(13, 3), F32)
        first, second = images[newest], images[1 - newest]
        last = p.update_frames(first, second, w, h, still, c.sc, more)
        torch.cuda.synchronize()
        got = (first, second)[last].cpu().numpy()
    finally:
        p.close()
    want, _ = expected("up2_fill", var)
    assert bits_equal(rep, want)[0]
    after, _ = oracle.render(want, still.blob, c.cur.spheres, more)
    assert bits_equal(got, after)[0]


@gpu
def test_upscale_is_resize_carry_with_its_settings(rt, pipe):
    """With the planes the GPU traces for both views, given and traced by upscale itself."""
    import torch
    c = case("up2_fill")
    small, size = (c.pw, c.ph), (c.w, c.h)
    prev = torch.from_numpy(c.prev_rgba.copy()).to(pipe.torch_device)
    guides_small = pipe.trace_aov(c.pw, c.ph, c.prev.cam, c.sc, planes=("sphere_id", "hit"))
    guides = pipe.trace_aov(c.w, c.h, c.cur.cam, c.sc)
    want = pipe.resize_carry(prev, small, size, c.prev.cam, c.cur.cam, guides_small, guides,
                             lambertian_only=False, sky=True, fill=NEAREST)
    given = pipe.upscale(prev, small, size, c.prev.cam, c.cur.cam, guides_small, guides)
    traced = pipe.upscale(prev, small, size, c.prev.cam, c.cur.cam, spheres=c.sc)
    half = pipe.upscale(prev, small, size, c.prev.cam, c.cur.cam, guides_small, spheres=c.sc,
                        out=pipe.new_image(c.w, c.h))
    with pytest.raises(ValueError):
        pipe.upscale(prev, small, size, c.prev.cam, c.cur.cam)          # no scene to trace
    with pytest.raises(ValueError):
        pipe.upscale(prev, small, size, c.prev.cam, c.cur.cam, guides_small)
    torch.cuda.synchronize()
    assert (guides["sphere_id"].cpu().numpy() == c.cur.sphere_id).all()
    assert (guides_small["sphere_id"].cpu().numpy() == c.prev.sphere_id).all()
    assert want.shape == (c.h, c.w, 4)
    check(want.cpu().numpy(), "up2_fill", variant(fill=NEAREST))
    for other in (given, traced, half):
        assert bits_equal(other.cpu().numpy(), want.cpu().numpy())[0]
    # every pixel shows a colour source: none is left (0, 0, 0, 0) by a rule
    _, n = expected("up2_fill", variant(fill=NEAREST))
    assert n["zeroed"] == 0 and n["not_projected"] == 0
    present = pipe.present(given, c.w, c.h)
    assert present.shape == (c.h, c.w, 4)
    with pytest.raises(ValueError):
        pipe.resize_carry(prev, small, size, c.prev.cam, None, guides_small, guides, sky=True)
    with pytest.raises(ValueError):
        pipe.resize_carry(prev, small, size, c.prev.cam, c.cur.cam, guides_small,
                          {k: v for k, v in guides.items() if k != "material"})
    with pytest.raises(ValueError):
        pipe.resize_carry(prev, size, size, c.prev.cam, c.cur.cam, guides_small, guides)
    with pytest.raises(ValueError):
        pipe.resize_carry(prev.cpu(), small, size, c.prev.cam, c.cur.cam, guides_small, guides)
