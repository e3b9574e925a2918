"""Reprojection (include/rt_reproject.h): rt_reproject, rt_reproject_basis,
rt_reproject_params_default.

The reference is in this file: `reproject_basis_ref`, NumPy float64 with the header's operation
order, and `reproject_ref`, a vectorised NumPy float32 restatement of the header's per-pixel text
that also tallies how often each rule fires.  The guide planes come from the oracle's sphere_hit
along each pixel's centre ray (tests/test_denoise.py's construction, imported), the material plane
from the sphere records, the previous accumulator from the CPU oracle (16 frames, max_depth 4).
Every GPU output is compared bit for bit (NaN == NaN).

The CPU tests check the boundary and the basis, count from the reference alone that every case
reaches the rules it is there for (printed with -s), and check that carried history beats a reset
against a 512-sample render: a strict inequality, not a tolerance.
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
from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_reproject.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
W, H = 37, 21                  # partial 32 x 8 tiles both ways
MISS = -1
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
SENT = -12345.0
TAIL = 16                      # 64 bytes of sentinel after dst
HISTORY = 16                   # samples in the previous accumulator
PIXEL_RULES = ("miss", "specular", "behind", "out_of_range")
TAP_RULES = ("off_image", "id_mismatch", "plane", "no_samples", "zero_weight")
TALLIES = PIXEL_RULES + TAP_RULES + ("four", "some", "none", "capped")


# ---- the reference ---------------------------------------------------------------------------------
def reproject_basis_ref(blob):
    """rt_reproject.h's basis from a camera's 44 f32: (9 float32, ok)."""
    b = np.asarray(blob, F32).astype(np.float64)
    o, ul, du, dv = b[0:3], b[4:7], b[8:11], b[12:15]
    e = ul - o

    def cross(a, c):
        return np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2],
                         a[0] * c[1] - a[1] * c[0]])

    c0, c1, c2 = cross(dv, e), cross(e, du), cross(du, dv)
    det = (du[0] * c0[0] + du[1] * c0[1]) + du[2] * c0[2]
    with np.errstate(all="ignore"):
        out = (np.concatenate([c0, c1, c2]) / det).astype(F32)
    ok = bool(det != 0.0 and np.isfinite(det) and np.isfinite(out).all())
    return out, ok


def _dot3(r, v):
    return (r[0] * v[..., 0] + r[1] * v[..., 1]) + r[2] * v[..., 2]


def reproject_ref(prev, prev_ids, prev_hit, ids, hit, normal, material, prev_blob, max_history,
                  lambertian_only, tol2, counts=None, detail=None):
    """rt_reproject.h's per-pixel text over (H, W, .) float32 arrays (ids: (H, W) int32).  With
    `counts` (a dict) it tallies the pixels each of rules 1-4 stops, the taps each skip rule
    drops (each tap counted at the first rule that drops it, in the header's order), the pixels
    with 4, 1-3 and no kept taps, and the pixels max_history caps.  `detail` receives "used", the
    previous pixels some kept tap read, and "kept", the kept taps per pixel."""
    prev = np.ascontiguousarray(prev, F32)
    prev_hit = np.ascontiguousarray(prev_hit, F32)
    hit = np.ascontiguousarray(hit, F32)
    normal = np.ascontiguousarray(normal, F32)
    h, w = ids.shape
    basis, ok = reproject_basis_ref(prev_blob)
    assert ok
    r0, r1, r2 = basis[0:3], basis[3:6], basis[6:9]
    o = np.asarray(prev_blob, F32)[0:3]
    one, half = F32(1.0), F32(0.5)
    tally = dict.fromkeys(TALLIES, 0)
    with np.errstate(all="ignore"):
        p, nP = hit[..., :3], normal[..., :3]
        miss = ids == MISS
        live = ~miss
        tally["miss"] = int(miss.sum())
        if lambertian_only:
            spec = live & ~(np.ascontiguousarray(material, F32)[..., 3] < F32(-1.0))
            tally["specular"] = int(spec.sum())
            live = live & ~spec
        q = p - o
        a, b, c = _dot3(r0, q), _dot3(r1, q), _dot3(r2, q)
        front = c > 0
        tally["behind"] = int((live & ~front).sum())
        live = live & front
        px, py = a / c - half, b / c - half
        assert px.dtype == F32 and c.dtype == F32
        inside = (px >= -1) & (px < F32(w)) & (py >= -1) & (py < F32(h))
        tally["out_of_range"] = int((live & ~inside).sum())
        live = live & inside
        fx, fy = np.floor(px), np.floor(py)
        tx, ty = px - fx, py - fy
        x0 = np.where(live, fx, 0).astype(np.int64)
        y0 = np.where(live, fy, 0).astype(np.int64)
        r2q = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        lim = F32(tol2) * r2q
        sw = np.zeros((h, w), F32)
        acc = np.zeros((h, w, 3), F32)
        n = np.full((h, w), np.inf, F32)
        kept = np.zeros((h, w), np.int64)
        used = np.zeros((h, w), bool)
        for j in (0, 1):
            for i in (0, 1):
                X, Y = x0 + i, y0 + j
                bw = (ty if j else one - ty) * (tx if i else one - tx)
                on = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
                Xc, Yc = np.clip(X, 0, w - 1), np.clip(Y, 0, h - 1)
                same = prev_ids[Yc, Xc] == ids
                e = p - prev_hit[Yc, Xc, :3]
                dl = _dot3(nP.transpose(2, 0, 1), e)
                near = dl * dl <= lim
                pc = prev[Yc, Xc]
                has = pc[..., 3] > 0
                pos = bw > 0
                assert bw.dtype == F32 and dl.dtype == F32 and lim.dtype == F32
                left = live
                for rule, passes in (("off_image", on), ("id_mismatch", same), ("plane", near),
                                     ("no_samples", has), ("zero_weight", pos)):
                    tally[rule] += int((left & ~passes).sum())
                    left = left & passes
                keep = left
                sw = np.where(keep, sw + bw, sw)
                acc = np.where(keep[..., None], acc + bw[..., None] * pc[..., :3], acc)
                n = np.where(keep, np.minimum(n, pc[..., 3]), n)
                kept += keep
                used[Yc[keep], Xc[keep]] = True
        got = kept > 0
        out = np.zeros((h, w, 4), F32)
        out[..., :3] = np.where(got[..., None], acc / sw[..., None], F32(0.0))
        out[..., 3] = np.where(got, np.minimum(n, F32(max_history)), F32(0.0))
        assert sw.dtype == F32 and acc.dtype == F32 and n.dtype == F32
        tally["four"] = int((kept == 4).sum())
        tally["some"] = int(((kept >= 1) & (kept <= 3)).sum())
        tally["none"] = int((live & (kept == 0)).sum())
        tally["capped"] = int((got & (n > F32(max_history))).sum())
    if counts is not None:
        counts.update(tally)
    if detail is not None:
        detail.update(used=used, kept=kept)
    return out


# ---- views, accumulators and cases -----------------------------------------------------------------
BASE = ()                                                   # the default camera
PAN = (("look_at", (0.3, 0.1, 0.0)),)
ORBIT = (("look_from", (12.0, 2.5, 5.0)),)
DOLLY = (("look_from", (10.0, 1.5, 2.3)),)
TURN = (("look_at", (0.0, 0.0, 3.5)),)
AWAY = (("look_at", (26.0, 4.0, 6.0)),)                     # looks away from the scene
MOVES = {"base": BASE, "pan": PAN, "orbit": ORBIT, "dolly": DOLLY, "turn": TURN, "away": AWAY}


def _scene(rt, kind):
    if kind == "zero":
        return np.zeros((0, 8), F32)
    return np.ascontiguousarray(rt.synthetic_scene(40).spheres, F32).reshape(-1, 8)


@functools.lru_cache(None)
def view(w, h, move, kind="n40"):
    """A camera (max_depth 4, seed 0.25) and its four planes, as rt_trace_aov defines them."""
    import gpu_ray_tracing as rt
    cam = td.default_camera(rt, w, h, **dict(move))
    spheres = _scene(rt, kind)
    g = td.guide_planes(cam.blob, spheres, w, h)
    material = np.zeros((h, w, 4), F32)
    hitmask = g["sphere_id"] != MISS
    material[hitmask] = spheres[g["sphere_id"][hitmask], 4:8]
    for a in (spheres, material, *g.values()):
        a.setflags(write=False)
    return SimpleNamespace(cam=cam, spheres=spheres, material=material, **g)


@functools.lru_cache(None)
def accumulator(w, h, move, kind="n40"):
    """The view's accumulator after HISTORY frames of the CPU oracle."""
    import gpu_ray_tracing as rt
    from oracle import oracle
    v = view(w, h, move, kind)
    out, _ = oracle.render(np.zeros((h, w, 4), F32), v.cam.blob, v.spheres,
                           np.array(rt.frame_seeds(3, HISTORY), F32))
    out.setflags(write=False)
    return out


def variant(max_history=64, lamb=1, tol2=1e-5):
    return (max_history, lamb, tol2)


BOTH = [variant(lamb=0), variant(lamb=1)]
# name -> (width, height, scene, previous view, current view, variants, rules it must reach)
CASES = {
    "identity": (W, H, "n40", BASE, BASE, BOTH, ("zero_weight", "plane", "four", "specular")),
    "pan": (W, H, "n40", BASE, PAN, BOTH,
            ("id_mismatch", "off_image", "plane", "four", "some", "none", "miss")),
    "orbit": (W, H, "n40", BASE, ORBIT, BOTH, ("out_of_range", "id_mismatch", "plane", "none")),
    "dolly": (W, H, "n40", BASE, DOLLY, BOTH, ("id_mismatch", "plane", "specular")),
    "turn": (W, H, "n40", BASE, TURN, BOTH, ("out_of_range", "off_image")),
    "behind": (W, H, "n40", AWAY, BASE, BOTH, ("behind",)),
    "counts": (W, H, "n40", BASE, PAN, [variant(32, 0), variant(32, 1)], ("no_samples",)),
    "cap": (W, H, "n40", BASE, PAN, [variant(1), variant(8), variant(1 << 24)], ("capped",)),
    "tolerance": (W, H, "n40", BASE, PAN,
                  [variant(tol2=t) for t in (0.0, 1e-6, 1e-4, 3e38)], ("plane",)),
    "nonfinite": (W, H, "n40", BASE, PAN, BOTH, ("plane",)),
    "zero": (W, H, "zero", BASE, PAN, BOTH, ("miss",)),
}
# the kernel's workgroup covers 32 x 8 pixels in 2 x 2 waves of 16 x 4: one tile exactly and one
# pixel more both ways, one wave and one pixel more, the denoiser's 64 x 4 likewise, and shapes
# narrower, lower and larger than a tile
SIZES = [(1, 1), (8, 8), (16, 4), (17, 5), (32, 8), (33, 9), (64, 4), (65, 5), (70, 3), (5, 40),
         (100, 52)]
for _w, _h in SIZES:
    CASES[f"{_w}x{_h}"] = (_w, _h, "n40", BASE, PAN, BOTH, ("off_image",))


def _planted(c0, prev):
    """nonfinite: NaN, +inf and -inf in the green of three previous pixels that kept taps read,
    and a NaN in the normal of a pixel that keeps four taps, chosen from the unmodified case."""
    detail = {}
    reproject_ref(prev, c0.prev.sphere_id, c0.prev.hit, c0.cur.sphere_id, c0.cur.hit,
                  c0.cur.normal, c0.cur.material, c0.prev.cam.blob, 64, 1, 1e-5, detail=detail)
    ys, xs = np.nonzero(detail["used"])
    assert ys.size >= 30
    spots = [(int(ys[k]), int(xs[k])) for k in (ys.size // 4, ys.size // 2, 3 * ys.size // 4)]
    fy, fx = np.nonzero(detail["kept"] == 4)
    assert fy.size >= 1
    return dict(zip(spots, (np.nan, np.inf, -np.inf))), (int(fy[fy.size // 2]),
                                                         int(fx[fx.size // 2]))


@functools.lru_cache(None)
def case(name):
    """A case's inputs (read-only arrays), computed once and shared."""
    import gpu_ray_tracing as rt
    w, h, kind, pmove, cmove, variants, rules = CASES[name]
    pv, cv = view(w, h, pmove, kind), view(w, h, cmove, kind)
    c = SimpleNamespace(name=name, w=w, h=h, prev=pv, cur=cv, variants=variants, rules=rules,
                        sc=rt.SphereCollection(cv.spheres), normal=cv.normal, planted=None,
                        nan_normal=None)
    prev = accumulator(w, h, pmove, kind)
    if name == "counts":
        prev = prev.copy()
        prev[::3, ::2, 3] = 0.0
        prev[1::3, 1::2, 3] = 100.0
    if name == "nonfinite":
        c.planted, c.nan_normal = _planted(c, prev)
        prev = prev.copy()
        for (y, x), v in c.planted.items():
            prev[y, x, 1] = v
        c.normal = cv.normal.copy()
        c.normal[c.nan_normal][0] = np.nan
    for a in (prev, c.normal):
        a.setflags(write=False)
    c.prev_rgba = prev
    return c


@functools.lru_cache(None)
def expected(name, var):
    """(reference output, its tallies) of one variant of a case."""
    c = case(name)
    max_history, lamb, tol2 = var
    counts = {}
    out = reproject_ref(c.prev_rgba, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit,
                        c.normal, c.cur.material, c.prev.cam.blob, max_history, lamb, tol2, counts)
    out.setflags(write=False)
    return out, counts


ALL = [(name, var) for name in CASES for var in CASES[name][5]]


def _id(v):
    name, (max_history, lamb, tol2) = v
    return f"{name}-h{max_history}-{'lambertian' if lamb else 'all'}-t{tol2:g}"


# ---- CPU tests -------------------------------------------------------------------------------------
def test_library_exports_the_reproject_entry_points(rt):
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", HEADER.read_text(), flags=re.M)
    assert declared == ["rt_reproject_params_default", "rt_reproject_basis", "rt_reproject"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert set(declared) <= exported
    assert {s for s in exported if "reproject" in s} == set(declared)
    L = rt._lib
    assert set(L.reproject_symbols()) == set(declared)
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.selftest_roots_symbols(), L.denoise_symbols()):
        assert not set(declared) & set(other)
    assert L.lib().rt_abi_version() == 7
    assert ctypes.sizeof(L.ReprojectParamsC) == 16
    assert ctypes.sizeof(L.ReprojectPlanesC) == 48
    assert [f for f, _ in L.ReprojectParamsC._fields_] == [
        "max_history", "lambertian_only", "position_tolerance2", "_reserved"]
    assert [f for f, _ in L.ReprojectPlanesC._fields_] == [
        "prev_sphere_id", "prev_hit", "sphere_id", "hit", "normal", "material"]
    p = L.ReprojectParamsC(99, 99, -1.0, 99)
    L.lib().rt_reproject_params_default(ctypes.byref(p))
    assert (p.max_history, p.lambertian_only, p._reserved) == (64, 1, 0)
    assert F32(p.position_tolerance2) == F32(1e-5)
    L.lib().rt_reproject_params_default(None)                   # a no-op, not a crash
    d = rt.REPROJECT_DEFAULTS
    assert (d["max_history"], d["lambertian_only"]) == (64, True)
    assert F32(d["position_tolerance2"]) == F32(1e-5)


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "rt_reproject.h"\n'
                   "typedef char params_are_16_bytes[sizeof(rt_reproject_params) == 16 ? 1 : -1];\n"
                   "typedef char planes_are_48_bytes[sizeof(rt_reproject_planes) == 48 ? 1 : -1];\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_basis_matches_the_reference(rt):
    cams = {f"default {w}x{h}": td.default_camera(rt, w, h)
            for w, h in ((W, H), (1, 1), (1920, 1080))}
    for name, move in MOVES.items():
        cams[name] = td.default_camera(rt, W, H, **dict(move))
    for name, cam in cams.items():
        want, ok = reproject_basis_ref(cam.blob)
        assert ok, name
        got = rt.reproject_basis(cam)
        assert got.shape == (3, 3) and got.dtype == F32
        assert bits_equal(got.reshape(9), want)[0], name
        # it is the inverse: du' -> (1, 0, 0), dv' -> (0, 1, 0), e' -> (0, 0, 1)
        b = cam.blob.astype(np.float64)
        m = np.stack([b[8:11], b[12:15], b[4:7] - b[0:3]], axis=1)
        assert np.allclose(got.astype(np.float64) @ m, np.eye(3), atol=1e-4), name
    blob = cams[f"default {W}x{H}"].blob.copy()
    blob[8:11] = 0.0                                            # pixel_delta_u = 0
    assert not reproject_basis_ref(blob)[1]
    with pytest.raises(rt.RtError) as e:
        rt.reproject_basis(rt.SceneCamera(blob))
    assert e.value.status == RT_ERR_INVALID_ARGUMENT
    out = (ctypes.c_float * 9)()
    cam = cams[f"default {W}x{H}"].to_c()
    assert rt._lib.lib().rt_reproject_basis(None, out) == RT_ERR_INVALID_ARGUMENT
    assert rt._lib.lib().rt_reproject_basis(ctypes.byref(cam), None) == RT_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", list(CASES))
def test_cases_reach_their_rules(name):
    c = case(name)
    reached = dict.fromkeys(TALLIES, 0)
    hits = int((c.cur.sphere_id != MISS).sum())
    per = {}
    for var in c.variants:
        out, n = expected(name, var)
        per[var] = n
        print(f"{_id((name, var))}: {c.w}x{c.h}, {hits} hit pixels: "
              + ", ".join(f"{k} {n[k]}" for k in TALLIES)
              + f"; {int((out[..., 3] > 0).sum())} pixels with history")
        assert int((out[..., 3] > 0).sum()) == n["four"] + n["some"]
        assert n["miss"] == c.w * c.h - hits
        if not var[1]:
            assert n["specular"] == 0
        for k in reached:
            reached[k] += n[k]
    for rule in c.rules:
        assert reached[rule] >= 1, f"{name} never reaches {rule}"
    if name == "identity":
        for var in c.variants:
            n = per[var]
            assert n["none"] == 0 and n["behind"] == 0 and n["out_of_range"] == 0
            assert n["four"] + n["some"] == hits - n["specular"]
    if name == "behind":
        for var in c.variants:
            assert per[var]["behind"] == hits - per[var]["specular"] and hits > 0
            assert not expected(name, var)[0].any()
        assert per[variant(lamb=0)]["behind"] == hits
    if name == "counts":
        # the minimum over the kept taps: 16 wherever a tap of count 16 is kept, and
        # min(100, max_history) = 32 only where every kept tap holds the planted 100
        for var in c.variants:
            alphas = set(np.unique(expected(name, var)[0][..., 3]))
            assert {0.0, 16.0} <= alphas <= {0.0, 16.0, 32.0}
            assert per[var]["capped"] == int((expected(name, var)[0][..., 3] == 32.0).sum())
    if name == "cap":
        assert per[variant(1)]["capped"] > 0 and per[variant(8)]["capped"] > 0
        assert per[variant(1 << 24)]["capped"] == 0
        assert expected(name, variant(8))[0][..., 3].max() == 8.0
    if name == "tolerance":
        rejects = [per[v]["plane"] for v in c.variants]
        assert rejects == sorted(rejects, reverse=True) and rejects[1] > rejects[2]
        assert rejects[3] == 0
    if name == "zero":
        for var in c.variants:
            assert per[var]["miss"] == c.w * c.h and not expected(name, var)[0].any()


def test_nonfinite_colours_propagate_and_a_nan_normal_restarts():
    c = case("nonfinite")
    plain = case("pan")
    for var in c.variants:
        out, _ = expected("nonfinite", var)
        clean, _ = expected("pan", var)
        bad = ~np.isfinite(out).all(-1)
        assert np.isnan(out[..., 1]).any() and np.isinf(out[..., 1]).any()
        assert bad.sum() >= 3
        # only green is planted: red, blue and the counts stay finite
        assert np.isfinite(out[..., (0, 2, 3)]).all()
        y, x = c.nan_normal
        assert clean[y, x, 3] > 0 and not out[y, x].any()
        same = ~bad
        same[y, x] = False
        assert bits_equal(out[same], clean[same])[0]
    assert np.isnan(c.normal[c.nan_normal][0]) and not np.isnan(plain.normal).any()


@pytest.mark.parametrize("name", ["pan", "orbit", "dolly", "turn"])
def test_history_beats_a_reset(name, oracle):
    """Over the pixels that got history: the reprojected image plus one sample is nearer a
    512-sample render of the new view than one sample alone."""
    import gpu_ray_tracing as rt
    c = case(name)
    rep = reproject_ref(c.prev_rgba, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit,
                        c.normal, c.cur.material, c.prev.cam.blob, HISTORY, 1, 1e-5)
    got = rep[..., 3] > 0
    assert got.sum() >= 50
    still = c.cur.cam.with_fields(camera_has_moved=0.0)
    moved = c.cur.cam.with_fields(camera_has_moved=1.0)
    kept, _ = oracle.update(rep, still.blob, c.cur.spheres)
    reset, _ = oracle.update(rep, moved.blob, c.cur.spheres)
    assert (reset[..., 3] == 1.0).all() and (kept[got][:, 3] == rep[got][:, 3] + 1.0).all()
    target, _ = oracle.render(np.zeros((c.h, c.w, 4), F32), c.cur.cam.blob, c.cur.spheres,
                              np.array(rt.frame_seeds(7, 512), F32))

    def mse(a):
        return float(np.mean((a[got][:, :3].astype(np.float64) - target[got][:, :3]) ** 2))
    with_history, without = mse(kept), mse(reset)
    print(f"{name}: {int(got.sum())} pixels with history, MSE against 512 spp: kept "
          f"{with_history:.5f}, reset {without:.5f}, ratio {without / with_history:.2f}")
    assert with_history < without


# ---- GPU side --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


def guarded(p, n):
    import torch
    return torch.full((n + TAIL,), SENT, dtype=torch.float32, device=p.torch_device)


HOST_PLANES = ("prev_rgba", "prev_ids", "prev_hit", "ids", "hit", "normal", "material")


def host_inputs(c):
    return dict(prev_rgba=c.prev_rgba, prev_ids=c.prev.sphere_id, prev_hit=c.prev.hit,
                ids=c.cur.sphere_id, hit=c.cur.hit, normal=c.normal, material=c.cur.material)


def device_inputs(p, c):
    import torch
    return SimpleNamespace(**{k: torch.from_numpy(v.copy()).to(p.torch_device)
                              for k, v in host_inputs(c).items()})


def guides_of(d, lamb=True):
    prev = {"sphere_id": d.prev_ids, "hit": d.prev_hit}
    cur = {"sphere_id": d.ids, "hit": d.hit, "normal": d.normal}
    if lamb:
        cur["material"] = d.material
    return prev, cur


def raw_call(rt, p, ctx, prev, dst, w, h, cam, planes, params):
    """rt_reproject through the C boundary (data pointers or None); raises RtError."""
    L = rt._lib
    pl = L.ReprojectPlanesC(*planes) if planes is not None else None
    pc = L.ReprojectParamsC(*params) if params is not None else None
    L.call("rt_reproject", ctx, prev, dst, w, h,
           ctypes.byref(cam) if cam is not None else None,
           ctypes.byref(pl) if pl is not None else None,
           ctypes.byref(pc) if pc is not None else None, p._stream())


def run(rt, p, c, var):
    """dst of one variant (numpy) through pipe.reproject, after the checks every call must pass:
    the tail of dst intact, prev_image and the six planes unchanged."""
    import torch
    max_history, lamb, tol2 = var
    d = device_inputs(p, c)
    px = c.w * c.h * 4
    dst = guarded(p, px)
    prev_guides, guides = guides_of(d, lamb)
    res = p.reproject(d.prev_rgba, c.w, c.h, c.prev.cam, prev_guides, guides,
                      max_history=max_history, position_tolerance2=tol2,
                      lambertian_only=bool(lamb), out=dst)
    assert res is dst
    torch.cuda.current_stream().synchronize()
    got = dst.cpu().numpy()
    assert (got[px:] == F32(SENT)).all(), "the 64 bytes after dst were written"
    for k, v in host_inputs(c).items():
        now = getattr(d, k).cpu().numpy()
        if v.dtype == np.int32:
            assert (now == v).all(), f"{k} was written"
        else:
            assert bits_equal(now, v)[0], f"{k} was written"
    return got[:px].reshape(c.h, c.w, 4)


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
def test_planes_the_gpu_traces_give_the_reference(rt, pipe):
    """trace_aov's own planes for both views and an allocated `out`."""
    import torch
    c = case("pan")
    prev_guides = pipe.trace_aov(c.w, c.h, c.prev.cam, c.sc, planes=("sphere_id", "hit"))
    guides = pipe.trace_aov(c.w, c.h, c.cur.cam, c.sc)
    prev = torch.from_numpy(c.prev_rgba.copy()).to(pipe.torch_device)
    out = pipe.reproject(prev, c.w, c.h, c.prev.cam, prev_guides, guides)
    assert out.shape == (c.h, c.w, 4)
    noid = {k: v for k, v in guides.items() if k != "material"}
    every = pipe.reproject(prev, c.w, c.h, c.prev.cam, prev_guides, noid, lambertian_only=False)
    torch.cuda.synchronize()
    assert (guides["sphere_id"].cpu().numpy() == c.cur.sphere_id).all()
    assert bits_equal(guides["material"].cpu().numpy(), c.cur.material)[0]
    check(out.cpu().numpy(), "pan", variant(lamb=1))
    check(every.cpu().numpy(), "pan", variant(lamb=0))
    with pytest.raises(ValueError):
        pipe.reproject(prev, c.w, c.h, c.prev.cam, prev_guides, noid)     # material missing
    with pytest.raises(ValueError):
        pipe.reproject(prev, c.w, c.h, c.prev.cam, {"hit": prev_guides["hit"]}, guides)
    with pytest.raises(ValueError):
        pipe.reproject(prev.cpu(), c.w, c.h, c.prev.cam, prev_guides, guides)


@gpu
def test_errors_launch_nothing(rt, pipe):
    import torch
    c = case("pan")
    d = device_inputs(pipe, c)
    px = c.w * c.h * 4
    dst = guarded(pipe, px)
    S, D = d.prev_rgba.data_ptr(), dst.data_ptr()
    planes = (d.prev_ids.data_ptr(), d.prev_hit.data_ptr(), d.ids.data_ptr(), d.hit.data_ptr(),
              d.normal.data_ptr(), d.material.data_ptr())
    ctx, w, h = pipe._ctx, c.w, c.h
    cam = c.prev.cam.to_c()
    flat = c.prev.cam.blob.copy()
    flat[8:11] = 0.0
    degenerate = rt.SceneCamera(flat).to_c()
    ok = (64, 1, 1e-5, 0)
    A, Z = RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE
    rows = {
        "ctx NULL": (RT_ERR_INVALID_CONTEXT, (None, S, D, w, h, cam, planes, ok)),
        "prev NULL": (A, (ctx, None, D, w, h, cam, planes, ok)),
        "dst NULL": (A, (ctx, S, None, w, h, cam, planes, ok)),
        "camera NULL": (A, (ctx, S, D, w, h, None, planes, ok)),
        "planes NULL": (A, (ctx, S, D, w, h, cam, None, ok)),
        "params NULL": (A, (ctx, S, D, w, h, cam, planes, None)),
        "dst == prev": (A, (ctx, D, D, w, h, cam, planes, ok)),
        "max_history 0": (A, (ctx, S, D, w, h, cam, planes, (0, 1, 1e-5, 0))),
        "max_history 2^24 + 1": (A, (ctx, S, D, w, h, cam, planes, ((1 << 24) + 1, 1, 1e-5, 0))),
        "lambertian_only 2": (A, (ctx, S, D, w, h, cam, planes, (64, 2, 1e-5, 0))),
        "_reserved 1": (A, (ctx, S, D, w, h, cam, planes, (64, 1, 1e-5, 1))),
        "degenerate camera": (A, (ctx, S, D, w, h, degenerate, planes, ok)),
        "width 0": (Z, (ctx, S, D, 0, h, cam, planes, ok)),
        "height 0": (Z, (ctx, S, D, w, 0, cam, planes, ok)),
        "width 65537": (Z, (ctx, S, D, 65537, h, cam, planes, ok)),
        "height 65537": (Z, (ctx, S, D, w, 65537, cam, planes, ok)),
    }
    fields = [f for f, _ in rt._lib.ReprojectPlanesC._fields_]
    for i, f in enumerate(fields):
        rows[f"{f} NULL"] = (A, (ctx, S, D, w, h, cam, planes[:i] + (None,) + planes[i + 1:], ok))
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf")),
                      ("-inf", float("-inf"))]:
        rows[f"tolerance {what}"] = (A, (ctx, S, D, w, h, cam, planes, (64, 1, bad, 0)))
    for what, (status, args) in rows.items():
        with pytest.raises(rt.RtError) as e:
            raw_call(rt, pipe, *args)
        assert e.value.status == status, what
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == F32(SENT)).all(), "a refused call wrote dst"
    # without lambertian_only the material plane is not required, and the context still works
    raw_call(rt, pipe, ctx, S, D, w, h, cam, planes[:5] + (None,), (64, 0, 1e-5, 0))
    torch.cuda.synchronize()
    check(dst.cpu().numpy()[:px].reshape(h, w, 4), "pan", variant(lamb=0))


@gpu
@pytest.mark.parametrize("v", [("pan", variant(lamb=1)), ("counts", variant(32, 1)),
                               ("counts", variant(32, 0))], ids=_id)
def test_the_tracer_takes_the_reprojected_image(rt, oracle, pipe, v):
    """Per-pixel mixed counts, zeros among them, through the one-frame and the fused kernels."""
    import torch
    name, var = v
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
    seeds = np.array(rt.frame_seeds(11, 3), F32)
    images = (rep, out)
    newest = pipe.update_frames(rep, out, c.w, c.h, still, c.sc, seeds)
    torch.cuda.synchronize()
    three, _ = oracle.render(want, still.blob, c.cur.spheres, seeds)
    assert bits_equal(images[newest].cpu().numpy(), three)[0]


@gpu
def test_reprojecting_into_a_rendered_image_drops_its_count(rt, oracle):
    """4 frames leave a uniform count on record for the image; reprojection into that image
    makes the counts per-pixel, and the next frames still equal the oracle's."""
    import torch
    c = case("pan")
    w, h = c.w, c.h
    seeds = np.array(rt.frame_seeds(3, 4), F32)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, b = p.new_image(w, h), p.new_image(w, h)
        images = (a, b)
        newest = p.update_frames(a, b, w, h, c.prev.cam, c.sc, seeds)
        torch.cuda.synchronize()
        prev = images[newest].clone()
        prev_host = prev.cpu().numpy()
        d = device_inputs(p, c)
        prev_guides, guides = guides_of(d)
        p.reproject(prev, w, h, c.prev.cam, prev_guides, guides, out=images[newest])
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
    want4, _ = oracle.render(np.zeros((h, w, 4), F32), c.prev.cam.blob, c.cur.spheres, seeds)
    assert bits_equal(prev_host, want4)[0]
    want = reproject_ref(want4, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit,
                         c.normal, c.cur.material, c.prev.cam.blob, 64, 1, 1e-5)
    assert bits_equal(rep, want)[0]
    assert set(np.unique(want[..., 3])) == {0.0, 4.0}
    after, _ = oracle.render(want, still.blob, c.cur.spheres, more)
    assert bits_equal(got, after)[0]


@gpu
def test_the_denoiser_takes_the_reprojected_image(rt, oracle, pipe):
    import torch
    c = case("pan")
    var = variant(lamb=1)
    want, _ = expected("pan", var)
    still = c.cur.cam.with_fields(camera_has_moved=0.0)
    d = device_inputs(pipe, c)
    prev_guides, guides = guides_of(d)
    rep = pipe.reproject(d.prev_rgba, c.w, c.h, c.prev.cam, prev_guides, guides)
    out = pipe.new_image(c.w, c.h)
    pipe.update(rep, out, c.w, c.h, still, c.sc)
    den = pipe.denoise(out, c.w, c.h, guides)
    torch.cuda.synchronize()
    one, _ = oracle.update(want, still.blob, c.cur.spheres)
    n, npow, ic, ip = td.DEFAULTS
    ref = td.denoise_ref(one, c.cur.hit, c.cur.normal, c.cur.sphere_id, n, npow, ic, ip)
    assert bits_equal(den.cpu().numpy(), ref)[0]
