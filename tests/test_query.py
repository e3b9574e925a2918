"""Ray queries (include/rt_query.h): rt_cast_rays (closest hit, occlusion) and rt_cast_ray.

Every plane is compared bit for bit (NaN == NaN) with cast_ref below: the oracle's exported
sphere_hit (oracle_sphere_hit, wgsl:182-221) chained over the spheres in index order with
tmin = 0.001 and a running tmax started at the ray's own bound T = tmax < 3.4e35 ? tmax : 3.4e35
— test_aov.reference's loop with the ray and the start bound taken from the record.

The ray families aim at the routes a camera does not choose: origins inside the scene's box
(grid walkers), inside the glass sphere (second roots), surface-to-surface segments with
tmax = 1, far coherent beams (the cone), far rays past the scene (the grid's far-ray rule), rays
with zero components from integer coordinates, degenerate and non-finite rays, bounds on and
beside the rays' own roots, and all of them interleaved lane by lane.  The CPU tests check, from
the reference alone, that every family reaches what it names; they print the tallies (run with
-s).  The GPU tests print the waves per route.
"""
import ctypes
import functools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import bits_equal
import test_aov as A

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_query.h"
LIB = ROOT / "gpu-ray-tracing_amd" / "build" / "librt_hip.so"
F32 = np.float32
PLANES = A.PLANES
MISS = A.MISS
SENT_F, SENT_I, TAIL = A.SENT_F, A.SENT_I, A.TAIL
T_SHADER = F32(3.4e35)                 # wgsl:266
TMIN = F32(0.001)
RT_ERR_INVALID_ARGUMENT, RT_ERR_INVALID_SIZE, RT_ERR_INVALID_CONTEXT = 1, 2, 6
MODES = ["culled", "exhaustive"]
ROUTES = ("grid", "cone", "exhaustive")
MAX_DEFAULT_RAYS = 257                 # per family on the default scene (the reference's cost)
INSIDE_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1000]      # wave and workgroup edges


# ---- scenes -----------------------------------------------------------------------------------
def _scene(name):
    import gpu_ray_tracing as rt
    if name == "three":
        s = rt.three_spheres().spheres
    elif name == "n40":
        s = rt.synthetic_scene(40).spheres
    elif name == "default":
        s = rt.create_default_spheres(1).spheres
    elif name == "empty":
        s = np.zeros((0, 8), F32)
    elif name == "tie":
        s = np.concatenate([rt.synthetic_scene(40).spheres, rt.synthetic_scene(40).spheres[-1:]])
    else:
        raise KeyError(name)
    s = np.ascontiguousarray(s, F32).reshape(-1, 8).copy()
    s.setflags(write=False)
    return s


SCENES = ["three", "n40", "default", "empty", "tie"]


@functools.lru_cache(None)
def scene(name):
    import gpu_ray_tracing as rt
    s = _scene(name)
    return SimpleNamespace(name=name, spheres=s, sc=rt.SphereCollection(s))


def _shape_of(name):
    """The spheres the ray families are built around: the scene's own, n40's for the empty one."""
    s = scene("n40" if name == "empty" else name).spheres
    return s[np.abs(s[:, 3]) < 100.0]                     # without the ground


# ---- ray families -----------------------------------------------------------------------------
def _rays(o, d, tmax=np.inf):
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    r = np.zeros((o.shape[0], 8), F32)
    r[:, 0:3], r[:, 4:7] = o, d
    r[:, 3] = tmax
    return r


def _units(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _box(small):
    lo = small[:, :3].min(0) - 1.0
    hi = small[:, :3].max(0) + 1.0
    lo[1], hi[1] = 0.05, 2.5
    return lo, hi


def fam_camera(name):
    import gpu_ray_tracing as rt
    cam = A.default_camera(rt, A.W, A.H)
    rays = np.array([A.centre_ray(cam.blob, x, y) for y in range(A.H) for x in range(A.W)])
    return _rays(rays[:, :3], rays[:, 3:])


def fam_inside(name, n=MAX_DEFAULT_RAYS, seed=11):
    rng = np.random.default_rng(seed)
    lo, hi = _box(_shape_of(name))
    o = lo + (hi - lo) * rng.random((n, 3))
    d = _units(rng, n) * rng.uniform(0.5, 2.0, (n, 1))
    return _rays(o, d)


def fam_glass(name, n=128, seed=12):
    rng = np.random.default_rng(seed)
    o = np.array([0.0, 1.0, 0.0]) + _units(rng, n) * 0.95 * rng.random((n, 1)) ** (1.0 / 3.0)
    d = _units(rng, n) * rng.uniform(0.5, 2.0, (n, 1))
    return _rays(o, d)


def fam_segments(name, n=256, seed=13):
    """o on one sphere's surface pushed out by 1 %, d to a point on a nearby sphere, tmax = 1."""
    rng = np.random.default_rng(seed)
    s = _shape_of(name)
    i = rng.integers(0, s.shape[0], n)
    dist = np.linalg.norm(s[i, None, :3] - s[None, :, :3], axis=2)
    dist[np.arange(n), i] = np.inf
    near = np.argsort(dist, axis=1)[:, :3]                # the three nearest other spheres
    j = near[np.arange(n), rng.integers(0, min(3, s.shape[0] - 1), n)]
    u1, u2 = _units(rng, n), _units(rng, n)
    # every other segment runs between the two spheres' facing sides, where the far end's own
    # root lies on either side of tmax = 1 by rounding alone; the rest start and end anywhere
    axis = s[j, :3] - s[i, :3]
    facing = (np.arange(n) % 2 == 0)[:, None]
    u1 = np.where(facing & ((u1 * axis).sum(1, keepdims=True) < 0), -u1, u1)
    u2 = np.where(facing & ((u2 * axis).sum(1, keepdims=True) > 0), -u2, u2)
    o = s[i, :3] + 1.01 * s[i, 3:4] * u1
    target = s[j, :3] + s[j, 3:4] * u2
    return _rays(o, target - o, 1.0)


def fam_far(name, seed=14):
    """Four waves: two coherent beams aimed at the scene from 1e3-1e5 away (one origin per
    wave), one wave of rays past the scene, one of rays away from it."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(_shape_of(name))
    mid = 0.5 * (lo + hi)
    waves = []
    for w, dist in enumerate([1.0e3, 1.0e5, 3.0e3, 3.0e4]):
        up = _units(rng, 1)[0]
        up[1] = abs(up[1]) + 0.2                          # above the ground
        origin = mid + dist * up / np.linalg.norm(up)
        o = origin + rng.normal(size=(64, 3)) * 1e-3 * dist * (w >= 2)
        to = lo + (hi - lo) * rng.random((64, 3)) - o
        to /= np.linalg.norm(to, axis=1, keepdims=True)
        if w == 2:                                        # past: 20-60 degrees off the scene
            side = np.cross(to, _units(rng, 64))
            side /= np.linalg.norm(side, axis=1, keepdims=True)
            ang = rng.uniform(0.35, 1.0, (64, 1))
            to = np.cos(ang) * to + np.sin(ang) * side
        if w == 3:
            to = -to
        waves.append(_rays(o, to * rng.uniform(0.5, 2.0, (64, 1))))
    return np.concatenate(waves)


def fam_axis(name, n=192, seed=15):
    """One or two zero components of d, origins on integer x / z."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(_shape_of(name))
    o = np.empty((n, 3))
    o[:, 0] = rng.integers(int(np.ceil(lo[0])), int(np.floor(hi[0])) + 1, n)
    o[:, 2] = rng.integers(int(np.ceil(lo[2])), int(np.floor(hi[2])) + 1, n)
    o[:, 1] = rng.choice([0.2, 0.5, 1.0, 3.0], n)
    d = rng.uniform(0.3, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    zero = rng.integers(0, 6, n)          # 0-2: one zero component, 3-5: two
    for k in range(n):
        if zero[k] < 3:
            d[k, zero[k]] = 0.0
        else:
            d[k, [c for c in range(3) if c != zero[k] - 3]] = 0.0
    return _rays(o, d)


TMAX_EDGES = [np.nan, -1.0, 0.0, 0.001, float(np.nextafter(F32(0.001), F32(1.0))), 1e38, np.inf]


def fam_degenerate(name, seed=16):
    base = fam_inside(name, 64, seed=seed)
    glass = fam_glass(name, 8, seed=seed)
    out = []
    z = base[:8].copy(); z[:, 4:7] = 0.0; out.append(z)                    # d = 0
    z = glass.copy(); z[:, 4:7] = 0.0; out.append(z)                       # d = 0 inside a sphere
    z = base[8:16].copy(); z[np.arange(8), np.arange(8) % 3] = np.nan; out.append(z)
    z = base[16:24].copy(); z[np.arange(8), 4 + np.arange(8) % 3] = np.inf; out.append(z)
    z = base[24:32].copy(); z[:, 4:7] *= F32(2.0 ** -11); out.append(z)    # |d|^2 < 2^-20
    z = base[32:40].copy(); z[:, 4:7] *= F32(2000.0); out.append(z)        # |d|^2 > 2^20
    for t in TMAX_EDGES:                                                   # the same eight rays
        z = base[40:48].copy(); z[:, 3] = t; out.append(z)
        z = glass.copy(); z[:, 3] = t; out.append(z)
    return np.concatenate(out)


def fam_bound(name):
    """The rays of `inside` that hit, with tmax at, just below and just above their own t."""
    ref = reference("inside", name)
    hit = np.nonzero(ref.want["sphere_id"] != MISS)[0][:85]
    t = ref.want["hit"][hit, 3]
    out = []
    for tm in (t, np.nextafter(t, F32(0.0)), np.nextafter(t, F32(np.inf))):
        z = ref.rays[hit].copy()
        z[:, 3] = tm
        out.append(z)
    return np.concatenate(out) if hit.size else np.zeros((0, 8), F32)


def fam_mixed(name):
    """The families interleaved ray by ray: walkers, far rays and degenerate lanes share waves."""
    parts = [family(f, name) for f in ("inside", "far", "degenerate", "axis", "segments")]
    n = 64
    out = np.empty((n * len(parts), 8), F32)
    for k, p in enumerate(parts):
        out[k::len(parts)] = p[np.arange(n) % p.shape[0]]
    return out


FAMILIES = {"camera": fam_camera, "inside": fam_inside, "glass": fam_glass,
            "segments": fam_segments, "far": fam_far, "axis": fam_axis,
            "degenerate": fam_degenerate, "bound": fam_bound, "mixed": fam_mixed}


@functools.lru_cache(None)
def family(fam, name):
    rays = np.ascontiguousarray(FAMILIES[fam](name), F32)
    if name == "default" and rays.shape[0] > MAX_DEFAULT_RAYS:
        rays = np.ascontiguousarray(rays[::-(-rays.shape[0] // MAX_DEFAULT_RAYS)])
    rays.setflags(write=False)
    return rays


# ---- the reference ----------------------------------------------------------------------------
def bound_of(tmax):
    tmax = F32(tmax)
    return tmax if tmax < T_SHADER else T_SHADER


def cast_ref(rays, spheres, own=False):
    """The four planes and the occlusion word of every ray (read-only arrays).  own: also
    "some sphere passes its own test against T" (a second call per sphere once the running tmax
    has left T)."""
    from oracle import oracle
    hit_fn = oracle.lib().oracle_sphere_hit
    sph = np.ascontiguousarray(spheres, F32).reshape(-1, 8)
    base = sph.ctypes.data
    recs = [ctypes.c_void_p(base + 32 * i) for i in range(sph.shape[0])]
    n = rays.shape[0]
    ray = np.zeros(6, F32)
    out = np.zeros(8, F32)
    pray, pout = ctypes.c_void_p(ray.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    tmin = ctypes.c_float(0.001)
    ids = np.full(n, MISS, np.int32)
    hit = np.zeros((n, 4), F32)
    hit[:, 3] = np.inf
    normal = np.zeros((n, 4), F32)
    material = np.zeros((n, 4), F32)
    own_any = np.zeros(n, np.int32)
    scratch = np.zeros(8, F32)
    pscratch = ctypes.c_void_p(scratch.ctypes.data)
    with np.errstate(all="ignore"):
        for r in range(n):
            ray[0:3], ray[3:6] = rays[r, 0:3], rays[r, 4:7]
            T = ctypes.c_float(bound_of(rays[r, 3]))
            tmax, moved = T, False
            for i, rec in enumerate(recs):
                accepted = hit_fn(rec, pray, tmin, tmax, pout)
                if not moved:                       # the running tmax is still T: the own test
                    own_any[r] |= int(accepted)
                elif own:
                    own_any[r] |= int(hit_fn(rec, pray, tmin, T, pscratch))
                if accepted:
                    tmax, moved = ctypes.c_float(out[0]), True
                    ids[r] = i
                    hit[r, :3], hit[r, 3] = out[1:4], out[0]
                    normal[r] = out[4:8]
                    material[r] = sph[i, 4:8]
    res = {"sphere_id": ids, "hit": hit, "normal": normal, "material": material}
    occluded = (ids != MISS).astype(np.int32)
    for a in list(res.values()) + [occluded, own_any]:
        a.setflags(write=False)
    return res, occluded, own_any


@functools.lru_cache(None)
def reference(fam, name):
    rays = family(fam, name)
    want, occluded, own_any = cast_ref(rays, scene(name).spheres, own=name != "default")
    return SimpleNamespace(rays=rays, want=want, occluded=occluded, own_any=own_any,
                           checked_own=name != "default")


# ---- CPU tests --------------------------------------------------------------------------------
def test_library_exports_the_query_entry_points(rt):
    want = {"rt_cast_rays", "rt_cast_ray"}
    assert set(rt._lib.query_symbols()) == want
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    assert want <= set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    declared = set(re.findall(r"RT_API\s+rt_status\s+(rt_\w+)\s*\(", HEADER.read_text()))
    assert declared == want
    assert rt._lib.lib().rt_abi_version() == 7
    assert ctypes.sizeof(rt._lib.RayC) == 32 and ctypes.sizeof(rt._lib.QueryPlanesC) == 40
    assert rt.QUERY_ROUTES == ROUTES


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc):
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                        "-I", str(HEADER.parent), "-include", "rt_query.h", "/dev/null"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_struct_sizes_in_a_compiled_c_program(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rt_query.h"\n'
                   'int main(void) { printf("%zu %zu %u %u\\n", sizeof(rt_ray), '
                   'sizeof(rt_query_planes), RT_QUERY_CLOSEST, RT_QUERY_OCCLUSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", str(HEADER.parent), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["32", "40", "0", "1"]


def test_camera_family_is_test_aovs_reference():
    c = A.case("n40")
    ref = reference("camera", "n40")
    assert ref.rays.shape[0] == c.w * c.h
    for k in PLANES:
        want = c.want[k].reshape(ref.want[k].shape)
        assert want.tobytes() == ref.want[k].tobytes(), k


def _tally(ref):
    ids, nrm, t = ref.want["sphere_id"], ref.want["normal"], ref.want["hit"][:, 3]
    hits = int((ids != MISS).sum())
    return SimpleNamespace(n=ids.size, hits=hits, miss=ids.size - hits,
                           back=int(((ids != MISS) & (nrm[:, 3] == 0.0)).sum()),
                           nan_t=int(((ids != MISS) & np.isnan(t)).sum()))


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_families_reach_what_they_name(fam):
    ref = reference(fam, "n40")
    rays, ids, t = ref.rays, ref.want["sphere_id"], ref.want["hit"][:, 3]
    s = _tally(ref)
    print(f"{fam} on n40: {s.n} rays, {s.hits} hit, {s.miss} miss, {s.back} back-face, "
          f"{s.nan_t} NaN t")
    assert s.n >= 64
    if fam in ("camera", "inside", "segments"):
        assert s.hits >= 0.1 * s.n and s.miss >= 0.1 * s.n
    if fam == "segments":
        assert (rays[:, 3] == 1.0).all()
    if fam == "glass":
        g = A.glass_index(scene("n40").spheres)
        assert s.back >= 5 and int(((ids == g) & (ref.want["normal"][:, 3] == 0.0)).sum()) >= 5
    if fam == "far":
        dist = np.linalg.norm(rays[:, :3], axis=1)
        assert dist.min() >= 9e2 and dist.max() <= 1.1e5
        assert int((ids == 0).sum()) >= 1 and s.miss >= 1     # sphere 0 is the ground
        print(f"far: {int((ids == 0).sum())} ground hits, {int((ids > 0).sum())} other hits")
    if fam == "axis":
        zeros = (rays[:, 4:7] == 0.0).sum(1)
        assert set(zeros) == {1, 2}
        assert (rays[:, 0] == np.round(rays[:, 0])).all() and (rays[:, 2] == np.round(rays[:, 2])).all()
        assert s.hits >= 1 and s.miss >= 1
    if fam == "degenerate":
        d2 = (rays[:, 4:7].astype(np.float64) ** 2).sum(1)
        assert (d2 == 0.0).any() and np.isnan(rays[:, :3]).any() and np.isinf(rays[:, 4:7]).any()
        assert ((d2 > 0) & (d2 < 2.0 ** -20)).any() and (np.isfinite(d2) & (d2 > 2.0 ** 20)).any()
        assert s.nan_t >= 1
        for tm in TMAX_EDGES:
            sel = np.isnan(rays[:, 3]) if np.isnan(tm) else rays[:, 3] == F32(tm)
            assert sel.sum() >= 16
            h = int((ids[sel] != MISS).sum())
            print(f"degenerate: tmax {tm}: {int(sel.sum())} rays, {h} hit")
            if tm <= 0.001:
                assert h == 0
        big = np.isnan(rays[:, 3]) | (rays[:, 3] >= F32(1e38))
        assert (ids[big & (d2 > 0)] != MISS).any()
    if fam == "bound":
        n = s.n // 3
        base = reference("inside", "n40")
        hit = np.nonzero(base.want["sphere_id"] != MISS)[0][:85]
        t0, id0 = base.want["hit"][hit, 3], base.want["sphere_id"][hit]
        assert n == hit.size >= 20
        for part, what in ((0, "tmax = t"), (1, "tmax = nextafter(t, 0)")):
            got_id, got_t = ids[part * n:(part + 1) * n], t[part * n:(part + 1) * n]
            missed = got_id == MISS
            # a miss, or something that is not nearer than the unbounded hit
            assert (missed | (got_id != id0) | (got_t != t0)).all(), what
            assert (missed | (got_t >= t0)).all(), what
            print(f"bound, {what}: {int(missed.sum())} of {n} now miss")
            assert missed.any()
        assert (ids[2 * n:] == id0).all() and t[2 * n:].tobytes() == t0.tobytes()
    if fam == "mixed":
        src = [family(f, "n40") for f in ("inside", "far", "degenerate", "axis", "segments")]
        for k, p in enumerate(src):
            assert rays[k].tobytes() == p[0].tobytes()
        assert s.n == 320


def test_the_duplicated_record_never_wins():
    """... for any ray whose t is a number.  A ray with d = 0 gets a NaN root from every sphere,
    "tmax <= NaN" rejects nothing, so the shader's walk ends on the last record: those rays are
    the only ones the upper twin wins, and the tally says how many."""
    n = scene("tie").spheres.shape[0]
    assert scene("tie").spheres[-1].tobytes() == scene("tie").spheres[-2].tobytes()
    lower = nan_upper = 0
    for fam in FAMILIES:
        want = reference(fam, "tie").want
        ids, t = want["sphere_id"], want["hit"][:, 3]
        assert not ((ids == n - 1) & ~np.isnan(t)).any(), fam
        lower += int((ids == n - 2).sum())
        nan_upper += int((ids == n - 1).sum())
    print(f"tie: {lower} rays won by the lower twin, {nan_upper} NaN-t rays by the upper")
    assert lower >= 1


@pytest.mark.parametrize("name", SCENES)
def test_occlusion_is_order_independent(name):
    """occluded == "CLOSEST hit" == "some sphere passes its own test against T"."""
    for fam in FAMILIES:
        ref = reference(fam, name)
        assert (ref.occluded == (ref.want["sphere_id"] != MISS)).all()
        if ref.checked_own:
            assert (ref.own_any == ref.occluded).all(), fam
    if name == "empty":
        assert all(not reference(f, name).occluded.any() for f in FAMILIES)


# ---- GPU side ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


def guarded(p, n, planes=PLANES):
    return A.guarded(p, n, 1, planes)


def to_host(res, n):
    got = A.to_host(res, n, 1)
    return {k: (v[0].reshape((n,) if k == "sphere_id" else (n, 4)), v[1]) for k, v in got.items()}


def sentinel(k):
    return SENT_I if k in ("sphere_id", "occluded") else F32(SENT_F)


def device_rays(p, rays):
    import torch
    return torch.from_numpy(np.array(rays, F32)).to(p.torch_device)


def cast(p, rays, sc, planes=PLANES, routes=True):
    """(planes as numpy, route counts) from guarded buffers; asserts the tails are untouched."""
    import torch
    n = rays.shape[0]
    out = guarded(p, n, planes)
    rc = torch.zeros(3, dtype=torch.int32, device=p.torch_device) if routes else None
    res = p.cast_rays(rays, sc, planes=planes, out=out, route_counts=rc)
    assert set(res) == set(planes)
    got = to_host(res, n)
    for k, (_, tail) in got.items():
        assert tail.size == TAIL and (tail == sentinel(k)).all(), f"{k}: tail written"
    return {k: v[0] for k, v in got.items()}, (rc.cpu().numpy() if routes else None)


def occluded(p, rays, sc):
    import torch
    n = rays.shape[0]
    out = torch.full((n + TAIL,), SENT_I, dtype=torch.int32, device=p.torch_device)
    rc = torch.zeros(3, dtype=torch.int32, device=p.torch_device)
    res = p.occluded(rays, sc, out=out, route_counts=rc)
    assert res is out
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[n:] == SENT_I).all(), "occluded: tail written"
    return a[:n], rc.cpu().numpy()


def check_routes(rc, n, mode, what):
    assert int(rc.sum()) == (n + 63) // 64, f"{what}: route counts {rc} for {n} rays"
    if mode == "exhaustive":
        assert rc[0] == 0 and rc[1] == 0, f"{what}: {rc} in exhaustive mode"


PAIRS = [(s, f) for s in SCENES for f in FAMILIES]


@gpu
@pytest.mark.parametrize("name,fam", PAIRS)
def test_closest_matches_reference(pipe, name, fam):
    ref, sc = reference(fam, name), scene(name).sc
    n = ref.rays.shape[0]
    rays = device_rays(pipe, ref.rays)
    for mode in MODES:
        pipe.set_scan_mode(mode)
        got, rc = cast(pipe, rays, sc)
        print(f"{name} {fam} {mode}: {n} rays, routes {dict(zip(ROUTES, rc.tolist()))}")
        assert not A.differences(got, ref.want, f"{mode} ")
        check_routes(rc, n, mode, f"{name} {fam}")
        for k in PLANES:
            # every plane's buffer goes in through `out`; only the requested one may change
            out = guarded(pipe, n)
            res = pipe.cast_rays(rays, sc, planes=(k,), out=out)
            assert set(res) == {k}
            host = to_host(out, n)
            for q in PLANES:
                assert (host[q][1] == sentinel(q)).all(), f"({k},): tail of {q} written"
                if q == k:
                    assert not A.differences({q: host[q][0]}, ref.want, f"{mode} ({k},) ")
                else:
                    assert (host[q][0] == sentinel(q)).all(), f"({k},): plane {q} written"
    pipe.set_scan_mode("culled")


@gpu
@pytest.mark.parametrize("name,fam", PAIRS)
def test_occlusion_matches_reference(pipe, name, fam):
    ref, sc = reference(fam, name), scene(name).sc
    rays = device_rays(pipe, ref.rays)
    for mode in MODES:
        pipe.set_scan_mode(mode)
        got, rc = occluded(pipe, rays, sc)
        bad = np.nonzero(got != ref.occluded)[0]
        assert bad.size == 0, f"{mode}: {bad.size} rays differ, first {bad[:8]}"
        check_routes(rc, ref.rays.shape[0], mode, f"{name} {fam}")
    pipe.set_scan_mode("culled")


@gpu
@pytest.mark.parametrize("name", ["n40", "default"])
def test_ray_counts_at_wave_and_workgroup_edges(pipe, name):
    top = max(INSIDE_COUNTS) if name == "n40" else MAX_DEFAULT_RAYS
    rays = np.ascontiguousarray(fam_inside(name, top))
    want, occ, _ = cast_ref(rays, scene(name).spheres)
    for n in [c for c in INSIDE_COUNTS if c <= top]:
        got, rc = cast(pipe, rays[:n].copy(), scene(name).sc)       # NumPy rays: uploaded
        assert not A.differences(got, {k: v[:n] for k, v in want.items()}, f"{n} rays ")
        check_routes(rc, n, "culled", f"{n} rays")
        o, _ = occluded(pipe, device_rays(pipe, rays[:n]), scene(name).sc)
        assert (o == occ[:n]).all(), f"{n} rays"
    # no ray: nothing launched, nothing written
    out = guarded(pipe, 1)
    res = pipe.cast_rays(np.zeros((0, 8), F32), scene(name).sc, planes=PLANES, out=out)
    assert set(res) == set(PLANES)
    for k, (img, tail) in to_host(out, 1).items():
        assert (img == sentinel(k)).all() and (tail == sentinel(k)).all()


def _record_equals(r, planes, i):
    sid = int(planes["sphere_id"][i])
    if sid == MISS:
        return r is None
    return (r is not None and r["sphere_id"] == sid
            and bits_equal(r["p"], planes["hit"][i, :3])[0]
            and bits_equal(r["t"], planes["hit"][i, 3])[0]
            and bits_equal(r["normal"], planes["normal"][i, :3])[0]
            and r["front_face"] == bool(planes["normal"][i, 3])
            and bits_equal(r["color"], planes["material"][i])[0])


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_cast_ray_equals_the_row_and_pick(rt, pipe, mode):
    pipe.set_scan_mode(mode)
    for name in ("n40", "default"):
        sc = scene(name).sc
        fams = ("camera", "inside", "glass", "segments", "far", "axis", "degenerate", "bound")
        kinds = set()
        for j, fam in enumerate(fams):
            ref = reference(fam, name)
            for i in (j % ref.rays.shape[0], ref.rays.shape[0] - 1 - j):
                ray = ref.rays[i]
                r = pipe.cast_ray(ray[0:3], ray[4:7], sc, tmax=ray[3])
                assert _record_equals(r, ref.want, i), (name, fam, i)
                kinds.add(r is None)
        assert kinds == {True, False}
    # a pixel's centre ray is rt_pick's ray
    c = A.case("n40")
    for x, y in A.pick_pixels(c):
        ray = A.centre_ray(c.cam.blob, x, y)
        a = pipe.cast_ray(ray[:3], ray[3:], c.sc)
        b = pipe.pick(c.w, c.h, x, y, c.cam, c.sc)
        assert (a is None) == (b is None), (x, y)
        if a is not None:
            assert a["sphere_id"] == b["sphere_id"] and a["front_face"] == b["front_face"]
            for k in ("t", "p", "normal", "color"):
                assert bits_equal(a[k], b[k])[0], (x, y, k)
    # a miss through the C struct itself
    rec, ray = rt._lib.PickResultC(), rt._lib.RayC((0, 50, 0), np.inf, (0, 1, 0), 0)
    p, n = pipe._spheres(c.sc)
    rt._lib.call("rt_cast_ray", pipe._ctx, ctypes.byref(ray), p, n, pipe._stream(),
                 ctypes.byref(rec))
    assert rec.sphere_id == rt.RT_AOV_MISS and np.isposinf(rec.t) and rec.front_face == 0
    assert not any(rec.p) and not any(rec.normal) and not any(rec.color)
    pipe.set_scan_mode("culled")


@gpu
@pytest.mark.parametrize("name", ["n40", "default"])
def test_camera_rays_equal_trace_aov_on_the_device(rt, pipe, name):
    import torch
    sc = scene(name).sc
    cam = A.default_camera(rt, A.W, A.H)
    rays = device_rays(pipe, fam_camera(name))
    for mode in MODES:
        pipe.set_scan_mode(mode)
        aov = pipe.trace_aov(A.W, A.H, cam, sc, planes=PLANES)
        got = pipe.cast_rays(rays, sc, planes=PLANES)
        for k in PLANES:
            a, b = aov[k].reshape(got[k].shape), got[k]
            same = a.view(torch.int32) == b.view(torch.int32)
            if k != "sphere_id":
                same |= torch.isnan(a) & torch.isnan(b)
            assert bool(same.all()), f"{name} {mode} {k}"
    pipe.set_scan_mode("culled")


@gpu
def test_every_route_is_reached(pipe):
    """In culled mode the grid, the cone and the exhaustive walk are each taken by some wave,
    by the family that aims at it."""
    pipe.set_scan_mode("culled")
    table = {}
    for name in ("n40", "default"):
        for fam in FAMILIES:
            rays = reference(fam, name).rays
            _, rc = cast(pipe, device_rays(pipe, rays), scene(name).sc, planes=("sphere_id",))
            table[name, fam] = rc
            print(f"routes {name:8s} {fam:10s} {dict(zip(ROUTES, rc.tolist()))}")
    # n40 is below the grid's 64 spheres: cone or exhaustive only
    assert all(table["n40", f][0] == 0 for f in FAMILIES)
    assert table["n40", "camera"][1] >= 1 and table["n40", "far"][1] >= 1
    assert table["n40", "mixed"][2] >= 1
    assert table["default", "inside"][0] >= 1          # walkers
    assert table["default", "far"][0] >= 1             # far rays that share a walk
    assert table["default", "far"][1] >= 1             # far coherent beams
    assert table["default", "mixed"][2] >= 1           # degenerate lanes in the wave
    assert table["default", "degenerate"][2] >= 1


@gpu
def test_a_context_that_only_answers_queries(rt, pipe):
    """No render, no G-buffer before the first query: the reference's bits, and the routes of
    a context that rendered first (the grid is built by the scene upload itself)."""
    import torch
    name = "default"
    refs = [reference(f, name) for f in ("inside", "far", "mixed")]
    sc = scene(name).sc
    fresh = rt.ComputeShaderPipeline(0)
    rendered = rt.ComputeShaderPipeline(0)
    try:
        w, h = 64, 40
        cam = rt.SceneCamera.from_settings(rt.CameraSettings(max_depth=3), w, h, 0.5)
        a, b = rendered.new_image(w, h), rendered.new_image(w, h)
        rendered.update(a, b, w, h, cam, sc)
        torch.cuda.synchronize()
        for ref in refs:
            g1, r1 = cast(fresh, ref.rays, sc)
            g2, r2 = cast(rendered, ref.rays, sc)
            assert not A.differences(g1, ref.want, "fresh ")
            assert not A.differences(g2, ref.want, "rendered ")
            assert (r1 == r2).all(), (r1, r2)
        assert cast(fresh, refs[0].rays, sc)[1][0] >= 1       # the fresh context has the grid
    finally:
        fresh.close()
        rendered.close()


@gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_render_is_undisturbed(rt, oracle, depth):
    """4 frames of update_frames, against 2 frames + queries + 2 frames on the same context:
    the same two images, the oracle's, and no trace of the queries in the launch info or the
    candidate lists."""
    import torch
    w, h = 64, 40
    g = A.case("undisturbed_aov")
    sc = rt.SphereCollection(g.spheres)
    cam = rt.SceneCamera.from_settings(rt.CameraSettings(max_depth=depth), w, h, 0.5)
    still = cam.with_fields(camera_has_moved=0.0)
    seeds = np.array(rt.frame_seeds(5, 4), F32)
    want, cur = [], np.zeros((h, w, 4), F32)
    for k, s in enumerate(seeds):
        cur, _ = oracle.update(cur, (cam if k == 0 else still).with_fields(
            random_seed=float(s)).blob, g.spheres)
        want.append(cur)
    ref = reference("mixed", "n40")
    assert g.spheres.tobytes() == scene("n40").spheres.tobytes()
    p = rt.ComputeShaderPipeline(0)
    try:
        a, b = p.new_image(w, h), p.new_image(w, h)
        p.update_frames(a, b, w, h, cam, sc, seeds)
        torch.cuda.synchronize()
        seq_a = (a.cpu().numpy(), b.cpu().numpy())
        a2, b2 = p.new_image(w, h), p.new_image(w, h)
        p.update_frames(a2, b2, w, h, cam, sc, seeds[:2])
        info, stats = p.last_launch_info(), p.candidate_stats()
        planes = p.cast_rays(ref.rays, sc, planes=PLANES)
        occ = p.occluded(ref.rays, sc)
        one = p.cast_ray(ref.rays[0, 0:3], ref.rays[0, 4:7], sc, tmax=ref.rays[0, 3])
        assert p.last_launch_info() == info
        assert p.candidate_stats() == stats
        p.update_frames(a2, b2, w, h, still, sc, seeds[2:])
        torch.cuda.synchronize()
        seq_b = (a2.cpu().numpy(), b2.cpu().numpy())
        got = {k: v.cpu().numpy() for k, v in planes.items()}
        occ = occ.cpu().numpy()
    finally:
        p.close()
    assert not A.differences(got, ref.want, "the queries in between ")
    assert (occ == ref.occluded).all() and _record_equals(one, ref.want, 0)
    for i, nm in enumerate("ab"):
        assert bits_equal(seq_b[i], seq_a[i])[0], f"image_{nm} differs between the sequences"
    assert bits_equal(seq_a[0], want[3])[0] and bits_equal(seq_a[1], want[2])[0]
    assert bits_equal(seq_b[0], want[3])[0] and bits_equal(seq_b[1], want[2])[0]


@gpu
def test_queries_on_a_side_stream(rt):
    import torch
    a, b = reference("inside", "n40"), reference("mixed", "default")
    p = rt.ComputeShaderPipeline(0)
    try:
        first = p.cast_rays(a.rays, scene("n40").sc, planes=PLANES)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            res = p.cast_rays(b.rays, scene("default").sc, planes=PLANES)
            occ = p.occluded(b.rays, scene("default").sc)
        side.synchronize()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        got_a = {k: v.cpu().numpy() for k, v in first.items()}
        occ = occ.cpu().numpy()
    finally:
        p.close()
    assert not A.differences(got_a, a.want, "first scene ")
    assert not A.differences(got, b.want, "new scene on the side stream ")
    assert (occ == b.occluded).all()


@gpu
def test_errors_launch_nothing(rt, pipe):
    import torch
    L = rt._lib
    ref, sc = reference("inside", "three"), scene("three").sc
    n = ref.rays.shape[0]
    rays = device_rays(pipe, ref.rays)
    out = guarded(pipe, n)
    occ = torch.full((n + TAIL,), SENT_I, dtype=torch.int32, device=pipe.torch_device)
    rc = torch.full((3,), SENT_I, dtype=torch.int32, device=pipe.torch_device)
    record = [out[k].data_ptr() for k in PLANES]
    closest = L.QueryPlanesC(*record, None)
    occl = L.QueryPlanesC(None, None, None, None, occ.data_ptr())
    both = L.QueryPlanesC(*record, occ.data_ptr())
    mixed = L.QueryPlanesC(record[0], None, None, None, occ.data_ptr())
    sp, ns = pipe._spheres(sc)
    stream = pipe._stream()
    r, cr = rays.data_ptr(), rc.data_ptr()

    def rays_call(ctx, rp, count, mode, planes, spheres, nsph):
        return lambda: L.call("rt_cast_rays", ctx, rp, count, mode,
                              ctypes.byref(planes) if planes is not None else None, spheres,
                              nsph, cr, stream)

    one, rec = L.RayC((0, 1, 5), np.inf, (0, 0, -1), 0), L.PickResultC()
    calls = {
        "ctx NULL": (RT_ERR_INVALID_CONTEXT, rays_call(None, r, n, 0, closest, sp, ns)),
        "rays NULL": (RT_ERR_INVALID_ARGUMENT, rays_call(pipe._ctx, None, n, 0, closest, sp, ns)),
        "planes NULL": (RT_ERR_INVALID_ARGUMENT, rays_call(pipe._ctx, r, n, 0, None, sp, ns)),
        "mode 2": (RT_ERR_INVALID_ARGUMENT, rays_call(pipe._ctx, r, n, 2, closest, sp, ns)),
        "closest, no plane": (RT_ERR_INVALID_ARGUMENT,
                              rays_call(pipe._ctx, r, n, 0, L.QueryPlanesC(), sp, ns)),
        "closest with occluded": (RT_ERR_INVALID_ARGUMENT,
                                  rays_call(pipe._ctx, r, n, 0, both, sp, ns)),
        "closest, occluded only": (RT_ERR_INVALID_ARGUMENT,
                                   rays_call(pipe._ctx, r, n, 0, occl, sp, ns)),
        "occlusion with a record plane": (RT_ERR_INVALID_ARGUMENT,
                                          rays_call(pipe._ctx, r, n, 1, mixed, sp, ns)),
        "occlusion without occluded": (RT_ERR_INVALID_ARGUMENT,
                                       rays_call(pipe._ctx, r, n, 1, closest, sp, ns)),
        "spheres NULL": (RT_ERR_INVALID_ARGUMENT, rays_call(pipe._ctx, r, n, 0, closest, None, 3)),
        "count above 2^32 - 64": (RT_ERR_INVALID_SIZE,
                                  rays_call(pipe._ctx, r, 2 ** 32 - 63, 0, closest, sp, ns)),
        "cast_ray ctx NULL": (RT_ERR_INVALID_CONTEXT,
                              lambda: L.call("rt_cast_ray", None, ctypes.byref(one), sp, ns,
                                             stream, ctypes.byref(rec))),
        "cast_ray ray NULL": (RT_ERR_INVALID_ARGUMENT,
                              lambda: L.call("rt_cast_ray", pipe._ctx, None, sp, ns, stream,
                                             ctypes.byref(rec))),
        "cast_ray out NULL": (RT_ERR_INVALID_ARGUMENT,
                              lambda: L.call("rt_cast_ray", pipe._ctx, ctypes.byref(one), sp, ns,
                                             stream, None)),
        "cast_ray spheres NULL": (RT_ERR_INVALID_ARGUMENT,
                                  lambda: L.call("rt_cast_ray", pipe._ctx, ctypes.byref(one),
                                                 None, 3, stream, ctypes.byref(rec))),
    }
    for what, (status, fn) in calls.items():
        with pytest.raises(rt.RtError) as e:
            fn()
        assert e.value.status == status, what
    for bad in (ref.rays[:, :7], ref.rays.astype(np.float64).reshape(-1)):
        with pytest.raises(ValueError):
            pipe.cast_rays(bad, sc)
    with pytest.raises(ValueError):
        pipe.cast_rays(rays, sc, out={"hit": out["hit"][:8]})
    torch.cuda.synchronize()
    for k, (img, tail) in to_host(out, n).items():
        assert (img == sentinel(k)).all() and (tail == sentinel(k)).all(), f"a refused call wrote {k}"
    assert (occ.cpu().numpy() == SENT_I).all() and (rc.cpu().numpy() == SENT_I).all()
    # the context still works
    got, _ = cast(pipe, rays, sc)
    assert not A.differences(got, ref.want)
