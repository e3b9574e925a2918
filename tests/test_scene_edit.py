"""Carrying the accumulator across scene edits (include/rt_scene_edit.h): rt_edit_plan,
rt_edit_carry, rt_edit_plan_bytes, rt_edit_params_default.

The references are in this file: `edit_plan_ref`, a NumPy float32 restatement of the header's plan
rules that returns the table's bytes, and `carry_ref`, its per-pixel text vectorised, which also
tallies how often each rule fires (tests/test_reproject.py's tallies plus `guard`, `link_none`,
`near`, `near_restart`, `near_capped`, `moved`).  Planes, cameras and the previous accumulator
(16 frames of the CPU oracle, max_depth 4) are built as tests/test_reproject.py builds them, for
the previous and the edited scene.  Every GPU output is compared bit for bit (NaN == NaN).

The rule cases are 96 x 64, where the edited sphere (index 38: radius 1, Lambertian) covers about
130 pixels; the size sweep and the plans with 0, 1 and 32 balls use smaller images.  No GPU test
feeds an id >= n_records: that guard runs in the reference only and is read in the kernel.
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
import test_reproject as tr
from conftest import bits_equal

gpu = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rt_scene_edit.h"
LIB = tr.LIB
F32 = np.float32
U32 = np.uint32
MISS = tr.MISS
NONE, MOVED, MAX_BALLS = 0xFFFFFFFF, 0x80000000, 32
A, Z, C = tr.RT_ERR_INVALID_ARGUMENT, tr.RT_ERR_INVALID_SIZE, tr.RT_ERR_INVALID_CONTEXT
SENT, TAIL, HISTORY = tr.SENT, tr.TAIL, tr.HISTORY
W, H = 96, 64                  # the rule cases
SW, SH = tr.W, tr.H            # 37 x 21: the plans that only need some pixels
TARGET = 38                    # the largest Lambertian sphere other than the ground
EDIT_TALLIES = ("guard", "link_none", "near", "near_restart", "near_capped", "moved")
TALLIES = tr.TALLIES + EDIT_TALLIES
KEYWORDS = ("reproject", "aov", "denoise", "variance", "moments", "adaptive", "converge",
            "progress")


# ---- the references --------------------------------------------------------------------------------
def edit_plan_ref(prev, cur, prev_index=None, influence=3.0):
    """rt_scene_edit.h's plan: (table, info), the table a (n_cur + 32, 8) uint32 array."""
    prev = np.ascontiguousarray(prev, F32).reshape(-1, 8)
    cur = np.ascontiguousarray(cur, F32).reshape(-1, 8)
    pw, cw = prev.view(U32), cur.view(U32)
    n_prev, n_cur = prev.shape[0], cur.shape[0]
    index = list(range(n_cur)) if prev_index is None else [int(j) & NONE for j in prev_index]
    table = np.zeros((n_cur + MAX_BALLS, 8), U32)
    tf = table.view(F32)
    balls = []
    infl = F32(influence)

    def ball(s, owner):
        t = infl * np.abs(s[3])
        row = np.zeros(8, U32)
        row.view(F32)[0:3] = s[0:3]
        row.view(F32)[3] = t * t
        row[4] = owner
        balls.append(row)

    n_changed = 0
    with np.errstate(all="ignore"):
        for i, j in enumerate(index):
            tf[i, 4:7] = cur[i, 0:3]
            link, geometry = NONE, False
            if j == NONE:
                tf[i, 0:3], tf[i, 3] = cur[i, 0:3], F32(1.0)
            else:
                scale = prev[j, 3] / cur[i, 3]
                assert scale.dtype == F32
                tf[i, 0:3], tf[i, 3] = prev[j, 0:3], scale
                geometry = not (pw[j, 0:4] == cw[i, 0:4]).all()
                if (pw[j, 4:8] == cw[i, 4:8]).all():
                    if not geometry:
                        link = j
                    elif (np.isfinite(prev[j, 3]) and np.isfinite(cur[i, 3]) and prev[j, 3] != 0
                          and cur[i, 3] != 0 and np.isfinite(scale) and scale > 0):
                        link = j | MOVED
            table[i, 7] = link
            if link == j and j != NONE:
                continue
            n_changed += 1
            ball(cur[i], i)
            if geometry:
                ball(prev[j], i)
        deleted = [j for j in range(n_prev) if j not in set(index)]
        for j in deleted:
            ball(prev[j], NONE)
    full = len(balls) > MAX_BALLS
    if full:
        balls = []
        table[:n_cur, 7] = NONE
    for k, row in enumerate(balls):
        table[n_cur + k] = row
    links = table[:n_cur, 7]
    info = dict(n_records=n_cur, n_balls=len(balls), n_changed=n_changed,
                n_moved=int(((links != NONE) & (links & MOVED != 0)).sum()),
                n_restart=int((links == NONE).sum()), n_deleted=len(deleted),
                full_restart=int(full))
    return table, info


def carry_ref(prev, prev_ids, prev_hit, ids, hit, normal, material, prev_blob, plan, max_history,
              lambertian_only, tol2, edit_history, counts=None, detail=None):
    """rt_edit_carry's per-pixel text over (H, W, .) float32 arrays (ids: (H, W) int32), `plan`
    the (table, info) pair.  `counts` receives test_reproject's tallies and: `guard` and
    `link_none`, the pixels rule 1b stops; `near`, the near pixels that pass rules 1-2;
    `near_restart`, those rule 2b stops; `near_capped`, the pixels with history whose count
    edit_history lowers; `moved`, the pixels with history taken through a moved link.  `detail`
    receives "kept" (kept taps per pixel), "near" and "used"."""
    table, info = plan
    n_records, n_balls = info["n_records"], info["n_balls"]
    table = np.ascontiguousarray(table, U32).reshape(-1, 8)
    prev = np.ascontiguousarray(prev, F32)
    prev_hit = np.ascontiguousarray(prev_hit, F32)
    hit = np.ascontiguousarray(hit, F32)
    normal = np.ascontiguousarray(normal, F32)
    h, w = ids.shape
    basis, ok = tr.reproject_basis_ref(prev_blob)
    assert ok
    r0, r1, r2 = basis[0:3], basis[3:6], basis[6:9]
    o = np.asarray(prev_blob, F32)[0:3]
    one, half = F32(1.0), F32(0.5)
    tally = dict.fromkeys(TALLIES, 0)
    with np.errstate(all="ignore"):
        p, nP = hit[..., :3], normal[..., :3]
        uid = ids.astype(np.int64) & NONE
        miss = uid == NONE
        live = ~miss
        tally["miss"] = int(miss.sum())
        guard = live & (uid >= n_records)
        tally["guard"] = int(guard.sum())
        live = live & ~guard
        rec = np.zeros((h, w, 8), U32)                    # read only where live
        rec[live] = table[uid[live]]
        link = rec[..., 7]
        none = live & (link == NONE)
        tally["link_none"] = int(none.sum())
        live = live & ~none
        if lambertian_only:
            spec = live & ~(np.ascontiguousarray(material, F32)[..., 3] < F32(-1.0))
            tally["specular"] = int(spec.sum())
            live = live & ~spec
        near = np.zeros((h, w), bool)
        for k in range(n_balls):
            B = table[n_records + k]
            bc, r2b, owner = B[0:3].view(F32), B[3:4].view(F32)[0], int(B[4])
            d = p - bc
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == F32
            near |= (uid != owner) & (d2 < r2b)
        tally["near"] = int((live & near).sum())
        if edit_history == 0:
            tally["near_restart"] = int((live & near).sum())
            live = live & ~near
        cap = np.where(near, F32(edit_history), F32(max_history)).astype(F32)
        is_moved = (link & MOVED) != 0
        recf = rec.view(F32)
        mapped = recf[..., 0:3] + (p - recf[..., 4:7]) * recf[..., 3:4]
        assert mapped.dtype == F32
        ps = np.where(is_moved[..., None], mapped, p)     # p'
        source = (link & (MOVED - 1)).astype(np.int64)
        q = ps - o
        a, b, c = tr._dot3(r0, q), tr._dot3(r1, q), tr._dot3(r2, q)
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
        prev_uid = prev_ids.astype(np.int64) & NONE
        for j in (0, 1):
            for i in (0, 1):
                X, Y = x0 + i, y0 + j
                bw = (ty if j else one - ty) * (tx if i else one - tx)
                on = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
                Xc, Yc = np.clip(X, 0, w - 1), np.clip(Y, 0, h - 1)
                same = prev_uid[Yc, Xc] == source
                e = ps - prev_hit[Yc, Xc, :3]
                dl = tr._dot3(nP.transpose(2, 0, 1), e)
                close = dl * dl <= lim
                pc = prev[Yc, Xc]
                has = pc[..., 3] > 0
                pos = bw > 0
                assert bw.dtype == F32 and dl.dtype == F32 and lim.dtype == F32
                left = live
                for rule, passes in (("off_image", on), ("id_mismatch", same), ("plane", close),
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
        out[..., 3] = np.where(got, np.minimum(n, cap), F32(0.0))
        assert sw.dtype == F32 and acc.dtype == F32 and n.dtype == F32 and out.dtype == F32
        tally["four"] = int((kept == 4).sum())
        tally["some"] = int(((kept >= 1) & (kept <= 3)).sum())
        tally["none"] = int((live & (kept == 0)).sum())
        tally["capped"] = int((got & ~near & (n > F32(max_history))).sum())
        tally["near_capped"] = int((got & near & (n > F32(edit_history))).sum())
        tally["moved"] = int((got & is_moved).sum())
    if counts is not None:
        counts.update(tally)
    if detail is not None:
        detail.update(used=used, kept=kept, near=near)
    return out


# ---- scenes, views and cases -----------------------------------------------------------------------
def base_scene():
    import gpu_ray_tracing as rt
    return np.ascontiguousarray(rt.synthetic_scene(40).spheres, F32).reshape(-1, 8).copy()


def _moved(frac):
    s = base_scene()
    s[TARGET, 0:3] += F32(frac) * s[TARGET, 3] * np.array([1.0, 0.0, 0.5], F32)
    return s


def _with(index, column, value):
    s = base_scene()
    s[index, column] = value
    return s


def _many(n):
    """n small spheres (1 .. n) moved a little: 2 n balls."""
    s = base_scene()
    s[1:n + 1, 0] += F32(0.05)
    return s


DELETED = 13                                       # visible (7 pixels), eight visible ids after it
SCENES = {                                         # name -> () -> (spheres, prev_index or None)
    "base": lambda: (base_scene(), None),
    "move": lambda: (_moved(0.5), None),
    "nudge": lambda: (_moved(0.1), None),
    "resize": lambda: (_with(TARGET, 3, 1.25), None),
    "move_resize": lambda: (_with(TARGET, slice(0, 4), (-3.8, 1.2, 0.1, 1.2)), None),
    "recolour": lambda: (_with(TARGET, slice(4, 7), (0.1, 0.6, 0.2)), None),
    "delete": lambda: (np.delete(base_scene(), DELETED, axis=0),
                       [j for j in range(40) if j != DELETED]),
    "edits16": lambda: (_many(16), None),
    "edits17": lambda: (_many(17), None),
    "zero": lambda: (np.zeros((0, 8), F32), None),
}


@functools.lru_cache(None)
def scene(name):
    spheres, index = SCENES[name]()
    spheres = np.ascontiguousarray(spheres, F32)
    spheres.setflags(write=False)
    return spheres, index


@functools.lru_cache(None)
def view(w, h, move, name):
    """tests/test_reproject.py's view() for one of SCENES."""
    import gpu_ray_tracing as rt
    if name == "base":
        return tr.view(w, h, move)
    cam = td.default_camera(rt, w, h, **dict(move))
    spheres = scene(name)[0]
    g = td.guide_planes(cam.blob, spheres, w, h)
    material = np.zeros((h, w, 4), F32)
    hitmask = g["sphere_id"] != MISS
    material[hitmask] = spheres[g["sphere_id"][hitmask], 4:8]
    for a in (material, *g.values()):
        a.setflags(write=False)
    return SimpleNamespace(cam=cam, spheres=spheres, material=material, **g)


def variant(max_history=64, lamb=1, tol2=1e-5, edit_history=4):
    return (max_history, lamb, tol2, edit_history)


DEFAULT = [variant()]
# name -> (width, height, previous scene, current scene, previous view, current view, variants)
CASES = {
    "move": (W, H, "base", "move", tr.BASE, tr.BASE,
             [variant(), variant(lamb=0), variant(edit_history=0), variant(edit_history=64),
              variant(8, edit_history=8)]),
    "resize": (W, H, "base", "resize", tr.BASE, tr.BASE, DEFAULT),
    "move_resize": (W, H, "base", "move_resize", tr.BASE, tr.BASE, DEFAULT),
    # (a panned view: under an unmoved camera three of a pixel's four taps have zero weight)
    "delete": (W, H, "base", "delete", tr.BASE, tr.PAN, DEFAULT),
    "recolour": (W, H, "base", "recolour", tr.BASE, tr.BASE, DEFAULT),
    "move_pan": (W, H, "base", "move", tr.BASE, tr.PAN, [variant(), variant(lamb=0)]),
    "identity": (SW, SH, "base", "base", tr.BASE, tr.PAN, [variant(), variant(lamb=0)]),   # 0 balls
    "one_ball": (SW, SH, "base", "recolour", tr.BASE, tr.BASE, DEFAULT),
    "balls32": (SW, SH, "base", "edits16", tr.BASE, tr.BASE, DEFAULT),
    "full_restart": (SW, SH, "base", "edits17", tr.BASE, tr.BASE, DEFAULT),
    "zero": (SW, SH, "zero", "zero", tr.BASE, tr.PAN, DEFAULT),
}
# one tile exactly and one pixel more both ways, one wave and one pixel more, narrower and lower
SIZES = [(1, 1), (16, 4), (17, 5), (32, 8), (33, 9), (65, 5), (5, 40)]
for _w, _h in SIZES:
    CASES[f"{_w}x{_h}"] = (_w, _h, "base", "move", tr.BASE, tr.PAN, DEFAULT)
RULE_CASES = ("move", "resize", "move_resize", "delete", "recolour", "move_pan")


@functools.lru_cache(None)
def case(name):
    """A case's inputs (read-only arrays), computed once and shared."""
    import gpu_ray_tracing as rt
    w, h, pscene, cscene, pmove, cmove, variants = CASES[name]
    pv, cv = view(w, h, pmove, pscene), view(w, h, cmove, cscene)
    index = scene(cscene)[1]
    plan = edit_plan_ref(pv.spheres, cv.spheres, index)
    plan[0].setflags(write=False)
    prev = tr.accumulator(w, h, pmove, "zero" if pscene == "zero" else "n40")
    return SimpleNamespace(name=name, w=w, h=h, prev=pv, cur=cv, variants=variants, index=index,
                           plan=plan, prev_rgba=prev, sc=rt.SphereCollection(cv.spheres),
                           prev_sc=rt.SphereCollection(pv.spheres))


def ref_of(c, var, plan=None, ids=None, prev_rgba=None, **kw):
    max_history, lamb, tol2, edit_history = var
    return carry_ref(c.prev_rgba if prev_rgba is None else prev_rgba, c.prev.sphere_id,
                     c.prev.hit, c.cur.sphere_id if ids is None else ids, c.cur.hit, c.cur.normal,
                     c.cur.material, c.prev.cam.blob, plan or c.plan, max_history, lamb, tol2,
                     edit_history, **kw)


@functools.lru_cache(None)
def expected(name, var):
    """(reference output, tallies, detail) of one variant of a case."""
    counts, detail = {}, {}
    out = ref_of(case(name), var, counts=counts, detail=detail)
    out.setflags(write=False)
    return out, counts, detail


ALL = [(name, var) for name in CASES for var in CASES[name][6]]


def _id(v):
    name, (max_history, lamb, tol2, edit_history) = v
    return f"{name}-h{max_history}-{'lambertian' if lamb else 'all'}-e{edit_history}"


# ---- CPU tests: the boundary -----------------------------------------------------------------------
def test_library_exports_the_edit_entry_points(rt):
    text = HEADER.read_text()
    declared = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", text, flags=re.M)
    assert declared == ["rt_edit_params_default", "rt_edit_plan_bytes", "rt_edit_plan",
                        "rt_edit_carry"]
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r" T (rt_\w+)$", nm, flags=re.M))
    assert {s for s in exported if s.startswith("rt_edit_")} == set(declared)
    for s in declared:
        assert not any(k in s for k in KEYWORDS), s
    L = rt._lib
    assert L.edit_symbols() == declared
    for other in (L.exported_symbols(), L.aov_symbols(), L.chain_parts_symbols(),
                  L.selftest_roots_symbols(), L.denoise_symbols(), L.reproject_symbols(),
                  L.variance_symbols(), L.adaptive_symbols(), L.converge_symbols(),
                  L.progress_symbols()):
        assert not set(declared) & set(other)
    abi = (ROOT / "include" / "rt_abi.h").read_text()
    assert "rt_edit_" not in abi
    in_abi = re.findall(r"^RT_API [^(]*?\b(rt_\w+)\(", abi, flags=re.M)
    assert sorted(L.exported_symbols()) == sorted(in_abi) and len(in_abi) == 52
    assert L.lib().rt_abi_version() == 7
    assert '#include "rt_reproject.h"' in text
    assert "rt_scene_edit.h" in (ROOT / "include" / "rt_reproject.h").read_text()
    assert callable(rt.edit_plan) and callable(rt.ComputeShaderPipeline.carry_edit)
    assert (rt.RT_EDIT_NONE, rt.RT_EDIT_MOVED, rt.RT_EDIT_MAX_BALLS) == (NONE, MOVED, MAX_BALLS)


def test_structs_and_defaults(rt):
    L = rt._lib
    for s in (L.EditRecordC, L.EditBallC, L.EditParamsC, L.EditInfoC):
        assert ctypes.sizeof(s) == 32, s
    assert [f for f, _ in L.EditRecordC._fields_] == ["prev_center", "scale", "center", "link"]
    assert [f for f, _ in L.EditBallC._fields_] == ["center", "radius2", "owner", "_pad"]
    assert [f for f, _ in L.EditParamsC._fields_] == ["carry", "edit_history", "influence",
                                                      "_reserved"]
    assert [f for f, _ in L.EditInfoC._fields_] == [
        "n_records", "n_balls", "n_changed", "n_moved", "n_restart", "n_deleted", "full_restart",
        "_reserved"]
    p = L.EditParamsC()
    ctypes.memset(ctypes.byref(p), 0xAB, 32)
    L.lib().rt_edit_params_default(ctypes.byref(p))
    assert (p.carry.max_history, p.carry.lambertian_only, p.carry._reserved) == (64, 1, 0)
    assert F32(p.carry.position_tolerance2) == F32(1e-5)
    assert (p.edit_history, p.influence, tuple(p._reserved)) == (4, 3.0, (0, 0))
    L.lib().rt_edit_params_default(None)                        # a no-op, not a crash
    assert rt.EDIT_DEFAULTS == {"edit_history": 4, "influence": 3.0}
    for n in (0, 1, 40, 1 << 20):
        assert L.lib().rt_edit_plan_bytes(n) == 32 * (n + 32)


@pytest.mark.parametrize("lang,std,cc", [("c", "c11", "gcc"), ("c++", "c++17", "g++")])
def test_header_compiles_on_its_own(lang, std, cc, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    lines = ['#include "rt_scene_edit.h"']
    for s in ("record", "ball", "params", "info"):
        lines.append(f"typedef char {s}_is_32_bytes[sizeof(rt_edit_{s}) == 32 ? 1 : -1];")
    lines += ["typedef char link_at_28[offsetof(rt_edit_record, link) == 28 ? 1 : -1];",
              "typedef char owner_at_16[offsetof(rt_edit_ball, owner) == 16 ? 1 : -1];",
              "typedef char history_at_16[offsetof(rt_edit_params, edit_history) == 16 ? 1 : -1];",
              "typedef char none[RT_EDIT_NONE == 0xFFFFFFFFu && RT_EDIT_MOVED == 0x80000000u "
              "&& RT_EDIT_MAX_BALLS == 32 ? 1 : -1];",
              "rt_reproject_planes uses_its_siblings_types;"]
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([cc, f"-std={std}", "-Wall", "-Werror", "-fsyntax-only", "-I",
                        str(HEADER.parent), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- CPU tests: the plan ---------------------------------------------------------------------------
def _plans():
    """name -> (prev, cur, prev_index, expectations of info)."""
    base = base_scene()
    nz = base.copy()
    nz[5, 2] = F32(0.0)
    negz = nz.copy()
    negz[5, 2] = F32(-0.0)
    perm = np.random.default_rng(5).permutation(40)
    inserted = np.concatenate([base[:7], [[0.5, 0.3, 0.5, 0.3, 0.2, 0.3, 0.4, -2.0]], base[7:]])
    inserted = inserted.astype(F32)
    return {
        "identity": (base, base, None, dict(n_balls=0, n_changed=0, n_restart=0)),
        "move": (base, scene("move")[0], None, dict(n_balls=2, n_moved=1, n_restart=0)),
        "resize": (base, scene("resize")[0], None, dict(n_balls=2, n_moved=1)),
        "move_resize": (base, scene("move_resize")[0], None, dict(n_balls=2, n_moved=1)),
        "recolour": (base, scene("recolour")[0], None, dict(n_balls=1, n_moved=0, n_restart=1)),
        "material kind": (base, _with(TARGET, 7, 0.25), None, dict(n_balls=1, n_restart=1)),
        "ground": (base, _with(0, 1, -1000.5), None, dict(n_balls=2, n_moved=1)),
        "delete": (base, *scene("delete"), dict(n_balls=1, n_deleted=1, n_changed=0, n_restart=0)),
        "insert": (base, inserted, list(range(7)) + [NONE] + list(range(7, 40)),
                   dict(n_balls=1, n_restart=1, n_changed=1, n_deleted=0)),
        "permutation": (base, base[perm], perm.tolist(), dict(n_balls=0, n_changed=0)),
        "sign flip": (base, _with(TARGET, 3, -1.0), None,
                      dict(n_balls=2, n_moved=0, n_restart=1)),
        "radius 0": (base, _with(TARGET, 3, 0.0), None, dict(n_balls=2, n_moved=0, n_restart=1)),
        "from radius 0": (_with(TARGET, 3, 0.0), base, None,
                          dict(n_balls=2, n_moved=0, n_restart=1)),
        "-0 against +0": (nz, negz, None, dict(n_balls=2, n_moved=1)),
        "16 edits": (base, scene("edits16")[0], None,
                     dict(n_balls=32, n_moved=16, full_restart=0)),
        "17 edits": (base, scene("edits17")[0], None,
                     dict(n_balls=0, n_moved=0, n_restart=40, n_changed=17, full_restart=1)),
        "n_cur 0": (base, np.zeros((0, 8), F32), [],
                    dict(n_records=0, n_balls=0, n_deleted=40, full_restart=1)),
        "both empty": (np.zeros((0, 8), F32), np.zeros((0, 8), F32), None, dict(n_balls=0)),
        "one deleted of two": (base[:2], base[:1], [0], dict(n_balls=1, n_deleted=1)),
    }


@pytest.mark.parametrize("name", ["identity", "move", "resize", "move_resize", "recolour",
                                  "material kind", "ground", "delete", "insert", "permutation",
                                  "sign flip", "radius 0", "from radius 0", "-0 against +0",
                                  "16 edits", "17 edits", "n_cur 0", "both empty",
                                  "one deleted of two"])
def test_plan_matches_the_reference(rt, name):
    prev, cur, index, expect = _plans()[name]
    for influence in (0.0, 1.7, 3.0):
        want, info = edit_plan_ref(prev, cur, index, influence)
        table, got = rt.edit_plan(prev, cur, index, influence=influence)
        assert got == info, name
        assert table.dtype == U32 and table.shape == want.shape
        assert (table == want).all(), f"{name}: the table differs from the reference"
    for k, v in expect.items():
        assert info[k] == v, (name, k, info)
    assert info["n_records"] == len(cur)
    links = want[:len(cur), 7]
    if name == "move":
        assert links[TARGET] == TARGET | MOVED and want[TARGET].view(F32)[3] == 1.0
        assert (np.delete(links, TARGET) == np.delete(np.arange(40), TARGET)).all()
        assert (want[40:42, 4] == TARGET).all() and want[40].view(F32)[3] == 9.0
    if name == "resize":
        assert want[TARGET].view(F32)[3] == F32(1.0) / F32(1.25)
    if name == "delete":
        assert (links == np.array(index)).all() and want[39, 4] == NONE
    if name == "insert":
        assert links[7] == NONE and links[8] == 7 and want[41, 4] == 7
    if name == "17 edits":
        assert (links == NONE).all() and not want[40:].any()


def test_plan_refuses_what_the_header_says(rt):
    L = rt._lib
    base = base_scene()
    table = np.zeros((72, 8), U32)
    info = L.EditInfoC()
    before = bytes(info)

    def params(max_history=64, edit_history=4, influence=3.0, reserved=(0, 0), carry_reserved=0):
        p = L.EditParamsC()
        p.carry = L.ReprojectParamsC(max_history, 1, 1e-5, carry_reserved)
        p.edit_history, p.influence = edit_history, influence
        p._reserved[0], p._reserved[1] = reserved
        return p

    def call(prev=base, n_prev=40, cur=base, n_cur=40, index=None, p=params(), tab=table,
             nbytes=None, inf=info):
        ptr = (lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data))
        idx = None if index is None else np.asarray(index, np.int64).astype(U32)
        return L.lib().rt_edit_plan(ptr(prev), n_prev, ptr(cur), n_cur, ptr(idx),
                                    ctypes.byref(p) if p is not None else None, ptr(tab),
                                    (tab.nbytes if tab is not None else 0) if nbytes is None
                                    else nbytes,
                                    ctypes.byref(inf) if inf is not None else None)

    ident = list(range(40))
    rows = {
        "params NULL": dict(p=None), "table NULL": dict(tab=None, nbytes=72 * 32),
        "info NULL": dict(inf=None), "spheres NULL": dict(cur=None),
        "prev_spheres NULL": dict(prev=None), "table too small": dict(nbytes=72 * 32 - 1),
        "NULL index, counts differ": dict(n_prev=39),
        "entry >= n_prev": dict(index=ident[:39] + [40]),
        "entry >= n_prev (n_prev 39)": dict(n_prev=39, index=ident),
        "named twice": dict(index=ident[:39] + [0]),
        "influence < 0": dict(p=params(influence=-1.0)),
        "influence NaN": dict(p=params(influence=float("nan"))),
        "influence inf": dict(p=params(influence=float("inf"))),
        "edit_history > max_history": dict(p=params(max_history=8, edit_history=9)),
        "_reserved[0]": dict(p=params(reserved=(1, 0))),
        "_reserved[1]": dict(p=params(reserved=(0, 1))),
        "carry._reserved": dict(p=params(carry_reserved=1)),
        "n_prev above 2^20": dict(n_prev=(1 << 20) + 1, index=ident),
        "n_cur above 2^20": dict(n_cur=(1 << 20) + 1, nbytes=1 << 40),
    }
    for what, kw in rows.items():
        assert call(**kw) == A, what
    assert not table.any() and bytes(info) == before, "a refused call wrote its outputs"
    assert call() == 0 and call(index=ident[:39] + [NONE]) == 0
    assert call(p=params(max_history=4, edit_history=4)) == 0
    assert call(prev=None, n_prev=0, cur=None, n_cur=0) == 0
    with pytest.raises(rt.RtError) as e:
        rt.edit_plan(base, base[:39])
    assert e.value.status == A
    with pytest.raises(ValueError):
        rt.edit_plan(base, base, ident[:39])


# ---- CPU tests: the per-pixel rules, from the reference alone --------------------------------------
@pytest.mark.parametrize("name", ["pan", "orbit", "counts"])
def test_an_identity_plan_is_reprojection(name):
    c = tr.case(name)
    plan = edit_plan_ref(c.cur.spheres, c.cur.spheres)
    assert plan[1]["n_balls"] == 0 and plan[1]["n_changed"] == 0
    for var in c.variants:
        max_history, lamb, tol2 = var
        want, counts = tr.expected(name, var)
        mine = {}
        got = carry_ref(c.prev_rgba, c.prev.sphere_id, c.prev.hit, c.cur.sphere_id, c.cur.hit,
                        c.normal, c.cur.material, c.prev.cam.blob, plan, max_history, lamb, tol2,
                        4, counts=mine)
        assert bits_equal(got, want)[0], (name, var)
        assert {k: mine[k] for k in tr.TALLIES} == counts
        assert not any(mine[k] for k in EDIT_TALLIES)


@pytest.mark.parametrize("name", RULE_CASES)
def test_cases_reach_their_rules(name):
    c = case(name)
    per = {}
    for var in c.variants:
        out, n, d = expected(name, var)
        per[var] = n
        print(f"{_id((name, var))}: " + ", ".join(f"{k} {n[k]}" for k in TALLIES)
              + f"; {int((out[..., 3] > 0).sum())} pixels with history")
        assert int((out[..., 3] > 0).sum()) == n["four"] + n["some"]
        assert n["guard"] == 0
    out, n, d = expected(name, variant())
    ids = c.cur.sphere_id
    own = ids == (TARGET - 1 if name == "delete" else TARGET)
    assert own.sum() >= 100
    if name in ("move", "resize", "move_resize", "move_pan"):
        assert n["moved"] >= 100 and n["near_capped"] >= 50 and n["link_none"] == 0
        # the owner exemption: the moved sphere's own pixels keep the full count
        assert (out[own][:, 3] > 4.0).sum() >= 100
        assert (out[~own][:, 3] <= 4.0)[d["near"][~own]].all()
        assert (out[~d["near"]][:, 3] == np.where(out[~d["near"]][:, 3] > 0, 16.0, 0.0)).all()
    if name == "move":
        # without the mapping one pixel of the sphere in a hundred keeps history
        ident = edit_plan_ref(c.prev.spheres, c.prev.spheres)
        plain = ref_of(c, variant(), plan=ident)
        assert (plain[own][:, 3] > 0).sum() * 10 < (out[own][:, 3] > 0).sum()
        zero = per[variant(edit_history=0)]
        assert zero["near_restart"] == zero["near"] >= 50 and zero["near_capped"] == 0
        assert not expected(name, variant(edit_history=0))[0][d["near"]].any()
        full = per[variant(edit_history=64)]
        assert full["near_capped"] == 0 and full["near"] == n["near"]
        assert expected(name, variant(edit_history=64))[0][..., 3].max() == 16.0
        assert expected(name, variant(8, edit_history=8))[0][..., 3].max() == 8.0
        assert per[variant(8, edit_history=8)]["capped"] > 0
        assert per[variant(lamb=0)]["specular"] == 0 < n["specular"]
    if name == "delete":
        # ids from DELETED on shifted by one: every unchanged sphere behind the deleted one is
        # still matched with itself
        behind = (ids >= DELETED) & (ids != MISS) & (c.cur.material[..., 3] < -1)
        print(f"delete: {int(behind.sum())} Lambertian pixels behind the deleted sphere, "
              f"{int((d['kept'][behind] >= 1).sum())} with history, "
              f"{int((d['kept'][behind] == 4).sum())} with four taps")
        # (a disc of 131 pixels has about 40 on its rim, which lose taps to the silhouette)
        assert behind.sum() >= 100 and (d["kept"][behind] == 4).sum() >= 0.5 * behind.sum()
        assert n["moved"] == 0 and n["link_none"] == 0 and n["near"] >= 1
        shifted = ref_of(c, variant(), plan=edit_plan_ref(c.cur.spheres, c.cur.spheres))
        assert (shifted[behind][:, 3] > 0).sum() == 0
    if name == "recolour":
        assert n["link_none"] == own.sum() and not out[own].any()
        assert n["moved"] == 0 and n["near_capped"] >= 50
    if name == "move_pan":
        assert n["off_image"] >= 1 and n["id_mismatch"] >= 1 and n["some"] >= 1


def test_a_stale_id_is_stopped_before_its_record_is_read():
    """Reference only: ids at and past n_records restart, whatever lies behind the table."""
    c = case("move")
    ids = c.cur.sphere_id.copy()
    ys, xs = np.nonzero(expected("move", variant())[0][..., 3] > 0)
    spots = [(int(ys[k]), int(xs[k])) for k in (0, ys.size // 2, ys.size - 1)]
    for (y, x), v in zip(spots, (40, 41, 0x7FFFFFFF)):
        ids[y, x] = v
    counts = {}
    out = ref_of(c, variant(), ids=ids, counts=counts)
    clean = expected("move", variant())[0]
    assert counts["guard"] == 3
    mask = np.zeros(ids.shape, bool)
    for y, x in spots:
        mask[y, x] = True
        assert not out[y, x].any()
    assert bits_equal(out[~mask], clean[~mask])[0]


@pytest.mark.parametrize("name", ["nudge", "move"])
def test_history_beats_a_reset(name, oracle):
    """The prototype's setup: the carried image plus one sample is nearer a 512-sample render of
    the edited scene than one sample alone, separately over all pixels with history, the moved
    sphere's and those inside the edit's balls.  Strict inequalities, not tolerances."""
    import gpu_ray_tracing as rt
    pv, cv = view(W, H, tr.BASE, "base"), view(W, H, tr.BASE, name)
    plan = edit_plan_ref(pv.spheres, cv.spheres)
    detail = {}
    rep = carry_ref(tr.accumulator(W, H, tr.BASE), pv.sphere_id, pv.hit, cv.sphere_id, cv.hit,
                    cv.normal, cv.material, pv.cam.blob, plan, HISTORY, 1, 1e-5, 4, detail=detail)
    got = rep[..., 3] > 0
    still = cv.cam.with_fields(camera_has_moved=0.0)
    moved = cv.cam.with_fields(camera_has_moved=1.0)
    kept, _ = oracle.update(rep, still.blob, cv.spheres)
    reset, _ = oracle.update(rep, moved.blob, cv.spheres)
    assert (reset[..., 3] == 1.0).all() and (kept[got][:, 3] == rep[got][:, 3] + 1.0).all()
    target, _ = oracle.render(np.zeros((H, W, 4), F32), cv.cam.blob, cv.spheres,
                              np.array(rt.frame_seeds(7, 512), F32))
    masks = {"all with history": got, "the moved sphere": got & (cv.sphere_id == TARGET),
             "near": got & detail["near"]}
    assert masks["the moved sphere"].sum() >= 100 and masks["near"].sum() >= 50
    for what, m in masks.items():
        def mse(a):
            return float(np.mean((a[m][:, :3].astype(np.float64) - target[m][:, :3]) ** 2))
        with_history, without = mse(kept), mse(reset)
        print(f"{name}, {what}: {int(m.sum())} pixels, MSE against 512 spp: carried "
              f"{with_history:.5f}, reset {without:.5f}, ratio {without / with_history:.2f}")
        assert with_history < without, what


# ---- GPU side --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe(rt):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = rt.ComputeShaderPipeline(0)
    yield p
    p.close()


def host_inputs(c):
    return dict(prev_rgba=c.prev_rgba, prev_ids=c.prev.sphere_id, prev_hit=c.prev.hit,
                ids=c.cur.sphere_id, hit=c.cur.hit, normal=c.cur.normal,
                material=c.cur.material)


def device_inputs(p, c):
    import torch
    return SimpleNamespace(**{k: torch.from_numpy(v.copy()).to(p.torch_device)
                              for k, v in host_inputs(c).items()})


def run(rt, p, c, var, plan=None, on_device=False):
    """dst of one variant (numpy) through pipe.carry_edit with the library's own plan, after the
    checks every call must pass: the plan is the reference's, the tail of dst intact, prev_image,
    the planes and a device table unchanged."""
    import torch
    max_history, lamb, tol2, edit_history = var
    if plan is None:
        plan = rt.edit_plan(c.prev.spheres, c.cur.spheres, c.index, max_history=max_history,
                            edit_history=edit_history)
        assert (plan[0] == c.plan[0]).all() and plan[1] == c.plan[1]
    d = device_inputs(p, c)
    px = c.w * c.h * 4
    dst = tr.guarded(p, px)
    prev_guides, guides = tr.guides_of(d, lamb)
    given = plan
    if on_device:
        given = (torch.from_numpy(plan[0].view(np.int32).copy()).to(p.torch_device), plan[1])
    res = p.carry_edit(d.prev_rgba, c.w, c.h, c.prev.cam, prev_guides, guides, given,
                       max_history=max_history, position_tolerance2=tol2,
                       lambertian_only=bool(lamb), edit_history=edit_history, out=dst)
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
    if on_device:
        assert (given[0].cpu().numpy().view(U32) == plan[0]).all(), "the table was written"
    return got[:px].reshape(c.h, c.w, 4)


def check(got, name, var):
    want = expected(name, var)[0]
    same, bad = bits_equal(got, want)
    assert same, f"{_id((name, var))}: {bad} values differ from the reference"


@gpu
@pytest.mark.parametrize("v", ALL, ids=_id)
def test_matches_reference(rt, pipe, v):
    name, var = v
    c = case(name)
    check(run(rt, pipe, c, var), name, var)
    want, n, _ = expected(name, var)
    if name == "full_restart":
        assert c.plan[1]["full_restart"] == 1 and not want.any()
    if name == "zero":
        assert c.plan[1]["n_records"] == 0 and not want.any()
    if name in ("identity", "one_ball", "balls32"):
        assert c.plan[1]["n_balls"] == {"identity": 0, "one_ball": 1, "balls32": 32}[name]
        assert want.any()


@gpu
def test_a_device_table_is_taken_as_it_is(rt, pipe):
    for name in ("move", "balls32"):
        c = case(name)
        check(run(rt, pipe, c, variant(), on_device=True), name, variant())


@gpu
@pytest.mark.parametrize("name", ["pan", "counts"])
def test_an_identity_plan_equals_reproject_on_the_gpu(rt, pipe, name):
    import torch
    c = tr.case(name)
    plan = rt.edit_plan(c.cur.spheres, c.cur.spheres)
    d = tr.device_inputs(pipe, c)
    for var in c.variants:
        max_history, lamb, tol2 = var
        prev_guides, guides = tr.guides_of(d, lamb)
        kw = dict(max_history=max_history, position_tolerance2=tol2, lambertian_only=bool(lamb))
        a = pipe.reproject(d.prev_rgba, c.w, c.h, c.prev.cam, prev_guides, guides, **kw)
        b = pipe.carry_edit(d.prev_rgba, c.w, c.h, c.prev.cam, prev_guides, guides, plan, **kw)
        torch.cuda.synchronize()
        assert bits_equal(b.cpu().numpy(), a.cpu().numpy())[0], (name, var)
        assert bits_equal(a.cpu().numpy(), tr.expected(name, var)[0])[0]


@gpu
def test_planes_the_gpu_traces_give_the_reference(rt, pipe):
    """trace_aov's own planes for the two scenes and the two cameras, and an allocated `out`."""
    import torch
    c = case("move_pan")
    prev_guides = pipe.trace_aov(c.w, c.h, c.prev.cam, c.prev_sc, planes=("sphere_id", "hit"))
    guides = pipe.trace_aov(c.w, c.h, c.cur.cam, c.sc)
    prev = torch.from_numpy(c.prev_rgba.copy()).to(pipe.torch_device)
    plan = rt.edit_plan(c.prev_sc, c.sc)
    out = pipe.carry_edit(prev, c.w, c.h, c.prev.cam, prev_guides, guides, plan)
    assert out.shape == (c.h, c.w, 4)
    noid = {k: v for k, v in guides.items() if k != "material"}
    every = pipe.carry_edit(prev, c.w, c.h, c.prev.cam, prev_guides, noid, plan,
                            lambertian_only=False)
    torch.cuda.synchronize()
    assert (guides["sphere_id"].cpu().numpy() == c.cur.sphere_id).all()
    assert (prev_guides["sphere_id"].cpu().numpy() == c.prev.sphere_id).all()
    check(out.cpu().numpy(), "move_pan", variant())
    check(every.cpu().numpy(), "move_pan", variant(lamb=0))
    with pytest.raises(ValueError):
        pipe.carry_edit(prev, c.w, c.h, c.prev.cam, prev_guides, noid, plan)   # material missing
    with pytest.raises(ValueError):
        pipe.carry_edit(prev, c.w, c.h, c.prev.cam, {"hit": prev_guides["hit"]}, guides, plan)
    with pytest.raises(ValueError):
        pipe.carry_edit(prev.cpu(), c.w, c.h, c.prev.cam, prev_guides, guides, plan)
    with pytest.raises(ValueError):
        pipe.carry_edit(prev, c.w, c.h, c.prev.cam, prev_guides, guides, plan[0])
    with pytest.raises(ValueError):
        pipe.carry_edit(prev, c.w, c.h, c.prev.cam, prev_guides, guides, (plan[0][:8], plan[1]))


def raw_call(rt, p, ctx, prev, dst, w, h, cam, planes, plan, n_records, n_balls, params):
    """rt_edit_carry through the C boundary (data pointers or None); raises RtError."""
    L = rt._lib
    pl = L.ReprojectPlanesC(*planes) if planes is not None else None
    pc = None
    if params is not None:
        max_history, lamb, tol2, reserved, edit_history, r0, r1 = params
        pc = L.EditParamsC()
        pc.carry = L.ReprojectParamsC(max_history, lamb, tol2, reserved)
        pc.edit_history, pc.influence = edit_history, 3.0
        pc._reserved[0], pc._reserved[1] = r0, r1
    L.call("rt_edit_carry", ctx, prev, dst, w, h,
           ctypes.byref(cam) if cam is not None else None,
           ctypes.byref(pl) if pl is not None else None, plan, n_records, n_balls,
           ctypes.byref(pc) if pc is not None else None, p._stream())


@gpu
def test_errors_launch_nothing(rt, pipe):
    import torch
    c = case("move")
    d = device_inputs(pipe, c)
    px = c.w * c.h * 4
    dst = tr.guarded(pipe, px)
    table = torch.from_numpy(c.plan[0].view(np.int32).copy()).to(pipe.torch_device)
    S, D, T = d.prev_rgba.data_ptr(), dst.data_ptr(), table.data_ptr()
    planes = (d.prev_ids.data_ptr(), d.prev_hit.data_ptr(), d.ids.data_ptr(), d.hit.data_ptr(),
              d.normal.data_ptr(), d.material.data_ptr())
    ctx, w, h = pipe._ctx, c.w, c.h
    cam = c.prev.cam.to_c()
    flat = c.prev.cam.blob.copy()
    flat[8:11] = 0.0
    degenerate = rt.SceneCamera(flat).to_c()
    nr, nb = c.plan[1]["n_records"], c.plan[1]["n_balls"]

    def ok(max_history=64, lamb=1, tol2=1e-5, reserved=0, edit_history=4, r0=0, r1=0):
        return (max_history, lamb, tol2, reserved, edit_history, r0, r1)

    rows = {
        "ctx NULL": (C, (None, S, D, w, h, cam, planes, T, nr, nb, ok())),
        "prev NULL": (A, (ctx, None, D, w, h, cam, planes, T, nr, nb, ok())),
        "dst NULL": (A, (ctx, S, None, w, h, cam, planes, T, nr, nb, ok())),
        "camera NULL": (A, (ctx, S, D, w, h, None, planes, T, nr, nb, ok())),
        "planes NULL": (A, (ctx, S, D, w, h, cam, None, T, nr, nb, ok())),
        "params NULL": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, None)),
        "dst == prev": (A, (ctx, D, D, w, h, cam, planes, T, nr, nb, ok())),
        "max_history 0": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, ok(0, edit_history=0))),
        "max_history 2^24 + 1": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb,
                                     ok((1 << 24) + 1))),
        "lambertian_only 2": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, ok(lamb=2))),
        "carry._reserved 1": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, ok(reserved=1))),
        "_reserved[0] 1": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, ok(r0=1))),
        "_reserved[1] 1": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, ok(r1=1))),
        "edit_history > max_history": (A, (ctx, S, D, w, h, cam, planes, T, nr, nb,
                                           ok(8, edit_history=9))),
        "plan NULL with records": (A, (ctx, S, D, w, h, cam, planes, None, nr, 0, ok())),
        "plan NULL with balls": (A, (ctx, S, D, w, h, cam, planes, None, 0, 1, ok())),
        "33 balls": (A, (ctx, S, D, w, h, cam, planes, T, nr, 33, ok())),
        "degenerate camera": (A, (ctx, S, D, w, h, degenerate, planes, T, nr, nb, ok())),
        "width 0": (Z, (ctx, S, D, 0, h, cam, planes, T, nr, nb, ok())),
        "height 0": (Z, (ctx, S, D, w, 0, cam, planes, T, nr, nb, ok())),
        "width 65537": (Z, (ctx, S, D, 65537, h, cam, planes, T, nr, nb, ok())),
        "height 65537": (Z, (ctx, S, D, w, 65537, cam, planes, T, nr, nb, ok())),
    }
    fields = [f for f, _ in rt._lib.ReprojectPlanesC._fields_]
    for i, f in enumerate(fields):
        rows[f"{f} NULL"] = (A, (ctx, S, D, w, h, cam, planes[:i] + (None,) + planes[i + 1:], T,
                                 nr, nb, ok()))
    for what, bad in [("negative", -1.0), ("NaN", float("nan")), ("+inf", float("inf"))]:
        rows[f"tolerance {what}"] = (A, (ctx, S, D, w, h, cam, planes, T, nr, nb, ok(tol2=bad)))
    for what, (status, args) in rows.items():
        with pytest.raises(rt.RtError) as e:
            raw_call(rt, pipe, *args)
        assert e.value.status == status, what
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == F32(SENT)).all(), "a refused call wrote dst"
    # without lambertian_only the material plane is not required, and the context still works
    raw_call(rt, pipe, ctx, S, D, w, h, cam, planes[:5] + (None,), T, nr, nb, ok(lamb=0))
    torch.cuda.synchronize()
    check(dst.cpu().numpy()[:px].reshape(h, w, 4), "move", variant(lamb=0))


@gpu
def test_the_tracer_takes_the_carried_image(rt, oracle, pipe):
    """Per-pixel mixed counts (0, up to 4 near the edit, 16) through the one-frame and the fused
    kernels, tracing the edited scene."""
    import torch
    c = case("move")
    var = variant()
    want = expected("move", var)[0]
    assert len(np.unique(want[..., 3])) >= 3
    still = c.cur.cam.with_fields(camera_has_moved=0.0)
    got = run(rt, pipe, c, var)
    check(got, "move", var)
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
def test_render_is_undisturbed(rt, oracle):
    """4 frames of update_frames, against 2 frames + a carry into a third image + 2 frames on the
    same context: the same two images, and no trace of the carry in the launch info or the
    candidate lists."""
    import torch
    c = case("move")
    w, h = c.w, c.h
    cam = c.prev.cam
    still = cam.with_fields(camera_has_moved=0.0)
    seeds = np.array(rt.frame_seeds(5, 4), F32)
    p = rt.ComputeShaderPipeline(0)
    try:
        a, b = p.new_image(w, h), p.new_image(w, h)
        p.update_frames(a, b, w, h, cam, c.prev_sc, seeds)
        torch.cuda.synchronize()
        seq_a = (a.cpu().numpy(), b.cpu().numpy())
        a2, b2 = p.new_image(w, h), p.new_image(w, h)
        newest = p.update_frames(a2, b2, w, h, cam, c.prev_sc, seeds[:2])
        info, stats = p.last_launch_info(), p.candidate_stats()
        d = device_inputs(p, c)
        prev_guides, guides = tr.guides_of(d)
        out = p.carry_edit((a2, b2)[newest], w, h, cam, prev_guides, guides,
                           rt.edit_plan(c.prev_sc, c.sc))
        assert p.last_launch_info() == info
        assert p.candidate_stats() == stats
        torch.cuda.synchronize()
        mid = (a2, b2)[newest].cpu().numpy()
        got = out.cpu().numpy()
        p.update_frames(a2, b2, w, h, still, c.prev_sc, seeds[2:])
        torch.cuda.synchronize()
        seq_b = (a2.cpu().numpy(), b2.cpu().numpy())
    finally:
        p.close()
    assert bits_equal(got, ref_of(c, variant(), prev_rgba=mid))[0]
    for i, name in enumerate("ab"):
        assert bits_equal(seq_b[i], seq_a[i])[0], f"image_{name} differs between the sequences"
