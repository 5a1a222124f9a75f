"""Cases, restatement and tolerances of the colour renderer's tests (tests/test_render_frames_host.py,
tests/test_render_frames_gpu.py).

`restate_frame(objs, K, light, ambient, bg, H, W, dtype, edge_offset)` is the renderer's definition
(kd6d/libs/render.py) written out once more, independently of render_frame_host (the host tests compare the two), in
the form the kernel uses -- the normal formed in the object frame, all triangles of a size class at once -- and run in
float64 (the reference of every device comparison) and in float32 (the same code, inputs rounded as an upload rounds
them).  Projection, the triangles' size classes and the meaning of `edge_offset` are those of tests/bop_vsd_cases.py
(`_project`, `_classes`, imported, not copied): a pixel centre is covered when each edge function divided by its edge's
length is >= -edge_offset.

Comparison rule of the device tests.  The reference is rendered at the offsets -eps_px and +eps_px (the eps_px of
bop_vsd_cases; the host test checks that 4 x the edge deviation of THIS module's cases stays below it).  A pixel where
the two renders differ in owner or in depth, bit for bit, is AMBIGUOUS and left out.  On every other pixel the device's
mask must equal the reference's, its depth must lie within eps_d (bop_vsd_cases, profiles/bop_vsd_device.md), and a
colour channel must equal floor(c64 + 0.5) wherever c64 is further than eps_c from a rounding boundary (k + 0.5) and be
within 1 level of it elsewhere.  The cases keep the ambiguous pixels below 1 % of the covered pixels (host-tested).
Two different triangles can also meet in depth AWAY from an edge (case 8, interpenetrating objects): the cases are
chosen so that on every unambiguous pixel the runner-up triangle lies more than eps_d behind the owner (host-tested),
so rounding cannot decide an owner there either.

    eps_c = 4 * max |c32 - c64| over the unambiguous covered pixels of the cases, c the channel value before rounding,
            in levels -- the project's x4 rule, from the float32 restatement, never from the kernel.
`python tests/render_cases.py` prints it (recorded in profiles/render_frames.md); the host test checks that it still is
the RECORDED one.  Nothing is read from outside the repository.
"""
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "kd-6d-pose-adlp_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import bop_vsd_cases as C  # noqa: E402

MARGIN = 4.0
FACE_BITS = 28
EPS_PX = C.RECORDED["eps_px"]
EPS_D = C.RECORDED["eps_d"]
# what `python tests/render_cases.py` printed when profiles/render_frames.md was written
RECORDED = {"eps_c": 3.838e-03}


def mesh_colors(mesh, seed=0):
    """Per-vertex uint8 RGB: a smooth function of the vertex position (no two vertices of a mesh need the same colour)."""
    v = mesh.vertices
    s = v / max(float(np.abs(v).max()), 1e-9)
    c = np.stack([128 + 110 * np.sin(2.1 * s[:, 0] + 0.3 + seed), 128 + 110 * np.sin(1.7 * s[:, 1] + 1.1 * s[:, 2] + 1.0),
                  128 + 110 * np.cos(2.6 * s[:, 2] - 0.8 * s[:, 0] + 0.5 * seed)], axis=1)
    return np.clip(np.rint(c), 0, 255).astype(np.uint8)


def uniform_colors(mesh, rgb):
    return np.tile(np.asarray(rgb, np.uint8).reshape(1, 3), (len(mesh.vertices), 1))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _candidates(mesh, slot, K, R, T, H, W, f, edge_offset, probe):
    """Every (pixel, depth, owner key) a mesh's triangles produce -- coverage and depth as bop_vsd_cases.restate_render."""
    v, Rf, Tf, Kf, X, u, w = C._project(mesh, K, R, T, f)
    fc = mesh.faces
    pix, zs, keys = [], [], []
    for idx, xa, ya, xb, yb, S in C._classes(mesh, K, R, T, H, W, 1):
        i0, i1, i2 = fc[idx, 0], fc[idx, 1], fc[idx, 2]
        g = np.arange(S)
        px = (xa[:, None, None] + g[None, None, :]) * np.ones((1, S, 1), np.int64)
        py = (ya[:, None, None] + g[None, :, None]) * np.ones((1, 1, S), np.int64)
        live = (px <= xb[:, None, None]) & (py <= yb[:, None, None])
        pxf, pyf = px.astype(f), py.astype(f)
        U = [u[i][:, None, None] for i in (i0, i1, i2)]
        V = [w[i][:, None, None] for i in (i0, i1, i2)]
        area = (U[1] - U[0]) * (V[2] - V[0]) - (V[1] - V[0]) * (U[2] - U[0])
        sg = np.where(area > 0, f(1), f(-1))
        inside = live & (area != 0)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            ex, ey = U[b] - U[a], V[b] - V[a]
            E = (ex * (pyf - V[a]) - ey * (pxf - U[a])) * sg
            ln = np.sqrt(ex.astype(np.float64) ** 2 + ey.astype(np.float64) ** 2)
            En = E.astype(np.float64) / np.where(ln > 0, ln, 1.0)
            if probe is not None:
                probe.append(En[live & (area != 0)])
            inside &= En >= -edge_offset
        a0 = v[i0]
        b1, c1 = v[i1] - a0, v[i2] - a0
        no = np.stack([b1[:, 1] * c1[:, 2] - b1[:, 2] * c1[:, 1], b1[:, 2] * c1[:, 0] - b1[:, 0] * c1[:, 2],
                       b1[:, 0] * c1[:, 1] - b1[:, 1] * c1[:, 0]], axis=1)
        n = (no[:, 0, None] * Rf[None, :, 0] + no[:, 1, None] * Rf[None, :, 1]) + no[:, 2, None] * Rf[None, :, 2]
        d = ((no[:, 0] * a0[:, 0] + no[:, 1] * a0[:, 1]) + no[:, 2] * a0[:, 2]) + \
            ((n[:, 0] * Tf[0] + n[:, 1] * Tf[1]) + n[:, 2] * Tf[2])
        ry = (pyf - Kf[1, 2]) / Kf[1, 1]
        rx = (pxf - Kf[0, 2] - Kf[0, 1] * ry) / Kf[0, 0]
        den = (n[:, 0, None, None] * rx + n[:, 1, None, None] * ry) + n[:, 2, None, None]
        Zt = np.stack([X[i0, 2], X[i1, 2], X[i2, 2]], axis=1)
        zlo, zhi = Zt.min(axis=1)[:, None, None], Zt.max(axis=1)[:, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(den != 0, d[:, None, None] / den, zlo)
        z = np.minimum(np.maximum(z, zlo), zhi)
        assert z.dtype == f
        key = (np.int64(slot) << FACE_BITS) | idx.astype(np.int64)
        pix.append((py * W + px)[inside])
        zs.append(z[inside])
        keys.append((key[:, None, None] * np.ones((1, S, S), np.int64))[inside])
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)  # noqa: E731
    return cat(pix, np.int64), cat(zs, f), cat(keys, np.int64), (v, Rf, Tf, Kf, X, u, w)


def _resolve(mesh, colors, proj, face, pix, W, light, ambient, f):
    """The colour of the pixels `pix` owned by the faces `face` of one object, in dtype f -> (len, 3) BGR before rounding."""
    v, Rf, Tf, Kf, X, u, w = proj
    i0, i1, i2 = (mesh.faces[face, k] for k in range(3))
    px, py = (pix % W).astype(f), (pix // W).astype(f)
    U, V = [u[i] for i in (i0, i1, i2)], [w[i] for i in (i0, i1, i2)]
    area = (U[1] - U[0]) * (V[2] - V[0]) - (V[1] - V[0]) * (U[2] - U[0])
    sg = np.where(area > 0, f(1), f(-1))
    E = [((U[b] - U[a]) * (py - V[a]) - (V[b] - V[a]) * (px - U[a])) * sg for a, b in ((0, 1), (1, 2), (2, 0))]
    b = [E[1] / X[i0, 2], E[2] / X[i1, 2], E[0] / X[i2, 2]]
    s = (b[0] + b[1]) + b[2]
    ok = s > 0
    b = [np.where(ok, x, f(1)) for x in b]
    s = np.where(ok, s, f(3))
    col = colors.astype(f)
    albedo = ((b[0][:, None] * col[i0] + b[1][:, None] * col[i1]) + b[2][:, None] * col[i2]) / s[:, None]
    a0 = v[i0]
    b1, c1 = v[i1] - a0, v[i2] - a0
    no = np.stack([b1[:, 1] * c1[:, 2] - b1[:, 2] * c1[:, 1], b1[:, 2] * c1[:, 0] - b1[:, 0] * c1[:, 2],
                   b1[:, 0] * c1[:, 1] - b1[:, 1] * c1[:, 0]], axis=1)
    n = (no[:, 0, None] * Rf[None, :, 0] + no[:, 1, None] * Rf[None, :, 1]) + no[:, 2, None] * Rf[None, :, 2]
    d = ((no[:, 0] * a0[:, 0] + no[:, 1] * a0[:, 1]) + no[:, 2] * a0[:, 2]) + ((n[:, 0] * Tf[0] + n[:, 1] * Tf[1]) + n[:, 2] * Tf[2])
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    L = np.asarray(light, np.float64).astype(f)
    ndl = ((n[:, 0] * L[0] + n[:, 1] * L[1]) + n[:, 2] * L[2]) / ln
    ndl = np.where(d > 0, -ndl, ndl)
    amb = f(ambient)
    shade = amb + (f(1) - amb) * np.maximum(ndl, f(0))
    out = albedo * shade[:, None]
    assert out.dtype == f
    return out[:, ::-1]


def restate_frame(objs, K, light, ambient, bg, H, W, dtype=np.float64, edge_offset=0.0, probe=None):
    """objs: (Mesh, colors (nv, 3) uint8, slot, R, T).  -> dict mask (H, W) uint8, depth (H, W) dtype (0 = background),
    owner (H, W) int64 (slot << 28 | face, -1 = none), colour (H, W, 3) float64 BGR before rounding (NaN = background),
    gap (H, W) float64: how far the runner-up triangle lies behind the owner (inf: there is none), frame (H, W, 3) uint8."""
    f = dtype
    pix, zs, keys, by_slot = [], [], [], {}
    for mesh, colors, slot, R, T in objs:
        p, z, k, proj = _candidates(mesh, slot, K, R, T, H, W, f, edge_offset, probe)
        pix.append(p); zs.append(z); keys.append(k)
        by_slot[int(slot)] = (mesh, colors, proj)
    owner = np.full(H * W, -1, np.int64)
    depth = np.zeros(H * W, f)
    gap = np.full(H * W, np.inf)
    colour = np.full((H * W, 3), np.nan)
    if pix and sum(len(p) for p in pix):
        pix, zs, keys = np.concatenate(pix), np.concatenate(zs), np.concatenate(keys)
        order = np.lexsort((keys, zs, pix))                     # per pixel: the smallest depth, then the lowest key
        pix, zs, keys = pix[order], zs[order], keys[order]
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        at = np.nonzero(first)[0]
        owner[pix[at]] = keys[at]
        depth[pix[at]] = zs[at]
        nxt = at + 1
        has = (nxt < len(pix))
        has[has] &= pix[nxt[has]] == pix[at[has]]
        gap[pix[at[has]]] = zs[nxt[has]].astype(np.float64) - zs[at[has]].astype(np.float64)
        for slot, (mesh, colors, proj) in by_slot.items():
            sel = at[(keys[at] >> FACE_BITS) == slot]
            if len(sel):
                colour[pix[sel]] = _resolve(mesh, colors, proj, keys[sel] & ((1 << FACE_BITS) - 1), pix[sel], W, light,
                                            ambient, f).astype(np.float64)
    mask = np.where(owner >= 0, (owner >> FACE_BITS) + 1, 0).astype(np.uint8)
    frame = (np.zeros((H, W, 3), np.uint8) if bg is None else np.asarray(bg, np.uint8)).reshape(H * W, 3).copy()
    own = owner >= 0
    frame[own] = np.clip(np.floor(colour[own] + 0.5), 0, 255).astype(np.uint8)
    return dict(mask=mask.reshape(H, W), depth=depth.reshape(H, W), owner=owner.reshape(H, W),
                colour=colour.reshape(H, W, 3), gap=gap.reshape(H, W), frame=frame.reshape(H, W, 3))


# ---- cases ---------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


LIGHT_AXIS = np.array([0.0, 0.0, -1.0])                # from the surface towards the camera: along the view axis
LIGHT_SIDE = unit([0.35, -0.45, -1.0])


@functools.lru_cache(maxsize=None)
def meshes():
    """plate, cube, the 320-face ellipsoid of bop_vsd_cases -- with smooth per-vertex colours."""
    ms = C.meshes()[:3]
    return [(m, mesh_colors(m, seed=i)) for i, m in enumerate(ms)]


def backgrounds(H, W, n=2, seed=5):
    return np.random.default_rng(seed + 131 * H + W).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _frame(K, objs, light=LIGHT_SIDE, ambient=0.4, bg=0):
    """objs: (mesh index, slot, R, T)."""
    return dict(K=np.asarray(K, np.float64), light=np.asarray(light, np.float64), ambient=float(ambient), bg=int(bg),
                objs=[(int(mi), int(g), np.asarray(R, np.float64), np.asarray(T, np.float64)) for mi, g, R, T in objs])


@functools.lru_cache(maxsize=None)
def cases(seed=7):
    """The ten scenes of the tests: (name, H, W, [frames]).  One kd6d_render_frames call per case."""
    rng = np.random.default_rng(seed)
    rr = lambda: C.random_rot(rng)  # noqa: E731
    I3 = np.eye(3)
    k70, k200, k130 = C._k(35.0, 25.0), C._k(100.0, 75.0), C._k(65.0, 48.0)
    out = [
        ("1 plate 64x48", 48, 64, [_frame(C.K_PLATE, [(0, 0, I3, [0.0, 0, 1000.0])], LIGHT_AXIS, 0.3)]),
        ("2 tilted plate 70x50", 50, 70, [_frame(k70, [(0, 2, C.rot([1, 2, 0], 0.7), [3.0, -2, 700.0])], bg=1)]),
        ("3 cube 200x150", 150, 200, [_frame(k200, [(1, 0, rr(), [-8.0, 5, 400.0])])]),
        ("4 ellipsoid cut by the border 130x97", 97, 130, [_frame(k130, [(2, 1, rr(), [-62.0, 40, 560.0])], bg=1)]),
        ("5 behind the camera, off-frame 70x50", 50, 70,
         [_frame(k70, [(2, 0, rr(), [0.0, 0, -600.0]), (1, 3, rr(), [400.0, 0, 800.0])])]),
        ("6 no object 70x50", 50, 70, [_frame(k70, [], bg=1)]),
        ("7 plates at two depths, both slot orders 70x50", 50, 70,
         [_frame(k70, [(0, 0, C.rot([0, 0, 1], 0.2), [-6.0, 3, 760.0]), (0, 1, C.rot([1, 0, 0], 0.3), [8.0, -4, 700.0])]),
          _frame(k70, [(0, 1, C.rot([0, 0, 1], 0.2), [-6.0, 3, 760.0]), (0, 0, C.rot([1, 0, 0], 0.3), [8.0, -4, 700.0])])]),
        ("8 cube and ellipsoid interpenetrating 130x97", 97, 130,
         [_frame(k130, [(1, 0, rr(), [0.0, 0, 500.0]), (2, 1, rr(), [18.0, 6, 490.0])])]),
        ("9 four objects 200x150", 150, 200,
         [_frame(k200, [(1, 0, rr(), [-40.3, -20, 520.0]), (2, 1, rr(), [30.0, 25, 480.0]), (0, 2, rr(), [35.0, -30, 600.0]),
                        (2, 3, rr(), [-15.5, 10, 430.0])], bg=1)]),
        ("10 frames of 3, 0 and 1 objects 130x97", 97, 130,
         [_frame(k130, [(2, 0, rr(), [-30.0, 10, 600.0]), (1, 1, rr(), [25.0, -12, 640.0]), (0, 3, rr(), [5.0, 20, 700.0])]),
          _frame(k130, [], bg=1),
          _frame(C._k(60.0, 50.0), [(1, 2, rr(), [10.0, -5, 450.0])], LIGHT_AXIS, 0.7, bg=1)]),
    ]
    return out


SINGLE_OBJECT_CASES = (0, 1, 2, 3)                     # one frame with one drawn object: depth == ops.render_depth's


def frame_objects(fr):
    ms = meshes()
    return [(ms[mi][0], ms[mi][1], g, R, T) for mi, g, R, T in fr["objs"]]


def pack(frames, H, W, mesh_list=None, order=None):
    """The arrays of one kd6d_render_frames call (numpy, float64 where the call takes fp32).  order: a permutation of
    the items (their list position must not matter)."""
    ms = meshes() if mesh_list is None else mesh_list
    voffs = np.concatenate([[0], np.cumsum([len(m.vertices) for m, _ in ms])])
    foffs = np.concatenate([[0], np.cumsum([len(m.faces) for m, _ in ms])])
    items = [(f, mi, g, R, T) for f, fr in enumerate(frames) for mi, g, R, T in fr["objs"]]
    if order is not None:
        items = [items[i] for i in order]
    i32 = lambda xs: np.asarray(xs, np.int32).reshape(-1)  # noqa: E731
    st = lambda xs, shape: np.stack(xs) if xs else np.zeros((0,) + shape)  # noqa: E731
    return dict(verts=np.concatenate([m.vertices for m, _ in ms]), faces=np.concatenate([m.faces for m, _ in ms]),
                vcol=np.concatenate([c for _, c in ms]),
                voff=i32([voffs[mi] for _, mi, *_ in items]), vcnt=i32([len(ms[mi][0].vertices) for _, mi, *_ in items]),
                foff=i32([foffs[mi] for _, mi, *_ in items]), fcnt=i32([len(ms[mi][0].faces) for _, mi, *_ in items]),
                item_frame=i32([f for f, *_ in items]), item_slot=i32([g for _, _, g, _, _ in items]),
                R=st([R for *_, R, _ in items], (3, 3)), T=st([T for *_, T in items], (3,)),
                K=np.stack([fr["K"] for fr in frames]), light=np.stack([fr["light"] for fr in frames]),
                ambient=np.asarray([fr["ambient"] for fr in frames], np.float64),
                bg_index=i32([fr["bg"] for fr in frames]), backgrounds=backgrounds(H, W))


ARG_ORDER = ("verts", "faces", "vcol", "voff", "vcnt", "foff", "fcnt", "item_frame", "item_slot", "R", "T", "K", "light",
             "ambient", "bg_index", "backgrounds")


# ---- references and tolerances -------------------------------------------------------------------------------------------
def reference_frame(fr, H, W):
    """-> (the float64 restatement at offset 0, ambiguous bool map)."""
    objs, bg = frame_objects(fr), backgrounds(H, W)[fr["bg"]]
    lo = restate_frame(objs, fr["K"], fr["light"], fr["ambient"], bg, H, W, np.float64, -EPS_PX)
    hi = restate_frame(objs, fr["K"], fr["light"], fr["ambient"], bg, H, W, np.float64, +EPS_PX)
    ref = restate_frame(objs, fr["K"], fr["light"], fr["ambient"], bg, H, W)
    return ref, (lo["owner"] != hi["owner"]) | (lo["depth"] != hi["depth"])


@functools.lru_cache(maxsize=None)
def references():
    """Per case: [(ref, ambiguous)] per frame."""
    return [[reference_frame(fr, H, W) for fr in frames] for _, H, W, frames in cases()]


@functools.lru_cache(maxsize=None)
def tolerances():
    """-> {"dev_px", "dev_c", "eps_c"}: 4 x the float32 restatement's deviation from the float64 one on this module's cases."""
    dev_px, dev_c = 0.0, 0.0
    for (_, H, W, frames), refs in zip(cases(), references()):
        for fr, (ref, amb) in zip(frames, refs):
            objs, bg = frame_objects(fr), backgrounds(H, W)[fr["bg"]]
            p64, p32 = [], []
            restate_frame(objs, fr["K"], fr["light"], fr["ambient"], bg, H, W, np.float64, probe=p64)
            r32 = restate_frame(objs, fr["K"], fr["light"], fr["ambient"], bg, H, W, np.float32, probe=p32)
            if p64 and sum(len(p) for p in p64):
                dev_px = max(dev_px, float(np.abs(np.concatenate(p64) - np.concatenate(p32)).max()))
            sure = ~amb & (ref["owner"] >= 0) & (r32["owner"] == ref["owner"])
            if sure.any():
                dev_c = max(dev_c, float(np.abs(r32["colour"] - ref["colour"])[sure].max()))
    return {"dev_px": dev_px, "dev_c": dev_c, "eps_c": MARGIN * dev_c}


def colour_verdict(got, ref_colour, sure, eps_c):
    """got (H, W, 3) uint8 against the float64 pre-rounding colour on the pixels `sure` -> (channels that had to be exact and
    are not, channels further than 1 level, the worst |got - c64|)."""
    c = ref_colour[sure]
    g = got[sure].astype(np.float64)
    want = np.clip(np.floor(c + 0.5), 0, 255)
    frac = np.abs((c + 0.5) - np.rint(c + 0.5))                      # distance of c from the nearest rounding boundary
    strict = frac > eps_c                                            # 0 <= albedo * shade <= 255: the clamp never acts
    wrong = int((strict & (g != want)).sum())
    far = int((np.abs(g - want) > 1).sum())
    return wrong, far, float(np.abs(g - c).max()) if c.size else 0.0


if __name__ == "__main__":
    import time
    t0 = time.time()
    t = tolerances()
    print("edge function: worst |f32 - f64| %.3e px (x4 = %.3e, eps_px of bop_vsd_cases %.3e);  colour: worst %.3e levels "
          "-> eps_c %.3e" % (t["dev_px"], MARGIN * t["dev_px"], EPS_PX, t["dev_c"], t["eps_c"]))
    for (name, H, W, frames), refs in zip(cases(), references()):
        for i, (ref, amb) in enumerate(refs):
            cov = ref["owner"] >= 0
            sure = cov & ~amb
            print("%-52s frame %d covered %5d ambiguous %3d (%.2f %%) smallest runner-up gap %.3e mm (eps_d %.3e)"
                  % (name, i, int(cov.sum()), int((amb & cov).sum()), 100.0 * (amb & cov).sum() / max(cov.sum(), 1),
                     float(ref["gap"][sure].min()) if sure.any() else math.inf, EPS_D))
    print("%.1f s" % (time.time() - t0))
