"""The float64 definition of the colour renderer (csrc/render_frames.hip, kd6d.ops.render_frames): what a rendered
training frame IS.

Coverage and depth are the rasteriser contract of kd6d/libs/bop_metrics.py (render_depth_host), unchanged: pixel centres
at integer coordinates, inclusive edges, both windings, a triangle with a vertex at camera z <= 0 dropped whole, the
plane's depth along the pixel's ray clamped to the triangle's vertex z range, the minimum kept per pixel.  On top of it:

    owner    the triangle of the smallest depth at the pixel; among triangles whose depths there are equal, the one of the
             lowest (slot, face index).  The mask is slot + 1 (0 = background): the VISIBLE mask, as BOP's mask_visib.
    weights  b_i = E_i / Z_i, normalised to sum 1: E_i the edge function (of the pixel centre, in the image plane)
             of the edge OPPOSITE vertex i, Z_i the vertex' camera z -- perspective-correct barycentric coordinates.
    albedo   sum_i b_i colour_i (per-vertex uint8 RGB)
    normal   n = R normalize((v1 - v0) x (v2 - v0)), negated when n . X0 > 0, so that it faces the camera
    shade    ambient + (1 - ambient) max(0, n . light); light: a unit vector of the camera frame, from the surface
             towards the light
    channel  clamp(floor(albedo_c * shade + 0.5), 0, 255), stored BGR like the frames BOP_Dataset yields
    a pixel without an owner takes the background's pixel

Textures, near-plane clipping and anti-aliasing are not part of it.
"""
import math

import numpy as np

from .bop_metrics import _camera


def render_frame_host(objects, K, light, ambient, background, height, width):
    """One frame.  objects: dicts verts (n, 3), faces (m, 3), colors (n, 3) uint8 RGB, slot, R, T, at most one per slot;
    background (height, width, 3) uint8 or None (zeros).
    -> frame (height, width, 3) uint8 BGR, mask (height, width) uint8, depth (height, width) float64 (0 = background),
    colour (height, width, 3) float64 BGR: the channel values BEFORE floor(. + 0.5) (NaN on the background)."""
    fx, sk, cx, fy, cy = _camera(K)
    light = np.asarray(light, np.float64).reshape(3)
    ambient = float(ambient)
    depth = np.full((height, width), np.inf)
    mask = np.zeros((height, width), np.uint8)
    colour = np.full((height, width, 3), np.nan)
    slots = [int(o["slot"]) for o in objects]
    assert len(set(slots)) == len(slots), "one object per slot"
    for o in sorted(objects, key=lambda o: int(o["slot"])):       # ascending (slot, face) + strict "<": the lowest wins ties
        v = np.asarray(o["verts"], np.float64).reshape(-1, 3)
        f = np.asarray(o["faces"], np.int64).reshape(-1, 3)
        col = np.asarray(o["colors"], np.float64).reshape(-1, 3)
        R = np.asarray(o["R"], np.float64).reshape(3, 3)
        X = v @ R.T + np.asarray(o["T"], np.float64).reshape(1, 3)
        Z = X[:, 2]
        safe = np.where(Z > 0, Z, 1.0)
        pu, pv = (fx * X[:, 0] + sk * X[:, 1]) / safe + cx, fy * X[:, 1] / safe + cy
        for i0, i1, i2 in f:
            if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= len(v):
                continue                                                   # a face with an index outside the mesh
            if not (Z[i0] > 0 and Z[i1] > 0 and Z[i2] > 0):
                continue                                                   # dropped whole: no near-plane clipping
            u = np.array([pu[i0], pu[i1], pu[i2]])
            w = np.array([pv[i0], pv[i1], pv[i2]])
            xa, xb = max(int(math.ceil(u.min())), 0), min(int(math.floor(u.max())), width - 1)
            ya, yb = max(int(math.ceil(w.min())), 0), min(int(math.floor(w.max())), height - 1)
            if xa > xb or ya > yb:
                continue
            area = (u[1] - u[0]) * (w[2] - w[0]) - (w[1] - w[0]) * (u[2] - u[0])
            if area == 0:
                continue
            sg = 1.0 if area > 0 else -1.0
            px, py = np.meshgrid(np.arange(xa, xb + 1, dtype=np.float64), np.arange(ya, yb + 1, dtype=np.float64))
            E = [sg * ((u[b] - u[a]) * (py - w[a]) - (w[b] - w[a]) * (px - u[a])) for a, b in ((0, 1), (1, 2), (2, 0))]
            inside = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
            if not inside.any():
                continue
            n = np.cross(X[i1] - X[i0], X[i2] - X[i0])
            ry = (py - cy) / fy
            rx = (px - cx - sk * ry) / fx
            den = n[0] * rx + n[1] * ry + n[2]
            zlo, zhi = min(Z[i0], Z[i1], Z[i2]), max(Z[i0], Z[i1], Z[i2])
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(den != 0, float(n @ X[i0]) / den, zlo)
            z = np.clip(z, zlo, zhi)
            sub = depth[ya:yb + 1, xa:xb + 1]
            win = inside & (z < sub)
            if not win.any():
                continue
            sub[win] = z[win]
            mask[ya:yb + 1, xa:xb + 1][win] = int(o["slot"]) + 1
            b = np.stack([E[1] / Z[i0], E[2] / Z[i1], E[0] / Z[i2]], axis=-1)          # vertex i <- its opposite edge
            s = b.sum(axis=-1, keepdims=True)
            b = np.where(s > 0, b / np.where(s > 0, s, 1.0), 1.0 / 3.0)
            albedo = b @ col[[i0, i1, i2]]                                                  # (h, w, 3) RGB
            ln = np.linalg.norm(n)
            nu = n / ln if ln > 0 else n
            if nu @ X[i0] > 0:
                nu = -nu
            shade = ambient + (1.0 - ambient) * max(0.0, float(nu @ light))
            colour[ya:yb + 1, xa:xb + 1][win] = (albedo * shade)[win][:, ::-1]              # BGR
    bg = np.zeros((height, width, 3), np.uint8) if background is None else np.asarray(background, np.uint8)
    owned = mask > 0
    frame = bg.copy()
    frame[owned] = np.clip(np.floor(colour[owned] + 0.5), 0, 255).astype(np.uint8)
    depth[~owned] = 0.0
    return frame, mask, depth, colour


def render_frames_host(verts, faces, vcol, voff, vcnt, foff, fcnt, item_frame, item_slot, R, T, K, light, ambient,
                       bg_index, backgrounds, height, width):
    """kd6d.ops.render_frames on the host, in float64, from the same packed arrays (numpy) -> frames (n, H, W, 3) uint8,
    masks (n, H, W) uint8, depth (n, H, W) float64.  Every range must hold (what validate=True checks)."""
    K = np.asarray(K, np.float64).reshape(-1, 3, 3)
    n = len(K)
    R, T = np.asarray(R, np.float64).reshape(-1, 3, 3), np.asarray(T, np.float64).reshape(-1, 3)
    frames = np.zeros((n, height, width, 3), np.uint8)
    masks = np.zeros((n, height, width), np.uint8)
    depth = np.zeros((n, height, width))
    for fr in range(n):
        objs = [dict(verts=verts[voff[i]:voff[i] + vcnt[i]], faces=faces[foff[i]:foff[i] + fcnt[i]],
                     colors=vcol[voff[i]:voff[i] + vcnt[i]], slot=int(item_slot[i]), R=R[i], T=T[i])
                for i in range(len(voff)) if int(item_frame[i]) == fr]
        frames[fr], masks[fr], depth[fr], _ = render_frame_host(objs, K[fr], np.asarray(light).reshape(-1, 3)[fr],
                                                                np.asarray(ambient).reshape(-1)[fr],
                                                                backgrounds[int(bg_index[fr])], height, width)
    return frames, masks, depth
