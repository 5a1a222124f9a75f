"""Seeded LINEMOD-shaped synthetic batches (no dataset, no network): SURVEY.md 8(d).

Geometry follows the reference's data path: frames live in a 640x480 full frame with the
intrinsics of configs/ape.yaml:20; the network sees a 256x256 Dynamic-Zoom-In crop
(libs/dzi_libs.py:12,55-95) described by the 2x3 affine `bbox_trans` (full frame -> crop).
"""
import math

import numpy as np
import torch

from .libs.poses import ImageList, PoseAnnot

INTERNAL_K = [572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1]
MESH_DIAMETERS = [104.26, 250.85, 167.49, 177.43, 204.83, 154.63, 129.85, 264.12, 110.83, 164.65, 178.35,
                  145.61, 279.04, 287.24, 213.25]
LINEMOD_CLASSES = [0, 1, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14]


def cube_keypoints(diameters=MESH_DIAMETERS):
    """(n_class, 8, 3): corners of the cube whose diagonal is the mesh diameter."""
    signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    e = np.asarray(diameters, np.float32) / (2.0 * math.sqrt(3.0))
    return signs[None] * e[:, None, None]


# the 12 triangles of cube_keypoints' corners (corner index 4 ix + 2 iy + iz): what --bop_vsd renders for a surrogate mesh
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6],
                       [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(np.float32)


def batch_classes(image, instances=1, mixed_classes=False, class_id=0, class_offset=0):
    """Classes of image `image` of a make_batch() batch, one per instance, all distinct.  One instance: class_id, or
    with mixed_classes LINEMOD class (class_offset + image) mod 13.  Several: consecutive LINEMOD classes from there."""
    if instances == 1:
        return [LINEMOD_CLASSES[(class_offset + image) % len(LINEMOD_CLASSES)] if mixed_classes else class_id]
    first = (class_offset + image) * instances if mixed_classes else (
        LINEMOD_CLASSES.index(class_id) if class_id in LINEMOD_CLASSES else 0)
    return [LINEMOD_CLASSES[(first + g) % len(LINEMOD_CLASSES)] for g in range(instances)]


def teacher_cls_bias(instances=1, mixed_classes=False, class_id=0, hot=1.0, cold=-6.0):
    """head.cls_logits.bias of a synthetic (random-weight) teacher: `hot` for every class a make_batch() batch with
    these options can contain, `cold` elsewhere, so that the teacher emits cells for the objects in the batch."""
    if mixed_classes:
        present = set(LINEMOD_CLASSES)
    else:
        present = set(batch_classes(0, instances, False, class_id))
    return [hot if c in present else cold for c in range(len(MESH_DIAMETERS))]


def _make_multi(rng, imgs, batch, instances, crop, mixed_classes, full_frame, class_id, class_offset):
    """make_batch() for 2..4 instances per image: objects of distinct classes, masks with ids 1..N as non-overlapping
    rectangles, one per vertical strip (the last strip reaches the right edge, the last mask row stays free); the crop
    is a scaled view centred on the principal point."""
    K = np.asarray(INTERNAL_K, np.float32).reshape(3, 3)
    kp3d = cube_keypoints()
    H, W = (480, 640) if full_frame else (crop, crop)
    N = instances
    targets = []
    for i in range(batch):
        classes = batch_classes(i, N, mixed_classes, class_id, class_offset)
        R = np.stack([_random_rotation(rng) for _ in range(N)])
        T = np.stack([np.array([rng.normal(0, 60), rng.normal(0, 40), rng.uniform(700, 1600)], np.float32).reshape(3, 1)
                      for _ in range(N)])
        s = 1.0 if full_frame else float(rng.uniform(0.8, 1.6)) * crop / 256.0
        tx, ty = (0.0, 0.0) if full_frame else (W / 2.0 - s * K[0, 2], H / 2.0 - s * K[1, 2])
        bbox_trans = np.array([[s, 0, tx], [0, s, ty]], np.float32)
        mask = np.zeros((H, W), np.float32)
        for g in range(N):
            x0, x1 = g * W // N + 1, ((g + 1) * W // N - 1 if g < N - 1 else W)
            y0, y1 = int(rng.integers(0, max(H // 4, 1))), H - 1 - int(rng.integers(0, max(H // 4, 1)))
            mask[y0:y1, x0:x1] = g + 1
        targets.append(PoseAnnot(torch.from_numpy(kp3d.copy()), torch.from_numpy(K.copy()), torch.from_numpy(mask),
                                 torch.tensor(classes, dtype=torch.long), torch.from_numpy(R),
                                 torch.from_numpy(T), W, H, torch.tensor(float(s)), torch.from_numpy(bbox_trans)))
    return ImageList(torch.from_numpy(imgs), [(H, W)] * batch), targets


def make_batch(batch, seed, crop=256, mixed_classes=False, full_frame=False, class_id=0, class_offset=0, instances=1):
    """Returns (ImageList on CPU, list[PoseAnnot] on CPU).  mixed_classes: image i shows LINEMOD class
    (class_offset + i) mod 13 (a rank passes its first global image index as class_offset).  instances (1..4): objects
    per image, of distinct classes (batch_classes) with disjoint masks; 1 = the single centred object below."""
    if not 1 <= int(instances) <= 4:
        raise ValueError("make_batch: instances must be in 1..4 (got %r)" % (instances,))
    rng = np.random.default_rng(seed)
    K = np.asarray(INTERNAL_K, np.float32).reshape(3, 3)
    kp3d = cube_keypoints()
    H, W = (480, 640) if full_frame else (crop, crop)
    imgs = rng.standard_normal((batch, 3, H, W), dtype=np.float32)
    if int(instances) > 1:
        return _make_multi(rng, imgs, batch, int(instances), crop, mixed_classes, full_frame, class_id, class_offset)
    targets = []
    for i in range(batch):
        c = LINEMOD_CLASSES[(class_offset + i) % len(LINEMOD_CLASSES)] if mixed_classes else class_id
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))[None, :]
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        R = q.astype(np.float32)
        T = np.array([rng.normal(0, 60), rng.normal(0, 40), 900 + rng.normal(0, 80)], np.float32).reshape(3, 1)
        cam = R @ kp3d[c].T + T
        uv = K @ cam
        u, v = uv[0] / uv[2], uv[1] / uv[2]
        ext = max(u.max() - u.min(), v.max() - v.min())
        cx, cy = 0.5 * (u.max() + u.min()), 0.5 * (v.max() + v.min())
        if full_frame:
            s, tx, ty = 1.0, 0.0, 0.0
        else:
            s = crop / (1.5 * ext)                       # DZI box = 1.5 x max extent (dzi_libs.py:107)
            tx, ty = crop / 2.0 - s * cx, crop / 2.0 - s * cy
        bbox_trans = np.array([[s, 0, tx], [0, s, ty]], np.float32)
        mask = np.zeros((H, W), np.float32)
        hw = s * (u.max() - u.min()) / 3.0                # rectangle 2/3 of the projected extent
        hh = s * (v.max() - v.min()) / 3.0
        mx, my = s * cx + tx, s * cy + ty
        x0, x1 = int(max(0, round(mx - hw))), int(min(W, round(mx + hw)))
        y0, y1 = int(max(0, round(my - hh))), int(min(H, round(my + hh)))
        mask[y0:y1, x0:x1] = 1.0
        targets.append(PoseAnnot(torch.from_numpy(kp3d.copy()), torch.from_numpy(K.copy()), torch.from_numpy(mask),
                                 torch.tensor([c], dtype=torch.long), torch.from_numpy(R[None].copy()),
                                 torch.from_numpy(T[None].copy()), W, H,
                                 torch.tensor(float(s)), torch.from_numpy(bbox_trans)))
    return ImageList(torch.from_numpy(imgs), [(H, W)] * batch), targets


def _icosphere(level):
    """Unit icosphere: 12 vertices / 20 faces, each subdivision splits a face in four (level 4: 2562 / 5120)."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
         [9, 8, 1]]
    for _ in range(level):
        mid, nf = {}, []
        for a, b, c in f:
            m = []
            for i, j in ((a, b), (b, c), (c, a)):
                key = (min(i, j), max(i, j))
                if key not in mid:
                    p = v[i] + v[j]
                    v.append(p / np.linalg.norm(p))
                    mid[key] = len(v) - 1
                m.append(mid[key])
            nf += [[a, m[0], m[2]], [b, m[1], m[0]], [c, m[2], m[1]], m]
        f = nf
    return np.asarray(v, np.float64), np.asarray(f, np.int32)


SURROGATE_AXES = (1.0, 0.72, 0.5)       # semi-axes of surrogate_mesh in units of the half edge of the class's cube


def surrogate_mesh(class_id, level=4, diameters=MESH_DIAMETERS):
    """A mesh to RENDER for class `class_id` when no model file is read (--render_meshes surrogate): a subdivided
    ellipsoid with three different semi-axes, inscribed in the class's cube_keypoints box, coloured by a smooth function
    of the vertex position that no symmetry of the ellipsoid preserves -- no pose is ambiguous in colour or outline.
    -> (vertices (n, 3) float32, faces (m, 3) int32, colors (n, 3) uint8 RGB); level 4: 2562 vertices, 5120 faces."""
    s, f = _icosphere(int(level))
    e = float(diameters[int(class_id)]) / (2.0 * math.sqrt(3.0))
    v = s * (np.asarray(SURROGATE_AXES, np.float64) * e)[None]
    ph = 0.7 * int(class_id)
    c = np.stack([128 + 100 * np.sin(2.4 * s[:, 0] + 1.1 * s[:, 1] + ph), 128 + 100 * np.sin(2.9 * s[:, 1] - 1.3 * s[:, 2] + 1.0 + ph),
                  128 + 100 * np.sin(2.2 * s[:, 2] + 1.7 * s[:, 0] * s[:, 1] + 2.0 + ph)], axis=1)
    return v.astype(np.float32), f, np.clip(np.rint(c), 0, 255).astype(np.uint8)
