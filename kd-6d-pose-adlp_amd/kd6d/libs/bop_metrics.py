"""BOP pose-error metrics of the evaluation path: MSSD and MSPD (maximum symmetry-aware surface / projection distance),
their recalls and average recalls, and the BOP results file.

    e_MSSD = min_S max_v |(Rp v + Tp) - (Rg (S v) + Tg)|              S over the object's symmetry set, v over ALL vertices
    e_MSPD = min_S max_v |pi(Rp v + Tp) - pi(Rg (S v) + Tg)|          pi(q) = (K q).xy / ((K q).z + 1e-8), pixels

`symmetry_set` builds an object's set from `models_info.json` (BOP format) or from DATASETS.SYMMETRY_TYPES of the yaml,
`bop_errors_host` is the float64 numpy scorer of the definition above, `evaluate_bop_predictions` scores every object of a
validation in one kd6d_bop_errors call (csrc/bop_err.hip) and `bop_tables` turns errors into recalls:

    MSSD recall  e < theta * diameter,       theta = 0.05 ... 0.50 in steps of 0.05
    MSPD recall  e < theta * r pixels,       theta = 5 ... 50 in steps of 5, r = image width / 640
    AR_MSSD, AR_MSPD = mean over the ten thresholds per class, then the mean over the classes seen
    AR = (AR_MSSD + AR_MSPD) / 2

This AR has TWO terms and every place that prints it says so.  BOP's third, VSD, needs depth images and a renderer: it
is the opt-in second half of this module (--bop_vsd, csrc/bop_vsd.hip), which adds AR_VSD and the three-term
AR_BOP = (AR_VSD + AR_MSSD + AR_MSPD) / 3 beside the two-term number and leaves that one as it is.

VSD (visible surface discrepancy, BOP19: visib_mode bop19, delta = 15 mm, the step cost, normalised by the diameter).
For one (ground truth, estimate) pair of an object with mesh (V, F), camera K and the frame's depth image D_test (mm,
0 = missing):
    D_gt, D_est   depth renders of the mesh under (Rg, Tg) and (Rp, Tp)                       (render_depth_host)
    dist          = depth * sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1) per pixel, missing (0) stays 0
    vis(t, m)     = (t > 0 and m > 0 and m - t <= delta) or (t == 0 and m > 0)
    visib_gt      = vis(dist_test, dist_gt)
    visib_est     = vis(dist_test, dist_est) or (visib_gt and dist_est > 0)
    inter, union  = visib_gt & visib_est, visib_gt | visib_est;  n_u = |union|,  n_c = n_u - |inter|
    e_k           = (#{inter: |dist_gt - dist_est| >= tau_k * diameter} + n_c) / n_u,  1 when n_u == 0,  tau_k = 0.05 ... 0.50
    correct at (tau_k, theta_j) when e_k < theta_j, theta_j = 0.05 ... 0.50; AR_VSD of a class = the mean over the 100
    pairs, over the run the mean over the classes seen (bop_tables' convention; BOP itself averages over targets).
    An object without a prediction of its class has e_k = 1 for every k.
Rasteriser contract (render_depth_host in float64 and the kernel alike): pixel (u, v) has integer coordinates at its
centre, pi(q) = (K q).xy / (K q).z with K = [fx s cx; 0 fy cy; 0 0 1]; a triangle covers a pixel centre when all
three edge functions have the triangle's orientation sign or are zero (inclusive edges: a closed surface has no
cracks); both windings are drawn, zero-area projected triangles are skipped; a triangle with ANY vertex at camera
z <= 0 is dropped whole -- there is no near-plane clipping; the depth of a covered pixel is the depth of the triangle's
plane along the pixel's ray, z = (n . X0) / (n . r), r = K^-1 (u, v, 1), n = (X1 - X0) x (X2 - X0), clamped to the
triangle's vertex z range (which keeps edge-on slivers stable); the pixel keeps the minimum, background = 0.

Unpinned boundary: bop_toolkit is not available to this project, so the construction of the symmetry sets (the
discretisation of a continuous symmetry into ceil(pi / 0.01) = 315 rotations, the product of several generators, the
offset rule) and the two error functions are a RESTATEMENT of the published protocol, not a capture of the toolkit's
output.  They are pinned by closed-form answers instead (tests/test_bop_metrics_host.py), as the Sinkhorn is.  Our set
always contains the identity, and scoring takes a minimum: a superset of the toolkit's set can only lower an error.
The same holds for VSD: the visibility rule, the cost and the rasteriser above are a RESTATEMENT of the published BOP19
protocol, not a capture of the toolkit's output, pinned by closed-form answers (tests/test_bop_vsd_host.py).  Pixels on
a triangle's edge may differ from those of the toolkit's OpenGL rasteriser; that too is part of the unpinned boundary.
"""
import json
import math
import os

import numpy as np

from .evaluate import _depth_range, _scored_objects, _vertex_pool

CONTINUOUS_STEP = 0.01                                   # rad: bop_toolkit's max_sym_disc_step
CONTINUOUS_N = int(math.ceil(math.pi / CONTINUOUS_STEP))   # 315 rotations by 2 pi j / N
MSSD_THRESHOLDS = [round(0.05 * k, 2) for k in range(1, 11)]
MSPD_THRESHOLDS = [5 * k for k in range(1, 11)]
MSPD_REFERENCE_WIDTH = 640.0
AR_NOTE = "AR = (AR_MSSD + AR_MSPD) / 2 -- two terms; BOP's VSD term is not built, this is not BOP's three-term AR"
_AXES = {"X": (1.0, 0.0, 0.0), "Y": (0.0, 1.0, 0.0), "Z": (0.0, 0.0, 1.0)}


def _rotation(axis, angle):
    """Rodrigues: rotation by `angle` about the unit vector along `axis`."""
    a = np.asarray(axis, np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def _about_axis(axis, offset, n):
    """n rotations by 2 pi j / n about the axis through `offset`: (R, o - R o), j = 0 first (the identity, exactly)."""
    o = np.asarray(offset, np.float64).reshape(3)
    out = np.zeros((n, 3, 4))
    for j in range(n):
        R = np.eye(3) if j == 0 else _rotation(axis, 2.0 * math.pi * j / n)
        out[j, :, :3], out[j, :, 3] = R, o - R @ o
    return out


def _product(left, right):
    """Every (c, d) of left x right as R = R_c R_d, t = R_c t_d + t_c; left-major, so identity x identity stays first."""
    out = np.zeros((len(left) * len(right), 3, 4))
    k = 0
    for c in left:
        for d in right:
            out[k, :, :3] = c[:, :3] @ d[:, :3]
            out[k, :, 3] = c[:, :3] @ d[:, 3] + c[:, 3]
            k += 1
    return out


def _identity_set():
    out = np.zeros((1, 3, 4))
    out[0, :, :3] = np.eye(3)
    return out


def symmetry_set(cls, symmetry_types=None, model_info=None):
    """-> (S, 3, 4) float64 transforms [R | t] of class `cls`, the identity first.
    model_info: the object's entry of models_info.json, or None.  When given it is the source (it wins over the yaml):
    `symmetries_discrete` (a list of row-major 4x4, 16 numbers each; the identity is added) and
    `symmetries_continuous` (a list of {"axis", "offset"}, each discretised into CONTINUOUS_N rotations) combine as a
    product set.  Otherwise symmetry_types["cls_<cls>"] = [axis, period_deg, axis, period_deg, ...] with the meaning
    pose_symmetry_handling gives it: period > 0 -> the rotations by j * period about that axis through the origin,
    j = 0 ... round(360 / period) - 1; period == 0 -> a continuous symmetry.  No entry: the identity alone."""
    sets = []
    if model_info is not None:
        disc = [np.asarray(m, np.float64).reshape(4, 4)[:3, :] for m in model_info.get("symmetries_discrete", [])]
        if disc:
            sets.append(np.concatenate([_identity_set(), np.stack(disc)]))
        for c in model_info.get("symmetries_continuous", []):
            sets.insert(0, _about_axis(c["axis"], c.get("offset", [0, 0, 0]), CONTINUOUS_N))    # R = R_c R_d
    else:
        spec = (symmetry_types or {}).get("cls_" + str(cls), [])
        assert len(spec) % 2 == 0, "SYMMETRY_TYPES: [axis, period_deg, ...] expected, got %r" % (spec,)
        for i in range(len(spec) // 2):
            axis, period = spec[2 * i], float(spec[2 * i + 1])
            if axis not in _AXES:
                raise ValueError("symmetry axis should be 'X', 'Y' or 'Z'")
            n = CONTINUOUS_N if period == 0 else int(round(360.0 / period))
            sets.append(_about_axis(_AXES[axis], [0, 0, 0], n))
    out = _identity_set()
    for s in sets:
        out = _product(out, s)
    return out


def load_models_info(mesh_dir):
    """models_info.json of a BOP model directory -> {str(obj_id): entry}, or None when the file is absent."""
    path = os.path.join(mesh_dir or "", "models_info.json")
    if not mesh_dir or not os.path.isfile(path):
        return None
    with open(path, "r") as f:
        return {str(int(k)): v for k, v in json.load(f).items()}


def class_object_ids(mesh_dir):
    """-> [obj_id per class id]: the inverse of load_bop_meshes' objID_2_clsID (obj_XXXXXX.ply sorted by name)."""
    files = sorted(f for f in os.listdir(mesh_dir) if f.endswith(".ply"))
    return [int(os.path.splitext(f)[0][4:]) for f in files]


def dataset_symmetry_sets(datasets_cfg, n_cls):
    """The symmetry set of every class id 0 ... n_cls - 1 of a DATASETS section: from MESH_DIR/models_info.json when that
    file exists (an object without an entry there is asymmetric), from SYMMETRY_TYPES otherwise."""
    mesh_dir = datasets_cfg.get("MESH_DIR")
    info = load_models_info(mesh_dir)
    if info is None:
        return [symmetry_set(c, datasets_cfg.get("SYMMETRY_TYPES", {})) for c in range(n_cls)]
    ids = class_object_ids(mesh_dir)
    return [symmetry_set(c, None, info.get(str(ids[c]), {}) if c < len(ids) else {}) for c in range(n_cls)]


def pack_symmetries(sets):
    """(S, 3, 4) transforms [R | t] -> (S, 12) rows of kd6d_bop_errors' symmetry pool: R row-major (9), then t (3)."""
    S = np.asarray(sets, np.float64).reshape(-1, 3, 4)
    return np.concatenate([S[:, :, :3].reshape(-1, 9), S[:, :, 3]], axis=1)


def unpack_symmetries(pool):
    """(Ns, 12) pool rows (R row-major, then t) -> (Ns, 3, 4) transforms [R | t]; an (Ns, 3, 4) array passes through."""
    pool = np.asarray(pool, np.float64)
    if pool.ndim == 3:
        return pool.reshape(-1, 3, 4)
    pool = pool.reshape(-1, 12)
    return np.concatenate([pool[:, :9].reshape(-1, 3, 3), pool[:, 9:, None]], axis=2)


def bop_errors_host(verts, voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp):
    """float64 numpy scorer with kd6d_bop_errors' arguments and contract: verts (Nv, 3), syms (Ns, 12) pool rows (R
    row-major, then t: pack_symmetries) or (Ns, 3, 4) transforms,
    voff / vcnt / soff / scnt (P,), K / Rg / Rp (P, 3, 3), Tg / Tp (P, 3) -> err (P, 2) = (mssd, mspd).  scnt <= 0: the
    identity alone; vcnt <= 0: {0, 0}."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    syms = unpack_symmetries(syms)
    P = len(voff)
    err = np.zeros((P, 2))
    for p in range(P):
        n = int(vcnt[p])
        if n <= 0:
            continue
        v = verts[int(voff[p]):int(voff[p]) + n]
        S = syms[int(soff[p]):int(soff[p]) + int(scnt[p])] if int(scnt[p]) > 0 else _identity_set()
        Kp = np.asarray(K[p], np.float64).reshape(3, 3)
        R1, T1 = np.asarray(Rg[p], np.float64).reshape(3, 3), np.asarray(Tg[p], np.float64).reshape(3)
        R2, T2 = np.asarray(Rp[p], np.float64).reshape(3, 3), np.asarray(Tp[p], np.float64).reshape(3)
        pred = v @ R2.T + T2                                                       # (n, 3)
        sv = np.einsum("sij,nj->sni", S[:, :, :3], v) + S[:, None, :, 3]           # (S, n, 3)
        gt = sv @ R1.T + T1

        def pin(x):
            q = x @ Kp.T
            return q[..., :2] / (q[..., 2:3] + 1e-8)
        err[p, 0] = np.linalg.norm(gt - pred[None], axis=2).max(axis=1).min()
        err[p, 1] = np.linalg.norm(pin(gt) - pin(pred)[None], axis=2).max(axis=1).min()
    return err


def _recalls(errors, limits):
    e = np.asarray(errors, np.float64)
    return [float((e < lim).sum()) / len(e) for lim in limits]


def bop_tables(n_cls, objects, errors, mesh_diameters):
    """objects: (class, r) per ground-truth object, r = image width / 640; errors: (e_mssd, e_mspd) per object, None = no
    prediction of its class = an infinite error, missed at every threshold.  Recalls are fractions with a strict `<`.
    -> the dict valid() fills: per class {threshold: recall} and AR_MSSD / AR_MSPD, and over the classes seen AR_MSSD,
    AR_MSPD, AR (two terms, see AR_NOTE)."""
    per_cls = [([], []) for _ in range(n_cls)]
    for (c, r), e in zip(objects, errors):
        e3, e2 = (float("inf"), float("inf")) if e is None else (float(e[0]), float(e[1]))
        per_cls[c][0].append(e3 / float(mesh_diameters[c]))        # in diameters
        per_cls[c][1].append(e2 / float(r))                        # in pixels of a 640-wide image
    out = {"mssd_thresholds": list(MSSD_THRESHOLDS), "mspd_thresholds": list(MSPD_THRESHOLDS), "per_class": [],
           "n_objects": len(objects), "note": AR_NOTE}
    seen = []
    for c, (e3, e2) in enumerate(per_cls):
        if not e3:
            out["per_class"].append({})
            continue
        r3, r2 = _recalls(e3, MSSD_THRESHOLDS), _recalls(e2, MSPD_THRESHOLDS)
        entry = {"n": len(e3), "mssd_recall": {"%.2f" % t: v for t, v in zip(MSSD_THRESHOLDS, r3)},
                 "mspd_recall": {"%d" % t: v for t, v in zip(MSPD_THRESHOLDS, r2)},
                 "AR_MSSD": float(np.mean(r3)), "AR_MSPD": float(np.mean(r2))}
        out["per_class"].append(entry)
        seen.append(entry)
    out["AR_MSSD"] = float(np.mean([s["AR_MSSD"] for s in seen])) if seen else 0.0
    out["AR_MSPD"] = float(np.mean([s["AR_MSPD"] for s in seen])) if seen else 0.0
    out["AR"] = 0.5 * (out["AR_MSSD"] + out["AR_MSPD"])
    return out


def evaluate_bop_predictions(predictions, class_number, meshes, mesh_diameters, sym_sets, device, errors_fn=None):
    """predictions: {name: {'meta': {'K', 'class_ids', 'rotations', 'translations'[, 'width']}, 'pred': [[score, cls,
    R, T, ...], ...]}} -- the walk of evaluate._scored_objects: class-major, items in dict order, one object per class
    and image (asserted), scored against the first (most confident) prediction of its class.  sym_sets: per class id an
    (S, 3, 4) array (symmetry_set).  Every scored pair goes into ONE kd6d_bop_errors call over all vertices of its
    mesh (evaluate._vertex_pool); objects without a prediction never reach the device and count as infinite errors.
    A meta without 'width' (the synthetic loaders) scores MSPD at r = 1.
    errors_fn(verts, voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp) -> err (P, 2) replaces upload + call + copy back:
    numpy arrays in kd6d_bop_errors' argument order -- verts (Nv, 3) and syms (Ns, 12) float64 pools, the four index
    arrays int32 (P,), K / Rg / Rp (P, 3, 3) and Tg / Tp (P, 3) float64 (rounded to fp32 only at the upload) -- in walk
    order.  Without it a missing device is an error, not a fall-back.  -> bop_tables' dict."""
    n_cls = class_number - 1
    depth_min, depth_max = _depth_range(predictions)
    pool, offs = _vertex_pool(meshes, None if errors_fn is not None else device)
    sets = [np.asarray(s, np.float64).reshape(-1, 3, 4) for s in sym_sets]
    assert len(sets) >= n_cls and all(len(s) >= 1 for s in sets), "one symmetry set (identity at least) per class"
    s_offs = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    sym_pool = pack_symmetries(np.concatenate(sets))
    metas = [item["meta"] for c in range(n_cls) for item in predictions.values() if c in list(item["meta"]["class_ids"])]
    objects, slot = [], []
    voff, vcnt, soff, scnt, Ks, Rg, Tg, Rp, Tp = [], [], [], [], [], [], [], [], []
    for k, (c, K, R1, T1, _, cand) in enumerate(_scored_objects(predictions, n_cls, depth_min, depth_max)):
        objects.append((c, float(metas[k].get("width", MSPD_REFERENCE_WIDTH)) / MSPD_REFERENCE_WIDTH))
        if cand is None:
            slot.append(-1)
            continue
        slot.append(len(voff))
        n = int(offs[c + 1] - offs[c])
        assert n >= 1, "class %d has an empty mesh" % c
        voff.append(offs[c]); vcnt.append(n); soff.append(s_offs[c]); scnt.append(len(sets[c]))
        Ks.append(np.asarray(K, np.float64).reshape(3, 3))
        Rg.append(np.asarray(R1, np.float64).reshape(3, 3)); Tg.append(np.asarray(T1, np.float64).reshape(3))
        Rp.append(np.asarray(cand[2], np.float64).reshape(3, 3)); Tp.append(np.asarray(cand[3], np.float64).reshape(3))
    assert len(objects) == len(metas)
    P = len(voff)
    err = np.zeros((0, 2), np.float64)
    if P:
        arrays = [np.asarray(voff, np.int32), np.asarray(vcnt, np.int32), sym_pool, np.asarray(soff, np.int32),
                  np.asarray(scnt, np.int32), np.stack(Ks), np.stack(Rg), np.stack(Tg), np.stack(Rp), np.stack(Tp)]
        if errors_fn is not None:
            err = np.asarray(errors_fn(pool, *arrays), np.float64).reshape(P, 2)
        else:
            err = _device_errors(pool, arrays, device)
    errors = [None if s < 0 else (float(err[s, 0]), float(err[s, 1])) for s in slot]
    return bop_tables(n_cls, objects, errors, mesh_diameters)


def _device_errors(pool, arrays, device):
    """Upload the problem arrays, one ops.bop_errors call, copy err back once.  The index arrays were built above from
    the pools' own offsets."""
    import torch
    from .. import ops
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32 if a.dtype == np.float64 else a.dtype)).to(device)
           for a in arrays]
    voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp = dev
    err = ops.bop_errors(pool, voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp, validate=False,
                         max_scnt=int(arrays[4].max()))
    return err.cpu().numpy().astype(np.float64)


def format_ar_line(tables):
    """The one line train_kd.py and test.py print: it names what the AR is made of."""
    return "BOP AR_MSSD %.4f  AR_MSPD %.4f  AR %.4f over %d objects (%s)" % (
        tables["AR_MSSD"], tables["AR_MSPD"], tables["AR"], tables["n_objects"], AR_NOTE)


# ---- VSD: the float64 definitions ---------------------------------------------------------------------------------------
VSD_DELTA = 15.0                                         # mm: bop19's visibility tolerance
VSD_TAUS = [round(0.05 * k, 2) for k in range(1, 11)]    # misalignment tolerances, in diameters
VSD_THETAS = [round(0.05 * k, 2) for k in range(1, 11)]  # correctness thresholds on the error
AR_BOP_NOTE = ("AR_BOP = (AR_VSD + AR_MSSD + AR_MSPD) / 3 -- three terms; VSD, MSSD and MSPD are this project's "
               "restatement of the BOP19 protocol (bop_toolkit is not available), VSD with its own depth rasteriser")


def _camera(K):
    K = np.asarray(K, np.float64).reshape(3, 3)
    assert K[1, 0] == 0 and K[2, 0] == 0 and K[2, 1] == 0 and K[2, 2] == 1, "K = [fx s cx; 0 fy cy; 0 0 1] expected"
    return K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]


def render_depth_host(verts, faces, K, R, T, height, width):
    """The float64 definition of the rasteriser contract (module docstring): verts (n, 3), faces (m, 3) indices into
    verts, pose (R, T), camera K -> (height, width) float64 depth, the camera-frame z of the nearest surface, 0 =
    background.  One triangle at a time over the pixels of its bounding box."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    fx, sk, cx, fy, cy = _camera(K)
    X = v @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(T, np.float64).reshape(1, 3)
    Z = X[:, 2]
    safe = np.where(Z > 0, Z, 1.0)
    pu, pv = (fx * X[:, 0] + sk * X[:, 1]) / safe + cx, fy * X[:, 1] / safe + cy
    depth = np.full((height, width), np.inf)
    for i0, i1, i2 in f:
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
        inside = np.ones(px.shape, bool)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            inside &= sg * ((u[b] - u[a]) * (py - w[a]) - (w[b] - w[a]) * (px - u[a])) >= 0
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
        sub[inside] = np.minimum(sub[inside], z[inside])
    depth[np.isinf(depth)] = 0.0
    return depth


def ray_lengths(K, height, width):
    """(height, width) float64: |K^-1 (u, v, 1)| -- distance from the camera centre = depth * this."""
    fx, sk, cx, fy, cy = _camera(K)
    px, py = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    ry = (py - cy) / fy
    rx = (px - cx - sk * ry) / fx
    return np.sqrt(rx * rx + ry * ry + 1.0)


def _visible(t, m, delta):
    return ((t > 0) & (m > 0) & (m - t <= delta)) | ((t == 0) & (m > 0))


def vsd_counts_host(d_test, d_gt, d_est, K, diameter, delta=VSD_DELTA, taus=VSD_TAUS):
    """Steps 2-5 of the definition on three (H, W) depth maps -> int64 counts (2 + n_tau,) = (n_u, n_inter, cost_k ...),
    cost_k = #{inter: |dist_gt - dist_est| >= tau_k * diameter} + n_u - n_inter."""
    H, W = np.asarray(d_test).shape
    L = ray_lengths(K, H, W)
    t, g, e = np.asarray(d_test, np.float64) * L, np.asarray(d_gt, np.float64) * L, np.asarray(d_est, np.float64) * L
    vg = _visible(t, g, delta)
    ve = _visible(t, e, delta) | (vg & (e > 0))
    inter = vg & ve
    n_u, n_i = int((vg | ve).sum()), int(inter.sum())
    ad = np.abs(g - e)[inter]
    return np.asarray([n_u, n_i] + [int((ad >= float(tau) * float(diameter)).sum()) + n_u - n_i for tau in taus], np.int64)


def vsd_errors_host(verts, faces, voff, vcnt, foff, fcnt, K, Rg, Tg, Rp, Tp, diameter, frame, depth, delta=VSD_DELTA,
                    taus=VSD_TAUS):
    """float64 numpy scorer with kd6d_bop_vsd's arguments and contract: verts (Nv, 3), faces (Nf, 3) with indices
    relative to the problem's voff, voff / vcnt / foff / fcnt / frame (P,), K / Rg / Rp (P, 3, 3), Tg / Tp (P, 3),
    diameter (P,), depth (n_img, H, W) in the vertices' unit (0 = missing)
    -> counts (P, 2 + n_tau) int64, err (P, n_tau) float64 = cost_k / n_u, 1 when n_u == 0."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    depth = np.asarray(depth, np.float64)
    P, (H, W) = len(voff), depth.shape[1:]
    counts = np.zeros((P, 2 + len(taus)), np.int64)
    err = np.ones((P, len(taus)))
    for p in range(P):
        v = verts[int(voff[p]):int(voff[p]) + int(vcnt[p])]
        f = faces[int(foff[p]):int(foff[p]) + int(fcnt[p])]
        d_gt = render_depth_host(v, f, K[p], Rg[p], Tg[p], H, W)
        d_est = render_depth_host(v, f, K[p], Rp[p], Tp[p], H, W)
        counts[p] = vsd_counts_host(depth[int(frame[p])], d_gt, d_est, K[p], diameter[p], delta, taus)
        if counts[p, 0] > 0:
            err[p] = counts[p, 2:] / float(counts[p, 0])
    return counts, err


def bop_vsd_tables(n_cls, classes, errors, taus=VSD_TAUS, thetas=VSD_THETAS, delta=VSD_DELTA):
    """classes: the class of every ground-truth object; errors: its (n_tau,) VSD errors, None = no prediction of its class
    = e_k = 1 for every k.  An estimate is correct at (tau_k, theta_j) when e_k < theta_j (strict); AR_VSD of a class is
    the mean over the n_tau x n_theta pairs, AR_VSD of the run the mean over the classes seen (bop_tables' convention;
    BOP itself averages over targets).  -> {"vsd_thresholds", "per_class": [{"n", "AR_VSD"} or {}], "AR_VSD"}."""
    per_cls = [[] for _ in range(n_cls)]
    for c, e in zip(classes, errors):
        per_cls[c].append(np.ones(len(taus)) if e is None else np.asarray(e, np.float64).reshape(len(taus)))
    th = np.asarray(thetas, np.float64)
    out = {"vsd_thresholds": {"delta": float(delta), "tau": list(taus), "theta": list(thetas)}, "per_class": []}
    seen = []
    for es in per_cls:
        if not es:
            out["per_class"].append({})
            continue
        e = np.stack(es)                                               # (n, n_tau)
        ar = float((e[:, :, None] < th[None, None, :]).mean())
        out["per_class"].append({"n": len(es), "AR_VSD": ar})
        seen.append(ar)
    out["AR_VSD"] = float(np.mean(seen)) if seen else 0.0
    return out


def _face_pool(meshes):
    """Every mesh's triangles back to back, (Nf, 3) int32 with indices relative to the mesh's own first vertex, and each
    mesh's first row."""
    arrays = []
    for c, m in enumerate(meshes):
        f = getattr(m, "faces", None)
        if f is None or len(f) == 0:
            raise ValueError("VSD renders surfaces: the mesh of class %d has no faces (load_bop_meshes reads them from the "
                             "PLY files; a vertex-only mesh cannot be scored)" % c)
        arrays.append(np.asarray(f, np.int32).reshape(-1, 3))
    offs = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
    return (np.concatenate(arrays) if arrays else np.zeros((0, 3), np.int32)), offs


def evaluate_bop_vsd(predictions, class_number, meshes, mesh_diameters, depth_fn, device, errors_fn=None,
                     max_images_per_call=256, delta=VSD_DELTA, taus=VSD_TAUS, thetas=VSD_THETAS):
    """VSD of every ground-truth object of `predictions` (the walk of evaluate._scored_objects, as
    evaluate_bop_predictions: one object per class and image, scored against the most confident prediction of its class;
    an object without one never reaches the scorer and has e_k = 1).  meshes carry `.vertices` and `.faces`.
    depth_fn(meta) -> the frame's (H, W) depth image in the vertices' unit (mm), 0 = missing: a numpy array or a tensor.
    Frames are scored in chunks of at most max_images_per_call frames of EQUAL size, each chunk in one kd6d_bop_vsd
    call (csrc/bop_vsd.hip) over a depth pool of its frames, so that the pool stays bounded whatever the run's length.
    errors_fn(verts, faces, voff, vcnt, foff, fcnt, K, Rg, Tg, Rp, Tp, diameter, frame, depth, delta, taus) ->
    (counts, err (P, n_tau)) replaces upload + call + copy back: numpy arrays in kd6d_bop_vsd's argument order, float64
    pools (rounded to fp32 only at the upload).  Without it a missing device is an error, not a fall-back.
    -> bop_vsd_tables' dict."""
    n_cls = class_number - 1
    depth_min, depth_max = _depth_range(predictions)
    pool, offs = _vertex_pool(meshes, None)
    faces, foffs = _face_pool(meshes[:n_cls])
    items = [(name, item) for c in range(n_cls) for name, item in predictions.items()
             if c in list(item["meta"]["class_ids"])]
    classes, slot, probs, by_frame = [], [], [], {}
    for k, (c, K, R1, T1, _, cand) in enumerate(_scored_objects(predictions, n_cls, depth_min, depth_max)):
        classes.append(c)
        if cand is None:
            slot.append(-1)
            continue
        slot.append(len(probs))
        by_frame.setdefault(items[k][0], []).append(len(probs))
        probs.append((c, np.asarray(K, np.float64).reshape(3, 3), np.asarray(R1, np.float64).reshape(3, 3),
                      np.asarray(T1, np.float64).reshape(3), np.asarray(cand[2], np.float64).reshape(3, 3),
                      np.asarray(cand[3], np.float64).reshape(3)))
    assert len(classes) == len(items)
    err = np.ones((len(probs), len(taus)))
    dev_pools = None
    chunk, shape = [], None

    def flush():
        nonlocal dev_pools
        if not chunk:
            return
        idx = [q for _, _, qs in chunk for q in qs]
        frame = np.asarray([i for i, (_, _, qs) in enumerate(chunk) for _ in qs], np.int32)
        cs = [probs[q][0] for q in idx]
        arrays = [np.asarray([offs[c] for c in cs], np.int32), np.asarray([offs[c + 1] - offs[c] for c in cs], np.int32),
                  np.asarray([foffs[c] for c in cs], np.int32), np.asarray([foffs[c + 1] - foffs[c] for c in cs], np.int32),
                  np.stack([probs[q][1] for q in idx]), np.stack([probs[q][2] for q in idx]),
                  np.stack([probs[q][3] for q in idx]), np.stack([probs[q][4] for q in idx]),
                  np.stack([probs[q][5] for q in idx]), np.asarray([float(mesh_diameters[c]) for c in cs], np.float64), frame]
        depths = [d for _, d, _ in chunk]
        if errors_fn is not None:
            depth = np.stack([np.asarray(d.detach().cpu() if hasattr(d, "detach") else d, np.float64) for d in depths])
            _, e = errors_fn(pool, faces, *arrays, depth, delta, taus)
        else:
            if dev_pools is None:
                import torch
                dev_pools = (torch.from_numpy(pool.astype(np.float32)).to(device), torch.from_numpy(faces).to(device))
            e = _device_vsd(dev_pools, arrays, depths, device, delta, taus)
        err[idx] = np.asarray(e, np.float64).reshape(len(idx), len(taus))
        del chunk[:]

    for name, qs in by_frame.items():
        d = depth_fn(predictions[name]["meta"])
        if d is None or len(d.shape) != 2:
            raise ValueError("depth_fn: an (H, W) depth image expected for %r" % (name,))
        if chunk and (tuple(d.shape) != shape or len(chunk) >= max(int(max_images_per_call), 1)):
            flush()
        shape = tuple(d.shape)
        chunk.append((name, d, qs))
    flush()
    errors = [None if s < 0 else err[s] for s in slot]
    return bop_vsd_tables(n_cls, classes, errors, taus, thetas, delta)


def _device_vsd(dev_pools, arrays, depths, device, delta, taus):
    """Upload one chunk's problem arrays and depth pool, one ops.bop_vsd call, copy err back once.  The index arrays were
    built above from the pools' own offsets."""
    import torch
    from .. import ops
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32 if a.dtype == np.float64 else a.dtype)).to(device)
           for a in arrays]
    depth = torch.stack([(d if hasattr(d, "detach") else torch.from_numpy(np.ascontiguousarray(d, np.float32)))
                         .to(device=device, dtype=torch.float32) for d in depths]).contiguous()
    _, err = ops.bop_vsd(dev_pools[0], dev_pools[1], *dev, depth, delta, taus, validate=False)
    return err.cpu().numpy().astype(np.float64)


def rendered_depth_provider(meshes, device, height, width):
    """A depth_fn for frames that have no depth image (--synthetic): the frame's D_test is ops.render_depth of ALL its
    ground-truth objects at (height, width) -- the size of the frame meta["K"] belongs to -- the nearest surface per pixel.  meshes carry .vertices and .faces.
    -> depth_fn(meta) -> (height, width) fp32 device tensor."""
    import torch
    from .. import ops
    pool, offs = _vertex_pool(meshes, None)
    faces, foffs = _face_pool(meshes)
    verts_d = torch.from_numpy(pool.astype(np.float32)).to(device)
    faces_d = torch.from_numpy(faces).to(device)

    def depth_fn(meta):
        cs = [int(c) for c in meta["class_ids"]]
        if not cs:
            return torch.zeros(height, width, dtype=torch.float32, device=device)

        def i32(x):
            return torch.tensor(x, dtype=torch.int32, device=device)

        def f32(x, shape):
            return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64).reshape(shape), np.float32)).to(device)
        n = len(cs)
        maps = ops.render_depth(verts_d, faces_d, i32([offs[c] for c in cs]), i32([offs[c + 1] - offs[c] for c in cs]),
                                i32([foffs[c] for c in cs]), i32([foffs[c + 1] - foffs[c] for c in cs]),
                                f32(np.stack([np.asarray(meta["K"], np.float64).reshape(3, 3)] * n), (n, 3, 3)),
                                f32(np.stack([np.asarray(r) for r in meta["rotations"]]), (n, 3, 3)),
                                f32(np.stack([np.asarray(t).reshape(3) for t in meta["translations"]]), (n, 3)),
                                height, width, validate=False)
        far = torch.where(maps > 0, maps, torch.full_like(maps, float("inf"))).amin(dim=0)
        return torch.where(torch.isinf(far), torch.zeros_like(far), far)
    return depth_fn


def add_vsd_tables(bop, vsd_tables):
    """Merge bop_vsd_tables' dict into the dict valid() filled with bop_tables': the existing keys stay as they are ("AR"
    remains the two-term mean with its note); new are vsd_thresholds, AR_VSD per class and over the run, AR_BOP and
    AR_BOP_note."""
    bop["vsd_thresholds"] = vsd_tables["vsd_thresholds"]
    for entry, v in zip(bop["per_class"], vsd_tables["per_class"]):
        if entry and v:
            assert entry["n"] == v["n"]
            entry["AR_VSD"] = v["AR_VSD"]
    bop["AR_VSD"] = vsd_tables["AR_VSD"]
    bop["AR_BOP"] = (bop["AR_VSD"] + bop["AR_MSSD"] + bop["AR_MSPD"]) / 3.0
    bop["AR_BOP_note"] = AR_BOP_NOTE
    return bop


def format_ar_bop_line(tables):
    """The one line train_kd.py and test.py print with --bop_vsd, instead of format_ar_line's."""
    return "BOP AR_VSD %.4f  AR_MSSD %.4f  AR_MSPD %.4f  AR_BOP %.4f over %d objects (%s)" % (
        tables["AR_VSD"], tables["AR_MSSD"], tables["AR_MSPD"], tables["AR_BOP"], tables["n_objects"], AR_BOP_NOTE)


# ---- the BOP results file ---------------------------------------------------------------------------------------------
BOP_CSV_SYNTHETIC_ERROR = ("--bop_csv cannot be combined with --synthetic: a BOP results file names the scene and image "
                           "of every estimate, and synthetic batches have neither")


def bop_scene_im_id(path):
    """'<...>/<scene>/rgb/<im>.png' -> (scene_id, im_id)."""
    parts = path.strip().replace("\\", "/").split("/")
    if len(parts) < 3 or parts[-2] != "rgb":
        raise ValueError("BOP layout <scene>/rgb/<image> expected, got %r" % path)
    try:
        return int(parts[-3]), int(os.path.splitext(parts[-1])[0])
    except ValueError:
        raise ValueError("BOP layout <scene>/rgb/<image> with numeric scene and image names expected, got %r" % path)


def write_bop_csv(path, predictions, class_obj_ids):
    """The BOP results format, one line per kept prediction: scene_id,im_id,obj_id,score,R,t,time -- R nine and t three
    space-separated values in the dataset's units, time -1 (not measured).  predictions: valid()'s collection of every
    remapped prediction per image; class_obj_ids[class id] = obj_id (class_object_ids).  -> the number of lines."""
    n = 0
    with open(path, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for name, item in predictions.items():
            scene_id, im_id = bop_scene_im_id(name)
            for pred in item["pred"]:
                score, cls, R, T = pred[0], int(pred[1]), pred[2], pred[3]
                f.write("%d,%d,%d,%.9g,%s,%s,-1\n" % (
                    scene_id, im_id, int(class_obj_ids[cls]), float(score),
                    " ".join("%.9g" % x for x in np.asarray(R, np.float64).reshape(9)),
                    " ".join("%.9g" % x for x in np.asarray(T, np.float64).reshape(3))))
                n += 1
    return n
