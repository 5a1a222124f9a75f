"""Cases, restatement and tolerances of the BOP metric tests (tests/test_bop_metrics_host.py, tests/test_bop_metrics_gpu.py).

`restate(case, dtype)` is MSSD / MSPD written out once and run in float64 (the reference of every device comparison) and
in float32 (the same code: inputs rounded to fp32 as an upload rounds them, every operation in fp32, in the difference
form the kernel uses -- (Rg S_R) v + (Rg S_t + (Tg - Tp)) - Rp v -- element by element, no BLAS call, so the numbers do
not depend on the machine).  It is independent of kd6d.libs.bop_metrics.bop_errors_host, which the host tests compare
with it.  Nothing is read from outside the repository; `write_bop_tree` writes a small BOP tree with a
models_info.json into a directory the test provides.

Tolerances.  A device error is accepted when |got - ref64| <= rel * |ref64| + abs, per metric.  Both numbers come from
the deviation d = |restate32 - restate64| over the cases of THIS module (the mixed launch and the closed forms), never
from the kernel:
    abs = 4 * max d over the cases whose float64 error is below 1 (mm or px): the floor that rounding the inputs to
          fp32 leaves (a 1000 mm translation carries 3e-5 mm), which does not scale with the error;
    rel = 4 * max d / ref64 over the cases whose float64 error is at least 1: the part that does.
The float32 restatement therefore meets the bound with a margin of 4 on every case, the margin pose_err uses; it covers
the device's different rounding of the 3x3 products (fused multiply-adds) and of the division.
`python tests/bop_metric_cases.py` prints the deviations and the bounds (recorded in profiles/bop_err_device.md).
"""
import functools
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "kd-6d-pose-adlp_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

V_SIZES = (1, 2, 63, 64, 65, 257, 1500)          # lane and wave tails of a 256-thread workgroup
S_SIZES = (1, 2, 3, 16, 17, 315, 630)            # tails of the 16-symmetry tile, one and two continuous sets
K0 = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])
SMALL = 1.0                                      # mm / px: below it a deviation counts as absolute, from it on as relative
MARGIN = 4.0
# what `python tests/bop_metric_cases.py` printed when profiles/bop_err_device.md was written; the host test checks
# that the bounds computed from the cases still are these
RECORDED = {"mssd": {"rel": 6.661e-05, "abs": 7.667e-05}, "mspd": {"rel": 1.031e-04, "abs": 2.441e-04}}


# ---- rotations, symmetry sets (through the module under test: its own tests pin it) ------------------------------------
def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def random_rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.linalg.det(q)


MODEL_INFO_630 = {"diameter": 100.0,
                  "symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 10.0, 0, 0, 0, 1]],   # half turn about X through (0,0,5)
                  "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 5.0]}]}


def sym_set(S):
    from kd6d.libs.bop_metrics import symmetry_set
    if S == 630:
        out = symmetry_set(0, None, MODEL_INFO_630)
    else:
        spec = {1: [], 2: ["Z", 180], 3: ["Z", 120], 16: ["Z", 22.5], 17: ["Z", 360.0 / 17], 315: ["Z", 0]}[S]
        out = symmetry_set(0, {"cls_0": spec})
    assert out.shape == (S, 3, 4)
    return out


def pack_syms(S):
    """(S, 3, 4) [R | t] -> (S, 12) pool rows as kd6d_bop_errors reads them: R row-major (9 floats), then t (3)."""
    S = np.asarray(S, np.float64).reshape(-1, 3, 4)
    return np.concatenate([S[:, :, :3].reshape(-1, 9), S[:, :, 3]], axis=1)


def unpack_syms(pool):
    pool = np.asarray(pool).reshape(-1, 12)
    return np.concatenate([pool[:, :9].reshape(-1, 3, 3), pool[:, 9:, None]], axis=2)


# ---- a case: the arrays of one kd6d_bop_errors call, float64 ----------------------------------------------------------
def pack(meshes, sets, probs):
    """meshes: list of (n, 3); sets: list of (S, 3, 4); probs: dicts mesh, sym (index or None = scnt 0), K, Rg, Tg, Rp, Tp."""
    voffs = np.concatenate([[0], np.cumsum([len(m) for m in meshes])])
    soffs = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    return dict(verts=np.concatenate(meshes).reshape(-1, 3),
                voff=np.asarray([voffs[p["mesh"]] for p in probs], np.int32),
                vcnt=np.asarray([len(meshes[p["mesh"]]) for p in probs], np.int32),
                syms=pack_syms(np.concatenate(sets)),
                soff=np.asarray([0 if p["sym"] is None else soffs[p["sym"]] for p in probs], np.int32),
                scnt=np.asarray([0 if p["sym"] is None else len(sets[p["sym"]]) for p in probs], np.int32),
                K=np.stack([p["K"] for p in probs]), Rg=np.stack([p["Rg"] for p in probs]),
                Tg=np.stack([p["Tg"] for p in probs]), Rp=np.stack([p["Rp"] for p in probs]),
                Tp=np.stack([p["Tp"] for p in probs]))


def subset(case, idx):
    """The problems idx of a case, over the same pools."""
    out = dict(case)
    for k in ("voff", "vcnt", "soff", "scnt", "K", "Rg", "Tg", "Rp", "Tp"):
        out[k] = np.ascontiguousarray(case[k][idx])
    return out


def restate(case, dtype=np.float64):
    """-> err (P, 2) float64 = (mssd, mspd), every operation carried out in `dtype`."""
    f = dtype
    verts, syms = case["verts"].astype(f), unpack_syms(case["syms"].astype(f))
    P = len(case["voff"])
    err = np.zeros((P, 2))
    eps = f(1e-8)
    for p in range(P):
        n = int(case["vcnt"][p])
        if n <= 0:
            continue
        v = verts[int(case["voff"][p]):int(case["voff"][p]) + n]
        if int(case["scnt"][p]) > 0:
            S = syms[int(case["soff"][p]):int(case["soff"][p]) + int(case["scnt"][p])]
        else:
            S = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(f)[None]
        K, Rg, Rp = case["K"][p].astype(f), case["Rg"][p].astype(f), case["Rp"][p].astype(f)
        Tg, Tp = case["Tg"][p].astype(f).reshape(3), case["Tp"][p].astype(f).reshape(3)

        def mat3(A, B):        # (3,3) x (...,3,m) -> (...,3,m), sums in the order ((0 + 1) + 2)
            return (A[:, 0, None] * B[..., 0, None, :] + A[:, 1, None] * B[..., 1, None, :]) + A[:, 2, None] * B[..., 2, None, :]

        def apply(M, x):       # (...,3,3) on (n,3) -> (...,n,3)
            return (M[..., None, :, 0] * x[:, 0, None] + M[..., None, :, 1] * x[:, 1, None]) + M[..., None, :, 2] * x[:, 2, None]

        def pin(x):
            q = apply(K, x.reshape(-1, 3)).reshape(x.shape)
            w = q[..., 2] + eps
            return q[..., 0] / w, q[..., 1] / w
        M = mat3(Rg, S[:, :, :3])                                     # (S,3,3) = Rg S_R
        c = mat3(Rg, S[:, :, 3:])[..., 0] + (Tg - Tp)                 # (S,3) = Rg S_t + (Tg - Tp)
        b = apply(Rp, v)                                              # (n,3)
        a = apply(M, v) + c[:, None, :]                               # (S,n,3)
        d = a - b[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        ua, va = pin(a + Tp)
        ub, vb = pin(b + Tp)
        du, dv = ua - ub[None], va - vb[None]
        p2 = du * du + dv * dv
        assert d2.dtype == f and p2.dtype == f
        err[p] = float(np.sqrt(d2.max(axis=1)).min()), float(np.sqrt(p2.max(axis=1)).min())
    return err


# ---- the mixed launch -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_case(seed=5):
    """49 problems, V_SIZES x S_SIZES.  One mesh per vertex count shared by its problems, except the 257-vertex row,
    where every problem has a mesh of its own; a different K per problem; pose errors rising from 0 (problem 0: the
    prediction IS the ground truth) to 20 degrees / 10 mm; every second problem predicts the ground truth composed with a
    symmetry other than the identity, so that the minimum is not at s = 0."""
    rng = np.random.default_rng(seed)
    meshes = [rng.normal(0, 23, (n, 3)) for n in V_SIZES] + [rng.normal(0, 23, (257, 3)) for _ in S_SIZES]
    sets = [sym_set(S) for S in S_SIZES]
    probs = []
    P = len(V_SIZES) * len(S_SIZES)
    for vi, n in enumerate(V_SIZES):
        for si, S in enumerate(S_SIZES):
            k = len(probs)
            Rg = random_rot(rng)
            Tg = np.array([rng.normal(0, 60), rng.normal(0, 40), rng.uniform(600, 1200)])
            K = K0.copy()
            K[0, 0] += rng.uniform(-30, 30); K[1, 1] += rng.uniform(-30, 30)
            K[0, 2] += rng.uniform(-15, 15); K[1, 2] += rng.uniform(-15, 15)
            Rb, Tb = Rg, Tg
            if k % 2 == 1 and S > 1:
                s = sets[si][int(rng.integers(1, S))]
                Rb, Tb = Rg @ s[:, :3], Rg @ s[:, 3] + Tg
            frac = k / (P - 1.0)
            axis = rng.normal(size=3)
            dirn = rng.normal(size=3)
            Rp = Rb @ rot(axis, math.radians(20.0) * frac)
            Tp = Tb + 10.0 * frac * dirn / np.linalg.norm(dirn)
            mesh = len(V_SIZES) + si if n == 257 else vi
            probs.append(dict(mesh=mesh, sym=si, K=K, Rg=Rg, Tg=Tg, Rp=Rp, Tp=Tp))
    return pack(meshes, sets, probs)


# ---- closed forms -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def closed_form_case(seed=9):
    """-> (case, exact (P, 2) with NaN where no closed form is claimed, names)."""
    rng = np.random.default_rng(seed)
    r, f, z, shift = 37.5, 600.0, 800.0, 6.0
    K = np.array([[f, 0, 320.0], [0, f, 240.0], [0, 0, 1.0]])
    one = np.array([[r, 0.0, 0.0]])
    cloud = rng.normal(0, 23, (300, 3))
    plane = np.concatenate([rng.normal(0, 23, (200, 2)), np.zeros((200, 1))], axis=1)
    meshes = [one, cloud, plane]
    sets = [sym_set(1), sym_set(2), sym_set(17), sym_set(315), sym_set(630)]
    Rg = random_rot(rng)
    Tg = np.array([35.0, -20.0, 900.0])
    half = rot([0, 0, 1], math.pi)
    d = np.array([3.0, -4.0, 12.0])
    probs, exact, names = [], [], []

    def add(name, mesh, sym, Kp, R1, T1, R2, T2, e3, e2):
        probs.append(dict(mesh=mesh, sym=sym, K=Kp, Rg=R1, Tg=T1, Rp=R2, Tp=T2))
        exact.append([e3, e2]); names.append(name)
    add("one vertex, half turn about Z, identity only", 0, 0, K0, Rg, Tg, Rg @ half, Tg, 2 * r, np.nan)
    add("one vertex, half turn about Z, Z-180 in the set", 0, 1, K0, Rg, Tg, Rg @ half, Tg, 0.0, 0.0)
    add("pure translation", 1, 0, K0, Rg, Tg, Rg, Tg + d, 13.0, np.nan)
    add("image-plane shift of a planar mesh at depth z", 2, 0, K, np.eye(3), np.array([0.0, 0.0, z]), np.eye(3),
        np.array([shift, 0.0, z]), shift, f * shift / (z + 1e-8))
    for si in (1, 2, 3, 4):                        # pred = gt o S_k, offsets included (the 630 set turns about (0,0,5))
        S = sets[si]
        for k in (1, len(S) // 2, len(S) - 1):
            add("pred = gt o S_%d of %d" % (k, len(S)), 1, si, K0, Rg, Tg, Rg @ S[k][:, :3], Rg @ S[k][:, 3] + Tg, 0.0, 0.0)
    return pack(meshes, sets, probs), np.asarray(exact), names


# ---- tolerances -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def references():
    """float64 and float32 restatement of the device cases, computed once."""
    out = {}
    for name, case in (("mixed", mixed_case()), ("closed", closed_form_case()[0])):
        out[name] = (restate(case, np.float64), restate(case, np.float32))
    return out


@functools.lru_cache(maxsize=None)
def tolerances():
    """-> {"mssd": {"rel", "abs", "dev_rel", "dev_abs"}, "mspd": {...}} by the rule of the module docstring."""
    r64 = np.concatenate([v[0] for v in references().values()])
    r32 = np.concatenate([v[1] for v in references().values()])
    out = {}
    for col, name in enumerate(("mssd", "mspd")):
        d, ref = np.abs(r32[:, col] - r64[:, col]), r64[:, col]
        small = ref < SMALL
        assert small.any() and (~small).any()
        dev_abs, dev_rel = float(d[small].max()), float((d[~small] / ref[~small]).max())
        out[name] = {"dev_abs": dev_abs, "dev_rel": dev_rel, "abs": MARGIN * dev_abs, "rel": MARGIN * dev_rel}
    return out


def within(got, ref, col):
    t = tolerances()[("mssd", "mspd")[col]]
    return np.abs(got - ref) <= t["rel"] * np.abs(ref) + t["abs"]


# ---- a scored collection: predictions as valid() keeps them ----------------------------------------------------------
class Mesh:
    def __init__(self, v):
        self.vertices = v


RECALL_DIAMETERS = [110.0, 95.0, 130.0]
RECALL_SYMMETRY_TYPES = {"cls_1": ["Z", 180], "cls_2": ["Z", 0]}


@functools.lru_cache(maxsize=None)
def recall_collection(seed=7):
    """24 images of 1 ... 3 objects of 3 classes (40, 700 and 1300 vertices; class 1 has a half turn, class 2 a continuous
    symmetry), pose errors spread over both threshold ranges, several objects without a prediction, images 640 and 1280
    wide.  The seed is one under which no float64 error lies within 1e-3 relative of a threshold (seeds 3, 4 and 5 have
    such an object; tests/test_bop_metrics_host.py checks the condition).  -> (predictions, meshes, diameters, symmetry
    sets)."""
    from kd6d.libs.bop_metrics import symmetry_set
    rng = np.random.default_rng(seed)
    meshes = [Mesh(rng.normal(0, 20, (n, 3))) for n in (40, 700, 1300)]
    sets = [symmetry_set(c, RECALL_SYMMETRY_TYPES) for c in range(3)]
    preds = {}
    for i in range(24):
        classes = sorted(rng.choice(3, size=int(rng.integers(1, 4)), replace=False).tolist())
        Rs = [random_rot(rng) for _ in classes]
        Ts = [np.array([[rng.normal(0, 60)], [rng.normal(0, 40)], [rng.uniform(600, 1200)]]) for _ in classes]
        pred = []
        for c, R, T in zip(classes, Rs, Ts):
            if rng.random() < 0.15:
                continue                                          # a missed object
            s = sets[c][int(rng.integers(0, len(sets[c])))]
            ang = math.radians(rng.uniform(0, 25))
            Rp = R @ s[:, :3] @ rot(rng.normal(size=3), ang)
            Tp = R @ s[:, 3:] + T + rng.normal(0, rng.uniform(0.2, 12), (3, 1))
            pred.append([float(rng.uniform(0.2, 1.0)), c, Rp, Tp])
        pred.sort(key=lambda q: -q[0])
        preds["000002/rgb/%06d.png" % i] = {
            "meta": {"K": K0 * (2.0 if i % 3 == 0 else 1.0) + np.diag([0, 0, -1.0 if i % 3 == 0 else 0.0]),
                     "width": 1280 if i % 3 == 0 else 640, "class_ids": classes, "rotations": Rs, "translations": Ts},
            "pred": pred}
    return preds, meshes, RECALL_DIAMETERS, sets


def near_threshold(err64, objects, diameters, rel=1e-3):
    """Scored objects (class, r) with float64 errors err64 (rows in the same order): those with an error within `rel`
    relative of an MSSD or MSPD threshold."""
    from kd6d.libs.bop_metrics import MSPD_THRESHOLDS, MSSD_THRESHOLDS
    hits = []
    for k, ((c, r), e) in enumerate(zip(objects, err64)):
        lims3 = [t * diameters[c] for t in MSSD_THRESHOLDS]
        lims2 = [t * r for t in MSPD_THRESHOLDS]
        if any(abs(e[0] - lim) <= rel * lim for lim in lims3) or any(abs(e[1] - lim) <= rel * lim for lim in lims2):
            hits.append(k)
    return hits


def restate_errors_fn(dtype=np.float64, seen=None):
    """An errors_fn for evaluate_bop_predictions that scores with restate(); `seen` collects (arrays, err)."""
    def fn(verts, voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp):
        case = dict(verts=verts, voff=voff, vcnt=vcnt, syms=syms, soff=soff, scnt=scnt, K=K, Rg=Rg, Tg=Tg, Rp=Rp, Tp=Tp)
        err = restate(case, dtype)
        if seen is not None:
            seen.append((case, err))
        return err
    return fn


def recall_collection_objects():
    """(class, r) of the collection's scored objects (those with a prediction) in walk order, and their float64 errors."""
    from kd6d.libs import bop_metrics as B
    preds, meshes, diam, sets = recall_collection()
    seen = []
    B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, None, errors_fn=restate_errors_fn(np.float64, seen))
    objects = []
    for c in range(3):
        for it in preds.values():
            if c in it["meta"]["class_ids"] and any(q[1] == c for q in it["pred"]):
                objects.append((c, it["meta"]["width"] / 640.0))
    (case, err), = seen
    assert len(objects) == len(err)
    return objects, err


# ---- a BOP tree with models_info.json --------------------------------------------------------------------------------
def write_bop_tree(root):
    """<root>/models/{obj_000001,obj_000005,obj_000009}.ply + models_info.json (object 5: a half turn about Z; object
    9: discrete + continuous, MODEL_INFO_630; object 1: no symmetry entry).  -> the models directory."""
    rng = np.random.default_rng(12)
    models = os.path.join(root, "models")
    os.makedirs(models)
    for oid, n in ((1, 12), (5, 20), (9, 15)):
        v = rng.normal(0, 30, (n, 3))
        with open(os.path.join(models, "obj_%06d.ply" % oid), "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                    "end_header\n" % n)
            for row in v:
                f.write("%.6f %.6f %.6f\n" % tuple(row))
    info = {"1": {"diameter": 90.0},
            "5": {"diameter": 80.0, "symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]},
            "9": MODEL_INFO_630}
    with open(os.path.join(models, "models_info.json"), "w") as f:
        json.dump(info, f)
    return models


if __name__ == "__main__":
    for name, (r64, r32) in references().items():
        d = np.abs(r32 - r64)
        print("%-6s %3d problems: float64 mssd %.4g ... %.4g mm, mspd %.4g ... %.4g px; worst |f32 - f64| mssd %.3e mm, "
              "mspd %.3e px" % (name, len(r64), r64[:, 0].min(), r64[:, 0].max(), r64[:, 1].min(), r64[:, 1].max(),
                                d[:, 0].max(), d[:, 1].max()))
    for name, t in tolerances().items():
        print("%s: deviation abs %.3e (errors < %g), rel %.3e (errors >= %g)  ->  bound abs %.3e, rel %.3e"
              % (name, t["dev_abs"], SMALL, t["dev_rel"], SMALL, t["abs"], t["rel"]))
    objects, err = recall_collection_objects()
    hits = near_threshold(err, objects, RECALL_DIAMETERS)
    print("recall collection: %d scored objects, %d within 1e-3 of a threshold" % (len(objects), len(hits)))
