"""Helper of tests/test_pose_remap_host.py and tests/test_pose_remap_gpu.py (not collected): the cases of
kd6d_pose_remap (csrc/pnp.hip, train_kd.py --aug_pose_remap device) and what they must give.

The comparison target is kd6d.libs.pnp.remap_pose, the project's fp64 host solver, chained as
kd6d.libs.augment.draw_params chains it: Resize (src_K -> INTERNAL_K), the result cast to float32, then
RandomShiftScaleRotate (INTERNAL_K -> INTERNAL_K), the result cast to float32.  A stage the host cannot solve returns
its source pose (cast to float32) and ok = 0.  A class id outside the box table has no host counterpart (the host would
raise): the header defines ok = 0 and a zero pose for it.

Agreement criterion: the 8 box corners projected through INTERNAL_K with the device pose and with the host pose differ
by at most TOL_PX = 1e-3 px (Euclidean, worst corner).  Gauss-Newton's minimum does not depend on its start, so a
different DLT cannot move it; rounding R and T to fp32 moves a corner by up to 3.4e-5 px; 1e-3 px is 30 x that and 30 x
under the warp kernel's 1/32 px tap resolution.

Every case uses INTERNAL_K of configs/ape.yaml and 640 x 480 frames; boxes have diameters of 100 ... 290 mm and unequal
half-extents; T.z lies in 300 ... 2000 mm.  Expected values are computed once per case and kept (`expected`); the
launch-size cases are prefixes of ONE pool of 256 instances (a lane's result does not depend on the batch around it,
so a prefix of the pool's expectation is the prefix's expectation)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
TOL_PX = 1e-3
SIZES = (1, 63, 64, 65, 256)
APE_SSR = (0.05, 0.05, 10.0)           # AUGMENTATION_SHIFT / _SCALE / _ROTATION of configs/ape.yaml
WIDE_SSR = (0.2, 0.3, 45.0)


def internal_k():
    import yaml
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        return np.array(yaml.safe_load(f)["INPUT"]["INTERNAL_K"], np.float64).reshape(3, 3)


def box(diameter, ratios):
    """8 corners (float32, the data set's dtype) of a box with the given diagonal and half-extent ratios."""
    r = np.asarray(ratios, np.float64)
    h = 0.5 * diameter * r / np.linalg.norm(r)
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)


BOXES = np.stack([box(100.0, (1.0, 1.3, 0.7)), box(290.0, (0.6, 1.0, 1.5)), box(172.0, (1.4, 0.5, 1.0))])


class _Fixed:
    """A stand-in for `random` that hands out the given numbers (randint, randint, uniform, uniform: the order in which
    augment.shift_scale_rotate_matrix draws)."""

    def __init__(self, values):
        self.values = list(values)

    def randint(self, a, b):
        v = self.values.pop(0)
        assert a <= v <= b
        return int(v)

    def uniform(self, a, b):
        v = self.values.pop(0)
        assert min(a, b) <= v <= max(a, b)
        return float(v)


def ssr(limits, pleft, ptop, angle, dscale):
    """The 2x3 matrix RandomShiftScaleRotate builds from these four draws (fractions of the limits in -1 ... 1)."""
    from kd6d.libs.augment import shift_scale_rotate_matrix
    sh, sc, rot = limits
    dw, dh = int(W * sh), int(H * sh)
    M = shift_scale_rotate_matrix(sh, sc, rot, W, H, _Fixed([round(pleft * dw), round(ptop * dh), angle * rot, dscale * sc]))
    return M[:2].astype(np.float64)


def other_camera(K, focal, dcx, dcy):
    K2 = K.copy()
    K2[0, 0] *= focal; K2[1, 1] *= focal; K2[0, 2] += dcx; K2[1, 2] += dcy
    return K2


def poses(rng, n):
    """n rotations and translations whose object centre projects inside the frame, T.z in 300 ... 2000 mm."""
    K = internal_k()
    Rs, Ts = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Rs[i] = q * np.linalg.det(q)
        z = rng.uniform(300.0, 2000.0)
        u, v = rng.uniform(0.2 * W, 0.8 * W), rng.uniform(0.2 * H, 0.8 * H)
        Ts[i] = [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]
    return Rs, Ts


def _case(name, seed, n, src_K, M_resize, M_ssr, inst_img=None, inst_cls=None, boxes=None):
    rng = np.random.default_rng(seed)
    Rs, Ts = poses(rng, n)
    src_K = np.asarray(src_K, np.float64).reshape(-1, 3, 3)
    return dict(name=name, dst_K=internal_k(), src_K=src_K,
                inst_img=np.zeros(n, np.int32) if inst_img is None else np.asarray(inst_img, np.int32),
                inst_cls=np.zeros(n, np.int32) if inst_cls is None else np.asarray(inst_cls, np.int32),
                src_R=Rs, src_T=Ts, box=BOXES[:1].copy() if boxes is None else np.asarray(boxes, np.float32),
                M_resize=np.asarray(M_resize, np.float64).reshape(-1, 2, 3),
                M_ssr=None if M_ssr is None else np.asarray(M_ssr, np.float64).reshape(-1, 2, 3))


def _resize(src_K):
    from kd6d.libs.augment import resize_matrix
    return resize_matrix(internal_k(), src_K)[:2]


def build_cases():
    K = internal_k()
    I = np.eye(3)[:2]
    half, double = other_camera(K, 0.5, 14.5, -9.25), other_camera(K, 2.0, -21.0, 12.5)
    cases = [
        _case("identity", 1, 4, K, I, None),
        _case("resize_half_focal", 2, 4, half, _resize(half), None),
        _case("resize_double_focal", 3, 4, double, _resize(double), None),
        # the extreme draws of the ape.yaml limits, and one inside them
        _case("ssr_ape_limits_a", 4, 4, K, I, ssr(APE_SSR, 1, -1, 1, 1)),
        _case("ssr_ape_limits_b", 5, 4, K, I, ssr(APE_SSR, -1, 1, -1, -1)),
        _case("ssr_ape_inside", 6, 4, K, I, ssr(APE_SSR, 0.3, -0.6, 0.45, -0.2)),
        _case("ssr_wide_a", 7, 4, K, I, ssr(WIDE_SSR, 1, 1, 1, -1)),
        _case("ssr_wide_b", 8, 4, K, I, ssr(WIDE_SSR, -1, -0.5, -1, 1)),
        _case("chain_resize_ssr", 9, 4, half, _resize(half), ssr(APE_SSR, -0.7, 0.9, 0.8, 0.6)),
        _case("chain_resize_ssr_wide", 10, 4, double, _resize(double), ssr(WIDE_SSR, 0.6, -1, -0.9, 0.4)),
        _case("no_ssr_matrix", 11, 3, half, _resize(half), None),
        _case("mixed_classes", 12, 6, half, _resize(half), ssr(APE_SSR, 0.5, 0.5, -1, 1), inst_cls=[2, 0, 1, 1, 2, 0],
              boxes=BOXES),
        _case("two_images", 13, 5, [half, double], [_resize(half), _resize(double)],
              [ssr(APE_SSR, 1, 0, -0.5, 0.5), ssr(WIDE_SSR, -0.4, 0.8, 0.7, -0.6)], inst_img=[0, 1, 1, 0, 1],
              inst_cls=[1, 1, 0, 2, 2], boxes=BOXES),
    ]
    n = max(SIZES)
    rng = np.random.default_rng(14)
    cases.append(_case("pool", 15, n, [half, double, K], [_resize(half), _resize(double), I],
                       [ssr(APE_SSR, -1, 1, 1, -1), ssr(WIDE_SSR, 0.5, 0.25, -0.75, 1), ssr(APE_SSR, 0.1, -0.2, 0.3, 0.4)],
                       inst_img=rng.integers(0, 3, n), inst_cls=rng.integers(0, 3, n), boxes=BOXES))
    # failures beside instances that succeed.  Table rows: 0 a proper box, 1 eight equal corners, 2 a flat face listed
    # twice (4 distinct corners)
    flat = box(180.0, (1.0, 1.4, 0.8))
    flat[:, 2] = 0.0
    fboxes = np.stack([BOXES[0], np.full((8, 3), 12.5, np.float32), flat])
    f = _case("failures", 16, 7, half, _resize(half), ssr(APE_SSR, 0.5, -0.5, 0.5, 0.5), inst_cls=[0, 1, 2, 0, 0, 7, -1],
              boxes=fboxes)
    f["src_T"][3, 1] = np.inf           # a non-finite translation (instance 4 is its proper twin)
    cases.append(f)
    return cases


FAILING = {"failures": {1: "equal corners", 2: "4 distinct corners", 3: "non-finite T", 5: "class id 7 of 3",
                        6: "class id -1"}}
CASES = build_cases()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def prefix(case, n):
    """The first n instances of a case (same images, classes and matrices)."""
    out = dict(case, name="%s[:%d]" % (case["name"], n))
    for k in ("inst_img", "inst_cls", "src_R", "src_T"):
        out[k] = case[k][:n].copy()
    return out


def _m3(M):
    return np.vstack([M, [0.0, 0.0, 1.0]])


def host_chain(case):
    """-> pose (n, 2, 12) float32 = per stage {R 9, T 3}, ok (n, 2) int32: kd6d.libs.pnp.remap_pose chained as
    augment.draw_params chains it."""
    from kd6d.libs.pnp import remap_pose
    n = len(case["inst_img"])
    pose, ok = np.zeros((n, 2, 12), np.float32), np.zeros((n, 2), np.int32)
    K = case["dst_K"]
    for i in range(n):
        b, c = int(case["inst_img"][i]), int(case["inst_cls"][i])
        if not 0 <= c < len(case["box"]):
            continue
        X = case["box"][c].astype(np.float64)
        with np.errstate(all="ignore"):
            R, T, e = remap_pose(case["src_K"][b], case["src_R"][i], case["src_T"][i], X, K, _m3(case["M_resize"][b]))
        R, T = np.asarray(R, np.float32).reshape(3, 3), np.asarray(T, np.float32).reshape(3)
        pose[i, 0], ok[i, 0] = np.concatenate([R.reshape(9), T]), int(e != -1)
        if case["M_ssr"] is None:
            pose[i, 1], ok[i, 1] = pose[i, 0], ok[i, 0]
            continue
        with np.errstate(all="ignore"):
            R, T, e = remap_pose(K, R, T, X, K, _m3(case["M_ssr"][b]))
        R, T = np.asarray(R, np.float32).reshape(3, 3), np.asarray(T, np.float32).reshape(3)
        pose[i, 1], ok[i, 1] = np.concatenate([R.reshape(9), T]), int(e != -1)
    return pose, ok


_EXPECTED = {}


def expected(case):
    """host_chain(case), computed once per case; a prefix of a case takes the prefix of the case's expectation."""
    name = case["name"]
    if "[:" in name:
        pose, ok = expected(by_name(name.split("[:")[0]))
        n = len(case["inst_img"])
        return pose[:n], ok[:n]
    if name not in _EXPECTED:
        pose, ok = host_chain(case)
        pose.setflags(write=False); ok.setflags(write=False)
        _EXPECTED[name] = (pose, ok)
    return _EXPECTED[name]


def project(K, pose12, X):
    """(8, 2) px of the corners X seen through K with the pose {R 9, T 3} (float64 arithmetic)."""
    p = np.asarray(pose12, np.float64)
    cam = p[:9].reshape(3, 3) @ np.asarray(X, np.float64).T + p[9:].reshape(3, 1)
    uv = np.asarray(K, np.float64) @ cam
    return (uv[:2] / uv[2]).T


def pixel_gap(K, X, pose_a, pose_b):
    """The criterion's figure: the largest distance between a corner's two projections."""
    return float(np.linalg.norm(project(K, pose_a, X) - project(K, pose_b, X), axis=1).max())


def source_pose32(case, i):
    """Instance i's source pose as its fp32 rounding, {R 9, T 3}."""
    return np.concatenate([case["src_R"][i].reshape(9), case["src_T"][i].reshape(3)]).astype(np.float32)
