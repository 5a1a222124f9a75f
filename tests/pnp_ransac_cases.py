"""Helper of tests/test_pnp_ransac_cases_host.py and tests/test_pnp_ransac_gpu.py (not collected): the cases of
kd6d_pnp_ransac / kd6d_teacher_pnp_gate (csrc/pnp.hip), an fp64 reference of ONE hypothesis, and the comparisons of a
launch's workspace with it.  Needs neither a GPU nor libkd6d.

Reference.  `reference(problem, seed, h, reproj_err)` follows the algorithm as DESIGN.md ("PnP-RANSAC on the device") and
the header of csrc/pnp.hip state it, written the plain way: one explicit row pair per correspondence, float64
throughout, numpy solvers (np.linalg.solve / svd / lstsq) -- none of the kernel's per-corner moment sums, packed
Cholesky or polar iteration.  The sampling hash is exact (Python integers masked to 64 bits).  The DLT's null vector is
DEFINED as 12 inverse-iteration steps on N + 1e-10 tr(N) I from (0.1, ..., 0.1, 1): an exact SVD null vector
(kd6d.libs.pnp._dlt) differs from it on poorly separated samples, so pnp._dlt is not the reference of that stage.  The
Gauss-Newton steps are kd6d.libs.pnp._refine as it is (its early exit below a step of 1e-10 moves no corner by 1e-9 px:
the steps it skips are smaller than the one it saw).

Decidable hypotheses.  The device scores in fp32 from a pose rounded to fp32 and RANSAC is discontinuous at its
threshold, so a hypothesis is compared only when THE REFERENCE ALONE says its result does not hang on rounding:
  * every float comparison on its path is at least a margin from flipping: |d - thr| >= DELTA_PX = 0.01 px for every
    correspondence (of a corner in front of the camera) of every scoring pass -- 10 x TOL_PX and ~100 x the fp32
    projection error at 640 px --, |z| >= DELTA_Z_MM = 1 mm for every corner of every scoring pass, and the DLT's failure
    conditions hold by DELTA_REL: every Cholesky pivot of N + mu I is >= 0.5 mu (exactly it is >= mu; fp64 rounding is
    ~1e-5 mu) and |det| is a factor 2 from its 1e-18 bound;
  * a second reference run whose votes are multiplied by 1 + 1e-10 g (g a seeded standard normal) ends in the same branch
    with the same count and a pose within PERTURB_PX = 1e-6 px at the corners (an ill-conditioned fit fails this).  The
    run is repeated for PERTURB_DRAWS = 4 seeded draws of g and every one has to pass: one draw measures the pose's
    sensitivity along one random direction and can underrate it several times over.  (The first GPU run showed it: the
    4-step pose of noise_half_r12 p 1 h 53, branch tight_lt6 with no inlier, moved 6.8e-7 px under the one draw first
    used, 3.4e-6 ... 6.0e-6 px under three of five others -- and 5e-4 ... 6e-3 px under 1e-7 g, the fp32 resolution of the
    votes themselves; the kernel's fp32 per-corner sums moved it 1.09e-3 px.  That is conditioning, not a kernel fault:
    the thresholds stay, the estimate of the sensitivity got better.)
The device result never decides whether a hypothesis is compared.  In every case at most MAX_UNDECIDABLE = 10 % of the
hypotheses may be undecidable (tests/test_pnp_ransac_cases_host.py asserts it).

Agreement criterion of a decidable hypothesis: the same count as an integer; with count -1 a zero pose; with a pose, the
8 corners projected through the problem's K with the slot's pose and with the reference pose differ by at most
pose_remap_cases.TOL_PX (1e-3 px, worst corner: fp32 storage of R, T moves a corner ~3.4e-5 px) and |det R - 1| <= 1e-5."""
import functools
from collections import namedtuple

import numpy as np

import pose_remap_cases as PR
from pose_remap_cases import TOL_PX

DELTA_PX = 0.01
DELTA_Z_MM = 1.0
DELTA_REL = 0.5
PERTURB_REL = 1e-10
PERTURB_PX = 1e-6
PERTURB_DRAWS = 4
MAX_UNDECIDABLE = 0.10
DET_TOL = 1e-5
SLOT = 16                       # workspace floats per hypothesis: count (int bits), R (9), T (3), 3 unused
INV_ITERS = 12
BRANCHES = ("invalid", "dlt0_failed", "loose_lt6", "refit_failed", "tight_lt6", "refined")
UNREACHABLE = {
    "dlt0_failed": "a unit null vector whose 3x3 part has |det| < 1e-18 (or a non-positive pivot of N + mu I, mu > 0) "
                   "needs every corner observed in one pixel; rounding alone then decides det: never decidable",
    "refit_failed": "the same conditions on the loose set, which holds >= 6 corners within 3 x reproj_err of a pose's "
                    "projections",
}
_MASK = (1 << 64) - 1
Margin = namedtuple("Margin", "px z_mm rel")
Result = namedtuple("Result", "branch count R T margin")


# ---- sampling (exact) --------------------------------------------------------------------------------------------------
def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def sample_cell(seed, h, k, n, swapped=False):
    """The cell through which hypothesis h observes corner k (swapped: the mutation that exchanges h and k)."""
    a, b = (k, h) if swapped else (h, k)
    z = splitmix64((int(seed) & _MASK) ^ splitmix64((((a & 0xFFFFFFFF) << 3) | (b & 0xFFFFFFFF)) & _MASK))
    return (z >> 32) % n


# ---- a problem: the cells that count, a box and an intrinsic, as the fp32 values the kernel reads -----------------------------
class Problem:
    def __init__(self, kp, box, K):
        self.kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 8, 2)
        self.box = np.ascontiguousarray(box, np.float32).reshape(8, 3)
        self.K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        for a in (self.kp, self.box, self.K):
            a.setflags(write=False)
        self._key = (self.kp.tobytes(), self.box.tobytes(), self.K.tobytes())

    def __hash__(self):
        return hash(self._key)

    def __eq__(self, other):
        return isinstance(other, Problem) and self._key == other._key


class _Prep:
    """What load_problem derives; votes: the fp32 votes as float64 (perturbed = 0), or a perturbed copy of them."""

    def __init__(self, pb, perturbed):
        self.n = pb.kp.shape[0]
        self.X = pb.box.astype(np.float64)
        self.K = pb.K.astype(np.float64)
        votes = pb.kp.astype(np.float64)
        with np.errstate(all="ignore"):
            fin = np.isfinite(votes).all() and np.isfinite(self.X).all() and np.isfinite(self.K).all()
            self.valid = bool(self.n >= 1 and fin and len(np.unique(pb.box, axis=0)) >= 6)
            if self.valid:
                self.c = self.X.mean(0)
                self.rms = float(np.sqrt(((self.X - self.c) ** 2).sum() / 8.0))
                det = float(np.linalg.det(self.K))
                self.valid = bool(self.rms > 0.0 and np.isfinite(det) and abs(det) > 0.0)
        if not self.valid:
            return
        if perturbed:                                # draw number 1 ... PERTURB_DRAWS
            g = np.random.default_rng(20240606 + perturbed).standard_normal(votes.shape)
            votes = votes * (1.0 + PERTURB_REL * g)
        self.votes = votes
        self.Kinv = np.linalg.inv(self.K)
        self.Xn = np.concatenate([(self.X - self.c) / self.rms, np.ones((8, 1))], 1)


@functools.lru_cache(maxsize=None)
def _prep(pb, perturbed):
    return _Prep(pb, perturbed)


# ---- the stages ---------------------------------------------------------------------------------------------------------
def _dlt(pp, corner, uv):
    """Pose of the correspondences (corner index, pixel) -> (R, T, relative margin) or (None, None, margin)."""
    m = len(corner)
    xn = np.concatenate([uv, np.ones((m, 1))], 1) @ pp.Kinv.T
    Xh = pp.Xn[corner]
    A = np.zeros((2 * m, 12))
    A[0::2, 0:4] = Xh
    A[0::2, 8:12] = -xn[:, 0:1] * Xh
    A[1::2, 4:8] = Xh
    A[1::2, 8:12] = -xn[:, 1:2] * Xh
    N = A.T @ A
    tr = float(np.trace(N))
    if not (tr > 0.0 and np.isfinite(tr)):
        return None, None, np.inf
    mu = 1e-10 * tr
    S = N + mu * np.eye(12)
    try:
        piv = float((np.diag(np.linalg.cholesky(S)) ** 2).min())
    except np.linalg.LinAlgError:
        return None, None, 0.0
    rel = piv / mu - (1.0 - DELTA_REL)          # >= DELTA_REL when the smallest pivot is the exact bound mu
    v = np.full(12, 0.1)
    v[11] = 1.0
    for _ in range(INV_ITERS):
        v = np.linalg.solve(S, v)
        v = v / np.linalg.norm(v)
    P = v.reshape(3, 4)
    M, p4 = P[:, :3], P[:, 3]
    det = float(np.linalg.det(M))
    if not np.isfinite(det):
        return None, None, 0.0
    rel = min(rel, abs(abs(det) / 1e-18 - 1.0))
    if abs(det) < 1e-18:
        return None, None, rel
    sg = -1.0 if det < 0.0 else 1.0
    M = sg * M / pp.rms
    p4 = sg * p4 - M @ pp.c
    U, S3, Vt = np.linalg.svd(M)
    R = U @ Vt
    scale = float(S3.mean())
    if not (scale > 0.0 and np.isfinite(scale) and np.linalg.det(R) > 0.0):
        return None, None, 0.0
    return R, p4 / scale, rel


def _score(pp, R, T, thr, mut):
    """-> inlier mask (n, 8), Margin of this pass."""
    from kd6d.libs import pnp
    pred, z = pnp.project(pp.K, R, T, pp.X)
    d = np.linalg.norm(pp.votes - pred[None], axis=2)
    front = np.ones(8, bool) if mut == "z_check_dropped" else z > 0
    inl = ((d <= thr) if mut == "strict_to_nonstrict" else (d < thr)) & front[None]
    px = float(np.abs(d[:, front] - thr).min()) if front.any() else np.inf
    return inl, Margin(px, float(np.abs(z).min()), np.inf)


def _enough(inl):
    return int(inl.sum()) >= 6 and int(inl.any(0).sum()) >= 6


def _run(pb, seed, h, reproj_err, mut, perturbed):
    from kd6d.libs import pnp
    pp = _prep(pb, perturbed)
    zero = (np.zeros((3, 3)), np.zeros(3))
    if not pp.valid:
        return Result("invalid", -1, *zero, Margin(np.inf, np.inf, np.inf))
    thr = float(np.float32(reproj_err))
    loose_thr = (2.0 if mut == "loose_factor_2" else 3.0) * thr
    marg = [Margin(np.inf, np.inf, np.inf)]

    def out(branch, count, R, T):
        return Result(branch, count, R, T, Margin(*[min(m[i] for m in marg) for i in range(3)]))

    corners = np.arange(8)
    cells = [sample_cell(seed, h, k, pp.n, swapped=mut == "hash_swapped") for k in range(8)]
    R0, T0, rel = _dlt(pp, corners, pp.votes[cells, corners])
    marg.append(Margin(np.inf, np.inf, rel))
    if R0 is None:
        return out("dlt0_failed", -1, *zero)
    loose, m = _score(pp, R0, T0, loose_thr, mut)
    marg.append(m)
    if not _enough(loose):
        return out("loose_lt6", -1, *zero)
    ci, ki = np.nonzero(loose)                      # cell-major, as the kernel walks them
    if mut == "refit_ignored":
        R, T = R0, T0
    else:
        R, T, rel = _dlt(pp, ki, pp.votes[ci, ki])
        marg.append(Margin(np.inf, np.inf, rel))
        if R is None:
            return out("refit_failed", -1, *zero)
    R, T = pnp._refine(pp.K, R, T, pp.X[ki], pp.votes[ci, ki], iters=3 if mut == "gn_steps_3" else 4)
    tight, m = _score(pp, R, T, thr, mut)
    marg.append(m)
    if not _enough(tight):
        return out("tight_lt6", int(tight.sum()), R, T)
    if mut == "skip_second_refinement":
        return out("refined", int(tight.sum()), R, T)
    ci, ki = np.nonzero(tight)
    R, T = pnp._refine(pp.K, R, T, pp.X[ki], pp.votes[ci, ki], iters=6)
    again, m = _score(pp, R, T, thr, mut)
    marg.append(m)
    return out("refined", int((tight if mut == "stale_count" else again).sum()), R, T)


@functools.lru_cache(maxsize=None)
def reference(problem, seed, h, reproj_err, mutate=None):
    """-> Result(branch, count, R (3,3), T (3,), margin) of hypothesis h of `problem` (its cells already clamped to the
    capacity).  mutate: one of the hypothesis-stage names of MUTATIONS."""
    with np.errstate(all="ignore"):
        return _run(problem, seed, h, reproj_err, mutate, 0)


def corner_gap(pb, Ra, Ta, Rb, Tb):
    a = PR.project(pb.K, np.concatenate([np.reshape(Ra, 9), np.reshape(Ta, 3)]), pb.box)
    b = PR.project(pb.K, np.concatenate([np.reshape(Rb, 9), np.reshape(Tb, 3)]), pb.box)
    return float(np.linalg.norm(a - b, axis=1).max())


@functools.lru_cache(maxsize=None)
def decidable(problem, seed, h, reproj_err):
    r = reference(problem, seed, h, reproj_err)
    if r.branch == "invalid":
        return True                                  # exact comparisons of the inputs
    if not (r.margin.px >= DELTA_PX and r.margin.z_mm >= DELTA_Z_MM and r.margin.rel >= DELTA_REL):
        return False
    for draw in range(1, PERTURB_DRAWS + 1):
        with np.errstate(all="ignore"):
            q = _run(problem, seed, h, reproj_err, None, draw)
        if q.branch != r.branch or q.count != r.count:
            return False
        if r.count >= 0 and corner_gap(problem, r.R, r.T, q.R, q.T) > PERTURB_PX:
            return False
    return True


# ---- mutations: one per stage --------------------------------------------------------------------------------------------
# where: "hyp" a switch of reference(); "batch" of case_slots(); "pick" of host_pick().  cases: where the host test looks
# for the failure.  unobservable: why no decidable hypothesis can show it (the entry stays).
MUTATIONS = {
    "skip_second_refinement": dict(where="hyp", cases=("noise_half_r12",)),
    "stale_count": dict(where="hyp", cases=("noise_half_r12",)),
    "loose_factor_2": dict(where="hyp", cases=("batch8_cnt_edges", "noise_half_r12")),
    "refit_ignored": dict(where="hyp", cases=("noise_half_r12",)),
    "gn_steps_3": dict(where="hyp", cases=("noise_half_r12",)),
    "hash_swapped": dict(where="hyp", cases=("batch8_cnt_edges",)),
    "z_check_dropped": dict(where="hyp", cases=("batch8_cnt_edges",)),
    "strict_to_nonstrict": dict(where="hyp", cases=("batch8_cnt_edges", "noise_half_r12"), unobservable=(
        "d < thr against d <= thr differ only at d == thr; a decidable hypothesis has |d - thr| >= DELTA_PX for every "
        "correspondence of every pass, so by construction none can show it (checked: the mutated reference equals the "
        "reference on every hypothesis of the listed cases)")),
    "cap_stride": dict(where="batch", cases=("batch8_cnt_edges",)),
    "tie_highest_h": dict(where="pick", cases=("noise_half_r12", "outliers_cap32")),
}


# ---- cases ---------------------------------------------------------------------------------------------------------------
def ape_k():
    return PR.internal_k()


def other_k():
    return PR.other_camera(PR.internal_k(), 1.35, -23.5, 17.25)


def skewed_k():
    """A camera with a skew term: K^-1 gets an off-diagonal entry, the only way the cross moment (sum of e f) of the
    kernel's refit sums enters a result.  Gauss-Newton models fx, fy, cx, cy alone, in the kernel as in pnp._refine."""
    K = PR.other_camera(PR.internal_k(), 0.9, 11.0, -6.5)
    K[0, 1] = 1.75
    return K


BOXES = np.concatenate([PR.BOXES, np.stack([PR.box(230.0, (1.2, 0.8, 1.0)), PR.box(140.0, (0.7, 1.0, 1.6))])])


def votes(seed, cells, box, K, sigma=0.0, far=0.0, near=0.0, reproj_err=5.0, mirrored=False):
    """(cells, 8, 2) fp32 votes of a drawn pose: Gaussian noise sigma px; a share `far` moved 30-90 px off and a share
    `near` moved 1.4-2.4 x reproj_err off (loose but not tight).  mirrored: the votes of corner k are those of the
    corner opposite in z, so the only projective fit has the object behind the camera."""
    from kd6d.libs import pnp
    rng = np.random.default_rng(seed)
    Rs, Ts = PR.poses(rng, 1)
    X = np.asarray(box, np.float64)
    if mirrored:
        X = X * np.array([1.0, 1.0, -1.0])
    K32 = np.asarray(K, np.float32).astype(np.float64)
    uv, _ = pnp.project(K32, Rs[0], Ts[0], np.tile(X, (cells, 1)))
    if sigma:
        uv = uv + rng.normal(0.0, sigma, uv.shape)
    u = rng.random(len(uv))
    for sel, lo, hi in ((u < far, 30.0, 90.0), ((u >= far) & (u < far + near), 1.4 * reproj_err, 2.4 * reproj_err)):
        a = rng.uniform(0, 2 * np.pi, int(sel.sum()))
        uv[sel] += rng.uniform(lo, hi, int(sel.sum()))[:, None] * np.stack([np.cos(a), np.sin(a)], 1)
    return uv.reshape(cells, 8, 2).astype(np.float32)


def _ransac_case(name, cap, iters, seed, reproj_err, probs):
    """probs: list of (kp (cells, 8, 2), cnt, box, K); cells beyond min(cnt, cap) are filler the kernel must not read
    into a result."""
    P = len(probs)
    kp = np.zeros((P, cap, 8, 2), np.float32)
    for p, (v, _, _, _) in enumerate(probs):
        v = np.asarray(v, np.float32)[:cap]
        kp[p, :len(v)] = v
    return dict(name=name, kind="ransac", cap=cap, iters=iters, seed=seed, reproj_err=float(reproj_err), kp=kp,
                cnt=np.array([c for _, c, _, _ in probs], np.int32),
                box=np.stack([np.asarray(b, np.float32) for _, _, b, _ in probs]),
                K=np.stack([np.asarray(k, np.float32) for _, _, _, k in probs]))


def _gate_case(name, cap, iters, seed, reproj_err, threshold, n_cls, n_class_rows, images, rows=12):
    """images: list of (kp, cnt, true box, K, logits (n_cls), row of cls, class that holds the true box).  Every other
    class row of kp3d is a zero box, so a wrong class choice ends in t_cnt = 0."""
    B = len(images)
    c = _ransac_case(name, cap, iters, seed, reproj_err, [(v, n, b, k) for v, n, b, k, _, _, _ in images])
    rng = np.random.default_rng(99)
    cls = rng.normal(0.0, 3.0, (rows, 16)).astype(np.float32)          # the rows no image points at mislead
    t_row = rng.integers(0, rows, (B, cap)).astype(np.int32)
    kp3d = np.zeros((B, n_class_rows, 8, 3), np.float32)
    for p, (_, _, b, _, logits, row, holder) in enumerate(images):
        cls[row, :n_cls] = np.asarray(logits, np.float32)
        t_row[p, 0] = row
        kp3d[p, holder] = b
    pr = np.float32(1.0) / (np.float32(1.0) + np.exp(-cls[t_row[:, 0], :n_cls]).astype(np.float32))
    chosen = [int(np.nonzero(q > np.float32(threshold))[0][0]) if (q > np.float32(threshold)).any() else int(np.argmax(q))
              for q in pr]
    c.update(kind="gate", threshold=float(threshold), n_cls=n_cls, n_class_rows=n_class_rows, cls=cls, t_row=t_row,
             kp3d=kp3d, chosen=chosen, prob=pr, box=np.stack([kp3d[p, chosen[p]] for p in range(B)]))
    return c


# Found with the reference: of the data seeds 502 ... 559 the first whose problem (40 % far outliers, launch seed 0) has its
# first best hypothesis beyond h = 64, in a lane other than 0, tied with a later one, and no undecidable hypothesis.
LATE_WINNER_DATA_SEED = 508


def build_cases():
    K, K2, K3 = ape_k(), other_k(), skewed_k()
    B = BOXES
    full = votes(104, 10, B[1], K, sigma=1.0)
    nan_vote = votes(205, 4, B[0], K)
    nan_vote[1, 3, 0] = np.nan
    tail_nan = votes(206, 10, B[2], K2, sigma=1.0)
    tail_nan[8, 2, 1] = np.nan                       # a cell behind cnt: not part of the problem
    inf_k = K.copy()
    inf_k[0, 0] = np.inf
    five = B[0].copy()
    five[5:] = five[0]
    zero_cnt_filler = np.full((10, 8, 2), np.nan, np.float32)
    v200, v201 = votes(200, 10, B[0], K, sigma=1.0), votes(201, 10, B[3], K2)
    h6a, h6b = votes(300, 10, B[1], K, sigma=6.0), votes(301, 10, B[4], K2, sigma=6.0)
    v102, v103 = votes(102, 6, B[2], K, sigma=1.0), votes(103, 7, B[3], K2, sigma=0.5, far=0.15, near=0.10)
    one = votes(700, 1, B[0], K)
    cases = [
        # every cnt class in one launch; different boxes, intrinsics and cell counts; 5 == 4 slot for slot
        _ransac_case("batch8_cnt_edges", 10, 65, 0, 5.0, [
            (votes(100, 1, B[0], K), 1, B[0], K), (votes(101, 2, B[1], K2, sigma=1.0), 2, B[1], K2),
            (v102, 6, B[2], K), (v103, 7, B[3], K2), (full, 10, B[1], K), (full, 13, B[1], K),
            (zero_cnt_filler, 0, B[0], K), (votes(107, 10, B[4], K2, mirrored=True), 10, B[4], K2)]),
        # sigma = reproj_err / 2: the tight set changes during the second refinement
        _ransac_case("noise_half_r12", 10, 130, 7, 12.0, [(h6a, 10, B[1], K), (h6b, 10, B[4], K2),
                                                          (votes(302, 10, B[3], K3, sigma=6.0), 10, B[3], K3)]),
        _ransac_case("iters63_r12", 10, 63, 7, 12.0, [(h6b, 10, B[4], K2), (h6a, 10, B[1], K)]),
        # loose is a proper superset of tight; capacity 32 full and partly used
        _ransac_case("outliers_cap32", 32, 300, 2 ** 40 + 3, 5.0, [
            (votes(400, 10, B[0], K, sigma=0.5, far=0.15, near=0.10), 10, B[0], K),
            (votes(401, 32, B[3], K2, sigma=1.0), 35, B[3], K2)]),
        # 40 % far outliers: nearly every hypothesis fails, the winner lies beyond the pick's first stride
        _ransac_case("late_winner", 10, 130, 0, 5.0, [
            (votes(LATE_WINNER_DATA_SEED, 10, B[2], K2, sigma=0.5, far=0.4), 10, B[2], K2),
            (votes(501, 10, B[0], K, sigma=0.5, far=0.4), 10, B[0], K)]),
        _ransac_case("invalid_among_valid", 10, 64, 7, 5.0, [
            (v200, 10, B[0], K), (nan_vote, 4, B[0], K), (v200, 10, B[0], inf_k), (v200, 10, five, K),
            (v200, 10, np.zeros((8, 3)), K), (v201, 10, B[3], K2), (tail_nan, 6, B[2], K2)]),
        # capacity 1: 4 clamps to 1
        _ransac_case("single_iter_cap1", 1, 1, 2 ** 40 + 3, 12.0, [(one, 1, B[0], K), (one, 4, B[0], K),
                                                                   (np.full((1, 8, 2), np.nan), 0, B[0], K)]),
        # gate.  threshold 0.5 = sigmoid(0) exactly
        _gate_case("gate_rows3", 10, 63, 7, 5.0, 0.5, 3, 3, [
            (v200, 10, B[0], K, (2.0, 3.0, -5.0), 5, 0),          # two classes above: the first wins
            (v201, 10, B[3], K2, (-3.0, -1.0, -2.0), 2, 1),       # none above: the argmax
            (tail_nan, 6, B[2], K2, (0.0, -4.0, 1.0), 7, 2),      # exactly at the threshold is not above it
            (zero_cnt_filler, 0, B[0], K, (4.0, 4.0, 4.0), 0, 0)]),
        _gate_case("gate_rows5", 10, 65, 0, 5.0, 0.5, 3, 5, [
            (votes(600, 10, B[0], K, sigma=60.0), 10, B[0], K, (1.0, -1.0, -2.0), 9, 0),    # no pose: t_cnt -> 0
            (v102, 6, B[2], K, (-2.0, 0.5, 3.0), 1, 1),
            (v103, 7, B[3], K2, (-0.5, -0.25, -0.125), 4, 2),
            (full, 10, B[1], K, (0.0, 0.0, 0.0), 11, 0)]),         # all at the threshold: argmax, the first of equals
    ]
    return cases


CASES = build_cases()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def problem_of(case, p, cells_of=None):
    """Problem p as the kernel sees it: min(cnt, cap) cells (cells_of: the problem whose cells are read instead)."""
    n = min(int(case["cnt"][p]), case["cap"])
    q = p if cells_of is None else cells_of
    return Problem(case["kp"][q, :n], case["box"][p], case["K"][p])


def case_results(case, mutate=None):
    """{(p, h): Result} of every hypothesis of every problem with cnt > 0."""
    where = MUTATIONS[mutate]["where"] if mutate else None
    out = {}
    for p in range(len(case["cnt"])):
        if case["cnt"][p] <= 0:
            continue
        pb = problem_of(case, p, cells_of=0 if where == "batch" else None)
        for h in range(case["iters"]):
            out[p, h] = reference(pb, case["seed"], h, case["reproj_err"], mutate if where == "hyp" else None)
    return out


def case_decidable(case):
    return {(p, h): decidable(problem_of(case, p), case["seed"], h, case["reproj_err"])
            for p in range(len(case["cnt"])) if case["cnt"][p] > 0 for h in range(case["iters"])}


def pack_slots(case, results, fill=np.nan):
    """The workspace (P, iters, 16) fp32 as the kernel packs it; problems with cnt 0 keep the fill."""
    ws = np.full((len(case["cnt"]), case["iters"], SLOT), fill, np.float32)
    for (p, h), r in results.items():
        ws[p, h, 0] = np.array([r.count], np.int32).view(np.float32)[0]
        ws[p, h, 1:10] = r.R.reshape(9)
        ws[p, h, 10:13] = r.T.reshape(3)
    return ws


def host_pick(ws, cnt, mutate=None):
    """pnp_pick_kernel on the host: -> ok, R, T, n_inliers, winner h (-1 without one)."""
    P = len(cnt)
    ok, ni, win = np.zeros(P, np.int32), np.zeros(P, np.int32), np.full(P, -1)
    R, T = np.zeros((P, 3, 3), np.float32), np.zeros((P, 3), np.float32)
    for p in range(P):
        if cnt[p] <= 0:
            continue
        counts = ws[p, :, 0].view(np.int32)
        tied = np.nonzero(counts == counts.max())[0]
        h = int(tied[-1] if mutate == "tie_highest_h" else tied[0])
        win[p] = h
        if counts[h] >= 6 and np.isfinite(ws[p, h, 1:13]).all():
            ok[p], ni[p], R[p], T[p] = 1, counts[h], ws[p, h, 1:10].reshape(3, 3), ws[p, h, 10:13]
    return ok, R, T, ni, win


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def check_slots(ws, case):
    """Compare a launch's workspace (P, iters, 16) fp32 with the reference on every decidable hypothesis.
    -> dict(worst_px, compared, total); raises AssertionError naming (case, p, h, branch)."""
    ws = np.asarray(ws, np.float32).reshape(len(case["cnt"]), case["iters"], SLOT)
    res, dec = case_results(case), case_decidable(case)
    worst, compared, bad = 0.0, 0, []
    for (p, h), r in res.items():
        if not dec[p, h]:
            continue
        compared += 1
        where = (case["name"], p, h, r.branch)
        got = int(ws[p, h, 0:1].view(np.int32)[0])
        if got != r.count:
            bad.append((where, "count", got, r.count))
            continue
        R, T = ws[p, h, 1:10].astype(np.float64).reshape(3, 3), ws[p, h, 10:13].astype(np.float64)
        if r.count < 0:
            if not np.array_equal(ws[p, h, 1:13], np.zeros(12, np.float32)):
                bad.append((where, "pose not zero"))
            continue
        if not np.isfinite(ws[p, h, 1:13]).all():
            bad.append((where, "non-finite pose"))
            continue
        gap = corner_gap(problem_of(case, p), R, T, r.R, r.T)
        worst = max(worst, gap)
        if not gap <= TOL_PX:
            bad.append((where, "corner gap px", gap))
        if not abs(np.linalg.det(R) - 1.0) <= DET_TOL:
            bad.append((where, "det R", float(np.linalg.det(R))))
    print("pnp_ransac %s: worst corner gap %.3e px, compared %d of %d hypotheses (%.1f %%), %d disagree"
          % (case["name"], worst, compared, len(res), 100.0 * compared / max(len(res), 1), len(bad)))
    assert not bad, (len(bad), bad[:8])
    return dict(worst_px=worst, compared=compared, total=len(res))


def check_pick(ws, ok, R, T, n_inliers, cnt):
    """The pick against the launch's own workspace: exact, independent of the numerics."""
    cnt = np.asarray(cnt)
    P = len(cnt)
    ws = np.asarray(ws, np.float32).reshape(P, -1, SLOT)
    wok, wR, wT, wni, win = host_pick(ws, cnt)
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)  # noqa: E731
    for p in range(P):
        where = (p, int(win[p]))
        assert int(ok[p]) == int(wok[p]), (where, "ok", int(ok[p]), int(wok[p]))
        assert int(n_inliers[p]) == int(wni[p]), (where, "n_inliers", int(n_inliers[p]), int(wni[p]))
        assert np.array_equal(bits(np.reshape(R[p], 9)), bits(wR[p].reshape(9))), (where, "R is not the winner's slot")
        assert np.array_equal(bits(np.reshape(T[p], 3)), bits(wT[p])), (where, "T is not the winner's slot")
    return win


def gate_expected(case):
    """t_cnt after the gate, from the reference alone: unchanged where a decidable hypothesis holds a pose (count >= 6),
    0 where every hypothesis, decidable or not, stays below 6; None where neither holds (the case would be ill-posed)."""
    res, dec = case_results(case), case_decidable(case)
    out = []
    for p in range(len(case["cnt"])):
        n = int(case["cnt"][p])
        if n <= 0:
            out.append(n)
            continue
        counts = [(res[p, h].count, dec[p, h]) for h in range(case["iters"])]
        if any(c >= 6 and d for c, d in counts):
            out.append(n)
        elif all(c < 6 for c, _ in counts):
            out.append(0)
        else:
            out.append(None)
    return out
