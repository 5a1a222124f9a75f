"""Cases of the kernel-level tests of the small-set Sinkhorn kernel (csrc/sinkhorn.hip, kd6d_sinkhorn_div_fwd_bwd):
tests/test_sinkhorn_small_gpu.py runs them on the device, tests/test_sinkhorn_cases_host.py checks them on the CPU.

Reference of every numeric comparison: oracle/sinkhorn_ref.kd_loss_images in float64 on the fp32 inputs.  `reference()`
makes the same sinkhorn_divergence call as kd_loss_images (one image: its transposes, its arguments) because the eight
per-keypoint values S_k are summed away inside kd_loss_images; the host test asserts that loss, gx and ga are bitwise
kd_loss_images' and that loss_img is S_k.sum().  blur and scaling are fp32-representable numbers, the kernel's float
arguments, so that both sides see the same schedule.

Inputs: LINEMOD-like votes clustered round 8 keypoint centres in normalised coordinates, as in
test_kernels_gpu.test_sinkhorn_kernel_vs_oracle, but with weights drawn independently per (cell, keypoint).

Bounds (profiles/sinkhorn_small_tolerances.md): the restatement is evaluated in numpy float32 on the CPU, its largest
deviation from the float64 result per (group, output) is RECORDED_DEV, the bound is 8 x that with a floor of 4 fp32
ulps, relative to the largest magnitude of the output in the case: max|got - ref| <= bound * max|ref|.  A draw whose own
spread x 8 exceeds the cap of the existing test (loss 1e-4, gx and ga 2e-3, gx 5e-3 on the long schedules) is reseeded
(`choose_seed`, deterministic; the outcome is SEEDS) -- the restatement alone decides, never a device result.

`python tests/sinkhorn_cases.py` prints the deviations, the seed search and the table of the profile note."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.sinkhorn_ref import epsilon_schedule, kd_loss_images, sinkhorn_divergence  # noqa: E402

f32 = np.float32
F = lambda v: float(f32(v))                                     # noqa: E731  the value a float argument carries
REGIMES = {"unb": dict(blur=F(0.001), reach=0.5),               # production: unbalanced
           "bal": dict(blur=F(0.01), reach=None)}               # balanced, masses normalised per image and keypoint
LANE_MAX, CAP, SCHED_TABLE = 16, 128, 128                       # kernel: 16-lane path, kCap, kSched
SIZES = [(1, 1), (1, 5), (2, 3), (3, 2), (4, 4),
         (15, 16), (16, 16), (16, 17), (17, 16), (17, 17),
         (19, 33), (63, 64), (64, 64), (64, 65), (65, 64),
         (127, 128), (128, 128), (128, 1), (3, 128)]
SCHED_SIZES = [(12, 9), (23, 41)]                               # one lane-path, one general-path size
ZERO_SIZES = [(12, 16), (39, 68)]                               # N % 3 == 0, M % 4 == 0: exactly a third / a quarter
COINCIDENT_SIZES = [(7, 5), (20, 70)]
FLOOR = 4.0 * 2.0 ** -23
OUTPUTS = ("loss_kp", "loss_img", "gx", "ga")
CAPS = {"loss_kp": 1e-4, "loss_img": 1e-4, "gx": 2e-3, "ga": 2e-3}          # test_sinkhorn_kernel_vs_oracle's
CAPS_SCHED = dict(CAPS, gx=5e-3)
KNIFE = 1e-3

Case = namedtuple("Case", "name N M regime kind steps scaling seed")
# kind: plain | zero (a third of alpha, a quarter of beta exactly 0) | coincident | sched (steps = schedule length
# asked for; 0 = scaling given).  group of the bound: the regime, "sched" for the long schedules.

# seeds chosen by choose_seed() (first seed from 0 whose draw meets the knife-edge margins and the spread caps);
# cases not listed use seed 0.  `python tests/sinkhorn_cases.py --search` prints this table.
SEEDS = {
    "plain_4x4_unb": 2,
    "plain_15x16_unb": 1,
    "plain_19x33_unb": 9,
    "zero_12x16_unb": 5,
    "zero_39x68_unb": 2,
    "sched200_12x9_unb": 1,
    "sched128_23x41_unb": 8,
    "sched129_23x41_unb": 3,
    "sched200_23x41_unb": 11,
}

# cases that cannot meet the gx cap at blur 0.001 within the search and keep their place at blur 0.01 (unbalanced,
# reach 0.5): name -> blur
BLUR_OVERRIDE = {
    "plain_1x5_unb": F(0.01),
    "plain_3x128_unb": F(0.01),
}

# largest fp32-vs-fp64 deviation of the restatement per group/output over the cases (measure_deviations())
RECORDED_DEV = {
    "bal/ga": 6.262e-05,
    "bal/gx": 1.970e-06,
    "bal/loss_img": 3.900e-07,
    "bal/loss_kp": 8.011e-07,
    "sched/ga": 1.088e-06,
    "sched/gx": 6.231e-04,
    "sched/loss_img": 9.980e-07,
    "sched/loss_kp": 2.131e-06,
    "unb/ga": 2.615e-06,
    "unb/gx": 2.473e-04,
    "unb/loss_img": 3.562e-06,
    "unb/loss_kp": 6.026e-06,
}


def _name(N, M, regime, kind, steps=0):
    return "%s_%dx%d_%s" % (kind if kind != "sched" else "sched%d" % steps, N, M, regime)


def _table():
    out = []
    for regime in REGIMES:
        for N, M in SIZES:
            out.append(("plain", N, M, regime, 0, 0.5))
        for N, M in ZERO_SIZES:
            out.append(("zero", N, M, regime, 0, 0.5))
        for N, M in COINCIDENT_SIZES:
            out.append(("coincident", N, M, regime, 0, 0.5))
    for N, M in SCHED_SIZES:
        out.append(("sched", N, M, "unb", SCHED_TABLE, 0.0))          # last step still in the table
        out.append(("sched", N, M, "unb", SCHED_TABLE + 1, 0.0))      # first step past it
        out.append(("sched", N, M, "unb", 0, F(0.97)))                # about 200 steps
    cases = {}
    for kind, N, M, regime, steps, scaling in out:
        name = _name(N, M, regime, kind, steps if steps else 200) if kind == "sched" else _name(N, M, regime, kind)
        cases[name] = Case(name, N, M, regime, kind, steps, scaling, SEEDS.get(name, 0))
    return cases


def group(case):
    return "sched" if case.kind == "sched" else case.regime


def caps(case):
    return CAPS_SCHED if case.kind == "sched" else CAPS


def draw(N, M, regime, seed, kind="plain"):
    """fp32 xs (N,8,2), alpha (N,8), yt (M,8,2), beta (M,8)"""
    r = np.random.default_rng([seed, N, M])
    centres = r.uniform(0.3, 0.7, (8, 2))
    xs = (centres[None] + r.normal(0, 0.02, (N, 8, 2))).astype(f32)
    yt = (centres[None] + r.normal(0, 0.01, (M, 8, 2))).astype(f32)
    al = r.uniform(0.05, 0.95, (N, 8)).astype(f32)
    be = r.uniform(0.2, 0.99, (M, 8)).astype(f32)
    if kind == "zero":
        # a third / a quarter of every keypoint's column, other cells for every keypoint
        for w, share in ((al, 3), (be, 4)):
            for k in range(8):
                w[r.permutation(w.shape[0])[:w.shape[0] // share], k] = 0.0
    if kind == "coincident":
        p = r.uniform(0.3, 0.7, 2).astype(f32)
        xs[:] = p
        yt[:] = p
    if REGIMES[regime]["reach"] is None:
        al /= al.sum(0, keepdims=True)
        be /= be.sum(0, keepdims=True)
    return xs, al, yt, be


def diameters(xs, yt):
    """box diagonal of all 8*(N+M) points: in fp64 from the fp32 data (the oracle's) and in fp32 (the kernel's)"""
    pts = np.concatenate([xs.reshape(-1, 2), yt.reshape(-1, 2)])
    ext64 = pts.astype(np.float64).max(0) - pts.astype(np.float64).min(0)
    ext32 = pts.max(0) - pts.min(0)
    d32 = np.sqrt(ext32[0] * ext32[0] + ext32[1] * ext32[1], dtype=f32)
    return float(np.linalg.norm(ext64)), float(d32)


def schedule_facts(xs, yt, blur, scaling):
    """-> (steps, margin): len(epsilon_schedule) and the distance of q = (ln blur - ln d)/ln scaling from the nearest
    integer, the smaller over both evaluations of d.  Raises when the two disagree on the step count."""
    steps, margin = set(), 1.0
    for d in diameters(xs, yt):
        d = max(d, 1e-12)
        q = (np.log(blur) - np.log(d)) / np.log(scaling)
        margin = min(margin, -q if q < 0 else min(q - np.floor(q), np.ceil(q) - q))
        steps.add(len(epsilon_schedule(2, d, blur, scaling)))
    assert len(steps) == 1, ("fp32 and fp64 diameters give different schedules", steps)
    return steps.pop(), float(margin)


@functools.lru_cache(maxsize=None)
def _inputs(name, seed):
    c = _table()[name]
    xs, al, yt, be = draw(c.N, c.M, c.regime, seed, c.kind)
    blur = BLUR_OVERRIDE.get(name, REGIMES[c.regime]["blur"])
    scaling = c.scaling
    if c.kind == "sched" and c.steps:
        # steps = n_ar + 2, n_ar = ceil(q): put q in the middle of (n_ar - 1, n_ar]
        d = diameters(xs, yt)[0]
        scaling = F(np.exp((np.log(blur) - np.log(d)) / (c.steps - 2 - 0.5)))
    for a in (xs, al, yt, be):
        a.setflags(write=False)
    return dict(case=c, xs=xs, al=al, yt=yt, be=be, blur=blur, scaling=scaling, reach=REGIMES[c.regime]["reach"])


def inputs(name, seed=None):
    """the case's fp32 arrays (read-only, shared) and OT settings"""
    return _inputs(name, CASES[name].seed if seed is None else seed)


def check_conditions(inp):
    """input conditions of a case, so that no tolerance has to absorb a discontinuity; -> (steps, margin)"""
    c = inp["case"]
    steps, margin = schedule_facts(inp["xs"], inp["yt"], inp["blur"], inp["scaling"])
    assert margin >= KNIFE, (c.name, "schedule knife edge", margin)
    if c.kind == "coincident":
        assert steps == 2
    if c.kind == "sched":
        assert steps == c.steps if c.steps else 180 <= steps <= 230, (c.name, steps)
    for w in (inp["al"], inp["be"]):
        assert (w >= 0).all() and (w.max(0) > 0).all()
    if c.kind == "zero":
        assert c.N % 3 == 0 and c.M % 4 == 0
        assert ((inp["al"] == 0).sum(0) == c.N // 3).all() and ((inp["be"] == 0).sum(0) == c.M // 4).all()
    if inp["reach"] is None:
        np.testing.assert_allclose(inp["al"].sum(0), 1.0, rtol=1e-5)
        np.testing.assert_allclose(inp["be"].sum(0), 1.0, rtol=1e-5)
    return steps, margin


def ot_reference(xs, al, yt, be, blur, scaling, reach, dtype=np.float64):
    """ONE image through the oracle: dict(loss_kp (8), loss_img (), gx (N,8,2), ga (N,8)) in float64 holding `dtype`
    results; the call is kd_loss_images' (oracle/sinkhorn_ref.py)."""
    t = lambda a: np.transpose(a.astype(np.float64), (1, 0) + tuple(range(2, a.ndim)))     # noqa: E731
    S, g, fa = sinkhorn_divergence(t(al), t(xs), t(be), t(yt), blur, scaling, reach, with_grad=True, dtype=dtype)
    return dict(loss_kp=np.asarray(S, np.float64), loss_img=np.float64(S.sum()),
                gx=np.transpose(g, (1, 0, 2)).astype(np.float64), ga=np.transpose(fa, (1, 0)).astype(np.float64))


@functools.lru_cache(maxsize=None)
def _reference(name, seed, dtype):
    i = _inputs(name, seed)
    out = ot_reference(i["xs"], i["al"], i["yt"], i["be"], i["blur"], i["scaling"], i["reach"], dtype)
    for a in out.values():
        a.setflags(write=False)
    return out


def reference(name, dtype=np.float64, seed=None):
    """computed once per case and shared (read-only arrays)"""
    return _reference(name, CASES[name].seed if seed is None else seed, dtype)


def kd_loss_images_reference(name):
    """the same case through kd_loss_images itself -> loss (1), valid (1), gx, ga"""
    i = inputs(name)
    c = i["case"]
    s_off, t_off = np.array([0, c.N], np.int32), np.array([0, c.M], np.int32)
    return kd_loss_images(i["xs"].astype(np.float64), i["al"].astype(np.float64), s_off, i["yt"].astype(np.float64),
                          i["be"].astype(np.float64), t_off, blur=i["blur"], scaling=i["scaling"], reach=i["reach"])


def case_deviation(name, seed=None):
    """fp32-vs-fp64 deviation of the restatement per output: relative to max|ref64|, absolute for coincident points"""
    r64, r32 = reference(name, np.float64, seed), reference(name, np.float32, seed)
    dev = {}
    for o in OUTPUTS:
        err = float(np.max(np.abs(r32[o] - r64[o])))
        scale = float(np.max(np.abs(r64[o])))
        dev[o] = err if CASES[name].kind == "coincident" else err / scale
    return dev


def measure_deviations(per_case=False):
    """{"group/output": largest deviation over the group's cases}; coincident-point cases are compared absolutely
    against the regime's bound and do not enter.  per_case: also {case: {output: deviation}}."""
    dev, each = {}, {}
    for name, c in CASES.items():
        each[name] = case_deviation(name)
        if c.kind == "coincident":
            continue
        for o, v in each[name].items():
            k = "%s/%s" % (group(c), o)
            dev[k] = max(dev.get(k, 0.0), v)
    return (dev, each) if per_case else dev


def bound(grp, output):
    """relative bound of the device comparison"""
    return max(8.0 * RECORDED_DEV["%s/%s" % (grp, output)], FLOOR)


def seed_passes(name, seed):
    try:
        check_conditions(_inputs(name, seed))
    except AssertionError:
        return False
    c = CASES[name]
    if c.kind == "coincident":
        return True
    dev = case_deviation(name, seed)
    return all(8.0 * dev[o] <= caps(c)[o] for o in OUTPUTS)


def choose_seed(name, limit=400):
    """first seed from 0 whose draw meets the input conditions and whose own fp32-vs-fp64 spread x 8 stays within the
    caps; None when there is none below `limit`"""
    for seed in range(limit):
        if seed_passes(name, seed):
            return seed
    return None


CASES = _table()


# ---- launches of many problems ------------------------------------------------------------------------------------------
PREFILL = 0x7FC0BEEF            # a quiet NaN with a payload of its own


def launch_layout(regime, seed=0, n_small=210, n_mid=50, n_large=12):
    """One launch of > 300 problems in all size classes with empty, teacher-empty, student-empty and oversize ones.
    Segments lie in shuffled order with 1..3 unowned rows (NaN inputs) between and around them, student and teacher
    rows shuffled independently.  -> dict: xs, al, yt, be (fp32), s_start, s_cnt, t_start, t_cnt (int32), valid
    (expected, int32), owned (bool per student row: row of a valid problem), blur, scaling, reach."""
    r = np.random.default_rng([seed, 77])
    sizes = list(SIZES)
    sizes += [(int(a), int(b)) for a, b in r.integers(1, LANE_MAX + 1, (n_small, 2))]
    sizes += [(int(a), int(b)) for a, b in r.integers(LANE_MAX + 1, 65, (n_mid, 2))]
    sizes += [(int(a), int(b)) for a, b in r.integers(65, CAP + 1, (n_large, 2))]
    kinds = ["plain"] * len(sizes)
    for i in range(len(SIZES), len(SIZES) + 12):
        kinds[i] = "zero" if sizes[i][0] > 1 and sizes[i][1] > 1 else "plain"
    kinds[len(SIZES) + 12] = kinds[len(SIZES) + n_small] = "coincident"
    invalid = [(0, 0)] * 6 + [(5, 0), (16, 0), (17, 0), (64, 0), (128, 0), (1, 0)] + \
              [(0, 5), (0, 16), (0, 17), (0, 64), (0, 128), (0, 1)] + \
              [(CAP + 1, 5), (5, CAP + 1), (200, 200), (CAP, CAP + 1), (CAP + 1, 0), (0, 200)]
    sizes += invalid
    kinds += ["plain"] * len(invalid)
    order = r.permutation(len(sizes))
    sizes = [sizes[i] for i in order]
    kinds = [kinds[i] for i in order]
    B = len(sizes)
    valid = np.array([0 if (n == 0 or m == 0) else (-1 if (n > CAP or m > CAP) else 1) for n, m in sizes], np.int32)

    def place(counts):
        start, pos = np.zeros(B, np.int32), int(r.integers(1, 4))
        for b in r.permutation(B):
            start[b] = pos
            pos += counts[b] + int(r.integers(1, 4))
        return start, pos

    s_cnt = np.array([n for n, _ in sizes], np.int32)
    t_cnt = np.array([m for _, m in sizes], np.int32)
    s_start, P = place(s_cnt)
    t_start, Q = place(t_cnt)
    xs, al = np.full((P, 8, 2), np.nan, f32), np.full((P, 8), np.nan, f32)
    yt, be = np.full((Q, 8, 2), np.nan, f32), np.full((Q, 8), np.nan, f32)
    owned = np.zeros(P, bool)
    for b, (n, m) in enumerate(sizes):
        x, a, y, w = draw(max(n, 1), max(m, 1), regime, 1000 + b, kinds[b])
        xs[s_start[b]:s_start[b] + n], al[s_start[b]:s_start[b] + n] = x[:n], a[:n]
        yt[t_start[b]:t_start[b] + m], be[t_start[b]:t_start[b] + m] = y[:m], w[:m]
        if valid[b] == 1:
            owned[s_start[b]:s_start[b] + n] = True
    return dict(xs=xs, al=al, yt=yt, be=be, s_start=s_start, s_cnt=s_cnt, t_start=t_start, t_cnt=t_cnt, valid=valid,
                owned=owned, sizes=sizes, scaling=0.5, **REGIMES[regime])


def layout_problem(L, b):
    """problem b of a launch layout as ot_reference arguments"""
    s, n, t, m = int(L["s_start"][b]), int(L["s_cnt"][b]), int(L["t_start"][b]), int(L["t_cnt"][b])
    return (L["xs"][s:s + n], L["al"][s:s + n], L["yt"][t:t + m], L["be"][t:t + m], L["blur"], L["scaling"], L["reach"])


@functools.lru_cache(maxsize=None)
def layout(regime):
    """launch_layout(regime), built once and shared (treat as read-only)"""
    return launch_layout(regime)


@functools.lru_cache(maxsize=None)
def launch_sample(regime, per_class=(2, 2, 1)):
    """Problems of the big launch that are compared with the oracle: per size class (lane path, one strided pass, two)
    the first ones in launch order that meet the input conditions and whose own fp32-vs-fp64 spread x 8 stays within
    CAPS.  -> [(b, ref64, {output: absolute limit})], limit = max(8 x spread, 4 ulps) of the output's scale."""
    L = layout(regime)
    out = []
    for (lo, hi), want in zip(((1, LANE_MAX), (LANE_MAX + 1, 64), (65, CAP)), per_class):
        have = 0
        for b in np.flatnonzero(L["valid"] == 1):
            if have == want:
                break
            if not lo <= max(L["sizes"][b]) <= hi:
                continue
            args = layout_problem(L, int(b))
            if diameters(args[0], args[2])[1] <= args[4] or schedule_facts(args[0], args[2], args[4], args[5])[1] < KNIFE:
                continue
            r64, r32 = ot_reference(*args), ot_reference(*args, dtype=np.float32)
            scale = {o: float(np.abs(r64[o]).max()) for o in OUTPUTS}
            spread = {o: float(np.abs(r32[o] - r64[o]).max()) for o in OUTPUTS}
            if any(8.0 * spread[o] > CAPS[o] * scale[o] for o in OUTPUTS):
                continue
            out.append((int(b), r64, {o: max(8.0 * spread[o], FLOOR * scale[o]) for o in OUTPUTS}))
            have += 1
    return out


if __name__ == "__main__":
    if "--search" in sys.argv:
        for name in CASES:
            s = choose_seed(name)
            if s != 0:
                print('    "%s": %s,' % (name, s))
        sys.exit(0)
    dev, each = measure_deviations(per_case=True)
    for name, d in each.items():
        steps, margin = check_conditions(inputs(name))
        print("%-28s seed %3d steps %3d margin %.3f  " % (name, CASES[name].seed, steps, margin) +
              "  ".join("%s %.3e" % (o, d[o]) for o in OUTPUTS))
    print("RECORDED_DEV = {")
    for k in sorted(dev):
        print('    "%s": %.3e,' % (k, dev[k]))
    print("}")
    for k in sorted(dev):
        print("| %s | %.3e | %.3e | %.3e |" % (k, dev[k], 8 * dev[k], max(8 * dev[k], FLOOR)))
