"""GPU: the small-set Sinkhorn kernel (csrc/sinkhorn.hip, kd6d_sinkhorn_div_fwd_bwd) on its own through the C ABI, at
every size class (16-lane path, one strided pass, two strided passes, kCap), every lse_row residue, schedules on both
sides of the 128-step table, per-keypoint weights, zero weights, coincident points, and one launch of > 300 problems
with shuffled segments, gaps, empty and oversize sets.  Cases, references and bounds: tests/sinkhorn_cases.py (checked
on the CPU by tests/test_sinkhorn_cases_host.py); figures: profiles/sinkhorn_small_tolerances.md.

The tests own every word the kernel may write: outputs are prefilled with a NaN pattern, segments lie between unowned
rows whose inputs are NaN, and everything outside a valid problem's rows must come back bit for bit."""
import functools

import numpy as np
import pytest
import torch

import sinkhorn_cases as C

pytestmark = pytest.mark.gpu

f32 = np.float32
VALID_FILL = 0x5A5A5A5A
ALL = list(C.CASES)
SMALL = [n for n, c in C.CASES.items() if c.N <= C.LANE_MAX and c.M <= C.LANE_MAX]
PROPERTY_CASES = ["plain_4x4_unb", "plain_4x4_bal", "zero_12x16_unb", "zero_12x16_bal", "plain_19x33_unb",
                  "plain_16x17_bal", "plain_65x64_unb", "plain_3x128_bal", "zero_39x68_unb", "sched129_12x9_unb"]


def _with_lanes(names):
    """(case, sinkhorn.lanes): every case as it runs by default; the sets of up to 16 points also with lanes = 0, on the
    general path, whose row loops and lse_row then see the counts 1..16 (larger sets take that path anyway)"""
    return [(n, 1) for n in names] + [(n, 0) for n in names if n in SMALL]


def _ops():
    from kd6d import ops
    return ops


@pytest.fixture(autouse=True)
def _restore_lanes():
    yield
    _ops().set_option("sinkhorn.lanes", 1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return bool((_bits(a) == _bits(b)).all())


def _is_prefill(a):
    return bool((_bits(a) == C.PREFILL).all())


def _filled(shape, dev, pattern=C.PREFILL, dtype=torch.float32):
    t = torch.full(shape, pattern - (1 << 32) if pattern >= 1 << 31 else pattern, dtype=torch.int32, device=dev)
    return t.view(dtype)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Launch:
    """Device copies of one set of inputs and segment tables; run() launches problems [b0, b0 + n) into prefilled
    outputs (or into the buffers handed in) and returns host copies."""

    def __init__(self, dev, xs, al, s_start, s_cnt, yt, be, t_start, t_cnt, blur, scaling, reach):
        self.dev, self.B = dev, len(s_start)
        self.xs, self.al, self.yt, self.be = (_dev(a, dev) for a in (xs, al, yt, be))
        self.tabs = [_dev(np.asarray(a, np.int32), dev) for a in (s_start, s_cnt, t_start, t_cnt)]
        self.blur, self.scaling, self.reach = blur, scaling, -1.0 if reach is None else reach

    def buffers(self, want_kp=True):
        d = self.dev
        return dict(loss=_filled((self.B,), d), valid=_filled((self.B,), d, VALID_FILL, torch.int32),
                    loss_kp=_filled((self.B, 8), d) if want_kp else None,
                    gx=_filled(tuple(self.xs.shape), d), ga=_filled(tuple(self.al.shape), d))

    def launch(self, buf, b0=0, n=None):
        ops = _ops()
        P, n = ops._ptr, self.B - b0 if n is None else n
        kp = buf["loss_kp"]
        ops.check(ops.lib.kd6d_sinkhorn_div_fwd_bwd(
            P(self.xs), P(self.al), P(self.tabs[0][b0:]), P(self.tabs[1][b0:]), P(self.yt), P(self.be),
            P(self.tabs[2][b0:]), P(self.tabs[3][b0:]), n, 2.0, self.blur, self.scaling, self.reach,
            P(buf["loss"][b0:]), P(buf["valid"][b0:]), None if kp is None else P(kp[b0:]), P(buf["gx"]), P(buf["ga"]),
            ops._stream()), "kd6d_sinkhorn_div_fwd_bwd")

    def run(self, want_kp=True):
        buf = self.buffers(want_kp)
        self.launch(buf)
        return self.fetch(buf)

    @staticmethod
    def fetch(buf):
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy()) for k, v in buf.items()}


PAD_S, PAD_T = 2, 3        # unowned NaN rows in front of and behind the single problem of a case


def _case_launch(dev, xs, al, yt, be, blur, scaling, reach):
    def pad(a, p):
        out = np.full((a.shape[0] + 2 * p,) + a.shape[1:], np.nan, f32)
        out[p:p + a.shape[0]] = a
        return out
    return Launch(dev, pad(xs, PAD_S), pad(al, PAD_S), [PAD_S], [xs.shape[0]], pad(yt, PAD_T), pad(be, PAD_T), [PAD_T],
                  [yt.shape[0]], blur, scaling, reach)


def _run_arrays(dev, xs, al, yt, be, blur, scaling, reach, lanes=1):
    """one problem alone -> dict(loss_kp (8), loss_img (), gx (N,8,2), ga (N,8)); checks everything but the numbers"""
    _ops().set_option("sinkhorn.lanes", lanes)
    out = _case_launch(dev, xs, al, yt, be, blur, scaling, reach).run()
    N = xs.shape[0]
    assert out["valid"].tolist() == [1]
    own = slice(PAD_S, PAD_S + N)
    for k in ("gx", "ga"):
        assert _is_prefill(out[k][:PAD_S]) and _is_prefill(out[k][PAD_S + N:]), "wrote outside its segment"
        assert np.isfinite(out[k][own]).all()
    assert np.isfinite(out["loss"]).all() and np.isfinite(out["loss_kp"]).all()
    # loss_img is the sum of the eight per-keypoint values in wave order, in fp32
    tot = f32(0)
    for k in range(8):
        tot = f32(tot + out["loss_kp"][0, k])
    assert _same(out["loss"], np.array([tot], f32)), (out["loss"], tot)
    return dict(loss_kp=out["loss_kp"][0], loss_img=out["loss"][0], gx=out["gx"][own], ga=out["ga"][own])


@functools.lru_cache(maxsize=None)
def _run_case(dev, name, lanes):
    i = C.inputs(name)
    return _run_arrays(dev, i["xs"], i["al"], i["yt"], i["be"], i["blur"], i["scaling"], i["reach"], lanes)


def _report(name, out, err, limit):
    print("sinkhorn-tolerance %-28s %-8s max error / bound = %.4f" % (name, out, err / limit if limit > 0 else np.inf))


def _close(name, got, ref, grp, absolute=False, outputs=C.OUTPUTS):
    """max|got - ref| <= bound * max|ref| per output (absolute: the bound itself); every figure printed first"""
    bad = []
    for o in outputs:
        limit = C.bound(grp, o) * (1.0 if absolute else float(np.abs(ref[o]).max()))
        err = float(np.abs(got[o].astype(np.float64) - ref[o]).max())
        _report(name, o, err, limit)
        if not err <= limit:
            bad.append((o, err, limit))
    assert not bad, (name, bad)


# ---- numeric comparison with the fp64 oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,lanes", _with_lanes(ALL))
def test_case_vs_oracle(gpu_device, name, lanes):
    """Every case alone against oracle.sinkhorn_ref in float64, bound = 8 x the restatement's own fp32 spread
    (sinkhorn_cases.bound)."""
    c = C.CASES[name]
    C.check_conditions(C.inputs(name))
    got, ref = _run_case(gpu_device, name, lanes), C.reference(name)
    if c.kind == "coincident":
        assert np.abs(got["gx"]).max() == 0.0            # exactly: every difference r - c_j is 0
        _close(name, got, ref, c.regime, absolute=True, outputs=("loss_kp", "loss_img", "ga"))
    else:
        _close(name, got, ref, C.group(c))


# ---- exact properties ------------------------------------------------------------------------------------------------------
LANES_BITWISE = True       # property 4 as the kernel comment states it; see profiles/sinkhorn_small_tolerances.md


@pytest.mark.parametrize("name", SMALL)
def test_lane_path_equals_general_path(gpu_device, name):
    """N, M <= 16: the four-softmins-side-by-side path and the general path give bitwise the same gradients (same
    lse_row, same column order, same update formulas); the loss sums its terms in another order."""
    c = C.CASES[name]
    a, b, ref = _run_case(gpu_device, name, 1), _run_case(gpu_device, name, 0), C.reference(name)
    if LANES_BITWISE:
        assert _same(a["gx"], b["gx"]) and _same(a["ga"], b["ga"])
    for o in ("loss_kp", "loss_img"):
        scale = 1.0 if c.kind == "coincident" else float(np.abs(ref[o]).max())
        assert np.abs(a[o].astype(np.float64) - b[o]).max() <= C.bound(C.group(c), o) * scale


@pytest.mark.parametrize("name,lanes", _with_lanes(PROPERTY_CASES))
def test_keypoint_permutation(gpu_device, name, lanes):
    """Permuting the 8-axis of all four inputs permutes gx, ga and loss_kp bitwise: each wave does the same arithmetic
    on its keypoint and the joint diameter is order-free.  A kernel that mixed keypoints (weights read without + k)
    cannot pass with weights drawn per (cell, keypoint)."""
    i, c = C.inputs(name), C.CASES[name]
    base = _run_case(gpu_device, name, lanes)
    perm = np.random.default_rng(11).permutation(8)
    assert (perm != np.arange(8)).sum() >= 6
    got = _run_arrays(gpu_device, i["xs"][:, perm], i["al"][:, perm], i["yt"][:, perm], i["be"][:, perm], i["blur"],
                      i["scaling"], i["reach"], lanes)
    assert _same(got["gx"], base["gx"][:, perm]) and _same(got["ga"], base["ga"][:, perm])
    assert _same(got["loss_kp"], base["loss_kp"][perm])
    ref = C.reference(name)["loss_img"]
    assert abs(float(got["loss_img"]) - float(base["loss_img"])) <= C.bound(C.group(c), "loss_img") * abs(ref)


@pytest.mark.parametrize("name,lanes", _with_lanes(PROPERTY_CASES))
def test_symmetry_and_identity(gpu_device, name, lanes):
    """S(alpha, x; beta, y) = S(beta, y; alpha, x) within the loss bound: the only check on the b_y / a_y rows, which
    feed nothing but the loss.  S(alpha, x; alpha, x) = 0 with a zero gradient, within 8 x what the fp32 restatement
    leaves of that same case (floor: 4 ulps of the x-vs-y case's own values, which the vanishing terms are
    differences of)."""
    i, c, ref = C.inputs(name), C.CASES[name], C.reference(name)
    grp = C.group(c)
    base = _run_case(gpu_device, name, lanes)
    swapped = _run_arrays(gpu_device, i["yt"], i["be"], i["xs"], i["al"], i["blur"], i["scaling"], i["reach"], lanes)
    limit = C.bound(grp, "loss_kp") * float(np.abs(ref["loss_kp"]).max())
    err = float(np.abs(swapped["loss_kp"].astype(np.float64) - base["loss_kp"]).max())
    _report(name, "swap", err, limit)
    assert err <= limit
    _close(name + " swapped", swapped, ref, grp, outputs=("loss_kp", "loss_img"))
    same = _run_arrays(gpu_device, i["xs"], i["al"], i["xs"], i["al"], i["blur"], i["scaling"], i["reach"], lanes)
    r32 = C.ot_reference(i["xs"], i["al"], i["xs"], i["al"], i["blur"], i["scaling"], i["reach"], dtype=np.float32)
    for o in ("loss_kp", "loss_img", "gx"):
        limit = max(8.0 * float(np.abs(r32[o]).max()), C.FLOOR * float(np.abs(ref[o]).max()))
        err = float(np.abs(same[o]).max())
        _report(name, "same " + o, err, limit)
        assert err <= limit, (o, err, limit)


# ---- one launch of > 300 problems ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big(dev, regime):
    L = C.layout(regime)
    la = Launch(dev, L["xs"], L["al"], L["s_start"], L["s_cnt"], L["yt"], L["be"], L["t_start"], L["t_cnt"], L["blur"],
                L["scaling"], L["reach"])
    _ops().set_option("sinkhorn.lanes", 1)
    return L, la, la.run()


@pytest.mark.parametrize("regime", list(C.REGIMES))
def test_launch_footprint(gpu_device, regime):
    """valid is exactly 1 / 0 / -1; loss_img and the eight loss_kp of empty and oversize problems are exactly 0; gap
    rows and the rows of empty and oversize problems keep the prefill; a launch without loss_kp and a second launch
    give the same bits; ops.sinkhorn_div returns zeros where the kernel writes nothing."""
    L, la, out = _big(gpu_device, regime)
    assert la.B >= 300
    assert out["valid"].tolist() == L["valid"].tolist()
    bad = L["valid"] != 1
    assert (_bits(out["loss"][bad]) == 0).all() and (_bits(out["loss_kp"][bad]) == 0).all()
    own = L["owned"]
    for k in ("gx", "ga"):
        assert _is_prefill(out[k][~own]), "a row outside every valid problem was written"
        assert np.isfinite(out[k][own]).all()
    assert np.isfinite(out["loss"]).all() and np.isfinite(out["loss_kp"]).all()
    tot = np.zeros(la.B, f32)
    for k in range(8):
        tot = (tot + out["loss_kp"][:, k]).astype(f32)
    assert _same(tot, out["loss"])
    again, nokp = la.run(), la.run(want_kp=False)
    for k in ("loss", "valid", "gx", "ga"):
        assert _same(again[k], out[k]) and _same(nokp[k], out[k]), k
    assert _same(again["loss_kp"], out["loss_kp"]) and nokp["loss_kp"] is None
    loss, valid, gx, ga = _ops().sinkhorn_div(la.xs, la.al, *la.tabs[:2], la.yt, la.be, *la.tabs[2:], la.B, 2.0, L["blur"],
                                              L["scaling"], L["reach"])
    torch.cuda.synchronize()
    gx, ga = gx.cpu().numpy(), ga.cpu().numpy()
    assert (_bits(gx[~own]) == 0).all() and (_bits(ga[~own]) == 0).all()
    assert _same(gx[own], out["gx"][own]) and _same(ga[own], out["ga"][own])
    assert _same(loss.cpu().numpy(), out["loss"]) and valid.cpu().tolist() == L["valid"].tolist()


@pytest.mark.parametrize("regime", list(C.REGIMES))
def test_launch_isolation(gpu_device, regime):
    """Every problem of the big launch run alone (n_images = 1, same rows, same tables) gives bitwise the same
    loss_img, loss_kp, valid, gx and ga: a result depends on nothing but the problem's own segment."""
    L, la, out = _big(gpu_device, regime)
    buf = la.buffers()
    for b in range(la.B):
        la.launch(buf, b0=b, n=1)
    alone = la.fetch(buf)
    for k in ("valid", "loss", "loss_kp", "gx", "ga"):
        diff = _bits(alone[k]) != _bits(out[k])
        assert not diff.any(), (k, np.argwhere(diff)[:4].tolist())


@pytest.mark.parametrize("regime", list(C.REGIMES))
def test_launch_problems_vs_oracle(gpu_device, regime):
    """A sample of the big launch against the oracle (sinkhorn_cases.launch_sample: problems of every size class, chosen
    by the restatement alone), so that a wrong segment offset cannot hide behind the isolation test's agreement of the
    kernel with itself.  These draws are not in the case table: the bound is 8 x their own fp32 spread."""
    L, la, out = _big(gpu_device, regime)
    sample = C.launch_sample(regime)
    assert len(sample) == 5
    for b, ref, limit in sample:
        s, n = int(L["s_start"][b]), int(L["s_cnt"][b])
        got = dict(loss_kp=out["loss_kp"][b], loss_img=out["loss"][b], gx=out["gx"][s:s + n], ga=out["ga"][s:s + n])
        for o in C.OUTPUTS:
            err = float(np.abs(got[o].astype(np.float64) - ref[o]).max())
            _report("launch[%d] %dx%d" % (b, *L["sizes"][b]), o, err, limit[o])
            assert err <= limit[o], (b, o, err, limit[o])
