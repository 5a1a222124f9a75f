"""GPU: the kernel distances (csrc/kernel_loss.hip; --gtype gaussian | laplacian | energy under --kd_kernel_losses) --
the two kernels, SamplesLoss, KDLoss, a whole training step and the training entry -- against the fp64 torch reference of
tests/kernel_loss_cases.py.  Bounds: kernel_loss_cases.bound (profiles/kernel_loss_tolerances.md), relative to the
largest magnitude of the reference output; every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kd_object_cases as K
import kernel_loss_cases as C
import loss_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_I = -7
KD_BLUR = 0.05


def _kd():
    from kd6d import _lib, kd_losses, ops
    return _lib, ops, kd_losses


def _launch_small(dev, L, kind, blur, only=None):
    """kd6d_kernel_div_fwd_bwd on the launch L (kernel_loss_cases.small_launch) with canaries in every output; only:
    launch this one problem alone.  -> CPU tensors."""
    _lib, ops, _ = _kd()
    P = len(L["sizes"]) if only is None else 1
    sel = slice(None) if only is None else slice(only, only + 1)
    f32 = dict(dtype=torch.float32, device=dev)
    ins = {k: L[k].to(dev) for k in ("xs", "alpha", "yt", "beta")}
    seg = {k: L[k][sel].contiguous().to(dev) for k in ("s_start", "s_cnt", "t_start", "t_cnt")}
    loss_img, loss_kp = torch.full((P,), C.CANARY, **f32), torch.full((P, 8), C.CANARY, **f32)
    valid = torch.full((P,), SENT_I, dtype=torch.int32, device=dev)
    gx, ga = torch.full(tuple(L["xs"].shape), C.CANARY, **f32), torch.full(tuple(L["alpha"].shape), C.CANARY, **f32)
    p = ops._ptr
    _lib.check(_lib.lib.kd6d_kernel_div_fwd_bwd(_lib.KERNEL_KINDS[kind], p(ins["xs"]), p(ins["alpha"]), p(seg["s_start"]),
                                                p(seg["s_cnt"]), p(ins["yt"]), p(ins["beta"]), p(seg["t_start"]),
                                                p(seg["t_cnt"]), P, blur, p(loss_img), p(valid), p(loss_kp), p(gx), p(ga),
                                                ops._stream()), "kd6d_kernel_div_fwd_bwd")
    torch.cuda.synchronize()
    for k in ("xs", "alpha", "yt", "beta"):
        assert torch.equal(ins[k].cpu(), L[k]), "the launch wrote into its input " + k
    return dict(loss_img=loss_img.cpu(), loss_kp=loss_kp.cpu(), valid=valid.cpu(), grad_x=gx.cpu(), grad_alpha=ga.cpu())


def _fp32_sum_in_order(v):
    tot = np.float32(0.0)
    for x in v.numpy().astype(np.float32):
        tot = np.float32(tot + x)
    return float(tot)


# ---- 1. the small kernel against fp64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("blur", C.BLURS)
@pytest.mark.parametrize("size", C.SMALL_SIZES, ids=["%dx%d" % s for s in C.SMALL_SIZES])
@pytest.mark.parametrize("kind", C.KINDS)
def test_small_kernel_vs_fp64(gpu_device, kind, size, blur):
    """Six problems of one size in one launch, segments shuffled with gaps: loss_kp, loss_img, grad_xs, grad_alpha within
    their bounds; loss_img = the fp32 sum of its loss_kp in keypoint order; gaps untouched; a zero weight gives a
    finite grad_alpha and a zero grad_xs."""
    N, M = size
    L = C.small_case(N, M)
    ref = C.small_reference(N, M, kind, blur)
    got = _launch_small(gpu_device, L, kind, blur)
    what = "%dx%d blur %g" % (N, M, blur)
    assert got["valid"].tolist() == [1] * C.N_PROBLEMS
    w = ref["written"]
    assert bool((got["grad_x"][~w] == C.CANARY).all()) and bool((got["grad_alpha"][~w] == C.CANARY).all()), "canaries in the gaps"
    C.assert_within(got["loss_kp"], ref["loss"], kind, "loss", what + " loss_kp")
    C.assert_within(got["loss_img"], ref["loss"].sum(1), kind, "loss", what + " loss_img")
    gx, ga = got["grad_x"].clone(), got["grad_alpha"].clone()
    gx[~w], ga[~w] = 0, 0
    C.assert_within(ga, ref["grad_alpha"], kind, "grad_alpha", what)
    C.assert_within(gx, ref["grad_x"], kind, "grad_x", what)
    assert float(ref["grad_x"].abs().max()) > 1e-3, "the near pair keeps the largest gradient an ordinary number"
    for p in range(C.N_PROBLEMS):
        assert float(got["loss_img"][p]) == _fp32_sum_in_order(got["loss_kp"][p]), "loss_img is the ordered fp32 sum"
    if N >= 4:                                          # problem 0, row 2: weight 0 on every keypoint
        r = int(L["s_start"][0]) + 2
        assert bool((L["alpha"][r] == 0).all())
        assert bool((got["grad_x"][r] == 0).all()) and bool(torch.isfinite(got["grad_alpha"][r]).all())
        assert float(ref["grad_alpha"][r].abs().min()) > 0


# ---- 2. edge cases ------------------------------------------------------------------------------------------------------
EDGE_SIZES = [(0, 5), (5, 0), (129, 4), (7, 6), (4, 129), (0, 0)]


@pytest.mark.parametrize("kind", C.KINDS)
def test_small_kernel_edge_cases(gpu_device, kind):
    """Empty sets: valid 0, loss 0, gradient rows unwritten; more than 128 points: valid -1; the ordinary problem between
    them is unaffected; n_images = 0 launches nothing."""
    _lib, ops, _ = _kd()
    L = C.small_launch(EDGE_SIZES, 0)
    got = _launch_small(gpu_device, L, kind, 0.05)
    assert got["valid"].tolist() == [0, 0, -1, 1, -1, 0]
    ref = C.small_results(L, lambda a, x, b, y: C.reference(a, x, b, y, kind, 0.05))
    w = ref["written"]
    assert int(w.sum()) == 7
    assert bool((got["grad_x"][~w] == C.CANARY).all()) and bool((got["grad_alpha"][~w] == C.CANARY).all())
    for p in (0, 1, 2, 4, 5):
        assert float(got["loss_img"][p]) == 0.0 and bool((got["loss_kp"][p] == 0).all())
    C.assert_within(got["loss_kp"][3], ref["loss"][3], kind, "loss", "edge launch, the 7x6 problem")
    C.assert_within(got["grad_x"][w], ref["grad_x"][w], kind, "grad_x", "edge launch")
    C.assert_within(got["grad_alpha"][w], ref["grad_alpha"][w], kind, "grad_alpha", "edge launch")
    # n_images = 0
    dev = gpu_device
    buf = torch.full((16,), C.CANARY, dtype=torch.float32, device=dev)
    ib = torch.full((4,), SENT_I, dtype=torch.int32, device=dev)
    p = ops._ptr
    _lib.check(_lib.lib.kd6d_kernel_div_fwd_bwd(_lib.KERNEL_KINDS[kind], p(buf), p(buf), p(ib), p(ib), p(buf), p(buf), p(ib),
                                                p(ib), 0, 0.05, p(buf), p(ib), p(buf), p(buf), p(buf), ops._stream()),
               "kd6d_kernel_div_fwd_bwd")
    torch.cuda.synchronize()
    assert bool((buf.cpu() == C.CANARY).all()) and bool((ib.cpu() == SENT_I).all())
    # ops.kernel_div zeroes the gradient arrays like ops.sinkhorn_div
    d = {k: L[k].to(dev) for k in ("xs", "alpha", "s_start", "s_cnt", "yt", "beta", "t_start", "t_cnt")}
    loss, valid, gx, ga = ops.kernel_div(kind, d["xs"], d["alpha"], d["s_start"], d["s_cnt"], d["yt"], d["beta"], d["t_start"],
                                         d["t_cnt"], len(EDGE_SIZES), 0.05)
    torch.cuda.synchronize()
    assert valid.cpu().tolist() == got["valid"].tolist() and torch.equal(loss.cpu(), got["loss_img"])
    assert bool((gx.cpu()[~w] == 0).all()) and torch.equal(gx.cpu()[w], got["grad_x"][w]) and torch.equal(ga.cpu()[w], got["grad_alpha"][w])


# ---- 2b. one contract for both launch families ----------------------------------------------------------------------------
# (N, M): student-empty, teacher-empty, student / teacher one point over the cap, the smallest problem that runs, the
# largest the kernels accept (csrc/pointset_small.h)
CONTRACT_SIZES = [(0, 3), (3, 0), (129, 3), (3, 129), (1, 1), (128, 128)]
CONTRACT_VALID = [0, 0, -1, -1, 1, 1]
CONTRACT_SEED = 3                      # the first seed for which small_launch's clamp condition holds on these sizes
CONTRACT_SINKHORN = {4: "plain_1x1_unb", 5: "plain_128x128_unb"}      # the sinkhorn_cases cases of the two valid problems
FAMILIES = [("sinkhorn", 0), ("sinkhorn", 1)] + [(k, None) for k in C.KINDS]


def _contract_sinkhorn():
    """The launch of CONTRACT_SIZES from sinkhorn_cases' builders: problems 4 and 5 are its cases plain_1x1_unb and
    plain_128x128_unb, the skipped ones plain draws; one CANARY row between and around the segments.  -> the arrays of
    kernel_loss_cases.small_launch, the OT settings, and the cases' fp64 references."""
    import sinkhorn_cases as S
    parts, ot = [], None
    for p, (N, M) in enumerate(CONTRACT_SIZES):
        if p in CONTRACT_SINKHORN:
            i = S.inputs(CONTRACT_SINKHORN[p])
            assert (i["case"].N, i["case"].M) == (N, M)
            settings = dict(blur=i["blur"], scaling=i["scaling"], reach=i["reach"])
            assert ot in (None, settings), "the two cases share one launch: they must share its OT settings"
            ot = settings
            parts.append((i["xs"], i["al"], i["yt"], i["be"]))
        else:
            x, a, y, b = S.draw(max(N, 1), max(M, 1), "unb", 1000 + p)
            parts.append((x[:N], a[:N], y[:M], b[:M]))

    def lay(pts, wts):
        start, row = [], 1
        for q in pts:
            start.append(row)
            row += q.shape[0] + 1
        P_, W_ = torch.full((row, 8, 2), C.CANARY), torch.full((row, 8), C.CANARY)
        for s, q, w in zip(start, pts, wts):
            P_[s:s + q.shape[0]], W_[s:s + q.shape[0]] = torch.from_numpy(q.copy()), torch.from_numpy(w.copy())
        return P_, W_, torch.tensor(start, dtype=torch.int32), torch.tensor([q.shape[0] for q in pts], dtype=torch.int32)

    xs, alpha, s_start, s_cnt = lay([q[0] for q in parts], [q[1] for q in parts])
    yt, beta, t_start, t_cnt = lay([q[2] for q in parts], [q[3] for q in parts])
    return (dict(xs=xs, alpha=alpha, s_start=s_start, s_cnt=s_cnt, yt=yt, beta=beta, t_start=t_start, t_cnt=t_cnt), ot,
            {p: S.reference(n) for p, n in CONTRACT_SINKHORN.items()})


@pytest.mark.parametrize("family,lanes", FAMILIES, ids=["%s%s" % (f, "" if l is None else "-lanes%d" % l) for f, l in FAMILIES])
def test_both_launch_families_honour_one_contract(gpu_device, family, lanes):
    """ops.sinkhorn_div (16-lane path on and off) and ops.kernel_div on one launch of an empty student set, an empty
    teacher set, 129 points on either side, 1x1 and 128x128: valid = 0 / -1 / 1; loss_img and the loss_kp row of a skipped
    problem exactly 0, its gradient rows (and the gaps) as the caller left them; loss_img of a valid problem = its
    loss_kp row added in index order, bit for bit; the valid problems' values within the bounds of their case files."""
    import sinkhorn_cases as S
    _, ops, _ = _kd()
    dev = gpu_device
    if family == "sinkhorn":
        L, ot, refs = _contract_sinkhorn()
    else:
        L = C.small_launch(CONTRACT_SIZES, CONTRACT_SEED)
        ref = C.small_results(L, lambda a, x, b, y: C.reference(a, x, b, y, family, KD_BLUR))
    P = len(CONTRACT_SIZES)
    f32 = dict(dtype=torch.float32, device=dev)
    d = {k: L[k].to(dev) for k in ("xs", "alpha", "s_start", "s_cnt", "yt", "beta", "t_start", "t_cnt")}
    out = (torch.full((P,), C.CANARY, **f32), torch.full((P,), SENT_I, dtype=torch.int32, device=dev),
           torch.full(tuple(L["xs"].shape), C.CANARY, **f32), torch.full(tuple(L["alpha"].shape), C.CANARY, **f32))
    loss_kp = torch.full((P, 8), C.CANARY, **f32)
    sets = (d["xs"], d["alpha"], d["s_start"], d["s_cnt"], d["yt"], d["beta"], d["t_start"], d["t_cnt"], P)
    if family == "sinkhorn":
        ops.set_option("sinkhorn.lanes", lanes)
        try:
            got = ops.sinkhorn_div(*sets, 2.0, ot["blur"], ot["scaling"], ot["reach"], loss_kp=loss_kp, out=out)
        finally:
            ops.set_option("sinkhorn.lanes", 1)
    else:
        got = ops.kernel_div(family, *sets, KD_BLUR, loss_kp=loss_kp, out=out)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out)), "out= buffers are returned as they are"
    loss_img, valid, gx, ga = (t.cpu() for t in out)
    loss_kp = loss_kp.cpu()
    assert valid.tolist() == CONTRACT_VALID
    written = torch.zeros(L["xs"].shape[0], dtype=torch.bool)
    for p, (N, M) in enumerate(CONTRACT_SIZES):
        s0 = int(L["s_start"][p])
        if CONTRACT_VALID[p] != 1:
            assert float(loss_img[p]) == 0.0 and bool((loss_kp[p] == 0).all()), "problem %d: loss of a skipped problem" % p
            continue
        written[s0:s0 + N] = True
        assert float(loss_img[p]) == _fp32_sum_in_order(loss_kp[p]), "problem %d: loss_img is the ordered fp32 sum" % p
        what = "contract %dx%d" % (N, M)
        if family == "sinkhorn":
            mine = dict(loss_kp=loss_kp[p], loss_img=loss_img[p], gx=gx[s0:s0 + N], ga=ga[s0:s0 + N])
            for o in S.OUTPUTS:
                limit = S.bound(S.group(S.CASES[CONTRACT_SINKHORN[p]]), o) * float(np.abs(refs[p][o]).max())
                err = float(np.abs(mine[o].double().numpy() - refs[p][o]).max())
                print("  sinkhorn lanes %d %-8s %-16s max|err| %.3e  limit %.3e" % (lanes, o, what, err, limit))
                assert err <= limit, (p, o, err, limit)
        else:
            C.assert_within(loss_kp[p], ref["loss"][p], family, "loss", what + " loss_kp")
            C.assert_within(ga[s0:s0 + N], ref["grad_alpha"][s0:s0 + N], family, "grad_alpha", what)
            C.assert_within(gx[s0:s0 + N], ref["grad_x"][s0:s0 + N], family, "grad_x", what)
    assert int(written.sum()) == 129
    assert bool((gx[~written] == C.CANARY).all()) and bool((ga[~written] == C.CANARY).all()), "a skipped row was written"


# ---- 3. independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.KINDS)
def test_small_kernel_problems_are_independent(gpu_device, kind):
    """Two launches agree bitwise; a problem launched alone equals itself inside the batch, bitwise; permuting the
    keypoint axis of all inputs permutes the outputs, bitwise."""
    N, M = 65, 17
    L = C.small_case(N, M)
    dev = gpu_device
    a, b = _launch_small(dev, L, kind, 0.05), _launch_small(dev, L, kind, 0.05)
    for k in a:
        assert torch.equal(a[k], b[k]), "two launches differ in " + k
    for p in (0, 4):
        one = _launch_small(dev, L, kind, 0.05, only=p)
        s0 = int(L["s_start"][p])
        assert torch.equal(one["loss_kp"][0], a["loss_kp"][p]) and float(one["loss_img"][0]) == float(a["loss_img"][p])
        assert torch.equal(one["grad_x"][s0:s0 + N], a["grad_x"][s0:s0 + N])
        assert torch.equal(one["grad_alpha"][s0:s0 + N], a["grad_alpha"][s0:s0 + N])
        rest = torch.ones(L["xs"].shape[0], dtype=torch.bool)
        rest[s0:s0 + N] = False
        assert bool((one["grad_x"][rest] == C.CANARY).all()), "a problem writes its own rows only"
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    Lp = dict(L, xs=L["xs"][:, perm].contiguous(), alpha=L["alpha"][:, perm].contiguous(), yt=L["yt"][:, perm].contiguous(),
              beta=L["beta"][:, perm].contiguous())
    c = _launch_small(dev, Lp, kind, 0.05)
    assert torch.equal(c["loss_kp"], a["loss_kp"][:, perm])
    assert torch.equal(c["grad_x"], a["grad_x"][:, perm]) and torch.equal(c["grad_alpha"], a["grad_alpha"][:, perm])


# ---- 4. the dense kernel against fp64 -----------------------------------------------------------------------------------
def _dense(dev, kind, case, blur=C.DENSE_BLUR):
    _, ops, _ = _kd()
    a, x, b, y = (t.to(dev) for t in case)
    loss, gx, ga = ops.kernel_dense(kind, x, a, y, b, blur)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), grad_x=gx.cpu(), grad_alpha=ga.cpu())


@pytest.mark.parametrize("size", C.DENSE_SIZES, ids=["%dx%d" % s for s in C.DENSE_SIZES])
@pytest.mark.parametrize("D", C.DENSE_DIMS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_dense_kernel_vs_fp64(gpu_device, kind, D, size):
    """One point, a column tile minus / plus one, more than two tiles against a short set, several row blocks, a row
    block plus one: value and gradients within their bounds; two launches agree bitwise."""
    _lib, _, _ = _kd()
    assert (C.TILE, C.ROWS) == (128, 64) and int(_lib.lib.kd6d_kernel_dense_workspace_floats(C.ROWS + 1, 3, D)) == 3
    N, M = size
    case = C.dense_case(N, M, D)
    ref = C.dense_reference(N, M, D, kind)
    got, again = _dense(gpu_device, kind, case), _dense(gpu_device, kind, case)
    what = "D=%d %dx%d" % (D, N, M)
    for o in C.OUTPUTS:
        C.assert_within(got[o], ref[o], kind, o, what)
        assert torch.equal(got[o], again[o]), "two launches differ in " + o


@pytest.mark.parametrize("kind", C.KINDS)
def test_dense_kernel_agrees_with_the_small_kernel(gpu_device, kind):
    """D = 2, 100 x 90: both kernels within the bounds of the fp64 reference, and of each other (not bitwise: other
    summation orders)."""
    _, ops, _ = _kd()
    dev = gpu_device
    N, M = C.CROSS_SIZE
    a, x, b, y = C.dense_case(N, M, 2)
    ref = C.dense_reference(N, M, 2, kind)
    got = _dense(dev, kind, (a, x, b, y))
    i32 = dict(dtype=torch.int32, device=dev)
    xs, al = x[:, None, :].expand(N, 8, 2).contiguous().to(dev), a[:, None].expand(N, 8).contiguous().to(dev)
    yt, be = y[:, None, :].expand(M, 8, 2).contiguous().to(dev), b[:, None].expand(M, 8).contiguous().to(dev)
    zero = torch.zeros(1, **i32)
    loss_kp = torch.empty(1, 8, dtype=torch.float32, device=dev)
    _, valid, gx, ga = ops.kernel_div(kind, xs, al, zero, torch.full((1,), N, **i32), yt, be, zero, torch.full((1,), M, **i32), 1,
                                      C.DENSE_BLUR, loss_kp=loss_kp)
    torch.cuda.synchronize()
    assert int(valid) == 1
    small = dict(loss=loss_kp.cpu()[0, 3:4], grad_x=gx.cpu()[:, 3], grad_alpha=ga.cpu()[:, 3])
    assert bool((loss_kp.cpu()[0] == loss_kp.cpu()[0, 0]).all()), "eight copies of one problem: eight equal results"
    for o in C.OUTPUTS:
        C.assert_within(got[o], ref[o], kind, o, "dense 100x90")
        C.assert_within(small[o], ref[o], kind, o, "small 100x90")
        m = float(ref[o].abs().max())
        assert float((got[o].double() - small[o].double()).abs().max()) <= 2 * C.bound(kind, o) * m


# ---- 5. SamplesLoss -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.SAMPLES_SHAPES, ids=["%dx%dx%dx%d" % s for s in C.SAMPLES_SHAPES])
@pytest.mark.parametrize("kind", C.KINDS)
def test_samples_loss_values_and_autograd(gpu_device, kind, shape):
    """SamplesLoss(kind, blur=0.05, kernel_losses=True)(alpha, x, beta, y) -> (B,) and its autograd gradients into alpha
    and x; the (x, y) form uses uniform weights; a y that requires grad is refused."""
    from kd6d.losses import SamplesLoss
    dev = gpu_device
    B, N, M, D = shape
    a, x, b, y = C.samples_case(*shape)
    w = torch.linspace(0.5, 1.5, B, dtype=C.F64)
    ref = C.reference(a, x, b, y, kind, 0.05)
    ag, xg = a.to(dev).requires_grad_(True), x.to(dev).requires_grad_(True)
    L = SamplesLoss(kind, p=2, blur=0.05, scaling=0.5, reach=0.5, kernel_losses=True)
    got = L(ag, xg, b.to(dev), y.to(dev))
    assert got.shape == (B,)
    (got * w.to(dev).float()).sum().backward()
    what = "SamplesLoss %s" % (shape,)
    C.assert_within(got.detach(), ref["loss"], kind, "loss", what)
    # d sum_b w_b L_b: the bound of each row's gradient, scaled by its weight (w <= 1.5)
    for o, g in (("grad_alpha", ag.grad), ("grad_x", xg.grad)):
        want = ref[o] * w.view(-1, *([1] * (ref[o].dim() - 1)))
        err, m = float((g.cpu().double() - want).abs().max()), float(ref[o].abs().max())
        print("  %-9s %-10s %-36s max|err| %.3e  max|ref| %.3e  bound %.3e" % (kind, o, what, err, m, C.bound(kind, o)))
        assert err <= 1.5 * C.bound(kind, o) * m
    got_u = L(x.to(dev), y.to(dev))
    ref_u = C.reference(torch.full((B, N), 1.0 / N), x, torch.full((B, M), 1.0 / M), y, kind, 0.05)
    C.assert_within(got_u, ref_u["loss"], kind, "loss", what + " uniform")
    one = L(a[0].to(dev), x[0].to(dev), b[0].to(dev), y[0].to(dev))
    assert one.dim() == 0 and float(one.detach()) == float(got[0].detach()), "the unbatched form is row 0"
    with pytest.raises(NotImplementedError):
        L(ag, xg, b.to(dev), y.to(dev).requires_grad_(True))


@pytest.mark.parametrize("kind", C.KINDS)
def test_kd_loss_2d_packs_the_images_into_one_kernel_launch(gpu_device, kind):
    """kd6d.losses.kd_loss_2d with a kernel SamplesLoss: all images in one kd6d_kernel_div_fwd_bwd launch -- per-image sums
    over the eight keypoints and autograd gradients vs the fp64 reference; an image with an empty set is left out."""
    from kd6d.losses import SamplesLoss, kd_loss_2d
    dev = gpu_device
    sizes = [(7, 6), (0, 5), (16, 17)]
    L = C.small_launch(sizes, 0)
    x = torch.cat(L["x"]).to(dev).requires_grad_(True)              # (P,8,2), already in frame units
    a = torch.cat(L["a"]).to(dev).requires_grad_(True)
    y, b = torch.cat(L["y"]).to(dev), torch.cat(L["b"]).to(dev)
    crit = SamplesLoss(kind, blur=0.05, kernel_losses=True)
    out = kd_loss_2d(x.reshape(-1, 2), y.reshape(-1, 2), a, b, 640, 480, "point", crit, 2, [n for n, _ in sizes],
                     [m for _, m in sizes], normalize=False)
    assert len(out) == 2
    (out[0] + 2.0 * out[1]).backward()
    s0 = 0
    for p, (N, M) in enumerate(sizes):
        if N and M:
            r = C.reference(L["a"][p].t(), L["x"][p].permute(1, 0, 2), L["b"][p].t(), L["y"][p].permute(1, 0, 2), kind, 0.05)
            i, w = (0, 1.0) if p == 0 else (1, 2.0)
            what = "kd_loss_2d image %d" % p
            C.assert_within(out[i].detach().view(1), r["loss"].sum().view(1), kind, "loss", what)
            C.assert_within(a.grad[s0:s0 + N] / w, r["grad_alpha"].t(), kind, "grad_alpha", what)
            C.assert_within(x.grad[s0:s0 + N] / w, r["grad_x"].permute(1, 0, 2), kind, "grad_x", what)
        s0 += N


# ---- 6. KDLoss ------------------------------------------------------------------------------------------------------------
STUDENT, TEACHER = "full_640x480_l5_general_lam05", "full_640x480_l5_general"       # same frame, levels and batch


def _kd_cfg(kind, per_object=False, detach=False):
    return dict(GTYPE=kind, KERNEL_LOSSES=True, GLEVEL="point", GnD=2, GP=2.0, GBLUR=KD_BLUR, SCALING=0.5, REACH=0.5,
                WEIGHTED_OT=True, DETACH=detach, PER_OBJECT=per_object)


def _slot_arrays(c, dev):
    B, cap = len(c["targets"]), c["cap"]
    cnt = torch.tensor([len(p) for p in c["pos"]], dtype=torch.int32)
    row = torch.zeros(B, cap, dtype=torch.int32)
    gt = torch.zeros(B, cap, dtype=torch.int32)
    for b, p in enumerate(c["pos"]):
        for s, (r, g) in enumerate(p):
            row[b, s], gt[b, s] = r, g
    return cnt.to(dev), row.view(-1).to(dev), gt.view(-1).to(dev)


def _run_loss(c, dev, kind, per_object, tk, tgt, detach=False):
    """KDLoss forward + backward on the case's (row, instance) list (the assignment is not under test here)."""
    _, _, kl = _kd()
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    B, cap = len(c["targets"]), c["cap"]
    ev = kl.KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=_kd_cfg(kind, per_object, detach), cap=cap)
    nf, ni = ev._ws_sizes(B)
    wf = torch.zeros(nf, dtype=torch.float32, device=dev)
    wi = torch.zeros(ni, dtype=torch.int32, device=dev)
    cnt, row, gt = _slot_arrays(c, dev)
    n, bp = B * cap, (B + 3) // 4 * 4
    wi[0:B].copy_(cnt)
    wi[3 * bp + 4:3 * bp + 4 + n].copy_(row)
    wi[3 * bp + 4 + n:3 * bp + 4 + 2 * n].copy_(gt)
    rows = c["cls"].shape[0]
    pre = dict(rows=rows, levels=tuple(c["levels"]), batch=B, labels=torch.zeros(rows, dtype=torch.int32, device=dev),
               wf=wf, wi=wi, keys=None)
    cls, reg = c["cls"].to(dev), c["reg"].to(dev)
    losses = ev.forward(cls, reg, c["levels"], B, tgt, tk, pre=pre)
    dcls = torch.full((rows, 16), float("nan"), dtype=torch.float32, device=dev)
    dreg = torch.zeros(rows, 240, dtype=torch.float32, device=dev)
    w = torch.tensor(K.WEIGHTS, dtype=torch.float32, device=dev)
    ev.backward(w, torch.float32, dcls, dreg)
    torch.cuda.synchronize()
    ctx = ev.ctx
    out = dict(loss_kd=float(losses[2].cpu()), loss_img=wf[8:8 + B].cpu().clone(), dcls=dcls.cpu(), dreg=dreg.cpu(),
               n_valid=int(ctx["n_valid"].cpu()), valid=ctx["valid"].cpu().clone(), cnt=cnt.cpu())
    out.update({k: ctx[k].cpu().clone() for k in ("xs", "alpha", "g_xs", "g_alpha")})
    out.update({k: getattr(tk, k).cpu().clone() for k in ("t_kp_norm", "t_beta", "t_start", "t_cnt", "t_kp", "t_score")})
    if per_object:
        out["obj"] = {k: v.cpu().clone() for k, v in ev.obj.items()}
    return out


def _problem_reference(xs, alpha, s0, N, t, t0, M, kind):
    """fp64 reference of one problem on the arrays the launch read: student rows [s0, s0+N), teacher rows [t0, t0+M)."""
    x, y = xs[s0:s0 + N].permute(1, 0, 2), t["t_kp_norm"][t0:t0 + M].permute(1, 0, 2)
    # fp32 and fp64 must take the clamp alike: no clamped variable within 1e-5 (relative) of 1e-8
    for u, v in ((x, x), (x, y), (y, y)):
        r2 = ((u.double()[:, :, None] - v.double()[:, None]) ** 2).sum(-1)
        for s in (r2, r2 / KD_BLUR ** 2):
            assert not bool(((s - C.CLAMP).abs() <= 1e-5 * C.CLAMP).any()), "a pair on the clamp's edge: choose another case"
    return C.reference(alpha[s0:s0 + N].t(), x, t["t_beta"][t0:t0 + M].t(), y, kind, KD_BLUR)


def _oracle_grads(c, got, kind, detach):
    """dcls / dreg of w_reg loss_reg + w_kd loss_kd from the fp32 oracle (oracle.kd_step_ref.kd_pose_loss) with the torch
    kernel loss in its OT hook and the teacher cells the device selected."""
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    from oracle import kd_step_ref as O
    from test_loss_cases_host import _oracle_ssc, _unpack
    targets, levels = c["targets"], c["levels"]
    B = len(targets)
    lay = LC.Layout(B, levels)
    sc = LC.ssc_case(c["name"])
    labs, gids, auxs = zip(*[_oracle_ssc(sc, b)[:3] for b in range(B)])
    cls_r = [t.requires_grad_(True) for t in _unpack(c["cls"][:, :15], lay)]
    reg_r = [t.requires_grad_(True) for t in _unpack(c["reg"], lay)]
    t0, tm = got["t_start"].tolist(), got["t_cnt"].tolist()
    teacher = ([got["t_score"][t0[b]:t0[b] + tm[b]] for b in range(B)], [got["t_kp"][t0[b]:t0[b] + tm[b]] for b in range(B)])
    out = O.kd_pose_loss(cls_r, reg_r, [t.as_dict() for t in targets], teacher, INTERNAL_K, MESH_DIAMETERS, torch.stack(labs),
                         torch.stack(gids), torch.stack(auxs), kd=dict(blur=KD_BLUR, scaling=0.5, reach=0.5, weighted=True, detach=detach),
                         ot_fn=C.ot_fn(kind))
    assert out["pos_per_img"] == [len(p) for p in c["pos"]]
    (out["loss_reg"] * K.WEIGHTS[1] + out["loss_kd"] * K.WEIGHTS[2]).backward()

    def pack(per_level):
        return torch.cat([(torch.zeros_like(t) if t.grad is None else t.grad).permute(0, 2, 3, 1).reshape(-1, t.shape[1])
                          for t in per_level]).double()
    return float(out["loss_kd"].detach()), pack(cls_r), pack(reg_r)


@pytest.mark.parametrize("detach", [False, True], ids=["alpha_grad", "wot_detach"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_kdloss_per_image_vs_fp64_and_oracle(gpu_device, kind, detach):
    """KDLoss(GTYPE=kind, KERNEL_LOSSES) on a multi-instance full-frame student case against the teacher cells of the
    matching teacher case: the launch's outputs vs the fp64 reference on the arrays it read; dcls / dreg after backward
    vs the fp32 oracle with the torch kernel loss in its OT hook."""
    _, _, kl = _kd()
    dev = gpu_device
    c = LC.student_case(STUDENT, every_level=False)
    tc = LC.teacher_case(TEACHER)
    assert tc["levels"] == c["levels"] and tc["batch"] == len(c["targets"])
    B, cap = len(c["targets"]), c["cap"]
    tgt = kl.PackedTargets(c["targets"], dev)
    tk = kl.teacher_select(tc["cls"].to(dev), tc["reg"].to(dev), tc["levels"], B, tc["bbox_trans"].to(dev))
    got = _run_loss(c, dev, kind, False, tk, tgt, detach)
    assert got["n_valid"] == B and got["valid"][:B].tolist() == [1] * B and min(got["t_cnt"].tolist()) > 0
    ref_img = torch.zeros(B, dtype=C.F64)
    ref_gx, ref_ga = torch.zeros(B * cap, 8, 2, dtype=C.F64), torch.zeros(B * cap, 8, dtype=C.F64)
    for b in range(B):
        N, M, t0 = int(got["cnt"][b]), int(got["t_cnt"][b]), int(got["t_start"][b])
        r = _problem_reference(got["xs"], got["alpha"], b * cap, N, got, t0, M, kind)
        ref_img[b] = r["loss"].sum()
        ref_gx[b * cap:b * cap + N], ref_ga[b * cap:b * cap + N] = r["grad_x"].permute(1, 0, 2), r["grad_alpha"].t()
    what = "KDLoss %s" % STUDENT
    C.assert_within(got["loss_img"], ref_img, kind, "loss", what + " loss_img")
    C.assert_within(got["g_xs"], ref_gx, kind, "grad_x", what)
    C.assert_within(got["g_alpha"], ref_ga, kind, "grad_alpha", what)
    # losses[2] = the mean: the launch's bound on every loss_img plus kd6d_kd_mean's own on the mean
    want = float(ref_img.mean())
    tol = C.bound(kind, "loss") * float(ref_img.abs().max()) + LC.bound("loss_kd") * abs(want)
    print("  loss_kd %s: got %.8g ref %.8g tol %.3e" % (kind, got["loss_kd"], want, tol))
    assert abs(got["loss_kd"] - want) <= tol
    # the chain into the logits against the fp32 oracle, 5e-3 of the largest magnitude
    o_kd, o_dcls, o_dreg = _oracle_grads(c, got, kind, detach)
    assert abs(o_kd - want) <= 5e-3 * max(abs(want), float(ref_img.abs().max()))
    dreg, dcls = got["dreg"].double(), got["dcls"][:, :15].double()
    for nm, g_, r_ in (("dreg", dreg, o_dreg), ("dcls", dcls, o_dcls)):
        m, err = float(r_.abs().max()), float((g_ - r_).abs().max())
        print("  %-5s %s: max|err| %.3e  max|oracle| %.3e  rel %.3e" % (nm, kind, err, m, err / max(m, 1e-300)))
        assert err <= 5e-3 * m
    if detach:
        assert bool((got["dcls"] == 0).all()), "wot_detach: no KD gradient reaches the class logits (w_cls = 0)"
    else:
        assert float(o_dcls.abs().max()) > 0 and float(got["dcls"].abs().max()) > 0


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("name", ["mixed_c256_l5_general", "absent_same_class_c128_lam05"])
def test_kdloss_per_object_vs_fp64(gpu_device, name, kind):
    """KDLoss(PER_OBJECT, GTYPE=kind): loss_obj per object and the gradients scattered back into slot order vs the fp64
    reference on the object-major arrays the launch read; loss_kd = the mean over the valid objects."""
    _, _, kl = _kd()
    dev = gpu_device
    c = K.object_case(name)
    B, cap = len(c["targets"]), c["cap"]
    tgt = kl.PackedTargets(c["targets"], dev)
    tk = kl.teacher_select(c["tcls"].to(dev), c["treg"].to(dev), c["levels"], B, tgt.bbox_trans, per_object=True,
                           class_ids=tgt.class_ids, n_gt=tgt.n_gt)
    got = _run_loss(c, dev, kind, True, tk, tgt)
    o = got["obj"]
    nobj = B * 4
    want_valid = [1 if (int(o["cnt"][i]) > 0 and int(got["t_cnt"][i]) > 0) else 0 for i in range(nobj)]
    assert o["valid"].tolist() == want_valid and got["n_valid"] == sum(want_valid) > 0
    assert 0 in want_valid, "the cases hold empty object slots too"
    ref_loss = torch.zeros(nobj, dtype=C.F64)
    ref_gx, ref_ga = torch.zeros(B * cap, 8, 2, dtype=C.F64), torch.zeros(B * cap, 8, dtype=C.F64)     # object-major
    for i in range(nobj):
        if not want_valid[i]:
            continue
        s0, N, t0, M = int(o["start"][i]), int(o["cnt"][i]), int(got["t_start"][i]), int(got["t_cnt"][i])
        r = _problem_reference(o["xs"], o["alpha"], s0, N, got, t0, M, kind)
        ref_loss[i] = r["loss"].sum()
        ref_gx[s0:s0 + N], ref_ga[s0:s0 + N] = r["grad_x"].permute(1, 0, 2), r["grad_alpha"].t()
    what = "per object %s" % name
    C.assert_within(o["loss"], ref_loss, kind, "loss", what + " loss_obj")
    # scattered: slot s of image b holds the row dest[slot] of the object-major arrays (zero for an invalid object's slots)
    slots = torch.tensor([b * cap + s for b in range(B) for s in range(int(got["cnt"][b]))])
    dest = o["dest"][slots].long()
    want_gx, want_ga = torch.zeros_like(ref_gx), torch.zeros_like(ref_ga)
    want_gx[slots], want_ga[slots] = ref_gx[dest], ref_ga[dest]
    C.assert_within(got["g_xs"], want_gx, kind, "grad_x", what + " scattered")
    C.assert_within(got["g_alpha"], want_ga, kind, "grad_alpha", what + " scattered")
    want = float(ref_loss.sum() / sum(want_valid))
    tol = C.bound(kind, "loss") * float(ref_loss.abs().max()) + LC.bound("loss_kd") * abs(want)
    print("  loss_kd %s %s: got %.8g ref %.8g tol %.3e" % (name, kind, got["loss_kd"], want, tol))
    assert abs(got["loss_kd"] - want) <= tol
    assert bool(torch.isfinite(got["dreg"]).all()) and float(got["dreg"].abs().max()) > 0


# ---- 7. the whole step ----------------------------------------------------------------------------------------------------
def _make_cfg(arch, precision):
    import yaml
    from kd6d.arguments.argument import custom_cfg
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["RUNTIME"] = {"PRECISION": precision}
    cfg["MODEL"]["BACKBONE"] = arch
    cfg = custom_cfg(cfg)
    cfg["KD"] = dict(LOSS_WEIGHT_KD=5.0, LEVEL="pred", GLEVEL="point", GTYPE="laplacian", GP=2.0, GBLUR=0.05, GnD=2,
                     WEIGHTED_OT=True, DETACH=False, SCALING=0.5, REACH=0.5, KERNEL_LOSSES=True)
    return cfg


def _build(arch, seed, dev, cls_bias=None):
    from kd6d import backbone as BB
    from kd6d.models.model_kd import PoseModuleKD
    from oracle import kd_step_ref as O
    m = PoseModuleKD(_make_cfg(arch, "fp32"), getattr(BB, arch)())
    sd = O.seeded_state_dict(O.PoseNetRef(arch), seed)
    if cls_bias is not None:
        sd["head.cls_logits.bias"] = torch.as_tensor(cls_bias, dtype=torch.float32)
    m.load_state_dict(sd)
    return m.to(dev)


def test_whole_step_every_launch_mode_bitwise(gpu_device):
    """PoseModuleKD with GTYPE=laplacian, blur 0.05 on make_batch(4, seed, crop=64): eager, graph and the grouped pipeline
    (teacher group 3) give bitwise-equal losses of the first step and bitwise-equal weights after it; a second
    execution of a mode is bitwise equal to the first; loss_kd finite and >= 0 (a positive-definite kernel)."""
    from kd6d.graph import GraphedKDStep, GroupedTeacherKDStep
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.optim import FusedClipAdamW
    from kd6d.synthetic import make_batch, teacher_cls_bias
    dev = gpu_device
    B, crop = 4, 64
    images, targets = make_batch(B, 5, crop=crop)
    batch = (ImageList(images.tensors.to(dev), images.sizes), PackedTargets(targets, dev))
    rows = B * sum((crop // 8 // 2 ** i) ** 2 for i in range(4))
    keys = torch.rand(rows, generator=torch.Generator().manual_seed(3)).to(dev)
    bias = teacher_cls_bias(1, False)
    names = ("loss_cls", "loss_reg", "loss_kd")

    def run(mode):
        teacher = _build("darknet53", 2, dev, bias).eval()
        student = _build("darknet_tiny_h", 1, dev).train()
        assert student.loss_evaluator.kernel == 1
        student._debug_keys = keys
        opt = FusedClipAdamW(student, lr=1e-3)
        if mode == "eager":
            student.zero_grad()
            with torch.no_grad():
                pred_t = teacher(batch[0], targets=batch[1], is_teacher=True)
            _, ld = student(batch[0], targets=batch[1], pred_t=pred_t)
            (ld["loss_cls"] * 0.1 + ld["loss_reg"] + ld["loss_kd"] * 5.0).backward()
            opt.step()
        else:
            if mode == "graph":
                gs = GraphedKDStep(teacher, student, opt, (0.1, 1.0, 5.0), pipeline=False)
            else:
                gs = GroupedTeacherKDStep(teacher, student, opt, (0.1, 1.0, 5.0), group=3)
            ld = gs(*batch)
            while ld is None and mode != "graph" and gs.pending_steps and opt.steps == 0:
                ld = gs.flush()
        n_valid = int(student.loss_evaluator.ctx["n_valid"].cpu())
        torch.cuda.synchronize()
        assert opt.steps == 1, (mode, opt.steps)
        return [float(torch.as_tensor(ld[k]).detach()) for k in names], student.net.store.params.detach().cpu().clone(), n_valid

    out = {m: run(m) for m in ("eager", "graph", "pipeline3")}
    again = run("graph")
    again3 = run("pipeline3")
    l_e, p_e, nv = out["eager"]
    print("  losses %s  valid images %d of %d" % (l_e, nv, B))
    assert nv > 0 and all(np.isfinite(l_e)) and l_e[2] >= 0
    assert again[0] == out["graph"][0] and torch.equal(again[1], out["graph"][1]), "second execution differs"
    assert again3[0] == out["pipeline3"][0] and torch.equal(again3[1], out["pipeline3"][1]), "second grouped execution differs"
    for m in ("graph", "pipeline3"):
        l, p, v = out[m]
        print("  %-9s losses %s  max|dW| vs eager %.3e" % (m, l, float((p - p_e).abs().max())))
    for m in ("graph", "pipeline3"):
        l, p, v = out[m]
        assert v == nv and l == l_e, (m, l, l_e)
        assert torch.equal(p, p_e), (m, float((p - p_e).abs().max()))


# ---- 8. the training entry ------------------------------------------------------------------------------------------------
def _train_cmd(wd, extra):
    return [sys.executable, os.path.join(ROOT, "train_kd.py"), "--config_file", "configs/ape.yaml", "--config_file_t",
            "configs/ape.yaml", "--backbone", "darknet_tiny_h", "--backbone_t", "darknet53", "--kd_weight", "5.",
            "--working_dir", wd, "--synthetic", "--skip_teacher_eval", "--batch_size", "4", "--image_size", "64",
            "--gtype", "energy", "--launch", "pipeline", "--teacher_group", "3"] + extra


@pytest.mark.parametrize("extra", [[], ["--synthetic_instances", "3", "--mixed_classes"]], ids=["one_object", "three_objects"])
def test_train_entry_energy_pipelined(gpu_device, tmp_path, extra):
    """train_kd.py --gtype energy --kd_kernel_losses, grouped pipeline: ends with "Training finished" and a finite loss_kd.
    one_object: the command as it stands -- train_kd.py raises a synthetic random-weight teacher's class bias only for
    multi-instance batches, so this teacher emits no cell and loss_kd is 0 (every problem skipped, as with the
    Sinkhorn); three_objects: the teacher emits, the KD term is at work."""
    import json
    wd = str(tmp_path) + "/"
    r = subprocess.run(_train_cmd(wd, ["--kd_kernel_losses", "--max_iters", "10", "--val_freq", "100"] + extra), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Training finished" in r.stdout
    scal = [json.loads(l) for d, _, fs in os.walk(wd) for f in fs if f == "scalars.jsonl" for l in open(os.path.join(d, f))]
    kd = [s["value"] for s in scal if s["tag"] == "training/loss_kd"]
    print("  loss_kd", kd)
    assert kd and all(np.isfinite(v) for v in kd)
    if extra:
        assert all(v != 0 for v in kd)


def test_train_entry_refuses_energy_without_the_flag(tmp_path):
    r = subprocess.run(_train_cmd(str(tmp_path) + "/", ["--max_iters", "2"]), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--kd_kernel_losses" in r.stderr, (r.returncode, r.stderr[-1000:])
