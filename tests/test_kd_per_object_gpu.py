"""GPU: the per-object KD term (--kd_per_object) kernel by kernel, as a loss, and as a whole training step, against
the fp64 restatement of tests/kd_object_cases.py.  Tolerances: rows / integer outputs / copies exact; teacher values
within loss_cases.bound; the OT value and its direct gradients as tests/test_losses_gpu.py has them for SamplesLoss;
the chained dreg / dcls within kd_object_cases.bound (profiles/kd_per_object_tolerances.md)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kd_object_cases as K
import loss_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_CFG = dict(GTYPE="sinkhorn", GLEVEL="point", GnD=2, GP=2.0, GBLUR=0.001, SCALING=0.5, REACH=0.5, WEIGHTED_OT=True,
              DETACH=False)
SENT_I = -7


def _kd():
    from kd6d import _lib, kd_losses, ops
    return _lib, ops, kd_losses


def _slot_arrays(c, dev):
    B, cap = len(c["targets"]), c["cap"]
    cnt = torch.tensor([len(p) for p in c["pos"]], dtype=torch.int32)
    row = torch.zeros(B, cap, dtype=torch.int32)
    gt = torch.zeros(B, cap, dtype=torch.int32)
    for b, p in enumerate(c["pos"]):
        for s, (r, g) in enumerate(p):
            row[b, s], gt[b, s] = r, g
    return cnt.to(dev), row.view(-1).to(dev), gt.view(-1).to(dev)


def _teacher(c, dev, per_object, tcls=None):
    _, _, kl = _kd()
    tgt = kl.PackedTargets(c["targets"], dev)
    tcls = (c["tcls"] if tcls is None else tcls).to(dev)
    treg = c["treg"].to(dev)
    tk = kl.teacher_select(tcls, treg, c["levels"], len(c["targets"]), tgt.bbox_trans, per_object=per_object,
                           class_ids=tgt.class_ids, n_gt=tgt.n_gt)
    torch.cuda.synchronize()
    return tk, tgt


# ---- 1. teacher selection per object ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.STUDENT_CASES))
def test_teacher_select_objects_vs_reference_and_pose_candidates(gpu_device, name):
    """Several classes emit per image (every instance's class and a distractor with a lower id): block o = b*4 + g holds
    the cells of slot g's class -- rows exact, values within loss_cases.bound -- empty for g >= n_gt; kp and score are
    bitwise kd6d_pose_candidates' on the same inputs; one class twice in an image: the same cells in both blocks."""
    _lib, ops, kl = _kd()
    dev = gpu_device
    c = K.object_case(name)
    B, cap = len(c["targets"]), kl.CAP
    tk, tgt = _teacher(c, dev, True)
    assert tk.per_object and tk.t_cnt.numel() == B * K.MAX_GT
    ref = K.teacher_objects(c["tcls"], c["treg"], c["targets"], c["levels"], cap=cap)
    cnt = tk.t_cnt.cpu().tolist()
    rows, kp, sc = tk.t_row.cpu(), tk.t_kp.cpu(), tk.t_score.cpu()
    kpn, beta = tk.t_kp_norm.cpu(), tk.t_beta.cpu()
    n_emit = 0
    for o, r in enumerate(ref):
        n = len(r["rows"])
        assert cnt[o] == n, (o, cnt[o], n)
        if o % K.MAX_GT >= len(c["targets"][o // K.MAX_GT].class_ids):
            assert n == 0
        s = slice(o * cap, o * cap + n)
        assert rows[s].tolist() == r["rows"], ("rows", o)
        assert float(kp[o * cap + n:(o + 1) * cap].abs().max()) == 0 if n < cap else True
        if n:
            n_emit += 1
            what = "%s object %d" % (name, o)
            C.assert_within(kp[s], r["kp"], "t_kp", what)
            C.assert_within(sc[s], r["score"][:, None].expand(-1, 8), "t_score", what)
            C.assert_within(kpn[s], r["kp_norm"], "t_kp_norm", what)
            C.assert_within(beta[s], r["beta"][:, None].expand(-1, 8), "t_beta", what)
    assert n_emit > B - 1
    # bitwise against kd6d_pose_candidates
    lv = kl.make_levels(B, c["levels"])
    n = B * K.MAX_GT * cap
    f32 = dict(dtype=torch.float32, device=dev)
    p_cnt = torch.full((B * K.MAX_GT,), SENT_I, dtype=torch.int32, device=dev)
    p_kp, p_sc = torch.zeros(n, 8, 2, **f32), torch.zeros(n, 8, **f32)
    tcls, treg = c["tcls"].to(dev), c["treg"].to(dev)
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_pose_candidates(ctypes.byref(lv), P(tcls), P(treg), P(tgt.bbox_trans), P(tgt.class_ids),
                                             P(tgt.n_gt), 0.1, 10.0, 1.0, cap, P(p_cnt), P(p_kp), P(p_sc), ops._stream()),
               "kd6d_pose_candidates")
    torch.cuda.synchronize()
    assert torch.equal(p_cnt.cpu(), tk.t_cnt.cpu()) and torch.equal(p_kp.cpu(), kp) and torch.equal(p_sc.cpu(), sc)
    # per-image selection on the same logits picks ONE class per image (the defect the feature removes)
    tki, _ = _teacher(c, dev, False)
    assert tki.t_cnt.numel() == B and not tki.per_object


# ---- 2. grouping and scatter -------------------------------------------------------------------------------------------
def _group(dev, cnt, gt, xs, alpha, B, cap):
    _lib, ops, _ = _kd()
    n, nobj = B * cap, B * K.MAX_GT
    i32 = dict(dtype=torch.int32, device=dev)
    start, num, dest = torch.full((nobj,), SENT_I, **i32), torch.full((nobj,), SENT_I, **i32), torch.full((n,), SENT_I, **i32)
    xs_o, al_o = torch.full_like(xs, 777.0), torch.full_like(alpha, 777.0)
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_kd_group_objects(P(cnt), P(gt), P(xs), P(alpha), B, cap, P(start), P(num), P(dest), P(xs_o),
                                              P(al_o), ops._stream()), "kd6d_kd_group_objects")
    torch.cuda.synchronize()
    return start, num, dest, xs_o, al_o


@pytest.mark.parametrize("name", sorted(C.STUDENT_CASES) + ["foreign_gt"])
def test_group_and_scatter_objects_are_exact(gpu_device, name):
    """obj_start / obj_cnt / dest equal numpy's stable partition; xs_obj / alpha_obj are bit copies in that order and
    nothing else is written; scatter o group is the identity on the cells of valid objects and zero on every other
    positive slot, slots beyond pos_cnt untouched; valid_img = any valid object.  Cases: 0..4 instances per image, an
    absent instance, one class twice, and a slot list with instance ids outside 0..3 (they belong to no object)."""
    _lib, ops, _ = _kd()
    dev = gpu_device
    if name == "foreign_gt":
        B, cap = 3, 64
        g = torch.Generator().manual_seed(5)
        cnt = torch.tensor([64, 0, 17], dtype=torch.int32, device=dev)
        gt = torch.randint(-1, 6, (B * cap,), generator=g).to(torch.int32).to(dev)
    else:
        c = C.student_case(name)
        B, cap = len(c["targets"]), c["cap"]
        cnt, _, gt = _slot_arrays(c, dev)
    n = B * cap
    g = torch.Generator().manual_seed(11)
    xs = torch.randn(n, 8, 2, generator=g).to(dev)
    alpha = torch.rand(n, 8, generator=g).to(dev)
    start, num, dest, xs_o, al_o = _group(dev, cnt, gt, xs, alpha, B, cap)
    r_start, r_num, r_dest = K.group_reference(cnt.cpu().numpy(), gt.cpu().numpy(), B, cap)
    assert start.cpu().tolist() == r_start.tolist() and num.cpu().tolist() == r_num.tolist()
    used = r_dest >= 0
    d = dest.cpu().numpy()
    assert (d[used] == r_dest[used]).all() and (d[~used] == SENT_I).all()
    want_x, want_a = torch.full_like(xs, 777.0).cpu(), torch.full_like(alpha, 777.0).cpu()
    want_x[torch.from_numpy(r_dest[used])] = xs.cpu()[torch.from_numpy(used)]
    want_a[torch.from_numpy(r_dest[used])] = alpha.cpu()[torch.from_numpy(used)]
    assert torch.equal(xs_o.cpu(), want_x) and torch.equal(al_o.cpu(), want_a)
    # ascending slot order inside every object
    for o in range(B * K.MAX_GT):
        src = [int(np.nonzero(r_dest == j)[0][0]) for j in range(r_start[o], r_start[o] + r_num[o])]
        assert src == sorted(src)
    # scatter: a valid pattern with valid, invalid and oversize (-1) objects
    nobj = B * K.MAX_GT
    valid = torch.tensor([(1, 0, 1, -1)[o % 4] if (o // 4) % 2 == 0 else (0, 1, 1, 1)[o % 4] for o in range(nobj)],
                         dtype=torch.int32)
    if B > 1:
        valid[4:8] = torch.tensor([0, -1, 0, 0], dtype=torch.int32)          # image 1: no valid object
    g_xs_o, g_al_o = torch.randn(n, 8, 2, generator=g).to(dev), torch.randn(n, 8, generator=g).to(dev)
    g_xs, g_al = torch.full((n, 8, 2), 555.0, device=dev), torch.full((n, 8), 555.0, device=dev)
    v_img = torch.full((B,), SENT_I, dtype=torch.int32, device=dev)
    valid_d = valid.to(dev)
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_kd_scatter_objects(P(cnt), P(gt), P(dest), P(valid_d), P(g_xs_o), P(g_al_o), B, cap, P(g_xs),
                                                P(g_al), P(v_img), ops._stream()), "kd6d_kd_scatter_objects")
    torch.cuda.synchronize()
    want_x, want_a = torch.full((n, 8, 2), 555.0), torch.full((n, 8), 555.0)
    gt_c, cnt_c = gt.cpu().view(B, cap), cnt.cpu().tolist()
    for b in range(B):
        for s in range(cnt_c[b]):
            gg = int(gt_c[b, s])
            ok = 0 <= gg < K.MAX_GT and int(valid[b * K.MAX_GT + gg]) > 0
            want_x[b * cap + s] = g_xs_o.cpu()[r_dest[b * cap + s]] if ok else 0.0
            want_a[b * cap + s] = g_al_o.cpu()[r_dest[b * cap + s]] if ok else 0.0
    assert torch.equal(g_xs.cpu(), want_x) and torch.equal(g_al.cpu(), want_a)
    assert v_img.cpu().tolist() == [int(bool((valid[b * 4:b * 4 + 4] > 0).any())) for b in range(B)]
    # scatter o group = identity where every object is valid
    ones = torch.ones(nobj, dtype=torch.int32, device=dev)
    back_x, back_a = torch.zeros_like(xs), torch.zeros_like(alpha)
    _lib.check(_lib.lib.kd6d_kd_scatter_objects(P(cnt), P(gt), P(dest), P(ones), P(xs_o), P(al_o), B, cap, P(back_x),
                                                P(back_a), P(v_img), ops._stream()), "kd6d_kd_scatter_objects")
    torch.cuda.synchronize()
    in_obj = torch.zeros(n, dtype=torch.bool)
    for b in range(B):
        for s in range(cnt_c[b]):
            in_obj[b * cap + s] = 0 <= int(gt_c[b, s]) < K.MAX_GT
    assert torch.equal(back_x.cpu()[in_obj], xs.cpu()[in_obj]) and torch.equal(back_a.cpu()[in_obj], alpha.cpu()[in_obj])
    assert float(back_x.cpu()[~in_obj].abs().max() if (~in_obj).any() else 0.0) == 0


# ---- 3. the loss ---------------------------------------------------------------------------------------------------------
def _run_loss(c, dev, per_object, tk, tgt, weights=K.WEIGHTS, detach=False):
    """KDLoss forward + backward on the case's (row, instance) list (the assignment is not under test here)."""
    _, _, kl = _kd()
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    B, cap = len(c["targets"]), c["cap"]
    ev = kl.KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(KD_CFG, PER_OBJECT=per_object, DETACH=detach), cap=cap)
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
    w = torch.tensor(weights, dtype=torch.float32, device=dev)
    ev.backward(w, torch.float32, dcls, dreg)
    torch.cuda.synchronize()
    return dict(loss_kd=losses[2].cpu().clone(), dcls=dcls.cpu(), dreg=dreg.cpu(), n_valid=int(ev.ctx["n_valid"].cpu()),
                g_xs=ev.ctx["g_xs"].cpu().clone(), g_alpha=ev.ctx["g_alpha"].cpu().clone(), valid_img=ev.ctx["valid"].cpu().clone(),
                obj=getattr(ev, "obj", None), ev=ev)


@pytest.mark.parametrize("detach", [False, True], ids=["alpha_grad", "wot_detach"])
@pytest.mark.parametrize("name", sorted(C.STUDENT_CASES))
def test_per_object_loss_forward_backward_vs_fp64(gpu_device, name, detach):
    """KDLoss(PER_OBJECT) on the multi-instance student cases with the teacher sets of test 1.

    Figures measured on MI355X are printed before each assertion; see profiles/kd_per_object_tolerances.md for where the
    bounds of the chained gradients come from."""
    dev = gpu_device
    c = K.object_case(name)
    B, cap = len(c["targets"]), c["cap"]
    tk, tgt = _teacher(c, dev, True)
    got = _run_loss(c, dev, True, tk, tgt, detach=detach)
    ts = K.teacher_objects(c["tcls"], c["treg"], c["targets"], c["levels"])
    ref = K.kd_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], cap, ts, detach_alpha=detach)
    assert got["n_valid"] == ref["n_valid"] > 0
    assert got["obj"]["valid"].cpu().tolist() == ref["valid"].tolist()
    assert got["valid_img"][:B].tolist() == ref["img_valid"].tolist()
    print("  loss_kd %s: got %.8g ref %.8g rel %.3e" % (name, float(got["loss_kd"]), ref["loss_kd"],
                                                       abs(float(got["loss_kd"]) - ref["loss_kd"]) / ref["loss_kd"]))
    torch.testing.assert_close(got["loss_kd"].double().view(()), torch.tensor(ref["loss_kd"], dtype=torch.float64),
                               rtol=2e-4, atol=1e-7)
    lo = torch.from_numpy(ref["loss"][ref["valid"] > 0])
    torch.testing.assert_close(got["obj"]["loss"].cpu().double()[torch.from_numpy(ref["valid"] > 0)], lo, rtol=2e-4, atol=1e-7)
    # the OT's own gradients, in slot order (tests/test_losses_gpu.py's SamplesLoss tolerances)
    ga, gx = ref["g_alpha"], ref["g_xs"]
    print("  g_alpha max|err| %.3e of %.3e   g_xs max|err| %.3e of %.3e" % (
        float((got["g_alpha"].double() - ga).abs().max()), float(ga.abs().max()),
        float((got["g_xs"].double() - gx).abs().max()), float(gx.abs().max())))
    torch.testing.assert_close(got["g_alpha"].double(), ga, rtol=2e-3, atol=1e-6)
    torch.testing.assert_close(got["g_xs"].double(), gx, rtol=5e-3, atol=5e-3 * float(gx.abs().max()))
    # the chain into the logits
    rr, cc = ref["rows"], ref["cls_of"]
    cols = cc[:, None] * 16 + torch.arange(16)[None]
    d_reg, d_cls = got["dreg"][rr[:, None], cols].double(), got["dcls"][rr, cc].double()
    for nm, g_, r_ in (("dreg", d_reg, ref["draw"]), ("dcls", d_cls, ref["dz"])):
        m = float(r_.abs().max())
        err = float((g_ - r_).abs().max())
        print("  %-5s %s: max|err| %.3e  max|ref| %.3e  rel %.3e  bound %.3e" % (nm, name, err, m, err / max(m, 1e-300), K.bound(nm)))
    touched = torch.zeros(got["dreg"].shape, dtype=torch.bool)
    touched[rr[:, None], cols] = True
    assert bool((got["dreg"][~touched] == 0).all())
    hit = torch.zeros(got["dcls"].shape, dtype=torch.bool)
    hit[rr, cc] = True
    assert bool((got["dcls"][~hit] == 0).all()), "w_cls = 0: only the KD chain reaches dcls"
    if detach:
        assert bool((got["dcls"] == 0).all())
    else:
        assert float(ref["dz"].abs().max()) > 0
    assert float((d_reg - ref["draw"]).abs().max()) <= K.bound("dreg") * float(ref["draw"].abs().max())
    assert float((d_cls - ref["dz"]).abs().max()) <= K.bound("dcls") * float(ref["dz"].abs().max()) + 0.0


# ---- 4. reduction to the per-image path --------------------------------------------------------------------------------
def test_single_instance_batch_is_bitwise_the_per_image_path(gpu_device):
    """One instance per image, the teacher emits the ground-truth class only: same kernel, same sets, same order --
    loss_kd, dcls and dreg are bitwise equal with and without PER_OBJECT."""
    dev = gpu_device
    c = K.single_instance_case()
    w = (0.1, 1.0, 5.0)
    tk_o, tgt = _teacher(c, dev, True)
    tk_i, _ = _teacher(c, dev, False)
    a = _run_loss(c, dev, True, tk_o, tgt, weights=w)
    b = _run_loss(c, dev, False, tk_i, tgt, weights=w)
    assert a["n_valid"] == b["n_valid"] == len(c["targets"]) and float(a["loss_kd"]) > 0
    assert torch.equal(a["loss_kd"], b["loss_kd"])
    assert torch.equal(a["g_xs"], b["g_xs"]) and torch.equal(a["g_alpha"], b["g_alpha"])
    assert torch.equal(a["dreg"], b["dreg"]) and torch.equal(a["dcls"], b["dcls"])
    assert float(a["dreg"].abs().max()) > 0


# ---- 5. isolation ----------------------------------------------------------------------------------------------------------
def test_objects_are_isolated_from_each_other(gpu_device):
    """Two objects per image; the teacher's logits of object A's class (the lower class id: the per-image rule's pick)
    are perturbed.  PER_OBJECT: every gradient element on the rows of object B is bitwise unchanged (and A's change).
    Per image: B's rows change -- the defect this mode removes."""
    dev = gpu_device
    c = K.two_object_case()
    B, cap = len(c["targets"]), c["cap"]
    tcls2 = c["tcls"].clone()
    rows_a, rows_b = [], []
    for b, t in enumerate(c["targets"]):
        ids = [int(x) for x in t.class_ids]
        ga = ids.index(min(ids))
        tcls2[:, ids[ga]] = torch.where(tcls2[:, ids[ga]] > -4.0, tcls2[:, ids[ga]] * 0.8 + 0.3, tcls2[:, ids[ga]])
        for row, g in c["pos"][b]:
            (rows_a if g == ga else rows_b).append((row, ids[g]))
    assert rows_a and rows_b
    w = (0.0, 0.0, 5.0)                   # the KD term alone

    def grads(per_object, tcls):
        tk, tgt = _teacher(c, dev, per_object, tcls)
        r = _run_loss(c, dev, per_object, tk, tgt, weights=w)
        return r

    def pick(r, rows):
        reg = torch.stack([r["dreg"][row, cl * 16:cl * 16 + 16] for row, cl in rows])
        cls = torch.stack([r["dcls"][row, cl] for row, cl in rows])
        return reg, cls

    o0, o1 = grads(True, c["tcls"]), grads(True, tcls2)
    assert o0["n_valid"] == o1["n_valid"] == 2 * B
    assert float(pick(o0, rows_b)[0].abs().max()) > 0
    for x, y in zip(pick(o0, rows_b), pick(o1, rows_b)):
        assert torch.equal(x, y), "per object: B's gradients must not see A's teacher"
    assert not torch.equal(pick(o0, rows_a)[0], pick(o1, rows_a)[0]), "the perturbation must reach A"
    i0, i1 = grads(False, c["tcls"]), grads(False, tcls2)
    assert not torch.equal(pick(i0, rows_b)[0], pick(i1, rows_b)[0]), "per image: B's rows are transported onto A's votes"
    assert not torch.equal(pick(i0, rows_b)[0], pick(o0, rows_b)[0])


# ---- 5b. the loss-level drop-in -------------------------------------------------------------------------------------------
def test_kd_pose_loss_per_object_equals_kdloss(gpu_device):
    """kd6d.losses.KDPoseLoss(cfg_kd["PER_OBJECT"]) on per-level NCHW head outputs with a per-object TeacherKnowledge:
    the three losses and, through autograd, the gradients of their weighted sum are bitwise what KDLoss(per_object)
    gives on the same packed inputs and sampling keys (same kernels underneath); the KD term is active and every
    existing object is valid.  A per-image TeacherKnowledge is refused."""
    _, _, kl = _kd()
    from kd6d.losses import KDPoseLoss
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    dev = gpu_device
    c = K.two_object_case()
    B, levels = len(c["targets"]), c["levels"]
    lay = C.Layout(B, levels)
    keys = torch.from_numpy(c["keys"]).to(torch.float32).to(dev)
    tk, tgt = _teacher(c, dev, True)
    cls_p = c["cls"].clone()
    cls_p[:, 15] = 0.0
    w = (0.1, 1.0, 5.0)
    # KDLoss on the packed rows
    ev = kl.KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(KD_CFG, PER_OBJECT=True))
    cls_d, reg_d = cls_p.to(dev), c["reg"].to(dev)
    want = ev.forward(cls_d, reg_d, levels, B, tgt, tk, keys=keys).clone()
    dcls = torch.full((lay.rows, 16), float("nan"), dtype=torch.float32, device=dev)
    dreg = torch.zeros(lay.rows, 240, dtype=torch.float32, device=dev)
    ev.backward(torch.tensor(w, dtype=torch.float32, device=dev), torch.float32, dcls, dreg)
    torch.cuda.synchronize()
    n_valid = int(ev.ctx["n_valid"].cpu())
    assert n_valid == 2 * B and float(want[2]) > 0
    # the drop-in on per-level NCHW tensors
    def nchw(packed, ch):
        out = []
        for l, (h, wd) in enumerate(levels):
            blk = packed[lay.row0[l]:lay.row0[l] + B * h * wd, :ch]
            out.append(blk.reshape(B, h, wd, ch).permute(0, 3, 1, 2).contiguous().to(dev).requires_grad_(True))
        return out

    class Coder:
        target_type = "3D"

    crit = KDPoseLoss(2.0, 0.25, C.SIZES, C.STRIDES, "SSC", 10, 1.0, 9, INTERNAL_K, MESH_DIAMETERS, Coder(),
                      dict(KD_CFG, LOSS_WEIGHT_KD=5.0, LEVEL="pred", PER_OBJECT=True))
    crit.keys = keys
    pc, pr = nchw(cls_p, 15), nchw(c["reg"], 240)
    l_cls, l_reg, l_kd = crit(pc, pr, [t.to(dev) for t in c["targets"]], None, tk)
    (l_cls * w[0] + l_reg * w[1] + l_kd * w[2]).backward()
    torch.cuda.synchronize()
    got = torch.stack([l_cls, l_reg, l_kd]).detach()
    print("  KDPoseLoss %s  KDLoss %s" % (got.tolist(), want[:3].tolist()))
    assert torch.equal(got.cpu(), want[:3].cpu())

    def packed(grads, ch):
        return torch.cat([g.grad.permute(0, 2, 3, 1).reshape(-1, ch) for g in grads], 0).cpu()

    assert torch.equal(packed(pc, 15), dcls.cpu()[:, :15]) and torch.equal(packed(pr, 240), dreg.cpu())
    assert float(dreg.abs().max()) > 0
    tk_img, _ = _teacher(c, dev, False)
    with pytest.raises(TypeError, match="object axis"):
        crit(pc, pr, [t.to(dev) for t in c["targets"]], None, tk_img)


# ---- 6. whole step -----------------------------------------------------------------------------------------------------------
def _make_cfg(arch, precision):
    import yaml
    from kd6d.arguments.argument import custom_cfg
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["RUNTIME"] = {"PRECISION": precision}
    cfg["MODEL"]["BACKBONE"] = arch
    cfg = custom_cfg(cfg)
    cfg["KD"] = dict(LOSS_WEIGHT_KD=5.0, LEVEL="pred", GLEVEL="point", GTYPE="sinkhorn", GP=2.0, GBLUR=0.001, GnD=2,
                     WEIGHTED_OT=True, DETACH=False, SCALING=0.5, REACH=0.5, PER_OBJECT=True)
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
    """PoseModuleKD with PER_OBJECT on make_batch(16, seed, instances=3, mixed_classes=True): eager, graph and pipeline
    (teacher group 1 and 3) give bitwise-equal losses of the first step and bitwise-equal weights after it; a second
    execution of a mode is bitwise equal to the first; more valid objects than images."""
    from kd6d.graph import GraphedKDStep, GroupedTeacherKDStep
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.optim import FusedClipAdamW
    from kd6d.synthetic import make_batch, teacher_cls_bias
    dev = gpu_device
    B, crop = 16, 64
    images, targets = make_batch(B, 5, crop=crop, instances=3, mixed_classes=True)
    batch = (ImageList(images.tensors.to(dev), images.sizes), PackedTargets(targets, dev))
    rows = B * sum((crop // 8 // 2 ** i) ** 2 for i in range(4))
    keys = torch.rand(rows, generator=torch.Generator().manual_seed(3)).to(dev)
    bias = teacher_cls_bias(3, True)
    names = ("loss_cls", "loss_reg", "loss_kd")

    def run(mode):
        teacher = _build("darknet53", 2, dev, bias).eval()
        student = _build("darknet_tiny_h", 1, dev).train()
        student._debug_keys = keys
        opt = FusedClipAdamW(student, lr=1e-3)
        n_valid = None
        if mode == "eager":
            student.zero_grad()
            with torch.no_grad():
                pred_t = teacher(batch[0], targets=batch[1], is_teacher=True)
            assert pred_t.per_object and pred_t.t_cnt.numel() == B * 4
            _, ld = student(batch[0], targets=batch[1], pred_t=pred_t)
            (ld["loss_cls"] * 0.1 + ld["loss_reg"] + ld["loss_kd"] * 5.0).backward()
            opt.step()
            n_valid = int(student.loss_evaluator.ctx["n_valid"].cpu())
        else:
            if mode == "graph":
                gs = GraphedKDStep(teacher, student, opt, (0.1, 1.0, 5.0), pipeline=False)
            elif mode == "pipeline1":
                gs = GraphedKDStep(teacher, student, opt, (0.1, 1.0, 5.0), pipeline=True)
            else:
                gs = GroupedTeacherKDStep(teacher, student, opt, (0.1, 1.0, 5.0), group=3)
            ld = gs(*batch)
            while ld is None and mode != "graph" and gs.pending_steps and opt.steps == 0:
                ld = gs.flush()
            n_valid = int(student.loss_evaluator.ctx["n_valid"].cpu())
        torch.cuda.synchronize()
        assert opt.steps == 1, (mode, opt.steps)
        return [float(ld[k]) for k in names], student.net.store.params.detach().cpu().clone(), n_valid

    out = {m: run(m) for m in ("eager", "graph", "pipeline1", "pipeline3")}
    again = run("graph")
    again3 = run("pipeline3")
    l_e, p_e, nv = out["eager"]
    print("  losses %s  valid objects %d of %d images" % (l_e, nv, B))
    assert nv > B and l_e[2] > 0 and all(np.isfinite(l_e))
    assert again[0] == out["graph"][0] and torch.equal(again[1], out["graph"][1]), "second execution differs"
    assert again3[0] == out["pipeline3"][0] and torch.equal(again3[1], out["pipeline3"][1]), "second grouped execution differs"
    for m in ("graph", "pipeline1", "pipeline3"):
        l, p, v = out[m]
        print("  %-9s losses %s  max|dW| vs eager %.3e" % (m, l, float((p - p_e).abs().max())))
    for m in ("graph", "pipeline1", "pipeline3"):
        l, p, v = out[m]
        assert v == nv and l == l_e, (m, l, l_e)
        assert torch.equal(p, p_e), (m, float((p - p_e).abs().max()))


# ---- 7. the training entry ---------------------------------------------------------------------------------------------------
def _train_cmd(wd, extra):
    return [sys.executable, os.path.join(ROOT, "train_kd.py"), "--config_file", "configs/ape.yaml", "--config_file_t",
            "configs/ape.yaml", "--backbone", "darknet_tiny_h", "--backbone_t", "darknet53", "--kd_weight", "5.",
            "--working_dir", wd, "--synthetic", "--skip_teacher_eval", "--batch_size", "4", "--image_size", "64",
            "--synthetic_instances", "3", "--mixed_classes", "--kd_per_object", "--launch", "pipeline",
            "--teacher_group", "3"] + extra


def test_train_entry_per_object_pipelined(gpu_device, tmp_path):
    import json
    wd = str(tmp_path) + "/"
    r = subprocess.run(_train_cmd(wd, ["--max_iters", "10", "--val_freq", "100"]), cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "Training finished" in r.stdout
    scal = [json.loads(l) for d, _, fs in os.walk(wd) for f in fs if f == "scalars.jsonl" for l in open(os.path.join(d, f))]
    kd = [s["value"] for s in scal if s["tag"] == "training/loss_kd"]
    line = [l for l in r.stdout.splitlines() if l.startswith("steps: 1/")]
    print("  ", line, kd)
    assert line, r.stdout[-2000:]
    vals = {k: float(v) for k, v in (p.split(":") for p in line[0].replace(",", " ").split() if p[:3] in ("cls", "reg", "kd:"))}
    assert all(np.isfinite(v) for v in vals.values()) and vals["kd"] > 0, vals
    assert all(np.isfinite(v) and v > 0 for v in kd)


def test_train_entry_refuses_the_pnp_gate_per_object(tmp_path):
    from kd6d.kd_losses import PER_OBJECT_GATE_ERROR
    r = subprocess.run(_train_cmd(str(tmp_path) + "/", ["--max_iters", "2", "--teacher_pnp_gate", "--pnp_solver", "device"]),
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and PER_OBJECT_GATE_ERROR in r.stderr, (r.returncode, r.stderr[-1000:])
