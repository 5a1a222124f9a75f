"""The loss-level drop-in surface (kd6d.losses: SamplesLoss, kd_loss_2d, KDPoseLoss with the signatures of
losses/kd_loss.py:13-161 and losses/loss_libs.py:1-51 of the reference) against the CPU oracle, values and
gradients, through torch autograd the way a torch training loop would use them."""
import numpy as np
import pytest
import torch

import ctypes

import loss_cases
import loss_cases as C
from test_step_gpu import ref_to_packed_rows

pytestmark = pytest.mark.gpu


def _problem(B, N, M, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, N, D, generator=g) * 0.2 + 0.4
    y = x[:, torch.randperm(N, generator=g)[:M] % N] + 0.01 * torch.randn(B, M, D, generator=g) if M <= N else \
        torch.rand(B, M, D, generator=g) * 0.2 + 0.4
    a = torch.rand(B, N, generator=g) * 0.9 + 0.05
    b = torch.rand(B, M, generator=g) * 0.9 + 0.05
    return a, x, b, y


@pytest.mark.parametrize("B,N,M,reach", [(8, 10, 9, 0.5), (8, 10, 10, None), (3, 7, 12, 0.5), (1, 40, 33, 0.5)])
def test_samples_loss_small_sets_vs_oracle(gpu_device, B, N, M, reach):
    """SamplesLoss("sinkhorn", p=2, blur, scaling, reach)(alpha, x, beta, y) -> (B,): the call of
    losses/kd_loss.py:26-30 / loss_libs.py:47 (batch = the 8 keypoints of an image; shorter batches are padded)."""
    from kd6d.losses import SamplesLoss
    from oracle import kd_step_ref as O
    a, x, b, y = _problem(B, N, M, 2, 5 + B)
    xr, ar = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    ref = O.sinkhorn_divergence_torch(ar, xr, b, y, blur=0.001, scaling=0.5, reach=reach)
    w = torch.linspace(0.5, 1.5, B)
    (ref * w).sum().backward()
    dev = gpu_device
    xg, ag = x.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    L = SamplesLoss("sinkhorn", p=2, blur=0.001, scaling=0.5, reach=reach)
    got = L(ag, xg, b.to(dev), y.to(dev))
    assert got.shape == (B,)
    (got * w.to(dev)).sum().backward()
    torch.testing.assert_close(got.detach().cpu(), ref.detach(), rtol=2e-4, atol=1e-7)
    torch.testing.assert_close(ag.grad.cpu(), ar.grad, rtol=2e-3, atol=1e-6)
    scale = float(xr.grad.abs().max())
    torch.testing.assert_close(xg.grad.cpu(), xr.grad, rtol=5e-3, atol=5e-3 * scale)
    # (x, y) form: uniform weights
    got_u = L(x.to(dev), y.to(dev))
    ref_u = O.sinkhorn_divergence_torch(torch.full((B, N), 1.0 / N), x, torch.full((B, M), 1.0 / M), y, 0.001, 0.5, reach)
    torch.testing.assert_close(got_u.cpu(), ref_u, rtol=2e-4, atol=1e-7)
    with pytest.raises(NotImplementedError):
        SamplesLoss("gaussian")
    with pytest.raises(NotImplementedError):
        L(ag, xg, b.to(dev), y.to(dev).requires_grad_(True))


def test_samples_loss_large_sets_take_the_dense_kernel(gpu_device):
    """Above kd6d_sinkhorn_max_points (or D > 2) the same call runs the dense kernel per batch row with the joint
    diameter: D = 16, 300 x 280 points, blur 0.05, vs the fp64 oracle."""
    from kd6d.losses import SamplesLoss
    from oracle.sinkhorn_ref import sinkhorn_divergence
    B, N, M, D = 2, 300, 280, 16
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand(B, N, D, generator=g), torch.rand(B, M, D, generator=g)
    a, b = torch.rand(B, N, generator=g) + 0.1, torch.rand(B, M, generator=g) + 0.1
    pts = torch.cat([x.reshape(-1, D), y.reshape(-1, D)])
    diam = float((pts.max(0)[0] - pts.min(0)[0]).norm())
    dev = gpu_device
    xg, ag = x.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    got = SamplesLoss("sinkhorn", p=2, blur=0.05, scaling=0.5, reach=0.5)(ag, xg, b.to(dev), y.to(dev))
    got.sum().backward()
    for i in range(B):
        S, gx, fa = sinkhorn_divergence(a[i:i + 1].numpy().astype(np.float64), x[i:i + 1].numpy().astype(np.float64),
                                        b[i:i + 1].numpy().astype(np.float64), y[i:i + 1].numpy().astype(np.float64),
                                        blur=0.05, scaling=0.5, reach=0.5, diameter=diam, with_grad=True)
        S, gx, fa = S[0], gx[0], fa[0]
        assert float(got[i]) == pytest.approx(float(S), rel=5e-4)
        np.testing.assert_allclose(ag.grad[i].cpu().numpy(), fa, rtol=5e-3, atol=5e-3 * np.abs(fa).max())
        np.testing.assert_allclose(xg.grad[i].cpu().numpy(), gx, rtol=1e-2, atol=1e-2 * np.abs(gx).max())


def test_kd_loss_2d_matches_per_image_loop(gpu_device):
    """kd_loss_2d(pred_xy, target_xy, pred_cls, target_cls, w, h, level, kd_loss, dim, pos_per_img, pos_per_img_t):
    one packed launch for all images == the reference's per-image loop over the oracle OT (an image with an empty
    set is skipped, the inputs are normalised in place)."""
    from kd6d.losses import SamplesLoss, kd_loss_2d
    from oracle import kd_step_ref as O
    g = torch.Generator().manual_seed(9)
    pos, pos_t = [10, 0, 7, 9], [9, 8, 0, 10]
    P, M = sum(pos), sum(pos_t)
    pred = torch.rand(P * 8, 2, generator=g) * torch.tensor([640.0, 480.0])
    targ = pred[torch.randint(0, P * 8, (M * 8,), generator=g)] + torch.randn(M * 8, 2, generator=g) * 3.0
    a = torch.rand(P, 1, generator=g).expand(P, 8).contiguous() * 0.9 + 0.05
    b = torch.rand(M, 8, generator=g) * 0.9 + 0.05
    dev = gpu_device

    def run(kd, device):
        leaf = pred.clone().to(device).requires_grad_(True)
        al = a.clone().to(device).requires_grad_(True)
        pxy = leaf * 1.0                                        # non-leaf, as in the reference (decode output)
        txy = targ.clone().to(device)
        out = kd_loss_2d(pxy, txy, al, b.to(device), 640, 480, "point", kd, 2, pos_per_img=pos, pos_per_img_t=pos_t)
        (sum(out) / len(out)).backward()
        return out, leaf.grad.cpu(), al.grad.cpu(), pxy.detach().cpu(), txy.cpu()

    ref_fn = lambda al, x, be, y: O.sinkhorn_divergence_torch(al, x, be, y, 0.001, 0.5, 0.5)   # noqa: E731
    out_r, gx_r, ga_r, pn_r, tn_r = run(ref_fn, "cpu")
    kd = SamplesLoss("sinkhorn", p=2, blur=0.001, scaling=0.5, reach=0.5)
    out_g, gx_g, ga_g, pn_g, tn_g = run(kd, dev)
    assert len(out_g) == len(out_r) == 2
    torch.testing.assert_close(torch.stack([o.detach().cpu() for o in out_g]), torch.stack([o.detach() for o in out_r]),
                               rtol=2e-4, atol=1e-7)
    torch.testing.assert_close(pn_g, pn_r)                      # normalised in place on both sides
    torch.testing.assert_close(tn_g, tn_r)
    torch.testing.assert_close(ga_g, ga_r, rtol=2e-3, atol=1e-6)
    torch.testing.assert_close(gx_g, gx_r, rtol=5e-3, atol=5e-3 * float(gx_r.abs().max()))
    # any other callable is applied image by image (here: the oracle on CPU tensors through the same function)
    assert float(gx_r.abs().max()) > 0


@pytest.mark.parametrize("mixed", [False, True, "multi"])
def test_kd_pose_loss_call_signature_vs_oracle(gpu_device, mixed):
    """KDPoseLoss(gamma, alpha, anchor_sizes, anchor_strides, positive_type, positive_num, positive_lambda, top_k,
    internal_K, diameters, target_coder, cfg_kd)(pred_cls, pred_reg, targets, anchors, pred_t) on per-level NCHW
    head outputs that carry autograd, with pred_t in the reference's dict layout -> [cls, reg, kd] and the gradients
    of their weighted sum w.r.t. every level, vs oracle.kd_pose_loss.  "multi": 1, 3, 4 and 2 instances per image under
    a bbox_trans with rotation and shear (tests/loss_cases.py) instead of make_batch's one instance / diagonal affine."""
    from kd6d.losses import KDPoseLoss
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS, make_batch
    from oracle import kd_step_ref as O
    dev = gpu_device
    B, crop = 4, 128
    levels = [(crop // 8 // (2 ** i),) * 2 for i in range(4)]
    cells = sum(h * w for h, w in levels)
    counts = [h * w for h, w in levels]
    if mixed == "multi":
        targets = loss_cases.make_targets(B, (1, 3, 4, 2), 41, crop, affine="general")
    else:
        images, targets = make_batch(B, 77, crop=crop, mixed_classes=mixed)
    tds = [t.as_dict() for t in targets]
    g = torch.Generator().manual_seed(1)
    cls = [torch.randn(B, 15, h, w, generator=g) * 1.5 - 2.0 for h, w in levels]
    reg = [torch.randn(B, 240, h, w, generator=g) * 0.3 for h, w in levels]
    # teacher knowledge in the reference layout: 9 cells per image around the student's decode range
    t_scores = [torch.rand(9, 1, generator=g).expand(9, 8).contiguous() * 0.6 + 0.3 for _ in range(B)]
    t_kps = [torch.rand(9, 8, 2, generator=g) * torch.tensor([200.0, 150.0]) + torch.tensor([220.0, 160.0]) for _ in range(B)]
    t_kps[2] = t_kps[2][:0]; t_scores[2] = t_scores[2][:0]           # one image without teacher cells: skipped
    pred_t = {"post_kp_2d": torch.cat(t_kps), "post_kp_cls": torch.cat(t_scores), "post_pos_per_img": [len(s) for s in t_scores]}
    keys_ref = torch.rand(B * cells, generator=torch.Generator().manual_seed(4))

    def choose(vp, n, im, l, gt):
        off = im * cells + sum(counts[:l])
        return torch.argsort(keys_ref[off + vp], stable=True)[:n]

    # oracle
    cls_r = [c.clone().requires_grad_(True) for c in cls]
    reg_r = [r.clone().requires_grad_(True) for r in reg]
    labels, gt_idx, aux = O.ssc_assign(tds, levels, choose=choose)
    out = O.kd_pose_loss(cls_r, reg_r, tds, (t_scores, t_kps), INTERNAL_K, MESH_DIAMETERS, labels, gt_idx, aux)
    (out["loss_cls"] * 0.1 + out["loss_reg"] + out["loss_kd"] * 5.0).backward()
    # kd6d
    cfg_kd = dict(LOSS_WEIGHT_KD=5.0, LEVEL="pred", GLEVEL="point", GTYPE="sinkhorn", GP=2.0, GBLUR=0.001, GnD=2,
                  WEIGHTED_OT=True, DETACH=False, SCALING=0.5, REACH=0.5)

    class Coder:
        target_type = "3D"

    crit = KDPoseLoss(2.0, 0.25, [32, 64, 128, 256, 512], [8, 16, 32, 64, 128], "SSC", 10, 1.0, 9, INTERNAL_K,
                      MESH_DIAMETERS, Coder(), cfg_kd)
    crit.keys = keys_ref[ref_to_packed_rows(B, levels)].to(dev)
    cls_g = [c.clone().to(dev).requires_grad_(True) for c in cls]
    reg_g = [r.clone().to(dev).requires_grad_(True) for r in reg]
    tg = [t.to(dev) for t in targets]
    l_cls, l_reg, l_kd = crit(cls_g, reg_g, tg, None, {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in pred_t.items()})
    (l_cls * 0.1 + l_reg + l_kd * 5.0).backward()
    torch.cuda.synchronize()
    assert crit.pos_per_img == out["pos_per_img"] and crit.step == 1
    if mixed == "multi":
        assert max(out["pos_per_img"]) > 32, "the four-instance image must exceed the former 32 slots"
    assert float(out["loss_kd"]) > 0
    assert float(l_cls) == pytest.approx(float(out["loss_cls"]), rel=1e-4)
    assert float(l_reg) == pytest.approx(float(out["loss_reg"]), rel=1e-4)
    assert float(l_kd) == pytest.approx(float(out["loss_kd"]), rel=5e-4)
    for a_, b_ in zip(cls_g + reg_g, cls_r + reg_r):
        scale = max(float(b_.grad.abs().max()), 1e-12)
        torch.testing.assert_close(a_.grad.cpu(), b_.grad, rtol=5e-3, atol=5e-3 * scale)


# ======================================================================================================================
# Kernel-level tests of csrc/losses.hip: every entry point on its own, called the way kd_losses.py calls it, against the
# fp64 restatements of tests/loss_cases.py.  Discrete outputs are compared exactly (the restatements assert that the
# inputs sit on no knife edge); the bound of every continuous output is loss_cases.bound(name) -- 8 x the restatement's own
# fp32-vs-fp64 deviation, floor 4 fp32 ulps, relative to the output's largest magnitude: profiles/loss_kernel_tolerances.md.
# ======================================================================================================================
SENT_I, SENT_F = -7, -777.0


def _kd():
    from kd6d import _lib, ops
    from kd6d.kd_losses import PackedTargets, make_levels
    return _lib, ops, PackedTargets, make_levels


def _run_ssc(dev, sc, cap, positive_num=None):
    _lib, ops, PackedTargets, make_levels = _kd()
    lay = sc["layout"]
    B = lay.batch
    tgt = PackedTargets(sc["targets"], dev)
    lv = make_levels(B, sc["levels"])
    keys = torch.from_numpy(sc["keys"]).to(torch.float32).to(dev)
    i32 = dict(dtype=torch.int32, device=dev)
    labels, pos_cnt = torch.full((lay.rows,), SENT_I, **i32), torch.full((B,), SENT_I, **i32)
    pos_row, pos_gt = torch.full((B * cap,), SENT_I, **i32), torch.full((B * cap,), SENT_I, **i32)
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_ssc_assign(ctypes.byref(lv), P(tgt.mask), tgt.mask_h, tgt.mask_w, P(tgt.kp3d), P(tgt.K),
                                        P(tgt.class_ids), P(tgt.n_gt), P(tgt.rot), P(tgt.trans), P(tgt.bbox_trans), P(keys),
                                        float(positive_num or sc["positive_num"]), float(sc["positive_lambda"]), cap, P(labels),
                                        P(pos_cnt), P(pos_row), P(pos_gt), ops._stream()), "kd6d_ssc_assign")
    torch.cuda.synchronize()
    return labels.cpu().numpy(), pos_cnt.cpu().tolist(), pos_row.cpu().view(B, cap).tolist(), pos_gt.cpu().view(B, cap).tolist()


def _check_ssc(got, ref, cap):
    labels, cnt, rows, gts = got
    for b, pos in enumerate(ref["pos"]):
        n = len(pos)
        assert cnt[b] == n, ("pos_cnt", b, cnt[b], n, ref["picked"])
        assert rows[b][:n] == [r for r, _ in pos], ("pos_row", b)
        assert gts[b][:n] == [g for _, g in pos], ("pos_gt", b)
        assert rows[b][n:] == [SENT_I] * (cap - n) and gts[b][n:] == [SENT_I] * (cap - n), "slots beyond pos_cnt were written"
    np.testing.assert_array_equal(labels, ref["labels"])


@pytest.mark.parametrize("name", sorted(C.SSC_CASES))
def test_ssc_assign_kernel_equals_fp64_reference(gpu_device, name):
    """labels, pos_cnt, pos_row, pos_gt exactly: 0..4 instances mixed in one batch, 4 and 5 levels, square and 640x480
    level tables, positive_lambda 1 and 0.5, diagonal and general affine, odd / small / unaligned masks, a lone pixel in
    the scalar tail and beyond the unrolled block of the presence scan, an absent instance, one class twice."""
    from kd6d.kd_losses import POS_CAP
    sc = C.ssc_case(name)
    ref = C.ssc_reference(sc["targets"], sc["levels"], sc["keys"], sc["positive_num"], sc["positive_lambda"])
    assert max(ref["picked"]) <= POS_CAP
    _check_ssc(_run_ssc(gpu_device, sc, POS_CAP), ref, POS_CAP)


def test_ssc_assign_capacity_contract(gpu_device):
    """The four-instance image selects more than 32 cells (36 here; the reference keeps them all).  cap = 64 and the
    host's default capacity give the reference's positives; beyond the capacity (positive_num = 20: more than 64 picks)
    the documented truncation of include/kd6d.h holds: the cap smallest rows stay positive, the other picks stay -1."""
    from kd6d.kd_losses import POS_CAP
    sc = C.ssc_case(C.CAPACITY_CASE)
    ref = C.ssc_reference(sc["targets"], sc["levels"], sc["keys"])
    assert 32 < max(ref["picked"]) <= POS_CAP
    for cap in (64, POS_CAP):
        _check_ssc(_run_ssc(gpu_device, sc, cap), ref, cap)
    full = C.ssc_reference(sc["targets"], sc["levels"], sc["keys"], positive_num=20.0)
    assert max(full["picked"]) > 64
    for cap in (64, 32):
        cut = C.ssc_reference(sc["targets"], sc["levels"], sc["keys"], positive_num=20.0, cap=cap)
        assert int((cut["labels"] > 0).sum()) < int((full["labels"] > 0).sum())
        _check_ssc(_run_ssc(gpu_device, sc, cap, positive_num=20.0), cut, cap)


def _run_teacher(dev, c, cap, class_ids=None, n_gt=None):
    _lib, ops, _, make_levels = _kd()
    B = c["batch"]
    blocks = B if class_ids is None else B * 4
    n = blocks * cap
    lv = make_levels(B, c["levels"])
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    cls, reg, bt = c["cls"].to(dev), c["reg"].to(dev), c["bbox_trans"].contiguous().to(dev)
    out = dict(cnt=torch.full((blocks,), SENT_I, **i32), kp=torch.full((n, 8, 2), SENT_F, **f32),
               score=torch.full((n, 8), SENT_F, **f32), row=torch.full((n,), SENT_I, **i32),
               kp_norm=torch.full((n, 8, 2), SENT_F, **f32), beta=torch.full((n, 8), SENT_F, **f32))
    P = ops._ptr
    ids_d, ngt_d = (None, None) if class_ids is None else (class_ids.to(dev), n_gt.to(dev))     # kept alive over the launch
    if class_ids is None:
        _lib.check(_lib.lib.kd6d_teacher_select(ctypes.byref(lv), P(cls), P(reg), P(bt), c["th"], c["positive_num"],
                                                c["positive_lambda"], cap, C.FRAME_WH[0], C.FRAME_WH[1], P(out["cnt"]), P(out["kp"]),
                                                P(out["score"]), P(out["row"]), P(out["kp_norm"]), P(out["beta"]), ops._stream()),
                   "kd6d_teacher_select")
    else:
        _lib.check(_lib.lib.kd6d_pose_candidates(ctypes.byref(lv), P(cls), P(reg), P(bt), P(ids_d), P(ngt_d),
                                                 c["th"], c["positive_num"], c["positive_lambda"], cap, P(out["cnt"]), P(out["kp"]),
                                                 P(out["score"]), ops._stream()), "kd6d_pose_candidates")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check_teacher_block(got, o, cap, ref, what, with_ot=True, set_level=None):
    """Output block o (slots [o*cap, (o+1)*cap)) against one image's reference dict."""
    n = len(ref["rows"])
    assert int(got["cnt"][o]) == n == min(ref["emitted"], cap), (what, int(got["cnt"][o]), n)
    sl = slice(o * cap, o * cap + n)
    rest = slice(o * cap + n, (o + 1) * cap)
    for k in ("kp", "score") + (("kp_norm", "beta") if with_ot else ()):
        assert bool((got[k][rest] == SENT_F).all()), "%s: %s written beyond t_cnt" % (what, k)
    perm = list(range(n))
    if with_ot:
        assert bool((got["row"][rest] == SENT_I).all())
        rows = got["row"][sl].tolist()
        if set_level is None:
            assert rows == ref["rows"], (what, rows, ref["rows"])
        else:       # bit-equal scores inside the top-n of one level: the reference's order is unspecified there
            for l in set(ref["level"]):
                a = [r for r, q in zip(rows, ref["level"]) if q == l]
                b = [r for r, q in zip(ref["rows"], ref["level"]) if q == l]
                assert (a == b) if l != set_level else (sorted(a) == sorted(b)), (what, l, a, b)
            perm = [rows.index(r) for r in ref["rows"]]
    if n == 0:
        return
    idx = torch.tensor(perm) + o * cap
    C.assert_within(got["kp"][idx], ref["kp"], "t_kp", what)
    C.assert_within(got["score"][idx], ref["score"][:, None].expand(-1, 8), "t_score", what)
    if with_ot:
        C.assert_within(got["kp_norm"][idx], ref["kp_norm"], "t_kp_norm", what)
        C.assert_within(got["beta"][idx], ref["beta"][:, None].expand(-1, 8), "t_beta", what)


@pytest.mark.parametrize("name,tie", [(n, None) for n in sorted(C.TEACHER_CASES)]
                         + [(n, t) for n in ("c256_l5_diag", "full_640x480_l5_general") for t in ("inside", "straddle")])
def test_teacher_select_kernel_vs_fp64_reference(gpu_device, name, tie):
    """t_cnt / t_row exact (level ascending, score descending), t_kp / t_score / t_kp_norm / t_beta within their bounds,
    slots >= t_cnt untouched.  First class with cells is not class 0, two classes above threshold, an image with
    nothing above it, a level with fewer candidates than n_l, 4 and 5 levels, 640x480, general affine, cap below the
    emitted count; bit-equal scores inside the top-n_l (compared as a set) and straddling the cut-off (the smaller cell
    index wins -- block_argmax's documented rule)."""
    c = C.teacher_case(name, tie)
    ref = C.teacher_reference(c["cls"], c["reg"], c["batch"], c["levels"], c["bbox_trans"], c["th"], c["positive_num"],
                              c["positive_lambda"], c["cap"])
    if name == "cap5_c256_l5_general":
        assert all(r["emitted"] > c["cap"] for r in ref)
    got = _run_teacher(gpu_device, c, c["cap"])
    for b in range(c["batch"]):
        _check_teacher_block(got, b, c["cap"], ref[b], "%s image %d" % (name, b),
                             set_level=c["tie_level"] if (tie == "inside" and b == 0) else None)


def test_pose_candidates_kernel_vs_fp64_reference(gpu_device):
    """Every slot g < n_gt[b] gets exactly its own class; g >= n_gt[b], class ids -1 and 15 and a class without cells give
    cnt = 0; one class in two slots gives two identical blocks."""
    c = C.teacher_case("c128_l4_general")
    cap = 32
    class_ids = torch.tensor([[3, 7, 3, 0], [-1, 15, 0, 0], [0, 5, 0, 0]], dtype=torch.int32)
    n_gt = torch.tensor([3, 4, 2], dtype=torch.int32)
    got = _run_teacher(gpu_device, c, cap, class_ids, n_gt)
    emitted = []
    for g in range(4):
        class_of = [int(class_ids[b, g]) if g < int(n_gt[b]) else None for b in range(3)]
        ref = C.teacher_reference(c["cls"], c["reg"], 3, c["levels"], c["bbox_trans"], c["th"], c["positive_num"],
                                  c["positive_lambda"], cap, class_of=class_of)
        for b in range(3):
            _check_teacher_block(got, b * 4 + g, cap, ref[b], "image %d slot %d" % (b, g), with_ot=False)
            emitted.append(((b, g), ref[b]["emitted"]))
    emitted = dict(emitted)
    assert emitted[(0, 0)] > 0 and emitted[(0, 1)] > 0 and emitted[(2, 0)] > 0
    assert [k for k, v in emitted.items() if v > 0] == [(0, 0), (2, 0), (0, 1), (0, 2)]
    for k in ("kp", "score"):
        assert torch.equal(got[k][0:cap], got[k][2 * cap:3 * cap]), "the same class in two slots: identical blocks"


def _run_focal(dev, x, lab, gamma, alpha, dtype, weight):
    _lib, ops, _, _ = _kd()
    rows = x.shape[0]
    xg, lg = x.to(dev), lab.to(dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    ws = torch.zeros(8, dtype=torch.float32, device=dev)
    dcls = torch.full((rows, 16), float("nan"), dtype=dtype, device=dev)
    w = torch.tensor([weight], dtype=torch.float32, device=dev)
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_focal_fwd(P(xg), P(lg), rows, gamma, alpha, P(loss), P(ws), ops._stream()), "kd6d_focal_fwd")
    first = loss.clone()
    _lib.check(_lib.lib.kd6d_focal_fwd(P(xg), P(lg), rows, gamma, alpha, P(loss), P(ws), ops._stream()), "kd6d_focal_fwd")
    _lib.check(_lib.lib.kd6d_focal_bwd(ops.dt_code(dtype), P(xg), P(lg), rows, gamma, alpha, P(w), P(dcls), ops._stream()),
               "kd6d_focal_bwd")
    torch.cuda.synchronize()
    return first.cpu(), loss.cpu(), dcls.cpu()


def _check_focal(got, x, lab, ref_loss, ref_grad, weight, dtype, what):
    first, second, dcls = got
    C.assert_within(first, ref_loss.view(1), "loss_cls", what)
    C.assert_within(second, 2 * ref_loss.view(1), "loss_cls", what + " (workspace not re-zeroed: running total)")
    assert bool(torch.isfinite(dcls.float()).all()), "focal_bwd must write ALL of dcls"
    assert bool((dcls[:, 15] == 0).all()), "pad column"
    assert bool((dcls[lab < 0] == 0).all()), "ignored rows"
    zero = ref_grad == 0
    assert bool((dcls[:, :15][zero] == 0).all()), "saturated logits: the gradient is exactly 0"
    if dtype == torch.float32:
        C.assert_within(dcls[:, :15], ref_grad * weight, "dcls_focal", what)
    else:
        C.assert_bf16_within_one_ulp(dcls[:, :15], ref_grad * weight, what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,gamma,labels", C.FOCAL_CASES)
def test_focal_kernels_vs_fp64_reference(gpu_device, rows, gamma, labels, dtype):
    """Row counts off the 256-thread block, either side of the forward's 128-workgroup cap (2184 / 2185), beyond the
    backward's 2048-workgroup cap, the benchmark size (128 x 1364); labels in {-1, 0, 1..15} incl. all-ignored and
    all-background; a saturated share of logits; gamma 2 and 1.5; fp32 and bf16 dcls pre-filled with NaN."""
    x, lab = C.focal_inputs(rows, rows + 7, labels)
    ref_loss, ref_grad = C.focal_reference(x, lab, gamma, 0.25)
    if labels == "mixed" and rows >= 17:
        sat = (x[:, :15].abs() > 10) & (lab >= 0)[:, None]
        assert bool(sat.any()) and bool((ref_grad[sat] == 0).all())
    got = _run_focal(gpu_device, x, lab, gamma, 0.25, dtype, 0.125)
    _check_focal(got, x, lab, ref_loss, ref_grad, 0.125, dtype, "rows=%d gamma=%g %s" % (rows, gamma, labels))


def test_focal_kernels_vs_values_recorded_from_the_reference(gpu_device):
    """tests/golden/pieces.npz (loss and gradient recorded from the reference's SigmoidFocalLoss in fp32) through
    kd6d_focal_fwd / _bwd.  Against the fp64 restatement the usual bounds hold; the recorded fp32 values carry their own
    deviation (loss_cases.RECORDED_DEV) on top."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pieces.npz"))
    x = torch.nn.functional.pad(torch.from_numpy(z["focal_logits"]), (0, 1), value=50.0).contiguous()
    lab = torch.from_numpy(z["focal_labels"]).to(torch.int32)
    ref_loss, ref_grad = C.focal_reference(x, lab)
    got = _run_focal(gpu_device, x, lab, 2.0, 0.25, torch.float32, 1.0)
    _check_focal(got, x, lab, ref_loss, ref_grad, 1.0, torch.float32, "pieces.npz")
    rec_l, rec_g = float(z["focal_loss"]), torch.from_numpy(z["focal_grad"]).double()
    assert abs(float(got[0]) - rec_l) <= (C.bound("loss_cls") + C.RECORDED_DEV["loss_cls"]) * abs(rec_l)
    assert float((got[2][:, :15].double() - rec_g).abs().max()) <= \
        (C.bound("dcls_focal") + C.RECORDED_DEV["dcls_focal"]) * float(rec_g.abs().max())


def _slot_arrays(c, dev):
    B, cap = len(c["targets"]), c["cap"]
    cnt = torch.tensor([len(p) for p in c["pos"]], dtype=torch.int32)
    row = torch.zeros(B, cap, dtype=torch.int32)
    gt = torch.zeros(B, cap, dtype=torch.int32)
    for b, p in enumerate(c["pos"]):
        for s, (r, g) in enumerate(p):
            row[b, s], gt[b, s] = r, g
    return cnt.to(dev), row.view(-1).to(dev), gt.view(-1).to(dev)


@pytest.mark.parametrize("name", sorted(C.STUDENT_CASES))
def test_student_points_kernel_vs_fp64_reference(gpu_device, name):
    """xs, alpha, g_reg_xy, loss_reg, s_start: positives of one image from different instances and classes (own
    rotation / translation / diameter per slot), general affine, images without positives, cells on every level, both
    smooth-L1 branches (>= 10 % each, none within 1e-3 of |diff| = 1), logits on both alpha clamps."""
    _lib, ops, PackedTargets, make_levels = _kd()
    from kd6d.synthetic import MESH_DIAMETERS
    dev = gpu_device
    c = C.student_case(name)
    B, cap = len(c["targets"]), c["cap"]
    ref = C.student_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], cap)
    assert 0.1 <= ref["quad_share"] <= 0.9 and ref["branch_gap"] >= 1e-3
    assert float(ref["sigmoid"].min()) < 1e-3 and float(ref["sigmoid"].max()) > 1 - 1e-3
    assert len({int(l) for l in ref["level"]}) == len(c["levels"])
    tgt = PackedTargets(c["targets"], dev)
    lv = make_levels(B, c["levels"])
    cnt, row, gt = _slot_arrays(c, dev)
    n = B * cap
    f32 = dict(dtype=torch.float32, device=dev)
    xs, alpha, g_reg = torch.zeros(n, 8, 2, **f32), torch.zeros(n, 8, **f32), torch.zeros(n, 8, 2, **f32)
    loss, ws = torch.full((1,), float("nan"), **f32), torch.zeros(8, **f32)
    s_start = torch.full((B,), SENT_I, dtype=torch.int32, device=dev)
    dia = torch.tensor(MESH_DIAMETERS, **f32)
    kinv = (ctypes.c_float * 9)(*C.kinv_f32().reshape(-1).tolist())
    cls, reg = c["cls"].to(dev), c["reg"].to(dev)
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_student_points(ctypes.byref(lv), P(cls), P(reg), P(cnt), P(row), P(gt), P(tgt.class_ids), P(tgt.kp3d),
                                            P(tgt.rot), P(tgt.trans), P(tgt.bbox_trans), P(dia), kinv, C.FRAME_WH[0], C.FRAME_WH[1],
                                            cap, P(xs), P(alpha), P(g_reg), P(loss), P(ws), P(s_start), ops._stream()),
               "kd6d_student_points")
    torch.cuda.synchronize()
    assert s_start.cpu().tolist() == [b * cap for b in range(B)]
    C.assert_within(xs, ref["xs"], "xs", name)
    C.assert_within(alpha, ref["alpha"], "alpha", name)
    C.assert_within(g_reg, ref["g_reg_xy"], "g_reg_xy", name)
    C.assert_within(loss, ref["loss_reg"].view(1), "loss_reg", name)
    lo, hi = ref["sigmoid"] < 1e-3, ref["sigmoid"] > 1 - 1e-3
    a0 = alpha.cpu()[ref["slot"], 0]
    one, eps = torch.tensor(1.0, dtype=torch.float32), torch.tensor(1e-3, dtype=torch.float32)
    assert bool((a0[lo] == eps).all()) and bool((a0[hi] == one - eps).all()), "the clamp values themselves"


def test_kd_mean_kernel(gpu_device):
    """All valid, some invalid, none valid (loss_kd = 0, n_valid = 0), a -1 (oversize) entry."""
    _lib, ops, _, _ = _kd()
    dev = gpu_device
    g = torch.Generator().manual_seed(3)
    li = torch.rand(16, generator=g) * 3.0
    for valid in ([1] * 16, [1, 0] * 8, [0] * 16, [1, -1, 0, 1] * 4, [-1] * 16):
        v = torch.tensor(valid, dtype=torch.int32)
        out = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
        nv = torch.full((1,), SENT_I, dtype=torch.int32, device=dev)
        li_d, v_d = li.to(dev), v.to(dev)
        _lib.check(_lib.lib.kd6d_kd_mean(ops._ptr(li_d), ops._ptr(v_d), 16, ops._ptr(out), ops._ptr(nv), ops._stream()),
                   "kd6d_kd_mean")
        torch.cuda.synchronize()
        want, n = C.kd_mean_reference(li, v)
        assert int(nv) == n
        C.assert_within(out, torch.tensor([want]), "loss_kd", str(valid[:4]))
        if n == 0:
            assert float(out) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("variant", range(len(C.BACKWARD_VARIANTS)),
                         ids=["detach%d-seg_%s-valid_%s" % (v["detach"], v["seg"], v["valid"]) for v in C.BACKWARD_VARIANTS])
@pytest.mark.parametrize("name", sorted(C.STUDENT_CASES))
def test_loss_backward_kernel_vs_fp64_autograd(gpu_device, name, variant, dtype):
    """dreg (positive rows only, everything else still 0), dcls += on top of a non-zero dcls (bit-identical with
    detach_alpha = 1 and on alpha-clamped cells), dseg_scale through planar accumulators; seg_scale NULL / given / given
    without accumulators; n_valid = 0, one image invalid; general affine, multi-instance.  Reference: autograd in double
    of w_reg * loss_reg + (w_kd / n_valid) * sum_valid(<g_xs, xs> + <g_alpha, alpha>) with seeded upstream arrays."""
    _lib, ops, PackedTargets, make_levels = _kd()
    dev = gpu_device
    v = C.BACKWARD_VARIANTS[variant]
    c = C.student_case(name)
    B, cap = len(c["targets"]), c["cap"]
    n = B * cap
    up = C.upstream_grads(n, 5)
    valid = C.valid_pattern(v["valid"], B)
    seg = None if v["seg"] is None else torch.tensor(C.SEG_SCALE)
    ref = C.student_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], cap, upstream=up,
                              weights=C.BACKWARD_WEIGHTS, valid=valid, detach_alpha=bool(v["detach"]), seg_scale=seg)
    tgt = PackedTargets(c["targets"], dev)
    lv = make_levels(B, c["levels"])
    cnt, row, gt = _slot_arrays(c, dev)
    rows = c["cls"].shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(17)
    dcls_in = (torch.randn(rows, 16, generator=g) * 0.01).to(dtype)
    dcls = dcls_in.clone().to(dev)
    dreg = torch.zeros(rows, 240, dtype=dtype, device=dev)
    acc = ops.planar_acc(5, dev) if v["seg"] == "grad" else None
    weights = torch.tensor(C.BACKWARD_WEIGHTS, **f32)
    n_valid = torch.tensor([int((valid > 0).sum())], dtype=torch.int32, device=dev)
    cls, reg = c["cls"].to(dev), c["reg"].to(dev)
    g_reg = ref["g_reg_xy"].to(torch.float32).to(dev)
    gxs_d, gal_d, valid_d = up[0].to(dev), up[1].to(dev), valid.to(dev)                       # kept alive over the launch
    seg_d = None if seg is None else seg.to(dev)
    acc_lo = None if acc is None else acc[:5]
    P = ops._ptr
    _lib.check(_lib.lib.kd6d_loss_backward(ctypes.byref(lv), ops.dt_code(dtype), P(cls), P(reg), P(cnt), P(row), P(gt),
                                           P(tgt.class_ids), P(tgt.bbox_trans), P(g_reg), P(gxs_d), P(gal_d),
                                           P(n_valid), P(valid_d), P(weights), P(seg_d),
                                           P(acc_lo), 5 if acc is not None else 0, C.FRAME_WH[0],
                                           C.FRAME_WH[1], cap, int(v["detach"]), P(dcls), P(dreg), ops._stream()),
               "kd6d_loss_backward")
    torch.cuda.synchronize()
    what = "%s %s" % (name, v)
    rr, cc = ref["rows"], ref["cls_of"]
    cols = cc[:, None] * 16 + torch.arange(16)[None]
    dreg_c, dcls_c = dreg.cpu(), dcls.cpu()
    touched = torch.zeros(rows, 240, dtype=torch.bool)
    touched[rr[:, None], cols] = True
    assert bool((dreg_c[~touched] == 0).all()), "dreg written outside the positive rows' own class"
    if dtype == torch.float32:
        C.assert_within(dreg_c[rr[:, None], cols], ref["draw"], "dreg", what)
    else:
        C.assert_bf16_within_one_ulp(dreg_c[rr[:, None], cols], ref["draw"], what + " dreg")
    # dcls: += on the positive cells' own class, everything else bit-identical to its input
    hit = torch.zeros(rows, 16, dtype=torch.bool)
    hit[rr, cc] = True
    assert torch.equal(dcls_c[~hit], dcls_in[~hit]), "dcls changed outside the positive cells"
    clamped = (ref["sigmoid"] < 1e-3) | (ref["sigmoid"] > 1 - 1e-3)
    assert bool(clamped.any()) and bool((ref["dz"][clamped] == 0).all())
    assert torch.equal(dcls_c[rr, cc][clamped], dcls_in[rr, cc][clamped]), "alpha-clamped cells contribute nothing"
    if v["detach"]:
        assert torch.equal(dcls_c, dcls_in), "detach_alpha = 1: dcls must be bit-identical to its input"
    else:
        base = dcls_in[rr, cc].double()
        want = base + ref["dz"]
        if v["valid"] != "none":
            assert float(ref["dz"].abs().max()) > 0
        if dtype == torch.float32:
            # the kernel stores fp32(in + delta): the bound on delta plus half an fp32 ulp of the stored sum
            err = float((dcls_c[rr, cc].double() - want).abs().max())
            tol = C.bound("dcls_kd") * float(ref["dz"].abs().max()) + 2.0 ** -24 * float(want.abs().max())
            print("  dcls_kd    %-40s max|err| %.3e  tol %.3e" % (what, err, tol))
            assert err <= tol, (what, err, tol)
        else:
            got = dcls_c[rr, cc].double()
            mag = torch.maximum(want.abs(), torch.maximum(base.abs(), ref["dz"].abs()))
            ulp = 2.0 ** (torch.floor(torch.log2(mag.clamp_min(1e-30))) - 7)
            assert bool(((got - want.to(torch.bfloat16).double()).abs() <= ulp).all()), what + " dcls (bf16)"
    if acc is not None:
        C.assert_within(ops.planar_acc_value(acc).cpu(), ref["dscale"], "dseg_scale", what)
        assert float(ref["dscale"].abs().max()) > 0
