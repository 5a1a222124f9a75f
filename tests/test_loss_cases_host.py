"""CPU: the fp64 restatements of tests/loss_cases.py (the references of the kernel-level GPU tests in
tests/test_losses_gpu.py) agree with the fp32 oracle pinned by the goldens and with the values recorded from the
reference itself (tests/golden/pieces.npz), on single-instance cases and on the multi-instance / general-affine /
odd-mask cases; running them also asserts the knife-edge conditions of every seeded case."""
import os

import numpy as np
import pytest
import torch

import loss_cases as C
from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS, make_batch
from oracle import kd_step_ref as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _oracle_ssc(sc, image):
    """O.ssc_assign on ONE image of an ssc case with the case's keys -> labels in packed order of that image's rows."""
    lay, levels = sc["layout"], sc["levels"]
    keys = torch.from_numpy(sc["keys"])
    offs = [sum(lay.hw[:l]) for l in range(len(levels))]

    def choose(vp, n, im, l, g):
        rows = torch.tensor([lay.row(l, image, int(c)) for c in vp], dtype=torch.long)
        return torch.argsort(keys[rows], stable=True)[:n]

    lab, gidx, aux = O.ssc_assign([sc["targets"][image].as_dict()], levels, sc["positive_num"], sc["positive_lambda"], choose)
    return lab[0], gidx[0], aux[0], offs


@pytest.mark.parametrize("name", sorted(C.SSC_CASES))
def test_ssc_reference_matches_oracle(name):
    sc = C.ssc_case(name)
    lay = sc["layout"]
    ref = C.ssc_reference(sc["targets"], sc["levels"], sc["keys"], sc["positive_num"], sc["positive_lambda"])
    for b, t in enumerate(sc["targets"]):
        mine = np.concatenate([ref["labels"][lay.row(l, b, 0):lay.row(l, b, 0) + lay.hw[l]] for l in range(len(sc["levels"]))])
        if len(t.class_ids) == 0:
            assert (mine == 0).all() and ref["pos"][b] == []
            continue
        lab, gidx, _, _ = _oracle_ssc(sc, b)
        np.testing.assert_array_equal(mine, lab.numpy())
        assert ref["picked"][b] == int((lab > 0).sum()) == len(ref["pos"][b])
        for row, g in ref["pos"][b]:
            l, _, cell = lay.locate(row)
            assert int(gidx[sum(lay.hw[:l]) + cell]) == g


def test_capacity_case_exceeds_the_former_32_slots():
    sc = C.ssc_case(C.CAPACITY_CASE)
    ref = C.ssc_reference(sc["targets"], sc["levels"], sc["keys"])
    assert max(ref["picked"]) > 32 and max(ref["picked"]) <= 48
    from kd6d.kd_losses import POS_CAP, KDLoss, positives_bound
    assert POS_CAP == positives_bound(10) == 48
    assert KDLoss(INTERNAL_K, MESH_DIAMETERS).cap == 48
    assert KDLoss(INTERNAL_K, MESH_DIAMETERS, positive_num=13).cap == 60
    with pytest.raises(ValueError, match="64 slots"):
        KDLoss(INTERNAL_K, MESH_DIAMETERS, positive_num=15)
    with pytest.raises(ValueError, match="truncate"):
        KDLoss(INTERNAL_K, MESH_DIAMETERS, cap=32)


def _unpack(x, lay):
    """packed (rows, C) -> per-level (B, C, h, w) lists, the oracle's input."""
    out = []
    for l, (h, w) in enumerate(lay.levels):
        blk = x[lay.row0[l]:lay.row0[l] + lay.batch * lay.hw[l]]
        out.append(blk.view(lay.batch, h, w, -1).permute(0, 3, 1, 2).contiguous())
    return out


@pytest.mark.parametrize("name", sorted(C.TEACHER_CASES))
def test_teacher_reference_matches_oracle(name):
    c = C.teacher_case(name)
    lay = C.Layout(c["batch"], c["levels"])
    ref = C.teacher_reference(c["cls"], c["reg"], c["batch"], c["levels"], c["bbox_trans"], c["th"], c["positive_num"],
                              c["positive_lambda"], cap=64)
    sc, kp = O.teacher_select(_unpack(c["cls"][:, :15], lay), _unpack(c["reg"], lay), c["bbox_trans"], c["th"],
                              c["positive_num"], c["positive_lambda"])
    for b in range(c["batch"]):
        assert sc[b].shape[0] == ref[b]["emitted"]
        if ref[b]["emitted"]:
            torch.testing.assert_close(sc[b][:, 0].double(), ref[b]["score"], rtol=1e-5, atol=0)
            torch.testing.assert_close(kp[b].double(), ref[b]["kp"], rtol=1e-4, atol=1e-3)


def test_single_instance_teacher_and_ssc_match_oracle_on_make_batch():
    """The G = 1 / diagonal-affine generator the oracle is pinned on (kd6d.synthetic.make_batch)."""
    B, crop = 2, 128
    levels = C.level_shapes(crop, crop, 4)
    lay = C.Layout(B, levels)
    _, targets = make_batch(B, 77, crop=crop, mixed_classes=True)
    sc = dict(targets=targets, levels=levels, layout=lay, keys=C.make_keys(lay.rows, 5), positive_num=10.0, positive_lambda=1.0)
    ref = C.ssc_reference(targets, levels, sc["keys"])
    for b in range(B):
        lab, _, _, _ = _oracle_ssc(sc, b)
        mine = np.concatenate([ref["labels"][lay.row(l, b, 0):lay.row(l, b, 0) + lay.hw[l]] for l in range(4)])
        np.testing.assert_array_equal(mine, lab.numpy())


def test_focal_reference_matches_pieces_and_oracle():
    z = np.load(os.path.join(G, "pieces.npz"))
    x = torch.nn.functional.pad(torch.from_numpy(z["focal_logits"]), (0, 1))
    lab = torch.from_numpy(z["focal_labels"])
    loss, grad = C.focal_reference(x, lab)
    assert float(loss) == pytest.approx(float(z["focal_loss"]), rel=1e-5)
    np.testing.assert_allclose(grad.numpy(), z["focal_grad"], rtol=2e-3, atol=1e-6)
    for rows, gamma, labels in C.FOCAL_CASES[:-1]:
        x, lab = C.focal_inputs(rows, rows + 7, labels)
        loss, grad = C.focal_reference(x, lab, gamma)
        keep = lab >= 0
        xr = x[:, :15].clone().requires_grad_(True)
        o = O.focal_loss_sum(xr[keep], lab[keep].long(), gamma=gamma)
        assert float(o.detach()) == pytest.approx(float(loss), rel=1e-4, abs=1e-12)
        if keep.any():
            o.backward()
            np.testing.assert_allclose(xr.grad.numpy(), grad.numpy(), rtol=2e-3, atol=2e-6)
        sat = (x[:, :15].abs() > 10) & keep[:, None]
        assert bool((grad[sat] == 0).all()) and bool((grad[~keep] == 0).all())


@pytest.mark.parametrize("name", ["mixed_c256_l5_general", "full_640x480_l5_general_lam05"])
@pytest.mark.parametrize("detach", [False, True])
def test_student_reference_matches_oracle_kd_pose_loss(name, detach):
    """student_reference (values and the chain into the logits) vs O.kd_pose_loss with a stub OT that is linear in
    (xs, alpha): <g_xs, xs> + <g_alpha, alpha> per image."""
    c = C.student_case(name, every_level=False)
    targets, levels, cap = c["targets"], c["levels"], c["cap"]
    B = len(targets)
    lay = C.Layout(B, levels)
    up = C.upstream_grads(B * cap, 5)
    ref = C.student_reference(c["cls"], c["reg"], targets, levels, c["pos"], cap, upstream=up, weights=C.BACKWARD_WEIGHTS,
                              valid=torch.ones(B, dtype=torch.int32), detach_alpha=detach)
    assert 0.1 <= ref["quad_share"] <= 0.9 and ref["branch_gap"] >= 1e-3
    assert float(ref["sigmoid"].min()) < 1e-3 and float(ref["sigmoid"].max()) > 1 - 1e-3
    assert float(((ref["sigmoid"] - 1e-3).abs().min())) > 1e-5 and float(((ref["sigmoid"] - (1 - 1e-3)).abs().min())) > 1e-5
    # oracle inputs: labels / gt index / 3D points from O.ssc_assign with the same picks
    sc = C.ssc_case(name)
    labs, gids, auxs = [], [], []
    for b in range(B):
        lab, gidx, aux, _ = _oracle_ssc(sc, b)
        labs.append(lab); gids.append(gidx); auxs.append(aux)
    cls_r = [t.requires_grad_(True) for t in _unpack(c["cls"][:, :15], lay)]
    reg_r = [t.requires_grad_(True) for t in _unpack(c["reg"], lay)]
    calls = []

    def ot(al, xs, be, ys, blur, scaling, reach):
        b = len(calls)
        calls.append(b)
        n = al.shape[1]
        gx = up[0][b * cap:b * cap + n].transpose(0, 1)
        ga = up[1][b * cap:b * cap + n].transpose(0, 1)
        return (gx * xs).sum((1, 2)) + (ga * al).sum(1)

    teacher = ([torch.full((1, 8), 0.5)] * B, [torch.zeros(1, 8, 2)] * B)
    out = O.kd_pose_loss(cls_r, reg_r, [t.as_dict() for t in targets], teacher, INTERNAL_K, MESH_DIAMETERS, torch.stack(labs),
                         torch.stack(gids), torch.stack(auxs), kd=dict(blur=0.001, scaling=0.5, reach=0.5, weighted=True, detach=detach),
                         ot_fn=ot)
    assert out["pos_per_img"] == [len(p) for p in c["pos"]] and len(calls) == B
    (out["loss_reg"] * C.BACKWARD_WEIGHTS[1] + out["loss_kd"] * C.BACKWARD_WEIGHTS[2]).backward()
    assert float(out["loss_reg"]) == pytest.approx(float(ref["loss_reg"]), rel=1e-4)
    frame = torch.tensor(C.FRAME_WH, dtype=torch.float64)
    torch.testing.assert_close(out["student_pts"].double(), ref["xs"][ref["slot"]] * frame, rtol=1e-4, atol=2e-3)
    torch.testing.assert_close(out["alpha_cell"].double(), ref["alpha"][ref["slot"], 0], rtol=1e-5, atol=1e-7)
    # gradients, in the packed layout
    def pack(per_level):
        return torch.cat([(torch.zeros_like(t) if t.grad is None else t.grad).permute(0, 2, 3, 1).reshape(-1, t.shape[1])
                          for t in per_level]).double()
    dcls, dreg = pack(cls_r), pack(reg_r)
    want_reg = torch.zeros_like(dreg)
    cols = ref["cls_of"][:, None] * 16 + torch.arange(16)[None]
    want_reg[ref["rows"][:, None], cols] = ref["draw"]
    want_cls = torch.zeros_like(dcls)
    want_cls[ref["rows"], ref["cls_of"]] = ref["dz"]
    torch.testing.assert_close(dreg, want_reg, rtol=5e-3, atol=5e-3 * float(want_reg.abs().max()))
    torch.testing.assert_close(dcls, want_cls, rtol=5e-3, atol=5e-3 * max(float(want_cls.abs().max()), 1e-12))
    if detach:
        assert float(want_cls.abs().max()) == 0.0


def test_every_student_case_has_both_branches_and_both_clamps():
    for name in C.STUDENT_CASES:
        c = C.student_case(name)
        ref = C.student_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], c["cap"])
        assert 0.1 <= ref["quad_share"] <= 0.9 and ref["branch_gap"] >= 1e-3, (name, ref["quad_share"], ref["branch_gap"])
        assert float(ref["sigmoid"].min()) < 1e-3 and float(ref["sigmoid"].max()) > 1 - 1e-3
        assert len({int(x) for x in ref["level"]}) == len(c["levels"]), "positives on every level"
        multi = [b for b, p in enumerate(c["pos"]) if len({g for _, g in p}) > 1]
        assert multi, "an image whose positives belong to different instances"


def test_tie_cases_can_be_built():
    for name in ("c256_l5_diag", "full_640x480_l5_general"):
        for tie in ("inside", "straddle"):
            c = C.teacher_case(name, tie)
            C.teacher_reference(c["cls"], c["reg"], c["batch"], c["levels"], c["bbox_trans"], cap=c["cap"])


def test_recorded_deviations_are_current():
    """The fp32-vs-fp64 deviations the GPU bounds are derived from (profiles/loss_kernel_tolerances.md) are what the
    restatements give now; the bounds stay tighter than the end-to-end test's (1e-4 on losses, 5e-3 on gradients)."""
    dev = C.measure_deviations()
    assert sorted(dev) == sorted(C.RECORDED_DEV)
    for k, v in dev.items():
        assert v <= C.RECORDED_DEV[k] * 1.001 + 1e-12, (k, v, C.RECORDED_DEV[k])
    for k in ("loss_cls", "loss_reg", "loss_kd"):
        assert C.bound(k) <= 1e-4
    for k in ("dreg", "dcls_kd", "dcls_focal", "dseg_scale", "g_reg_xy"):
        assert C.bound(k) <= 5e-3
