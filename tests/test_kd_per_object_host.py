"""CPU: the host side of the per-object KD term (--kd_per_object): flags, refusals, multi-instance synthetic batches,
the fp64 restatement (tests/kd_object_cases.py) and the recorded tolerances of the chained gradients."""
import hashlib
import os

import numpy as np
import pytest
import torch

import kd_object_cases as K
import loss_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "ape.yaml")
BASE = ["--config_file", YAML, "--config_file_t", YAML]
KD_DEFAULT = dict(LOSS_WEIGHT_KD=5.0, LEVEL="pred", GLEVEL="point", GTYPE="sinkhorn", GP=2.0, GBLUR=0.001, GnD=2,
                  WEIGHTED_OT=True, DETACH=False, SCALING=0.5, REACH=0.5)


def test_flags_exist_and_default_off():
    from kd6d.arguments.argument_kd import get_argparser, get_args
    d = get_argparser().parse_args([])
    assert d.kd_per_object is False and d.synthetic_instances == 1
    cfg, cfg_t = get_args(BASE)
    assert cfg["KD"] == KD_DEFAULT and "PER_OBJECT" not in cfg_t["KD"]
    assert cfg["RUNTIME"]["SYNTHETIC_INSTANCES"] == 1
    cfg, cfg_t = get_args(BASE + ["--kd_per_object", "--synthetic_instances", "3"])
    assert cfg["KD"] == dict(KD_DEFAULT, PER_OBJECT=True) and cfg_t["KD"]["PER_OBJECT"] is True
    assert cfg["RUNTIME"]["SYNTHETIC_INSTANCES"] == 3
    for bad in ("0", "5"):
        with pytest.raises(SystemExit):
            get_argparser().parse_args(["--synthetic_instances", bad])


def test_pnp_gate_combination_is_refused():
    from kd6d.arguments.argument_kd import get_args
    from kd6d.kd_losses import PER_OBJECT_GATE_ERROR
    with pytest.raises(SystemExit) as e:
        get_args(BASE + ["--kd_per_object", "--teacher_pnp_gate"])
    assert str(e.value) == PER_OBJECT_GATE_ERROR and "--teacher_pnp_gate" in PER_OBJECT_GATE_ERROR
    # ... and by the module itself, for callers that build cfg by hand
    from kd6d import backbone as BB
    from kd6d.models.model_kd import PoseModuleKD
    cfg, _ = get_args(BASE + ["--kd_per_object"])
    cfg["RUNTIME"]["TEACHER_PNP_GATE"] = True
    with pytest.raises(ValueError, match="teacher_pnp_gate"):
        PoseModuleKD(cfg, BB.darknet_tiny_h())


def test_module_and_loss_carry_the_mode():
    from kd6d import backbone as BB
    from kd6d.arguments.argument_kd import get_args
    from kd6d.kd_losses import CAP, KDLoss, MAX_GT, TeacherKnowledge, teacher_flat_sizes, teacher_flats
    from kd6d.models.model_kd import PoseModuleKD
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    cfg, _ = get_args(BASE)
    m = PoseModuleKD(cfg, BB.darknet_tiny_h())
    assert m.kd_per_object is False and m.loss_evaluator.per_object is False
    cfg, _ = get_args(BASE + ["--kd_per_object"])
    m = PoseModuleKD(cfg, BB.darknet_tiny_h())
    assert m.kd_per_object is True and m.loss_evaluator.per_object is True
    assert KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg={"PER_OBJECT": True}).per_object
    # workspace and teacher buffer sizes: the default layout is untouched, per-object appends / multiplies
    a, b = KDLoss(INTERNAL_K, MESH_DIAMETERS), KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg={"PER_OBJECT": True})
    n = 16 * a.cap
    assert a._ws_sizes(16) == (8 + 16 + n * 64 + 16, 3 * 16 + 4 + 2 * n)
    assert b._ws_sizes(16) == (a._ws_sizes(16)[0] + n * 48 + 64, a._ws_sizes(16)[1] + 3 * 64 + n)
    assert teacher_flat_sizes(16) == (16 * CAP * 48, 16 * CAP + 16)
    assert teacher_flat_sizes(16, per_object=True) == (64 * CAP * 48, 64 * CAP + 64)
    wf, wi = teacher_flats(3, "cpu", per_object=True)
    tk = TeacherKnowledge.from_flats(wf, wi, 3, CAP, per_object=True)
    assert tk.per_object and tk.blocks == 3 * MAX_GT and tk.t_cnt.numel() == 12 and tk.t_kp.shape == (12 * CAP, 8, 2)
    assert tk.t_start.tolist() == [o * CAP for o in range(12)]
    assert tk.clone_static().per_object and tk.clone_static().t_cnt.numel() == 12
    with pytest.raises(AssertionError):
        TeacherKnowledge.from_flats(wf, wi, 3, CAP)               # buffers of the other layout
    views = TeacherKnowledge.group_views(*teacher_flats(6, "cpu", per_object=True), 3, 2, CAP, per_object=True)
    assert len(views) == 3 and all(v.t_cnt.numel() == 8 and v.t_row.numel() == 8 * CAP for v in views)


def test_reference_dict_pred_t_is_refused_per_object():
    """KDPoseLoss(cfg_kd PER_OBJECT): the reference's pred_t dict has no object axis (checked before any device work)."""
    from kd6d.kd_losses import CAP, TeacherKnowledge, teacher_flats
    from kd6d.losses import KDPoseLoss
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    kd = dict(KD_DEFAULT, PER_OBJECT=True)
    L = KDPoseLoss(2.0, 0.25, C.SIZES, C.STRIDES, "SSC", 10, 1.0, 0, INTERNAL_K, MESH_DIAMETERS, None, kd)
    assert L.per_object and L.impl.per_object
    ref_dict = {"post_kp_2d": torch.zeros(0, 8, 2), "post_kp_cls": torch.zeros(0, 8), "post_pos_per_img": [0]}
    per_image = TeacherKnowledge.from_flats(*teacher_flats(1, "cpu"), 1, CAP)
    for bad in (ref_dict, per_image):
        with pytest.raises(TypeError, match="object axis"):
            L._check_pred_t(bad)
    L._check_pred_t(None)
    L._check_pred_t(TeacherKnowledge.from_flats(*teacher_flats(1, "cpu", per_object=True), 1, CAP, per_object=True))
    assert not KDPoseLoss(2.0, 0.25, C.SIZES, C.STRIDES, "SSC", 10, 1.0, 0, INTERNAL_K, MESH_DIAMETERS, None, KD_DEFAULT).per_object


def _batch_hash(B, seed, **kw):
    from kd6d.synthetic import make_batch
    im, tg = make_batch(B, seed, **kw)
    m = hashlib.sha256()
    m.update(im.tensors.numpy().tobytes())
    for a in tg:
        for x in (a.keypoints_3d, a.K, a.mask, a.class_ids, a.rotations, a.translations, a.bbox_scale, a.bbox_trans):
            m.update(x.numpy().tobytes())
    return m.hexdigest()


# sha256 over the image tensor and every target field, taken on the commit BEFORE make_batch learnt `instances`
PARENT_HASHES = {
    (3, 7, (("crop", 64),)): "8d0be015a3712f1ee561614c4bf583e078d61f6f940811c729ecb82acc2d073f",
    (2, 1, (("crop", 64), ("mixed_classes", True), ("class_offset", 5))):
        "ad60b55e6403ca3d22ea6e736bf9897be4b6cdbc9f17831b9a4256993202f493",
    (1, 2, (("full_frame", True),)): "0e62aa10e660022d8086a8a7807ceea5296536642a1d3631c65cf8b0236e9905",
}


def test_make_batch_single_instance_is_bit_identical_to_the_parent():
    for (B, seed, kw), want in PARENT_HASHES.items():
        assert _batch_hash(B, seed, **dict(kw)) == want
        assert _batch_hash(B, seed, instances=1, **dict(kw)) == want


@pytest.mark.parametrize("N", [2, 3, 4])
@pytest.mark.parametrize("mixed", [False, True])
def test_make_batch_multi_instance(N, mixed):
    from kd6d.kd_losses import PackedTargets
    from kd6d.synthetic import LINEMOD_CLASSES, batch_classes, make_batch, teacher_cls_bias
    im, tg = make_batch(5, 9, crop=128, instances=N, mixed_classes=mixed)
    im2, tg2 = make_batch(5, 9, crop=128, instances=N, mixed_classes=mixed)
    assert torch.equal(im.tensors, im2.tensors) and im.tensors.shape == (5, 3, 128, 128)
    bias = teacher_cls_bias(N, mixed)
    assert len(bias) == 15
    for i, (t, u) in enumerate(zip(tg, tg2)):
        assert torch.equal(t.mask, u.mask) and torch.equal(t.rotations, u.rotations)
        cls = t.class_ids.tolist()
        assert len(cls) == N == len(set(cls)) and all(c in LINEMOD_CLASSES for c in cls)
        assert cls == batch_classes(i, N, mixed)
        assert all(bias[c] == 1.0 for c in cls)
        assert t.rotations.shape == (N, 3, 3) and t.translations.shape == (N, 3, 1) and t.mask.shape == (128, 128)
        ids = sorted(set(t.mask.unique().tolist()) - {0.0})
        assert ids == [float(g + 1) for g in range(N)]
        cols = [set(torch.nonzero((t.mask == g + 1).any(0)).view(-1).tolist()) for g in range(N)]
        for g in range(N):                        # disjoint masks: every instance owns its own vertical strip
            for h in range(g + 1, N):
                assert not (cols[g] & cols[h])
        R = t.rotations[0]
        assert torch.allclose(R @ R.T, torch.eye(3), atol=1e-5) and float(torch.det(R)) > 0
    pk = PackedTargets(tg, "cpu")
    assert pk.n_gt.tolist() == [N] * 5
    assert sum(1 for b in teacher_cls_bias(1, False) if b == 1.0) == 1 and teacher_cls_bias(1, False)[0] == 1.0
    with pytest.raises(ValueError):
        make_batch(1, 0, instances=5)


def test_group_reference_is_a_stable_partition():
    cnt = [5, 0, 3]
    gt = np.zeros((3, 8), np.int64)
    gt[0, :5] = [2, 0, 2, 1, 0]
    gt[2, :3] = [3, 3, 7]
    start, num, dest = K.group_reference(cnt, gt.reshape(-1), 3, 8)
    assert dest[:5].tolist() == [3, 0, 4, 2, 1] and (dest[5:16] == -1).all()
    assert start[:4].tolist() == [0, 2, 3, 5] and num[:4].tolist() == [2, 1, 2, 0]
    assert num[4:8].tolist() == [0, 0, 0, 0] and start[4:8].tolist() == [8] * 4
    assert dest[16:19].tolist() == [16, 17, 18] and num[8:12].tolist() == [0, 0, 0, 2]     # gt 7: behind the last object


def test_per_object_restatement_reduces_to_per_image_on_single_instance_batches():
    c = K.single_instance_case()
    args = (c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], c["cap"])
    t_obj = K.teacher_objects(c["tcls"], c["treg"], c["targets"], c["levels"])
    t_img = K.teacher_images(c["tcls"], c["treg"], c["targets"], c["levels"])
    for b in range(len(c["targets"])):
        assert t_obj[b * K.MAX_GT]["rows"] == t_img[b]["rows"] and len(t_img[b]["rows"]) > 0
        assert all(len(t_obj[b * K.MAX_GT + g]["rows"]) == 0 for g in range(1, K.MAX_GT))
    a = K.kd_reference(*args, t_obj)
    b = K.kd_reference(*args, t_img, per_object=False)
    assert a["n_valid"] == b["n_valid"] == len(c["targets"]) and a["loss_kd"] == b["loss_kd"] > 0
    assert torch.equal(a["draw"], b["draw"]) and torch.equal(a["dz"], b["dz"])
    assert torch.equal(a["g_xs"], b["g_xs"]) and torch.equal(a["g_alpha"], b["g_alpha"])


def test_per_object_restatement_on_multi_instance_cases():
    """What the cases cover: images with 0..4 instances, an instance without positives, one class twice in an image
    (both slots face the same teacher set), more valid objects than images; the weight of a cell is w_kd / n_valid
    objects and the cells of an invalid object get none."""
    seen_same = False
    for name in sorted(C.STUDENT_CASES):
        c = K.object_case(name)
        B, cap = len(c["targets"]), c["cap"]
        ts = K.teacher_objects(c["tcls"], c["treg"], c["targets"], c["levels"])
        r = K.kd_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], cap, ts)
        n_slots = sum(len(t.class_ids) for t in c["targets"])
        assert 0 < r["n_valid"] <= n_slots and r["loss_kd"] > 0
        if name != "absent_same_class_c128_lam05":
            assert r["n_valid"] > sum(1 for t in c["targets"] if len(t.class_ids))       # more objects than images
        for b, t in enumerate(c["targets"]):
            G = len(t.class_ids)
            for g in range(K.MAX_GT):
                o = b * K.MAX_GT + g
                has_pos = any(gg == g for _, gg in c["pos"][b])
                assert r["valid"][o] == int(g < G and has_pos and len(ts[o]["rows"]) > 0)
            if G >= 2 and int(t.class_ids[0]) == int(t.class_ids[1]):
                seen_same = True
                assert ts[b * K.MAX_GT]["rows"] == ts[b * K.MAX_GT + 1]["rows"]
        # cells of invalid objects: zero upstream, zero class-logit gradient
        for i, (b, s, row, g) in enumerate(C.student_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], cap)["idx"]):
            if not r["valid"][b * K.MAX_GT + g]:
                assert float(r["g_xs"][b * cap + s].abs().max()) == 0 and float(r["dz"][i]) == 0
    assert seen_same


def test_recorded_tolerances_of_the_chained_gradients():
    """profiles/kd_per_object_tolerances.md: the fp32-vs-fp64 deviation of the restatement, measured afresh, does not
    exceed what was recorded when the cases were fixed; the GPU bounds are 8 x that with a floor of 4 fp32 ulps."""
    dev = K.measure_deviations()
    assert sorted(dev) == sorted(K.RECORDED_DEV)
    for k, v in dev.items():
        print("  %s: measured %.3e recorded %.3e bound %.3e" % (k, v, K.RECORDED_DEV[k], K.bound(k)))
        assert v <= K.RECORDED_DEV[k] * 1.001 + 1e-12, (k, v, K.RECORDED_DEV[k])
    assert K.bound("dreg") == C.FACTOR * K.RECORDED_DEV["dreg"] and K.bound("dcls") >= C.FLOOR
    text = open(os.path.join(ROOT, "profiles", "kd_per_object_tolerances.md")).read()
    for k, v in K.RECORDED_DEV.items():
        assert "%.3e" % v in text, (k, v)


def test_workspace_layout_comes_from_one_place():
    """KDLoss._ws_layout: named segments, contiguous and disjoint, the per-image part first and unchanged; _ws_sizes is
    its total (forward() takes the per-object views from the same table)."""
    from kd6d.kd_losses import KDLoss, MAX_GT
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    a, b = KDLoss(INTERNAL_K, MESH_DIAMETERS), KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg={"PER_OBJECT": True})
    for B in (1, 3, 16):
        fa, ia, nfa, nia = a._ws_layout(B)
        fb, ib, nfb, nib = b._ws_layout(B)
        assert list(fa) == ["image"] == list(ia) and (nfa, nia) == a._ws_sizes(B) and (nfb, nib) == b._ws_sizes(B)
        assert fb["image"] == fa["image"] == (0, nfa) and ib["image"] == ia["image"] == (0, nia)
        n = B * b.cap
        assert {k: v[1] for k, v in fb.items() if k != "image"} == dict(xs_obj=n * 16, g_xs_obj=n * 16, alpha_obj=n * 8,
                                                                        g_alpha_obj=n * 8, loss_obj=B * MAX_GT)
        assert {k: v[1] for k, v in ib.items() if k != "image"} == dict(obj_start=B * MAX_GT, obj_cnt=B * MAX_GT,
                                                                        valid_obj=B * MAX_GT, dest=n)
        for seg, total in ((fb, nfb), (ib, nib)):
            end = 0
            for off, cnt in seg.values():
                assert off == end
                end += cnt
            assert end == total
