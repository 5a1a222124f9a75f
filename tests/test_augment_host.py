"""CPU side of train-time augmentation (train_kd.py --augment, kd6d/libs/augment.py): known answers of the numpy
restatement of csrc/augment.hip (tests/augment_ref.py; the cv2 arithmetic is unpinned), the goldens captured from the
imported reference (tests/golden/augment.npz), the pose remap, the dataset items and the flag."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, G)
sys.path.insert(0, HERE)
import augment_ref as AR  # noqa: E402

LINEMOD_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])


def _frame(rng, H=48, W=64):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


# ---- known answers of the restatement ------------------------------------------------------------------------------
def test_identity_warp_is_exact_copy():
    img = _frame(np.random.default_rng(0))
    M = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(AR.warp_u8(img, M, img.shape[:2]), img)
    m = np.random.default_rng(1).integers(0, 4, img.shape[:2]).astype(np.float32)
    assert np.array_equal(AR.warp_mask(m, M, img.shape[:2]), m)


def test_integer_shift_has_128_border():
    img = _frame(np.random.default_rng(2))
    out = AR.warp_u8(img, np.array([[1.0, 0, 3], [0, 1.0, -2]]), img.shape[:2])
    assert np.array_equal(out[:-2, 3:], img[2:, :-3])
    assert (out[:, :3] == 128).all() and (out[-2:] == 128).all()


def test_rot90_of_square_frame():
    img = _frame(np.random.default_rng(3), 32, 32)
    # forward map of np.rot90 (counter-clockwise): dst(x, y) = src(N-1-y, x)  <=>  dst = [[0, 1, 0], [-1, 0, N-1]] src
    M = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 31.0]])
    assert np.array_equal(AR.warp_u8(img, M, (32, 32)), np.rot90(img))


def test_mask_warp_keeps_input_values_and_zero():
    rng = np.random.default_rng(4)
    m = rng.choice(np.array([-1, 0, 1, 2, 3], np.float32), (40, 50))
    ang = np.deg2rad(7.0)
    M = np.array([[np.cos(ang) * 1.03, np.sin(ang), -4.2], [-np.sin(ang), np.cos(ang) * 1.03, 2.7]])
    out = AR.warp_mask(m, M, (40, 50))
    assert set(np.unique(out).tolist()) <= set(np.unique(m).tolist()) | {0.0}


def test_blur_constant_and_hsv_grey_and_gray_formula():
    c = np.full((20, 30, 3), 77, np.uint8)
    for ks in (1, 3, 5, 7):
        assert np.array_equal(AR.box_blur(c, ks), c)
    g = np.repeat(np.arange(0, 256, 5, dtype=np.uint8)[None, :, None], 3, 2)
    assert np.array_equal(AR.distort_hsv(g, np.ones(3, np.float32)), g)
    img = _frame(np.random.default_rng(5))
    y = AR.gray(img)
    b, gg, r = [img[:, :, k].astype(np.int64) for k in range(3)]
    assert np.array_equal(y[:, :, 1], ((1868 * b + 9617 * gg + 4899 * r + 8192) >> 14).astype(np.uint8))
    # a 3x3 blur at an interior pixel is the rounded mean
    out = AR.box_blur(img, 3)
    want = int(np.floor(img[10:13, 20:23, 0].astype(np.int64).sum() / 9 + 0.5))
    assert out[11, 21, 0] == want


def test_hsv_roundtrip_of_saturated_primaries():
    img = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 255, 255]]], np.uint8)
    assert np.array_equal(AR.distort_hsv(img, np.ones(3, np.float32)), img)


# ---- goldens of the imported reference -----------------------------------------------------------------------------
def test_occlusion_matches_reference_golden():
    z = np.load(os.path.join(G, "augment.npz"))
    for case in range(6):
        m_in, us = z["occ%d_mask_in" % case], z["occ%d_u" % case]
        n = us.shape[0]
        U = np.zeros((AR.MAX_GT, 5))
        U[:n] = us
        H, W = m_in.shape
        img = np.zeros((H, W, 3), np.uint8)
        _, m_out = AR.occlude(img, m_in, n, U, 0.7, 123, 0)
        assert np.array_equal(m_out, z["occ%d_mask_out" % case]), case


def test_remove_invalids_matches_reference_golden():
    z = np.load(os.path.join(G, "augment.npz"))
    for case in range(4):
        m_in = z["inv%d_mask_in" % case]
        n = int(m_in.max())
        keep, lut = AR.relabel_lut(m_in, n)
        assert np.array_equal(AR.relabel(m_in, lut), z["inv%d_mask_out" % case])
        assert np.array_equal(np.asarray(keep, np.int64), z["inv%d_ids" % case])


def test_ssr_matrix_matches_reference_golden():
    from kd6d.libs import augment as A
    z = np.load(os.path.join(G, "augment.npz"))
    for us, want in zip(z["ssr_u"], z["ssr_M"]):
        M = A.shift_scale_rotate_matrix(0.05, 0.05, 10, 640, 480, AR.Recorded(us))
        assert M.dtype == np.float32 and np.array_equal(M, want)


# ---- pose remap ----------------------------------------------------------------------------------------------------
def test_remap_projects_class_corners_through_M():
    from kd6d.libs import augment as A
    rng = np.random.default_rng(6)
    boxes = np.stack([np.array([[x, y, z] for x in (-a, a) for y in (-b, b) for z in (-c, c)])
                      for a, b, c in rng.uniform(20, 60, (3, 3))])
    class_ids = [2, 0]                                    # instance 0 is of class 2: index != class id
    Rs = [np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in class_ids]
    Rs = [R * np.linalg.det(R) for R in Rs]
    Ts = [np.array([[10.0], [-20.0], [900.0]]), np.array([[-40.0], [15.0], [880.0]])]
    for us in ([0.0, 1.0, 0.0, 1.0], [0.999, 0.0, 0.999, 0.0], [0.3, 0.6, 0.5, 0.2]):
        M = A.shift_scale_rotate_matrix(0.05, 0.05, 10, 640, 480, AR.Recorded(us)).astype(np.float64)
        newR, newT = A.remap_poses(LINEMOD_K, class_ids, Rs, Ts, boxes, LINEMOD_K, M)
        for i, c in enumerate(class_ids):
            def proj(R, T):
                p = LINEMOD_K @ (R @ boxes[c].T + T.reshape(3, 1))
                return p[:2] / p[2]
            src = proj(Rs[i], Ts[i])
            want = M[:2, :2] @ src + M[:2, 2:3]
            got = proj(newR[i].astype(np.float64), newT[i].astype(np.float64))
            assert np.abs(got - want).max() < 1.0, (us, i, np.abs(got - want).max())


# ---- dataset items / flag ------------------------------------------------------------------------------------------
def _cfg(tree, **solver):
    import yaml
    from kd6d.arguments.argument import custom_cfg
    with open(os.path.join(os.path.dirname(HERE), "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg = custom_cfg(cfg)
    cfg["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], MESH_DIR=tree["models"],
                           BBOX_FILE=tree["bbox"], N_CLASS=3)
    cfg["INPUT"].update(INTERNAL_WIDTH=32, INTERNAL_HEIGHT=24,
                        INTERNAL_K=[560.0, 0, 16.0, 0, 560.0, 12.0, 0, 0, 1])
    cfg["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2,
                         AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=5, AUGMENTATION_Noise=0.05)
    cfg["SOLVER"].update(solver)
    return cfg


@pytest.fixture()
def tree(tmp_path):
    from bop_fixture import write_tree
    return write_tree(str(tmp_path))


def test_items_without_augment_are_unchanged_and_draw_nothing(tree):
    from kd6d.libs import dataset as D
    a = D.BOP_Dataset(tree["list_file"], tree["models"], tree["bbox"], training=False)
    b = D.BOP_Dataset(tree["list_file"], tree["models"], tree["bbox"], training=False, augment=False)
    random.seed(3)
    state = random.getstate()
    for i in range(len(a)):
        x, y = a[i], b[i]
        assert len(x) == len(y) == 3
        assert torch.equal(x[0], y[0]) and torch.equal(x[1].mask, y[1].mask)
        assert torch.equal(x[1].rotations, y[1].rotations) and x[2]["path"] == y[2]["path"]
    assert random.getstate() == state
    frames, masks, targets, metas = D.collate_frames([b[0], b[1]])
    assert frames.shape[0] == 2


def test_augment_items_are_reproducible(tree):
    from kd6d.libs import dataset as D

    def items():
        random.seed(7); np.random.seed(7)
        ds = D.BOP_Dataset(tree["list_file"], tree["models"], tree["bbox"], training=True, augment=_cfg(tree))
        return [ds[i] for i in range(len(ds))]
    x, y = items(), items()
    for a, b in zip(x, y):
        assert len(a) == 4
        pa, pb = a[3], b[3]
        assert pa.keys() == pb.keys()
        for k in pa:
            assert np.array_equal(np.asarray(pa[k]), np.asarray(pb[k])), k
        assert {"occl_u", "M_ssr", "hsv", "ksize", "sigma", "key", "R", "T", "R_resize"} <= set(pa)
        assert pa["R"].shape == (pa["n"], 3, 3) and np.isfinite(pa["R"]).all()
    batch = D.collate_frames(x[:2])
    assert len(batch) == 5 and batch[4]["M_resize"].shape == (2, 2, 3) and batch[4]["occl_u"].shape == (2, 4, 5)


def test_flag_parses_and_unbuilt_transforms_raise(tree):
    from kd6d.arguments.argument_kd import get_argparser
    from kd6d.libs.augment import AugConfig
    assert get_argparser().parse_args(["--augment"]).augment is True
    assert get_argparser().parse_args([]).augment is False
    AugConfig(_cfg(tree))
    with pytest.raises(NotImplementedError, match="AUGMENTATION_BACKGROUND_DIR"):
        AugConfig(_cfg(tree, AUGMENTATION_BACKGROUND_DIR="/somewhere"))
    with pytest.raises(NotImplementedError, match="AUGMENTATION_Sharpen"):
        AugConfig(_cfg(tree, AUGMENTATION_Sharpen=0.3))


def test_identity_resize_is_detected():
    from kd6d.libs import augment as A
    assert A.is_identity_warp(A.resize_matrix(LINEMOD_K, LINEMOD_K), 640, 480)
    K2 = LINEMOD_K.copy()
    K2[0, 2] += 0.01
    assert not A.is_identity_warp(A.resize_matrix(LINEMOD_K, K2), 640, 480)
