"""GPU side of train-time augmentation (csrc/augment.hip): every kernel bit-equal to the numpy restatement
(tests/augment_ref.py) on seeded 480x640 frames, the device randomness, the loader end to end on the BOP fixture tree
and a 2-step `train_kd.py --augment` run."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import augment_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, W = 4, 480, 640
LINEMOD_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])


def _frames(seed, dev):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    f[:, 100:200, 100:300] = rng.integers(0, 256, (B, 1, 1, 3), dtype=np.uint8)   # flat patches: HSV / blur corner cases
    m = np.zeros((B, H, W), np.float32)
    for b in range(B):
        for i in range(3):
            y0, x0 = rng.integers(0, H - 120), rng.integers(0, W - 160)
            m[b, y0:y0 + rng.integers(20, 120), x0:x0 + rng.integers(20, 160)] = i + 1
    return f, m, torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev)


def test_warp_bitwise(gpu_device):
    from kd6d.libs import augment as A
    f, m, fd, md = _frames(0, gpu_device)
    us = [[0.0, 1.0, 0.0, 1.0], [0.999999, 0.0, 0.999999, 0.0], [0.5, 0.5, 0.5, 0.5], [0.13, 0.71, 0.37, 0.91]]
    mats = np.stack([A.shift_scale_rotate_matrix(0.05, 0.05, 10, W, H, AR.Recorded(u))[:2] for u in us]).astype(np.float64)
    out, mout = A.warp(fd, md, mats, (H, W))
    for b in range(B):
        assert np.array_equal(out[b].cpu().numpy(), AR.warp_u8(f[b], mats[b], (H, W))), b
        assert np.array_equal(mout[b].cpu().numpy(), AR.warp_mask(m[b], mats[b], (H, W))), b
    # Resize from another camera into a different size
    K2 = LINEMOD_K.copy(); K2[0, 0] *= 0.93; K2[1, 1] *= 0.95; K2[0, 2] -= 11.3; K2[1, 2] += 6.7
    Mr = np.stack([A.resize_matrix(K2, LINEMOD_K)[:2]] * B)
    out, mout = A.warp(fd, md, Mr, (360, 500))
    for b in range(B):
        assert np.array_equal(out[b].cpu().numpy(), AR.warp_u8(f[b], Mr[b], (360, 500))), b
        assert np.array_equal(mout[b].cpu().numpy(), AR.warp_mask(m[b], Mr[b], (360, 500))), b
    # identity: exact copy
    out, _ = A.warp(fd, None, np.stack([np.eye(3)[:2]] * B), (H, W))
    assert torch.equal(out, fd)


def test_hsv_blur_gray_bitwise(gpu_device):
    from kd6d.libs import augment as A
    f, _, fd, _ = _frames(1, gpu_device)
    factors = np.array([[0.8, 1.3, 0.7], [1.2, 0.6, 1.4], [1.0, 1.0, 1.0], [0.95, 1.05, 0.5]], np.float32)
    x = fd.clone()
    A.hsv(x, factors)
    got = x.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], AR.distort_hsv(f[b], factors[b])), b
    for ks in (1, 3, 5, 7, 9):
        y = A.filt(fd, np.full(B, ks, np.int32), None, False, 0).cpu().numpy()
        for b in range(B):
            assert np.array_equal(y[b], AR.box_blur(f[b], ks)), (ks, b)
    ks = np.array([1, 3, 5, 7], np.int32)
    y = A.filt(fd, ks, None, True, 0).cpu().numpy()
    for b in range(B):
        assert np.array_equal(y[b], AR.gray(AR.box_blur(f[b], int(ks[b])))), b


def test_stats_occlusion_relabel_bitwise(gpu_device):
    from kd6d.libs import augment as A
    f, m, fd, md = _frames(2, gpu_device)
    st = A.mask_stats(md, 4).cpu().numpy()
    for b in range(B):
        assert np.array_equal(st[b], AR.mask_stats(m[b], 4)), b
    rng = np.random.default_rng(3)
    U = rng.random((B, 4, 5))
    U[:, :, 0] *= 0.5                           # every instance qualifies at prob 0.7 ...
    U[1, 1, 0] = 0.9                            # ... but this one
    n_inst = np.array([3, 3, 2, 0], np.int32)
    key = 0x1234_5678_9ABC_DEF0
    x, xm = fd.clone(), md.clone()
    A.occlude(x, xm, A.mask_stats(xm, 4), U, n_inst, 0.7, key)
    for b in range(B):
        wi, wm = AR.occlude(f[b], m[b], int(n_inst[b]), U[b], 0.7, key, b)
        assert np.array_equal(x[b].cpu().numpy(), wi), b
        assert np.array_equal(xm[b].cpu().numpy(), wm), b
    assert (xm == -1).any()
    lut = np.zeros((B, 5), np.float32)
    keeps = []
    for b in range(B):
        keep, l = AR.relabel_lut(xm[b].cpu().numpy(), 4, min_area=3000)
        lut[b] = l; keeps.append(keep)
    A.relabel(xm, lut)
    for b in range(B):
        wm = AR.relabel(AR.occlude(f[b], m[b], int(n_inst[b]), U[b], 0.7, key, b)[1], lut[b])
        assert np.array_equal(xm[b].cpu().numpy(), wm), b


def test_device_randomness(gpu_device):
    from kd6d.libs import augment as A
    grey = torch.full((B, H, W, 3), 128, dtype=torch.uint8, device=gpu_device)
    sig = np.array([0.02, 0.05, 0.1, 0.0], np.float32)
    a = A.filt(grey, None, sig, False, 99)
    b = A.filt(grey, None, sig, False, 99)
    c = A.filt(grey, None, sig, False, 100)
    assert torch.equal(a, b) and not torch.equal(a, c)
    r = a.float() - 128.0
    for i in range(3):
        res = r[i]
        # truncation toward zero of 128 + g biases the mean by about -0.5 for g > 0 and +0.5 ... : loose bounds
        assert abs(res.mean().item()) < 0.75, (i, res.mean().item())
        assert abs(res.std().item() - sig[i] * 255) < 0.1 * sig[i] * 255 + 0.6, (i, res.std().item())
    assert torch.equal(a[3], grey[3])
    # clipping at 0 and 255
    lo = torch.zeros((B, 64, 64, 3), dtype=torch.uint8, device=gpu_device)
    hi = torch.full((B, 64, 64, 3), 255, dtype=torch.uint8, device=gpu_device)
    big = np.full(B, 0.5, np.float32)
    ylo, yhi = A.filt(lo, None, big, False, 5), A.filt(hi, None, big, False, 5)
    assert (ylo == 0).float().mean() > 0.4 and (ylo > 0).any() and (yhi == 255).float().mean() > 0.4 and (yhi < 255).any()
    # occlusion fill bytes: roughly uniform over 0..255
    f = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=gpu_device)
    m = torch.zeros((1, H, W), dtype=torch.float32, device=gpu_device)
    m[0, 40:440, 40:600] = 1
    U = np.zeros((1, 4, 5)); U[0, 0] = [0.0, 1.0, 0.5, 0.5, 0.5]
    A.occlude(f, m, A.mask_stats(m, 4), U, np.array([1], np.int32), 1.0, 7)
    vals = f[m == -1].reshape(-1).cpu().numpy()
    assert vals.size > 100000
    cnt = np.bincount(vals, minlength=256)
    e = vals.size / 256
    chi2 = ((cnt - e) ** 2 / e).sum()
    assert chi2 < 400, chi2                     # 255 dof: mean 255, sd ~23


def _aug_cfg(tree):
    from test_step_gpu import make_cfg
    cfg = make_cfg("darknet_tiny_h", "fp32")
    cfg["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], MESH_DIR=tree["models"], BBOX_FILE=tree["bbox"],
                           N_CLASS=3)
    # close to the fixture's cameras (fx 572.4, cx 15..21, cy 10) but not equal: Resize is a real warp
    cfg["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=[565.0, 0, 13.5, 0, 566.0, 10.5, 0, 0, 1])
    cfg["SOLVER"].update(IMS_PER_BATCH=2, AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2,
                         AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05,
                         AUGMENTATION_Grayscalize=False)
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False, NUM_WORKERS=0)
    return cfg


def test_build_dataset_with_augment_end_to_end(gpu_device, tmp_path):
    import random
    from bop_fixture import write_tree
    from kd6d.libs.train_libs import build_dataset
    tree = write_tree(str(tmp_path))
    cfg = _aug_cfg(tree)

    def run():
        random.seed(5); np.random.seed(5); torch.manual_seed(5)
        train_loader, _ = build_dataset(cfg, gpu_device, augment=True)
        return [next(iter(train_loader)) for _ in range(3)]
    x, y = run(), run()
    for (ia, ta, ma), (ib, tb, mb) in zip(x, y):
        assert ia.tensors.shape == (2, 3, 256, 256) and torch.isfinite(ia.tensors).all()
        assert torch.equal(ia.tensors, ib.tensors) and torch.equal(ta.mask, tb.mask)
        assert torch.equal(ta.bbox_trans, tb.bbox_trans)
        assert set(torch.unique(ta.mask).tolist()) <= {-1.0, 0.0, 1.0, 2.0}
    # bbox_trans maps the REMAPPED pose's box near the crop centre
    from kd6d.libs.augment import AugConfig, AugmentFront  # noqa: F401
    from kd6d.libs.dataset import projected_box
    from kd6d.libs.poses import PoseAnnot
    random.seed(5); np.random.seed(5); torch.manual_seed(5)
    train_loader, _ = build_dataset(cfg, gpu_device, augment=True)
    seen = []
    orig = train_loader.front.run

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(r[2])
        return r
    train_loader.front.run = spy
    images, tgt, metas = next(iter(train_loader))
    K = torch.tensor(np.array(cfg["INPUT"]["INTERNAL_K"]).reshape(3, 3), dtype=torch.float32)
    bbox = train_loader.loader.dataset.bbox_3d
    for b, (cls, Rs, Ts) in enumerate(seen[0]):
        if len(cls) == 0:
            continue
        a = PoseAnnot(bbox, K, None, torch.from_numpy(cls), torch.from_numpy(Rs), torch.from_numpy(Ts), tree["W"], tree["H"])
        box = projected_box(a, 0)
        A = tgt.bbox_trans[b].cpu().numpy().astype(np.float64)
        ctr = A[:, :2] @ np.array([0.5 * (box[0] + box[2]), 0.5 * (box[1] + box[3])]) + A[:, 2]
        side = max(box[2] - box[0], box[3] - box[1]) * A[0, 0]
        assert np.all(np.abs(ctr - 128.0) <= 0.25 * side + 1.0), (ctr, side)


def test_train_entry_with_augment(gpu_device, tmp_path):
    """train_kd.py --augment on the BOP fixture tree: two steps, finite losses."""
    import subprocess
    import yaml
    from bop_fixture import write_tree
    tree = write_tree(str(tmp_path / "data"))
    root = os.path.dirname(HERE)
    with open(os.path.join(root, "configs", "ape.yaml")) as f:
        y = yaml.safe_load(f)
    y["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], TEST=tree["list_file"],
                         MESH_DIR=tree["models"], BBOX_FILE=tree["bbox"])
    y["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=[565.0, 0, 13.5, 0, 566.0, 10.5, 0, 0, 1])
    y["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2, AUGMENTATION_ColorV=0.2,
                       AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05)
    cfgp = str(tmp_path / "aug.yaml")
    with open(cfgp, "w") as f:
        yaml.safe_dump(y, f)
    wd = str(tmp_path / "out") + "/"
    cmd = [sys.executable, os.path.join(root, "train_kd.py"), "--config_file", cfgp, "--config_file_t", cfgp,
           "--backbone", "darknet_tiny_h", "--backbone_t", "darknet53", "--kd_weight", "5.", "--working_dir", wd,
           "--augment", "--skip_teacher_eval", "--num_workers", "0", "--max_iters", "2", "--val_freq", "1000",
           "--batch_size", "2", "--launch", "eager"]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Training finished" in r.stdout
    import re
    steps = re.findall(r"steps: \d+/2, lr:\S+, cls:(\S+), reg:(\S+), kd:(\S+) ", r.stdout)
    assert steps, r.stdout[-3000:]
    assert all(np.isfinite(float(v.rstrip(","))) for row in steps for v in row), steps
