"""GPU side of `--aug_chain full` (csrc/augment.hip: kd6d_aug_background, kd6d_aug_sharpen): both kernels bit-equal to
the numpy restatement (tests/augment_full_ref.py) at sizes that are no multiple of any launch granule, the defined
no-ops on bad tables, the loaders end to end on the BOP fixture tree and two 2-step `train_kd.py` runs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import augment_full_ref as FR  # noqa: E402
import augment_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 37, 70
BG_SIZES = ((1, 1), (2, 3), (37, 70), (150, 261), (9, 200))      # 1 px, tiny, same size, 3.7x down, up in y / down in x


def _pool(dev, sizes=BG_SIZES, seed=20):
    from kd6d.libs.augment import BackgroundPool
    rng = np.random.default_rng(seed)
    imgs = {"bg%d" % i: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)}
    pool = BackgroundPool("", list(imgs), dev, 2 ** 24, probe=lambda p: imgs[p].shape[:2], decode=lambda p: imgs[p])
    return pool, list(imgs.values())


def _frames_masks(B, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    m = rng.choice(np.array([0, 0, 0, 1, 2, 3, -1], np.float32), (B, H, W))
    m[:, 5:20, 10:40] = 0
    return f, m


def test_background_bitwise(gpu_device):
    from kd6d.libs import augment as A
    pool, backs = _pool(gpu_device)
    f, m = _frames_masks(4, 21)
    md = torch.from_numpy(m).to(gpu_device)
    for index in ([-1, 0, 3, 4], [1, 2, -1, 1]):
        x = torch.from_numpy(f).to(gpu_device)
        A.background(x, md, pool, index)
        y = torch.from_numpy(f).to(gpu_device)
        A.background(y, md, pool, index)
        assert torch.equal(x, y)                                               # two calls are bitwise equal
        got = x.cpu().numpy()
        for b, i in enumerate(index):
            if i < 0:
                assert np.array_equal(got[b], f[b]), b                        # the -1 image is untouched
                continue
            assert np.array_equal(got[b], FR.merge_background(f[b], m[b], backs[i])), (b, i)
            assert np.array_equal(got[b][m[b] != 0], f[b][m[b] != 0]), (b, i)  # ids and the occlusion's -1 keep their bytes
            assert (got[b][m[b] == 0] != f[b][m[b] == 0]).any()
    assert np.array_equal(md.cpu().numpy(), m)                                 # masks are not written
    # the same-size background is an exact copy where the mask is 0
    x = torch.from_numpy(f).to(gpu_device)
    A.background(x, torch.zeros_like(md), pool, [2, 2, 2, 2])
    assert all(np.array_equal(x[b].cpu().numpy(), backs[2]) for b in range(4))
    with pytest.raises(ValueError, match="background index"):
        A.background(x, md, pool, [0, 5, 0, 0])


def test_background_bad_tables_are_no_ops(gpu_device):
    """An index outside [-1, n_bg) and table entries that reach past pool_bytes (or have no pixels) leave their images
    untouched: the kernel returns before it forms an address from them.  Straight through the C ABI: the wrapper
    refuses such an index on the host."""
    from kd6d import ops
    from kd6d.ops import check, lib
    pool, backs = _pool(gpu_device)
    f, m = _frames_masks(5, 22)
    x, md = torch.from_numpy(f).to(gpu_device), torch.from_numpy(m).to(gpu_device)
    hw, off = pool.hw_host.copy(), pool.off_host.copy()
    off[3] = pool.nbytes - 150 * 261 * 3 + 1          # entry 3 ends one byte past the pool
    hw[1] = (0, 3)                                    # entry 1 has no pixels
    off[4] = -8                                       # entry 4 starts before the pool
    hwd, offd = torch.from_numpy(hw).to(gpu_device), torch.from_numpy(off).to(gpu_device)
    index = torch.tensor([pool.n, 3, 1, 4, 0], dtype=torch.int32, device=gpu_device)
    check(lib.kd6d_aug_background(ops._ptr(x), ops._ptr(md), 5, H, W, ops._ptr(pool.pool), pool.nbytes, ops._ptr(offd),
                                  ops._ptr(hwd), pool.n, ops._ptr(index), ops._stream()), "kd6d_aug_background")
    torch.cuda.synchronize()
    got = x.cpu().numpy()
    for b in range(4):
        assert np.array_equal(got[b], f[b]), b
    assert np.array_equal(got[4], FR.merge_background(f[4], m[4], backs[0]))       # the good entry of the same launch ran


# ---- sharpen -------------------------------------------------------------------------------------------------------
def _sharpen_images(h, w, seed):
    """noise with a flat patch, a flat image, plain noise."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    f[0, h // 4:h // 4 + max(2, h // 2), w // 4:w // 4 + max(2, w // 2)] = (90, 160, 30)
    f[1] = 117
    return f


@pytest.mark.parametrize("mode", [1, 0], ids=["ratio", "difference"])
@pytest.mark.parametrize("ks", [5, 7, 9, 11])
@pytest.mark.parametrize("hw", [(37, 70), (7, 9)], ids=["37x70", "7x9"])
def test_sharpen_bitwise(gpu_device, hw, ks, mode):
    from kd6d.libs import augment as A
    f = _sharpen_images(hw[0], hw[1], 30 + ks)
    fd = torch.from_numpy(f).to(gpu_device)
    kss, alphas = [ks, ks, 0], [0.5 + 0.04 * ks, 0.95, 0.7]
    x = A.sharpen(fd, kss, [mode] * 3, alphas)
    y = A.sharpen(fd, kss, [mode] * 3, alphas)
    assert torch.equal(x, y) and torch.equal(fd.cpu(), torch.from_numpy(f))      # reproducible; the source is not written
    got = x.cpu().numpy()
    want = FR.pencil_sharpen(f[0], ks, bool(mode), alphas[0])
    assert np.array_equal(got[0], want), int((got[0] != want).sum())
    assert want.min() == 0 and want.max() in (254, 255)
    assert (got[1] == 0).all()                                                   # flat: max = min gives scale 0, twice
    assert np.array_equal(got[2], f[2])                                          # ks = 0: a copy
    alone = A.sharpen(fd[:1].contiguous(), kss[:1], [mode], alphas[:1])
    assert torch.equal(alone[0], x[0])                                           # the same alone and inside a batch


@pytest.mark.parametrize("ks,mode", [(5, 1), (11, 1), (11, 0), (7, 0)])
def test_sharpen_spans_tiles(gpu_device, ks, mode):
    """131 x 70: more than two tiles along each axis, the last ones partial."""
    from kd6d.libs import augment as A
    rng = np.random.default_rng(40 + ks)
    f = rng.integers(0, 256, (2, 131, 70, 3), dtype=np.uint8)
    f[1] = np.transpose(rng.integers(0, 256, (70, 131, 3), dtype=np.uint8), (1, 0, 2))
    f[1, 60:70, 30:34] = 255
    fd = torch.from_numpy(f).to(gpu_device)
    got = A.sharpen(fd, [ks, ks], [mode, 1 - mode], [0.61, 0.83]).cpu().numpy()
    for b, (md, al) in enumerate(((mode, 0.61), (1 - mode, 0.83))):
        want = FR.pencil_sharpen(f[b], ks, bool(md), al)
        assert np.array_equal(got[b], want), (b, int((got[b] != want).sum()))
    wide = np.ascontiguousarray(np.transpose(f, (0, 2, 1, 3)))                    # 70 x 131
    got = A.sharpen(torch.from_numpy(wide).to(gpu_device), [ks, 0], [mode, 0], [0.61, 0.5]).cpu().numpy()
    assert np.array_equal(got[0], FR.pencil_sharpen(wide[0], ks, bool(mode), 0.61)) and np.array_equal(got[1], wide[1])
    with pytest.raises(ValueError, match="box sizes"):
        A.sharpen(fd, [4, 5], [0, 0], [0.5, 0.5])


# ---- loaders end to end ----------------------------------------------------------------------------------------------
def _full_cfg(tree, bg_dir):
    from test_step_gpu import make_cfg
    cfg = make_cfg("darknet_tiny_h", "fp32")
    cfg["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], MESH_DIR=tree["models"], BBOX_FILE=tree["bbox"],
                           N_CLASS=3)
    cfg["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=[565.0, 0, 13.5, 0, 566.0, 10.5, 0, 0, 1])
    cfg["SOLVER"].update(IMS_PER_BATCH=2, AUGMENTATION_OCCLUSION=0, AUGMENTATION_SHIFT=0, AUGMENTATION_SCALE=0,
                         AUGMENTATION_ROTATION=0, AUGMENTATION_ColorH=0, AUGMENTATION_ColorS=0, AUGMENTATION_ColorV=0,
                         AUGMENTATION_Smooth=0, AUGMENTATION_Noise=0, AUGMENTATION_Grayscalize=False,
                         AUGMENTATION_Sharpen=0, AUGMENTATION_BACKGROUND_DIR=bg_dir)
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False, NUM_WORKERS=0, AUG_CHAIN="full")
    return cfg


def _write_backgrounds(d):
    from PIL import Image
    os.makedirs(d)
    rng = np.random.default_rng(50)
    for name, (h, w) in (("a.png", (20, 24)), ("b.png", (33, 17)), ("c.png", (6, 80))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(os.path.join(d, name))
    return d


@pytest.mark.parametrize("frame_cache", ["off", "device"])
def test_loader_replaces_backgrounds_end_to_end(gpu_device, tmp_path, frame_cache):
    import random
    from bop_fixture import write_tree
    from kd6d.libs.train_libs import build_dataset
    tree = write_tree(str(tmp_path / "data"))
    cfg = _full_cfg(tree, _write_backgrounds(str(tmp_path / "bg")))
    size = (tree["H"], tree["W"])
    seen = []

    def run(spy):
        random.seed(9); np.random.seed(9); torch.manual_seed(9)
        train_loader, _ = build_dataset(cfg, gpu_device, augment=True, frame_cache=frame_cache)
        front = train_loader.front
        assert front.pool.n == 3 and front.pool.hw_host.tolist() == [[20, 24], [33, 17], [6, 80]]
        if spy:
            orig = front.run

            def wrapped(frames, masks, targets, params):
                r = orig(frames, masks, targets, params)
                seen.append((frames.cpu().numpy(), masks.cpu().numpy(), params, r[0].cpu().numpy(), r[2], front.pool))
                return r
            front.run = wrapped
        return [next(iter(train_loader)) for _ in range(6)]
    x, y = run(True), run(False)
    for (ia, ta, _), (ib, tb, _) in zip(x, y):
        assert torch.equal(ia.tensors, ib.tensors) and torch.equal(ta.mask, tb.mask)       # two seeded runs: equal batches
    drew = []
    for frames, masks, params, out, poses, pool in seen:
        buf = pool.pool.cpu().numpy()
        for b in range(frames.shape[0]):
            M = params["M_resize"][b]
            want = AR.warp_u8(frames[b], M, size)
            i = int(params["bg"][b])
            if i >= 0 and len(poses[b][0]):       # an image that keeps no instance falls back to its Resize-only frame
                h, w = pool.hw_host[i]
                back = buf[pool.off_host[i]:pool.off_host[i] + h * w * 3].reshape(h, w, 3)
                want = FR.merge_background(want, AR.warp_mask(masks[b], M, size), back)
            assert np.array_equal(out[b], want), (b, i)
            drew.append(i)
    assert any(i >= 0 for i in drew) and any(i < 0 for i in drew), drew


def _train_yaml(tmp_path, tree, **inp):
    import yaml
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        y = yaml.safe_load(f)
    y["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], TEST=tree["list_file"],
                         MESH_DIR=tree["models"], BBOX_FILE=tree["bbox"])
    y["INPUT"].update(inp)
    y["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2, AUGMENTATION_ColorV=0.2,
                       AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05, AUGMENTATION_Sharpen=0.5,
                       AUGMENTATION_BACKGROUND_DIR=_write_backgrounds(str(tmp_path / "bg")))
    cfgp = str(tmp_path / "aug_full.yaml")
    with open(cfgp, "w") as f:
        yaml.safe_dump(y, f)
    return cfgp


@pytest.mark.parametrize("source", ["list", "render"])
def test_train_entry_with_the_full_chain(gpu_device, tmp_path, source):
    """train_kd.py --augment --aug_chain full with a background directory and AUGMENTATION_Sharpen 0.5: two steps, finite
    losses -- on the BOP fixture tree, and on rendered frames (their visible-instance masks select the background)."""
    import re
    import subprocess
    from bop_fixture import write_tree
    tree = write_tree(str(tmp_path / "data"))
    if source == "list":
        cfgp = _train_yaml(tmp_path, tree, INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"],
                           INTERNAL_K=[565.0, 0, 13.5, 0, 566.0, 10.5, 0, 0, 1])
        extra = []
    else:
        cfgp = _train_yaml(tmp_path, tree, INTERNAL_WIDTH=320, INTERNAL_HEIGHT=240,
                           INTERNAL_K=[286.2, 0, 162.6, 0, 286.8, 121.0, 0, 0, 1])
        extra = ["--frame_source", "render", "--render_meshes", "surrogate", "--render_frames", "4",
                 "--render_valid_frames", "2"]
    cmd = [sys.executable, os.path.join(ROOT, "train_kd.py"), "--config_file", cfgp, "--config_file_t", cfgp,
           "--backbone", "darknet_tiny_h", "--backbone_t", "darknet53", "--kd_weight", "5.",
           "--working_dir", str(tmp_path / "out") + "/", "--augment", "--aug_chain", "full", "--skip_teacher_eval",
           "--num_workers", "0", "--max_iters", "2", "--val_freq", "1000", "--batch_size", "2", "--launch", "eager"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Training finished" in r.stdout
    steps = re.findall(r"steps: \d+/2, lr:\S+, cls:(\S+), reg:(\S+), kd:(\S+) ", r.stdout)
    assert steps, r.stdout[-3000:]
    assert all(np.isfinite(float(v.rstrip(","))) for row in steps for v in row), steps
