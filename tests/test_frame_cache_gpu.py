"""GPU side of the device-resident frame cache (csrc/frame_cache.hip, kd6d/libs/frame_cache.py, --frame_cache device):
the two gather kernels bit for bit against torch / PackedTargets, the cached loader byte for byte against the host
loader (plain and with --augment), decode-once, and the two entry points with and without the flag."""
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import frame_cache_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 420
GUARD_BYTES, GUARD_FLOATS = 24, 3          # neither a multiple of 16 bytes: the outputs start off a granule


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return C.write_cache_tree(str(tmp_path_factory.mktemp("frame_cache")))


def _guarded(B, H, W, dev):
    fb = torch.full((GUARD_BYTES * 2 + B * H * W * 3,), 0xA5, dtype=torch.uint8, device=dev)
    mb = torch.full((GUARD_FLOATS * 2 + B * H * W,), -7.5, dtype=torch.float32, device=dev)
    return (fb, fb[GUARD_BYTES:GUARD_BYTES + B * H * W * 3].view(B, H, W, 3),
            mb, mb[GUARD_FLOATS:GUARD_FLOATS + B * H * W].view(B, H, W))


# (n, H, W, index): a repeat, frame 0 and frame n - 1 in every case.  37x52: 5772 bytes per frame, no multiple of 16 (the
# 16-byte, the 4-byte and -- from a source off by one byte -- the bytewise path all occur); 1x5: 15 bytes, smaller than
# one granule; 16x16: aligned.
@pytest.mark.parametrize("n,H,W,index", [(7, 37, 52, [3, 0, 6, 3, 0]), (3, 1, 5, [2, 0, 1, 2]), (2, 16, 16, [1, 0, 1])])
def test_gather_frames_bitwise(gpu_device, n, H, W, index):
    from kd6d import ops
    g = torch.Generator().manual_seed(n * 1000 + H)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(gpu_device)
    masks = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, generator=g).to(gpu_device)
    idx = torch.tensor(index, dtype=torch.int32, device=gpu_device)
    B = len(index)
    want_f = torch.index_select(frames, 0, idx.long())
    want_m = torch.index_select(masks, 0, idx.long()).float()
    # sources: as allocated, and one byte off (the cache itself never is, the kernel must not care)
    off_f = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device=gpu_device)
    off_m = torch.zeros(masks.numel() + 1, dtype=torch.uint8, device=gpu_device)
    off_f[1:].copy_(frames.reshape(-1)); off_m[1:].copy_(masks.reshape(-1))
    for src_f, src_m in ((frames, masks), (off_f[1:].view(n, H, W, 3), off_m[1:].view(n, H, W))):
        fb, fo, mb, mo = _guarded(B, H, W, gpu_device)
        got_f, got_m = ops.cache_gather_frames(src_f, src_m, idx, fo, mo)
        torch.cuda.synchronize()
        assert got_f.dtype == torch.uint8 and got_m.dtype == torch.float32
        assert torch.equal(got_f, want_f) and torch.equal(got_m.view(torch.int32), want_m.view(torch.int32))
        assert bool((fb[:GUARD_BYTES] == 0xA5).all()) and bool((fb[-GUARD_BYTES:] == 0xA5).all())
        assert bool((mb[:GUARD_FLOATS] == -7.5).all()) and bool((mb[-GUARD_FLOATS:] == -7.5).all())
        # outputs the wrapper allocates itself (aligned)
        got_f, got_m = ops.cache_gather_frames(src_f, src_m, idx)
        assert torch.equal(got_f, want_f) and torch.equal(got_m.view(torch.int32), want_m.view(torch.int32))


def _host_annots(ds, ids, crop_masks, trans, bscale, dev):
    """The PoseAnnots DziLoader builds from the data set's items for one batch (the existing way)."""
    from kd6d.libs.poses import PoseAnnot
    out = []
    R = crop_masks.shape[-1]
    for i, k in enumerate(ids):
        t = ds.getitem1(k)[1]
        out.append(PoseAnnot(t.keypoints_3d.to(dev), t.K.to(dev), crop_masks[i], t.class_ids.to(dev), t.rotations.to(dev),
                             t.translations.to(dev), R, R, bscale[i], trans[i]))
    return out


def test_gather_targets_bytes_equal_packed_targets(gpu_device, tree):
    from kd6d import ops
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.dzi_libs import dzi_batch, normalize_lut, test_bbox_DZI
    from kd6d.libs.frame_cache import DeviceFrameCache
    ds = C.datasets(tree, training=False)
    cache = DeviceFrameCache(ds, gpu_device, 1 << 30, log=None)
    ids = [0, 1, 4, 6, 0]                     # 3 instances, 1, none (unknown object only), 3, a repeat
    assert [int(cache.table_i[cache.slot_of[k], 0]) for k in ids] == [3, 1, 0, 3, 3]
    slots = [cache.resolve(k) for k in ids]
    cs = [test_bbox_DZI(cache.boxes[s], C.H, C.W) for s in slots]
    centers, scales = np.stack([c for c, _ in cs]), np.asarray([s for _, s in cs])
    lut = normalize_lut([0.485, 0.456, 0.406], [0.229, 0.224, 0.225], gpu_device)
    index, frames, masks = cache.gather(slots)
    images, crop_masks, trans, bscale = dzi_batch(frames, masks, centers, scales, lut)
    nf, ni = ops.cache_target_sizes(len(ids), int(cache.kp3d_dev.numel()))
    ff = torch.full((nf + 8,), -7.5, dtype=torch.float32, device=gpu_device)
    fi = torch.full((ni + 8,), -77, dtype=torch.int32, device=gpu_device)
    flat_f, flat_i = ops.cache_gather_targets(cache.table_f_dev, cache.table_i_dev, cache.kp3d_dev, index, trans,
                                              ff[4:4 + nf], fi[4:4 + ni])
    torch.cuda.synchronize()
    assert bool((ff[:4] == -7.5).all()) and bool((ff[-4:] == -7.5).all())
    assert bool((fi[:4] == -77).all()) and bool((fi[-4:] == -77).all())
    want = PackedTargets(_host_annots(ds, ids, crop_masks, trans, bscale, gpu_device), gpu_device)
    assert torch.equal(flat_f.view(torch.int32), want.flat_f.view(torch.int32))
    assert torch.equal(flat_i, want.flat_i)
    got = PackedTargets.from_packed(crop_masks, flat_f.clone(), flat_i.clone(), len(ids))
    assert torch.equal(got.block, want.block)
    for name in PackedTargets._SMALL_F + PackedTargets._SMALL_I + ("mask",):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), name
    assert (got.batch, got.mask_h, got.mask_w, got.frame_wh) == (want.batch, want.mask_h, want.mask_w, want.frame_wh)


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _collect(loader, epochs):
    out = []
    for _ in range(epochs):
        for images, tgt, metas in loader:
            out.append((images.tensors.clone(), list(images.sizes), tgt.block.clone(), metas))
    torch.cuda.synchronize()
    return out


def _assert_batches_equal(host, cached):
    assert len(host) == len(cached) and len(host) > 0
    for (ia, sa, ba, ma), (ib, sb, bb, mb) in zip(host, cached):
        assert ia.shape == ib.shape and torch.equal(ia.view(torch.int32), ib.view(torch.int32))
        assert sa == sb
        assert ba.shape == bb.shape and torch.equal(ba, bb)
        assert [m["path"] for m in ma] == [m["path"] for m in mb]
        for x, y in zip(ma, mb):
            assert set(x) == set(y) and x["class_ids"] == y["class_ids"] and (x["width"], x["height"]) == (y["width"], y["height"])
            assert np.array_equal(np.asarray(x["K"]), np.asarray(y["K"]))
            assert np.array_equal(np.asarray(x["rotations"]), np.asarray(y["rotations"]))
            assert np.array_equal(np.asarray(x["translations"]), np.asarray(y["translations"]))


def test_cached_loader_equals_host_loader(gpu_device, tree):
    """The main test: same seeds -> the same bytes, two training epochs (shuffled, drop_last, the unusable frame
    resampled) and one validation epoch (sequential, a last batch of one, a frame without instances)."""
    from kd6d.libs.train_libs import CachedDziLoader, DziLoader, build_dataset
    cfg = C.make_cfg(tree, batch=3)
    runs, resampled = {}, []
    for mode in ("off", "device"):
        _seed(12)
        train, valid = build_dataset(cfg, gpu_device, frame_cache=mode)
        assert type(train) is (CachedDziLoader if mode == "device" else DziLoader) and type(valid) is type(train)
        assert len(train) == 2 and len(valid) == 3 and len(train.loader.dataset) == 7
        if mode == "device":
            resolve = train.cache.resolve
            train.cache.resolve = lambda i: (resampled.append(i) if train.cache.slot_of[i] < 0 else None) or resolve(i)
        runs[mode] = _collect(train, 2) + _collect(valid, 1)
    assert len(runs["off"]) == 7
    assert resampled, "the seed must make the sampler draw the unusable frame within two epochs"
    _assert_batches_equal(runs["off"], runs["device"])
    from kd6d.libs.train_libs import dataset_meshes
    assert len(dataset_meshes(train)) == 2


def test_cached_loader_equals_host_loader_with_augment(gpu_device, tree):
    from kd6d.libs.train_libs import build_dataset
    cfg = C.make_cfg(tree, batch=3, augment=True)
    runs = {}
    for mode in ("off", "device"):
        _seed(21)
        train, _ = build_dataset(cfg, gpu_device, augment=True, frame_cache=mode)
        runs[mode] = _collect(train, 1)
    assert len(runs["off"]) == 2
    _assert_batches_equal(runs["off"], runs["device"])


def test_frames_are_decoded_once(gpu_device, tree, monkeypatch):
    from kd6d.libs import dataset as DS
    from kd6d.libs.train_libs import build_dataset
    calls = []
    real = DS.load_image_cached
    monkeypatch.setattr(DS, "load_image_cached", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    _seed(5)
    train, valid = build_dataset(C.make_cfg(tree, batch=3), gpu_device, frame_cache="device")
    built = len(calls)
    assert built >= 2 * 7                       # every frame and its masks, for both lists
    n = len(_collect(train, 2)) + len(_collect(valid, 1))
    assert n == 7 and len(calls) == built


def _yaml_for(tree, path):
    import yaml
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        y = yaml.safe_load(f)
    y["DATASETS"].update(TRAIN=tree["list"], VALID=tree["eval_list"], TEST=tree["eval_list"], MESH_DIR=tree["models"],
                         BBOX_FILE=tree["bbox"])
    y["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=list(C.INTERNAL_K))
    with open(path, "w") as f:
        yaml.safe_dump(y, f)
    return path


def _run(script, args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(ROOT, script)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_train_entry_same_losses_with_and_without_the_cache(gpu_device, tree, tmp_path):
    cfgp = _yaml_for(tree, str(tmp_path / "cache.yaml"))
    lines = {}
    for mode in ("off", "device"):
        out = _run("train_kd.py", ["--config_file", cfgp, "--config_file_t", cfgp, "--backbone", "darknet_tiny_h",
                                   "--backbone_t", "darknet53", "--kd_weight", "5.", "--working_dir",
                                   str(tmp_path / mode) + "/", "--skip_teacher_eval", "--num_workers", "0", "--max_iters", "2",
                                   "--val_freq", "1000", "--batch_size", "2", "--launch", "graph", "--frame_cache", mode])
        assert "Training finished" in out
        assert ("frame cache: " in out) == (mode == "device")
        lines[mode] = re.findall(r"steps: (\d+/2, lr:\S+ cls:\S+ reg:\S+ kd:\S+) ", out)
        assert lines[mode], out[-3000:]
        print(mode, lines[mode])
    assert lines["off"] == lines["device"]


def test_eval_entry_same_predictions_with_and_without_the_cache(gpu_device, tree, tmp_path):
    cfgp = _yaml_for(tree, str(tmp_path / "cache.yaml"))
    preds = {}
    for mode in ("off", "device"):
        wd = str(tmp_path / ("eval_" + mode))
        out = _run("test.py", ["--config_file", cfgp, "--backbone", "darknet_tiny_h", "--pnp_solver", "device",
                               "--eval_scorer", "device", "--num_workers", "0", "--working_dir", wd, "--frame_cache", mode])
        assert ("frame cache: 4 frames of 52x37" in out) == (mode == "device")
        preds[mode] = json.load(open(os.path.join(wd, "preds.json")))
    assert len(preds["off"]) == len(C.EVAL_IDS) and preds["off"] == preds["device"]
