"""GPU: the rendered frame source end to end -- RenderedFrames (kd6d/libs/render_source.py) with surrogate meshes, 8 frames
of 640 x 480 with up to 2 objects, drawn by kd6d_render_frames and fed through RenderedDziLoader (B = 4): the yielded
triple's documented layout, seeded equality, the masks against the projected vertices, the --augment path, one optimiser
step, --bop_vsd's depth provider and test.py --frame_source render."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B, H, W = 8, 4, 480, 640


def _cfg(augment=False):
    import yaml
    from kd6d.arguments.argument import custom_cfg
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["RUNTIME"] = {"PRECISION": "fp32", "N_GPU": 1, "DISTRIBUTED": False, "NUM_WORKERS": 0}
    cfg["MODEL"]["BACKBONE"] = "darknet_tiny_h"
    cfg = custom_cfg(cfg)
    cfg["SOLVER"]["IMS_PER_BATCH"] = B
    if augment:
        cfg["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2,
                             AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05,
                             AUGMENTATION_Grayscalize=False, AUGMENTATION_Sharpen=0, AUGMENTATION_BACKGROUND_DIR=None)
    return cfg


@functools.lru_cache(maxsize=None)
def _meshes():
    from kd6d.libs import render_source as RS
    return RS.surrogate_meshes(15)


def _store(dev, seed=11, **kw):
    from kd6d.libs import render_source as RS
    from kd6d.synthetic import INTERNAL_K
    meshes, kp3d = _meshes()
    return RS.RenderedFrames(meshes, kp3d, N, np.asarray(INTERNAL_K).reshape(3, 3), H, W, dev, seed=seed, instances=2,
                             classes=[0, 4, 8, 11], log=None, **kw)


@functools.lru_cache(maxsize=None)
def _shared_store(dev):
    return _store(dev)


def _loader(store, dev, training=True, augment=False):
    from kd6d.libs.train_libs import RenderedDziLoader
    return RenderedDziLoader(store, _cfg(augment), dev, training, B, augment=augment)


def _seed():
    random.seed(2); np.random.seed(2); torch.manual_seed(2)


def _bytes(batch):
    images, targets, metas = batch
    return (images.tensors.cpu(), targets.mask.cpu(), targets.flat_f.cpu(), targets.flat_i.cpu(), [m["path"] for m in metas])


def test_the_yielded_triple_has_the_cached_loaders_layout(gpu_device):
    """DziLoader's docstring: (ImageList of 256 x 256 normalised crops, PackedTargets with the cropped mask, bbox_trans,
    metas); PackedTargets' fields as kd_losses documents them."""
    from kd6d._lib import MAX_GT
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    st = _shared_store(gpu_device)
    _seed()
    ld = _loader(st, gpu_device)
    assert len(ld) == N // B and ld.loader.dataset.meshes is st.meshes
    batches = list(ld)
    assert len(batches) == N // B
    seen = []
    for images, t, metas in batches:
        assert isinstance(images, ImageList) and isinstance(t, PackedTargets) and isinstance(metas, list) and len(metas) == B
        assert images.tensors.shape == (B, 3, 256, 256) and images.tensors.dtype == torch.float32 and images.tensors.is_cuda
        assert list(images.sizes) == [(256, 256)] * B
        assert t.batch == B and t.mask.shape == (B, 256, 256) and t.mask.dtype == torch.float32
        assert t.kp3d.shape == (B, 15, 8, 3) and t.K.shape == (B, 3, 3) and t.bbox_trans.shape == (B, 2, 3)
        assert t.rot.shape == (B, MAX_GT, 3, 3) and t.trans.shape == (B, MAX_GT, 3)
        assert t.class_ids.shape == (B, MAX_GT) and t.class_ids.dtype == torch.int32 and t.n_gt.shape == (B,)
        assert torch.isfinite(images.tensors).all()
        for j, m in enumerate(metas):
            s = m["slot"]
            seen.append(s)
            assert m is st.metas[s] and int(t.n_gt[j]) == len(m["class_ids"])
            assert t.class_ids[j, :len(m["class_ids"])].tolist() == m["class_ids"]
            assert torch.equal(t.rot[j].reshape(-1).cpu(), torch.from_numpy(st.table_f[s, 9:9 + MAX_GT * 9]))
            ids = set(torch.unique(t.mask[j]).tolist())
            assert 1.0 in ids and ids <= set(float(k) for k in range(len(m["class_ids"]) + 1))  # the crop shows object 0
    assert sorted(seen) == list(range(N))                                      # one pass visits every frame once


def test_two_loaders_with_one_seed_yield_equal_bytes(gpu_device):
    runs = []
    for _ in range(2):
        st = _store(gpu_device, seed=5)
        _seed()
        runs.append([_bytes(b) for b in _loader(st, gpu_device)])
    for x, y in zip(*runs):
        assert all(torch.equal(p, q) for p, q in zip(x[:4], y[:4])) and x[4] == y[4]
    other = _store(gpu_device, seed=6)
    assert not torch.equal(other.frames, st.frames)


def test_masks_lie_inside_the_projected_vertices(gpu_device):
    st = _shared_store(gpu_device)
    masks = st.masks.cpu().numpy()
    frames = st.frames.cpu().numpy()
    K = st.K
    multi = 0
    for s, m in enumerate(st.metas):
        g_n = len(m["class_ids"])
        multi += g_n > 1
        boxes = []
        for c, R, T in zip(m["class_ids"], m["rotations"], m["translations"]):
            v = np.asarray(st.meshes[c].vertices, np.float64)
            uv = K @ (R @ v.T + T)
            boxes.append((uv[0] / uv[2], uv[1] / uv[2]))
        for g, (u, v) in enumerate(boxes):
            ys, xs = np.nonzero(masks[s] == g + 1)
            assert len(ys) > 0
            assert xs.min() >= np.floor(u.min()) and xs.max() <= np.ceil(u.max())
            assert ys.min() >= np.floor(v.min()) and ys.max() <= np.ceil(v.max())
            others = [b for k, b in enumerate(boxes) if k != g]
            apart = all(u.max() < ou.min() - 1 or u.min() > ou.max() + 1 or v.max() < ov.min() - 1 or v.min() > ov.max() + 1
                        for ou, ov in others)
            if apart:                                          # unoccluded: the mask reaches the outline, within a pixel
                assert abs(xs.min() - u.min()) <= 1 and abs(xs.max() - u.max()) <= 1
                assert abs(ys.min() - v.min()) <= 1 and abs(ys.max() - v.max()) <= 1
        assert (masks[s] > g_n).sum() == 0
        bg = st.pool["backgrounds"]
        assert any(np.array_equal(frames[s][masks[s] == 0], b[masks[s] == 0]) for b in bg)   # the rest is a background
    assert multi >= 1


def test_refresh_on_the_device_is_in_place_and_new(gpu_device):
    st = _store(gpu_device, seed=7)
    ptr, old = st.frames.data_ptr(), st.frames.clone()
    st.refresh()
    assert st.frames.data_ptr() == ptr and not torch.equal(st.frames, old)
    again = _store(gpu_device, seed=7)
    again.refresh()
    assert torch.equal(again.frames, st.frames) and torch.equal(again.masks, st.masks)


def test_the_augment_path_runs_one_batch(gpu_device):
    st = _shared_store(gpu_device)
    _seed()
    images, t, metas = next(iter(_loader(st, gpu_device, augment=True)))
    assert images.tensors.shape == (B, 3, 256, 256) and torch.isfinite(images.tensors).all()
    assert t.mask.shape == (B, 256, 256) and torch.isfinite(t.rot).all() and torch.isfinite(t.trans).all() and len(metas) == B


def test_one_optimiser_step_on_a_rendered_batch_is_finite_and_repeats_bitwise(gpu_device):
    from kd6d import backbone as BB
    from kd6d.models.model_kd import PoseModuleKD
    from kd6d.optim import FusedClipAdamW
    from oracle import kd_step_ref as O
    st = _shared_store(gpu_device)
    out = []
    for _ in range(2):
        _seed()
        from kd6d.libs.train_libs import RenderedDziLoader
        cfg = _cfg()
        images, t, _ = next(iter(RenderedDziLoader(st, cfg, gpu_device, True, 2)))
        cfg["KD"] = dict(LOSS_WEIGHT_KD=0.0, LEVEL="pred", GLEVEL="point", GTYPE="sinkhorn", GP=2.0, GBLUR=0.001, GnD=2,
                         WEIGHTED_OT=True, DETACH=False, SCALING=0.5, REACH=0.5)
        model = PoseModuleKD(cfg, BB.darknet_tiny_h())
        model.load_state_dict(O.seeded_state_dict(O.PoseNetRef("darknet_tiny_h"), 1))
        model = model.to(gpu_device).train()
        opt = FusedClipAdamW(model, lr=1e-3)
        model.zero_grad()
        _, ld = model(images, targets=t, pred_t=None)
        (ld["loss_cls"] * 0.1 + ld["loss_reg"]).backward()
        opt.step()
        torch.cuda.synchronize()
        vals = torch.stack([ld["loss_cls"].detach(), ld["loss_reg"].detach(), opt.grad_norm().detach().reshape(())]).cpu()
        print("rendered batch: loss_cls %.6f loss_reg %.6f grad_norm %.6f" % tuple(vals.tolist()))
        assert torch.isfinite(vals).all() and vals[0] > 0 and vals[1] > 0 and vals[2] > 0
        out.append(vals)
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


def test_vsd_setup_hands_out_the_renderers_depth(gpu_device):
    from kd6d import ops
    from kd6d.libs.train_libs import dataset_meshes, vsd_setup
    st = _store(gpu_device, seed=11, keep_depth=True)
    ld = _loader(st, gpu_device, training=False)
    verts = dataset_meshes(ld)
    assert len(verts) == 15 and verts[0].shape == (2562, 3)
    meshes, depth_fn = vsd_setup(_cfg() | {"RUNTIME": {"SYNTHETIC": False}}, ld, verts, gpu_device)
    assert meshes[3].faces.shape == (5120, 3)
    m = st.metas[1]
    d = depth_fn(m)
    assert d.shape == (H, W) and d.dtype == np.float32 and np.array_equal(d > 0, st.masks[1].cpu().numpy() > 0)
    # the first object's own depth render agrees wherever that object is the visible one
    c = m["class_ids"][0]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).to(gpu_device)  # noqa: E731
    own = ops.render_depth(t(meshes[c].vertices, np.float32), t(meshes[c].faces, np.int32), t([0], np.int32),
                           t([len(meshes[c].vertices)], np.int32), t([0], np.int32), t([len(meshes[c].faces)], np.int32),
                           t(st.K.reshape(1, 3, 3), np.float32), t(m["rotations"][0].reshape(1, 3, 3), np.float32),
                           t(m["translations"][0].reshape(1, 3), np.float32), H, W)[0].cpu().numpy()
    vis = st.masks[1].cpu().numpy() == 1
    assert vis.sum() > 100 and np.array_equal(own[vis].view(np.uint32), d[vis].view(np.uint32))


def test_eval_entry_on_rendered_frames(gpu_device, tmp_path):
    wd = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--config_file", os.path.join(ROOT, "configs", "ape.yaml"),
           "--backbone", "darknet_tiny_h", "--working_dir", wd, "--precision", "fp32", "--pnp_solver", "device",
           "--eval_scorer", "device", "--frame_source", "render", "--render_valid_frames", "8", "--render_instances", "2",
           "--bop_metrics", "--bop_vsd", "--num_workers", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rendered frames: 8 frames of 640x480" in r.stdout
    assert os.path.exists(os.path.join(wd, "preds.json"))
