"""Model / optimiser builders with the reference's names (libs/train_libs.py:80-206).

build_model   -> (model, optimizer, scheduler, total_steps): AdamW(lr=BASE_LR/N_GPU, wd 1e-4,
                 eps 1e-8) + OneCycleLR(linear, pct_start .05, MAX_ITER+100) exactly as the
                 reference, with the optimiser fused into kd6d_clip_adamw (clip folded in).
build_model_teacher -> frozen teacher.
Data-parallel: parameters are broadcast from rank 0 once (the reference's DDP constructor does the
same before being discarded) and gradients are mean-all-reduced every step over RCCL.
"""
import os

import numpy as np
import torch
from torch import optim

from .. import backbone as _bb
from ..optim import FusedClipAdamW
from . import distributed as D


def build_backbone(arch):
    if arch == "darknet_tiny":
        return _bb.darknet_tiny(pretrained=True)
    if arch == "darknet_tiny_h":
        return _bb.darknet_tiny_h(pretrained=False)     # no pretrained weights exist for it
    if arch == "darknet53":
        return _bb.darknet53(pretrained=True)
    raise ValueError("unsupported backbone %r" % (arch,))


def _load_weights(model, path):
    if not path or not os.path.exists(path):
        print("-- Random initialized weights.")
        return False
    chkpt = torch.load(path, map_location="cpu")
    if "model" in chkpt:
        chkpt = chkpt["model"]
    own = model.state_dict()
    model.load_state_dict({k: v for k, v in chkpt.items() if k in own}, strict=False)
    print("Weights are loaded from " + path)
    return True


def build_model(cfg, posemodule, device="cuda"):
    model = posemodule(cfg, build_backbone(cfg["MODEL"]["BACKBONE"]))
    _load_weights(model, cfg["RUNTIME"].get("WEIGHT_FILE", ""))
    model = model.to(device)
    n_gpu = cfg["RUNTIME"].get("N_GPU", 1)
    base_lr = cfg["SOLVER"]["BASE_LR"] / n_gpu
    optimizer = FusedClipAdamW(model, lr=base_lr, weight_decay=0.0001, eps=1e-8,
                               max_norm=cfg["SOLVER"].get("GRAD_CLIP", 1.0))
    scheduler = optim.lr_scheduler.OneCycleLR(optimizer, base_lr, cfg["SOLVER"]["MAX_ITER"] + 100, pct_start=0.05,
                                              cycle_momentum=False, anneal_strategy="linear")
    if cfg["RUNTIME"].get("DISTRIBUTED", False) and not cfg["RUNTIME"].get("DEFER_BROADCAST", False):
        # (DEFER_BROADCAST: train_kd.py broadcasts after the step's graphs have been recorded, see there)
        D.broadcast_(model.net.store.params, 0)
        D.broadcast_(model.net.store.bufs, 0)
        model.net.invalidate()
    total_steps = 0
    wd = cfg["RUNTIME"].get("WORKING_DIR", "")
    latest = os.path.join(wd, "latest.pth") if wd else ""
    if latest and os.path.exists(latest):
        chkpt = torch.load(latest, map_location="cpu", weights_only=False)
        total_steps = chkpt["steps"]
        model.load_state_dict(chkpt["model"])
        # The optimiser and the scheduler are resumed independently.  An `optim` entry this optimiser cannot take
        # (e.g. one written by the reference's torch.optim.AdamW: per-tensor moments, not the flat buffers) only
        # restarts the Adam moments; the OneCycle schedule still continues from step N -- the reference's `sched`
        # entry is a plain torch scheduler state and loads as is, and a missing / unusable one is replaced by
        # fast-forwarding the fresh scheduler to `total_steps`.
        resumed = []
        try:
            optimizer.load_state_dict(chkpt["optim"])
            resumed.append("optimizer")
        except (ValueError, KeyError, TypeError) as e:
            print("optimiser state of %s NOT resumed (Adam moments restart): %s" % (latest, e))
        try:
            scheduler.load_state_dict(chkpt["sched"])
            if int(scheduler.last_epoch) != int(total_steps):
                raise ValueError("scheduler state is at step %d, checkpoint at %d" % (scheduler.last_epoch, total_steps))
            resumed.append("scheduler")
        except (ValueError, KeyError, TypeError, AttributeError) as e:
            print("scheduler state of %s NOT loaded (%s): fast-forwarding OneCycle to step %d" % (latest, e, total_steps))
            scheduler = _fast_forward_scheduler(optimizer, base_lr, cfg["SOLVER"]["MAX_ITER"] + 100, total_steps)
        lr_now = scheduler.get_last_lr()[0]
        for g in optimizer.param_groups:
            g["lr"] = lr_now
        print("Weights%s are loaded from %s, starting from step %d (lr %.6g)" % (
            "".join(", " + r for r in resumed), latest, total_steps, lr_now))
    return model, optimizer, scheduler, total_steps


def _fast_forward_scheduler(optimizer, base_lr, total, steps):
    """A fresh OneCycleLR (libs/train_libs.py:118-120) advanced to `steps` without touching the weights."""
    import warnings
    for g in optimizer.param_groups:          # OneCycleLR's constructor derives initial_lr / max_lr / min_lr again
        for k in ("initial_lr", "max_lr", "min_lr"):
            g.pop(k, None)
    sched = optim.lr_scheduler.OneCycleLR(optimizer, base_lr, total, pct_start=0.05, cycle_momentum=False,
                                          anneal_strategy="linear")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # "lr_scheduler.step() before optimizer.step()": intended here
        for _ in range(int(steps)):
            sched.step()
    return sched


def build_model_teacher(cfg, posemodule, device):
    model = posemodule(cfg, build_backbone(cfg["MODEL"]["BACKBONE"]))
    _load_weights(model, cfg["RUNTIME"].get("WEIGHT_FILE", ""))
    model = model.to(device)
    if cfg["RUNTIME"].get("DISTRIBUTED", False) and not cfg["RUNTIME"].get("DEFER_BROADCAST", False):
        # (DEFER_BROADCAST: train_kd.py broadcasts after the step's graphs have been recorded, see there)
        D.broadcast_(model.net.store.params, 0)
        D.broadcast_(model.net.store.bufs, 0)
        model.net.invalidate()
    return model


class DziLoader:
    """DataLoader of full frames -> what the reference's loaders yield after `dzi_train` / `dzi_test`
    (libs/dzi_libs.py:55-140) and `collate_fn`: (ImageList of 256x256 normalised crops, targets with the cropped mask,
    bbox_trans and bbox_scale, meta_infos).  Normalize + the affine crop of image and mask run as ONE kd6d_dzi_crop
    launch per batch on the GPU; the three jitter numbers per image come from numpy's global RNG like the reference.
    Without `augment`, frames must already have the internal resolution.  With `augment=True` (train_kd.py --augment;
    the dataset must have been built with augment too) the reference's train transform chain -- Resize to INTERNAL_K,
    occlusion, shift-scale-rotate, HSV, blur, noise, grey, remove_invalids(10), symmetry handling -- runs first,
    on the GPU (kd6d/libs/augment.py, csrc/augment.hip), and the crop box comes from the remapped pose."""

    def __init__(self, loader, cfg, device, training, augment=False):
        from .dzi_libs import normalize_lut
        self.loader, self.cfg, self.device, self.training = loader, cfg, device, training
        self.lut = normalize_lut(cfg["INPUT"]["PIXEL_MEAN"], cfg["INPUT"]["PIXEL_STD"], device)
        self.size = (cfg["INPUT"]["INTERNAL_HEIGHT"], cfg["INPUT"]["INTERNAL_WIDTH"])
        self.front = None
        if augment:
            from .augment import AugConfig, AugmentFront
            self.front = AugmentFront(AugConfig(cfg), device)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from ..kd_losses import PackedTargets
        from .dataset import projected_box
        from .dzi_libs import aug_bbox_DZI, dzi_batch, test_bbox_DZI
        from .poses import ImageList, PoseAnnot
        if self.front is not None:
            yield from self._iter_augment()
            return
        for frames, masks, targets, metas in self.loader:
            B, H, W, _ = frames.shape
            if (H, W) != tuple(self.size):
                raise ValueError("frames are %dx%d but INPUT.INTERNAL_* is %dx%d: the CPU Resize transform of the reference "
                                 "is not rebuilt, store the frames at the internal resolution" % (W, H, self.size[1], self.size[0]))
            centers, scales = [], []
            for t in targets:
                # to_object_boxlist().bbox[0]; a frame without a known object (the reference would fail on it) is
                # cropped around the whole frame
                box = projected_box(t, 0) if len(t.class_ids) else np.array([0.0, 0.0, float(W), float(H)])
                c, s = aug_bbox_DZI(box, H, W) if self.training else test_bbox_DZI(box, H, W)
                centers.append(c); scales.append(s)
            images, crop_masks, trans, bscale = dzi_batch(frames.to(self.device, non_blocking=True).contiguous(),
                                                          masks.to(self.device, non_blocking=True).contiguous(),
                                                          np.stack(centers), np.asarray(scales), self.lut)
            R = images.shape[-1]
            dev = self.device
            out = [PoseAnnot(t.keypoints_3d.to(dev), t.K.to(dev), crop_masks[i], t.class_ids.to(dev), t.rotations.to(dev),
                             t.translations.to(dev), R, R, bscale[i], trans[i]) for i, t in enumerate(targets)]
            yield ImageList(images, [(R, R)] * B), PackedTargets(out, dev), metas

    def _iter_augment(self):
        dev = self.device
        for batch in self.loader:
            if len(batch) != 5:
                raise ValueError("DziLoader(augment=True) needs a dataset built with augment (BOP_Dataset(augment=cfg))")
            frames, masks, targets, metas, params = batch
            yield self._augment_batch(frames.to(dev, non_blocking=True).contiguous(),
                                      masks.to(dev, non_blocking=True).contiguous(), targets, metas, params)

    def _augment_batch(self, frames, masks, targets, metas, params):
        """Device frames / float masks of one batch, the items' PoseAnnots and collated parameters -> the yielded triple:
        the augmentation front-end, the DZI crop around the remapped pose's box, the targets from the remapped poses."""
        from ..kd_losses import PackedTargets
        from .dataset import projected_box
        from .dzi_libs import aug_bbox_DZI, dzi_batch, test_bbox_DZI
        from .poses import ImageList, PoseAnnot
        dev = self.device
        K = torch.tensor(self.front.ac.K, dtype=torch.float32)
        H, W = self.size
        frames, masks, poses = self.front.run(frames, masks, targets, params)
        B = frames.shape[0]
        annots, centers, scales = [], [], []
        for t, (cls, Rs, Ts) in zip(targets, poses):
            a = PoseAnnot(t.keypoints_3d, K, None, torch.from_numpy(cls), torch.from_numpy(Rs).reshape(-1, 3, 3),
                          torch.from_numpy(Ts).reshape(-1, 3, 1), W, H)
            box = projected_box(a, 0) if len(cls) else np.array([0.0, 0.0, float(W), float(H)])
            c, s = aug_bbox_DZI(box, H, W) if self.training else test_bbox_DZI(box, H, W)
            centers.append(c); scales.append(s)
            annots.append(a)
        images, crop_masks, trans, bscale = dzi_batch(frames, masks, np.stack(centers), np.asarray(scales), self.lut)
        R = images.shape[-1]
        out = [PoseAnnot(a.keypoints_3d.to(dev), a.K.to(dev), crop_masks[i], a.class_ids.to(dev), a.rotations.to(dev),
                         a.translations.to(dev), R, R, bscale[i], trans[i]) for i, a in enumerate(annots)]
        return ImageList(images, [(R, R)] * B), PackedTargets(out, dev), metas


class _Indices(torch.utils.data.Dataset):
    """Item i is i: a DataLoader over it yields the sampler's index batches and moves the RNGs exactly as the host
    loader's DataLoader does (the base seed an iterator draws, then the sampler's own)."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return int(i)


class CachedDziLoader(DziLoader):
    """DziLoader over a device-resident frame cache (--frame_cache device; kd6d/libs/frame_cache.py): same length, same
    `.loader.dataset`, same yielded triple, and -- with NUM_WORKERS=0 on the host side -- the same bytes, because the same
    sampler object orders the frames, the same `random` / numpy draws follow in the same order and the gathered frames
    go through the unchanged kd6d_dzi_crop / AugmentFront.  `loader` is the host DataLoader the run would have used; it
    is kept for its length, data set and sampler and never iterated."""

    def __init__(self, loader, cfg, device, training, augment=False, budget_bytes=64 * 2 ** 30, log=print, cache=None):
        """cache: a store with DeviceFrameCache's interface to iterate over instead of building one (RenderedDziLoader)."""
        super().__init__(loader, cfg, device, training, augment=augment)
        if cache is None:
            from .frame_cache import DeviceFrameCache
            cache = DeviceFrameCache(loader.dataset, device, budget_bytes,
                                     num_workers=cfg["RUNTIME"].get("NUM_WORKERS", 0), log=log)
        self.cache = cache
        H, W = self.cache.H, self.cache.W
        if self.front is None and (H, W) != tuple(self.size):
            raise ValueError("frames are %dx%d but INPUT.INTERNAL_* is %dx%d: the CPU Resize transform of the reference "
                             "is not rebuilt, store the frames at the internal resolution" % (W, H, self.size[1], self.size[0]))
        self.indices = torch.utils.data.DataLoader(_Indices(len(loader.dataset)), batch_size=loader.batch_size,
                                                   sampler=loader.sampler, num_workers=0, collate_fn=list,
                                                   drop_last=loader.drop_last)

    def __iter__(self):
        from .. import ops
        from ..kd_losses import PackedTargets
        from .dzi_libs import aug_bbox_DZI, dzi_batch, test_bbox_DZI
        from .poses import ImageList
        if self.front is not None:
            yield from self._iter_augment()
            return
        c = self.cache
        H, W = c.H, c.W
        for idx in self.indices:
            slots = [c.resolve(i) for i in idx]
            B = len(slots)
            centers, scales = [], []
            for s in slots:
                ctr, sc = aug_bbox_DZI(c.boxes[s], H, W) if self.training else test_bbox_DZI(c.boxes[s], H, W)
                centers.append(ctr); scales.append(sc)
            index, frames, masks = c.gather(slots)
            images, crop_masks, trans, bscale = dzi_batch(frames, masks, np.stack(centers), np.asarray(scales), self.lut)
            flat_f, flat_i = ops.cache_gather_targets(c.table_f_dev, c.table_i_dev, c.kp3d_dev, index, trans)
            R = images.shape[-1]
            yield (ImageList(images, [(R, R)] * B), PackedTargets.from_packed(crop_masks, flat_f, flat_i, B),
                   [c.metas[s] for s in slots])

    def _iter_augment(self):
        from .augment import collate_params, draw_params
        c = self.cache
        ac = self.front.ac
        bbox_3d = c.kp3d_host.numpy()
        for idx in self.indices:
            # per index, in batch order: the resample draws, then the item's augmentation parameters -- the order in which
            # BOP_Dataset.__getitem__ consumes `random` without workers
            slots, params = [], []
            for i in idx:
                s = c.resolve(i)
                m = c.metas[s]
                slots.append(s)
                params.append(draw_params(ac, m["K"], m["class_ids"], m["rotations"], m["translations"], bbox_3d))
            _, frames, masks = c.gather(slots)
            yield self._augment_batch(frames, masks, [c.targets[s] for s in slots], [c.metas[s] for s in slots],
                                      collate_params(params))


class RenderedDziLoader(CachedDziLoader):
    """CachedDziLoader over a store that is handed in, not built: the rendered frames of kd6d/libs/render_source.py
    (--frame_source render).  The sampler runs over the store's slots (shuffled and dropping the last partial batch when
    `training`, DistributedSampler semantics under torch.distributed), and everything after it -- the DZI jitter from
    numpy's global stream, kd6d_dzi_crop, AugmentFront with --augment, the device pose remap -- is CachedDziLoader's,
    unchanged.  `.loader.dataset` has the `meshes` / `bbox_3d` dataset_meshes and vsd_setup read.  refresh_every_epoch:
    the store is redrawn and re-rendered after each pass (train_kd.py --render_refresh epoch)."""

    def __init__(self, store, cfg, device, training, batch_size, augment=False, distributed=False, refresh_every_epoch=False):
        from torch.utils.data import DataLoader
        dset = store.dataset
        if distributed:
            smp = D.DistributedSampler(dset, shuffle=training)
        elif training:
            smp = torch.utils.data.RandomSampler(dset)
        else:
            smp = torch.utils.data.SequentialSampler(dset)
        loader = DataLoader(dset, batch_size=int(batch_size), sampler=smp, num_workers=0, collate_fn=list,
                            drop_last=bool(training))
        super().__init__(loader, cfg, device, training, augment=augment, cache=store)
        self.refresh_every_epoch = bool(refresh_every_epoch)

    def __iter__(self):
        yield from super().__iter__()
        if self.refresh_every_epoch:
            self.cache.refresh()


RENDER_TRAIN_LIST, RENDER_VALID_LIST = 0, 1     # the last element of a rendered list's seed sequence (seed, rank, list)


def build_rendered_dataset(cfg, device="cuda", augment=False, training=True, render_fn=None, log=print):
    """--frame_source render: -> (train RenderedDziLoader or None, valid RenderedDziLoader) over frames drawn by
    csrc/render_frames.hip (kd6d/libs/render_source.py) at INPUT.INTERNAL_* under INPUT.INTERNAL_K.  RUNTIME keys:
    RENDER_MESHES (dataset: the PLYs of DATASETS.MESH_DIR with DATASETS.BBOX_FILE; surrogate: synthetic.surrogate_mesh
    with cube_keypoints), RENDER_FRAMES / RENDER_VALID_FRAMES, RENDER_INSTANCES, RENDER_REFRESH, RENDER_BACKGROUNDS,
    RENDER_SEED (the training list is seeded with the sequence (seed, rank, 0): every rank renders its own frames; the valid
    list with (seed, 0, 1), the same on every rank and never refreshed), RENDER_CLASSES (default: class 0 alone for one
    instance per frame, the LINEMOD classes otherwise; every class with `dataset` meshes), FRAME_CACHE_GB (the budget of
    each list).  training=False (test.py): the valid list alone."""
    from . import render_source as RS
    rt, ds = cfg["RUNTIME"], cfg["DATASETS"]
    H, W = int(cfg["INPUT"]["INTERNAL_HEIGHT"]), int(cfg["INPUT"]["INTERNAL_WIDTH"])
    K = np.asarray(cfg["INPUT"]["INTERNAL_K"], np.float64).reshape(3, 3)
    kind = rt.get("RENDER_MESHES", "surrogate")
    inst = int(rt.get("RENDER_INSTANCES", 1))
    if kind == "dataset":
        from .dataset import load_bbox_3d
        meshes = RS.dataset_meshes_colored(ds["MESH_DIR"])
        kp3d = torch.tensor(load_bbox_3d(ds["BBOX_FILE"]), dtype=torch.float32)
        classes = rt.get("RENDER_CLASSES") or list(range(min(len(meshes), len(kp3d))))
    elif kind == "surrogate":
        from ..synthetic import LINEMOD_CLASSES
        diam = ds.get("MESH_DIAMETERS")
        meshes, kp3d = RS.surrogate_meshes(int(ds["N_CLASS"]) - 1, int(rt.get("RENDER_SURROGATE_LEVEL", 4)), diam)
        classes = rt.get("RENDER_CLASSES") or ([0] if inst == 1 else [c for c in LINEMOD_CLASSES if c < len(meshes)])
    else:
        raise ValueError("RENDER_MESHES must be dataset or surrogate (got %r)" % (kind,))
    rank = D.get_rank() if rt.get("DISTRIBUTED", False) else 0
    seed = int(rt.get("RENDER_SEED", 0))
    budget = int(float(rt.get("FRAME_CACHE_GB", 64.)) * 2 ** 30)
    common = dict(instances=inst, classes=classes, backgrounds=rt.get("RENDER_BACKGROUNDS", "noise"), budget_bytes=budget,
                  render_fn=render_fn, log=log)
    train = None
    if training:
        store = RS.RenderedFrames(meshes, kp3d, int(rt.get("RENDER_FRAMES", 2048)), K, H, W, device, seed=(seed, rank, RENDER_TRAIN_LIST), training=True,
                                  tag="render_train", **common)
        train = RenderedDziLoader(store, cfg, device, True, D.shard_batch(cfg["SOLVER"]["IMS_PER_BATCH"]), augment=bool(augment),
                                  refresh_every_epoch=rt.get("RENDER_REFRESH", "epoch") == "epoch")
        per_gpu = D.shard_batch(cfg["SOLVER"]["IMS_PER_BATCH"])
    else:
        per_gpu = int(cfg.get("TEST", {}).get("IMS_PER_BATCH", cfg["SOLVER"]["IMS_PER_BATCH"]))
    vstore = RS.RenderedFrames(meshes, kp3d, int(rt.get("RENDER_VALID_FRAMES", 256)), K, H, W, device,
                               seed=(seed, 0, RENDER_VALID_LIST), training=False, tag="render_valid",
                               keep_depth=bool(rt.get("BOP_VSD", False)), **common)
    # the valid list is the same on every rank (a fixed seed, no rank in it): the ranks share it out like a listed one;
    # a rank's training frames are its own, so its sampler runs over all of them
    return train, RenderedDziLoader(vstore, cfg, device, False, per_gpu, distributed=bool(rt.get("DISTRIBUTED", False)))


FRAME_CACHE_MODES = ("off", "device")


def _wrap_loader(loader, cfg, device, training, augment, frame_cache, frame_cache_gb):
    if frame_cache not in FRAME_CACHE_MODES:
        raise ValueError("frame_cache must be one of %s (got %r)" % (FRAME_CACHE_MODES, frame_cache))
    if frame_cache == "device":
        return CachedDziLoader(loader, cfg, device, training, augment=augment,
                               budget_bytes=int(float(frame_cache_gb) * 2 ** 30))
    return DziLoader(loader, cfg, device, training, augment=augment)


def build_dataset(cfg, device="cuda", augment=False, frame_cache="off", frame_cache_gb=64.):
    """libs/train_libs.py:209-291: (train_loader, valid_loader) over the BOP image lists of cfg['DATASETS'], batch
    = IMS_PER_BATCH / N_GPU per rank, DistributedSampler semantics of libs/distributed.py.  DATASETS.TRAIN may be one
    list file or several (configs/linemod13.yaml): the datasets are concatenated.  augment=True runs the reference's
    train transform chain on the training batches (DziLoader); the valid loader is untouched.  frame_cache="device"
    (train_kd.py --frame_cache device): both loaders are CachedDziLoaders -- every frame decoded once and kept in device
    memory, at most frame_cache_gb GiB per loader and process; same samplers, same batches."""
    from torch.utils.data import ConcatDataset, DataLoader
    from .dataset import BOP_Dataset, collate_frames
    ds = cfg["DATASETS"]

    aug = False
    if augment:
        from .augment import AugConfig
        aug = AugConfig(cfg)                 # raises NotImplementedError for the transforms that are not rebuilt

    def make(files, training, augment=False):
        files = [files] if isinstance(files, str) else list(files)
        sets = [BOP_Dataset(f, ds["MESH_DIR"], ds["BBOX_FILE"], ds.get("SYMMETRY_TYPES"), training=training,
                            augment=augment) for f in files]
        return sets[0] if len(sets) == 1 else ConcatDataset(sets)

    train_set, valid_set = make(ds["TRAIN"], True, aug), make(ds["VALID"], False)
    per_gpu = D.shard_batch(cfg["SOLVER"]["IMS_PER_BATCH"])
    dist_on = cfg["RUNTIME"].get("DISTRIBUTED", False)

    def loader(dset, shuffle):
        if dist_on:
            smp = D.DistributedSampler(dset, shuffle=shuffle)
        elif shuffle:
            smp = torch.utils.data.RandomSampler(dset)
        else:
            smp = torch.utils.data.SequentialSampler(dset)
        return DataLoader(dset, batch_size=per_gpu, sampler=smp, num_workers=cfg["RUNTIME"].get("NUM_WORKERS", 0),
                          collate_fn=collate_frames, drop_last=shuffle)

    return (_wrap_loader(loader(train_set, True), cfg, device, True, bool(augment), frame_cache, frame_cache_gb),
            _wrap_loader(loader(valid_set, False), cfg, device, False, False, frame_cache, frame_cache_gb))


def build_test_dataset(cfg, device="cuda", frame_cache="off", frame_cache_gb=64.):
    """test.py:74-134 of the reference: the valid-style loader (no shuffle, no augmentation, DZI crop) over the image
    list(s) of DATASETS.TEST, for one process.  frame_cache / frame_cache_gb: as in build_dataset."""
    from torch.utils.data import ConcatDataset, DataLoader
    from .dataset import BOP_Dataset, collate_frames
    ds = cfg["DATASETS"]
    files = [ds["TEST"]] if isinstance(ds["TEST"], str) else list(ds["TEST"])
    sets = [BOP_Dataset(f, ds["MESH_DIR"], ds["BBOX_FILE"], ds.get("SYMMETRY_TYPES"), training=False) for f in files]
    dset = sets[0] if len(sets) == 1 else ConcatDataset(sets)
    per_gpu = int(cfg.get("TEST", {}).get("IMS_PER_BATCH", cfg["SOLVER"]["IMS_PER_BATCH"]))
    loader = DataLoader(dset, batch_size=per_gpu, sampler=torch.utils.data.SequentialSampler(dset),
                        num_workers=cfg["RUNTIME"].get("NUM_WORKERS", 0), collate_fn=collate_frames)
    return _wrap_loader(loader, cfg, device, False, False, frame_cache, frame_cache_gb)


def dataset_meshes(loader):
    """Mesh vertex arrays per class id of a DziLoader's dataset (what valid() measures ADI / REP on)."""
    dset = loader.loader.dataset
    dset = dset.datasets[0] if hasattr(dset, "datasets") else dset
    return [m.vertices for m in dset.meshes]


def vsd_setup(cfg, loader, meshes, device):
    """--bop_vsd: -> (meshes WITH faces, depth provider) for valid(..., vsd=).  Real data: the dataset's meshes as
    load_bop_meshes read them and dataset.load_depth_mm of the frame's path.  --synthetic: the surrogate meshes (the 8
    cube corners) get the cube's 12 triangles, and a frame's depth is the render of all its ground-truth objects (there
    are no depth images) at INPUT.INTERNAL_WIDTH x INTERNAL_HEIGHT: the synthetic poses and the K of their metas belong
    to that frame, not to the crop the network sees -- at the crop's size most objects would lie outside the image."""
    from .dataset import Mesh, load_depth_mm
    if cfg["RUNTIME"]["SYNTHETIC"]:
        from ..synthetic import CUBE_FACES
        from .bop_metrics import rendered_depth_provider
        ms = [Mesh(m, CUBE_FACES) for m in meshes]
        return ms, rendered_depth_provider(ms, device, int(cfg["INPUT"].get("INTERNAL_HEIGHT", 480)),
                                           int(cfg["INPUT"].get("INTERNAL_WIDTH", 640)))
    dset = loader.loader.dataset
    dset = dset.datasets[0] if hasattr(dset, "datasets") else dset
    if hasattr(dset, "rendered_depth"):                  # --frame_source render: D_test is the depth the renderer wrote
        return list(dset.meshes), dset.rendered_depth
    cache = {}
    return list(dset.meshes), lambda meta: load_depth_mm(meta["path"], cache)


def start_exchange_after_graphs(gstep, model_t, model, first_batch, log=print):
    """Data-parallel run in the grouped launch mode (train_kd.py --launch pipeline --teacher_group > 1, `between` exchange):
    the step's hipGraphs are recorded BEFORE the process's first RCCL communicator exists (graphs instantiated after
    ncclCommInitRank replay ~18 % slower in that mode).  Order, every rank alike:
      1. gstep.prepare(first batch)      every graph recorded, pipeline left empty, training state untouched
      2. barrier, init_exchange()        the ranks agree, then the kd6d communicator (kd6d_comm_init is collective)
      3. broadcast rank 0's parameters and buffers of teacher and student (what build_model* deferred:
         libs/train_libs.py:123-130 of the reference, the DDP constructor's broadcast)
      4. refresh IN PLACE what the recorded kernels read of them: bf16 shadows, the student's dgrad packing and the
         teacher's eval-mode BatchNorm folds (PoseNet.refresh_derived_in_place; the teacher's segments were recorded on
         its pre-broadcast folds and shadow -- a rank whose initial teacher differed from rank 0's would otherwise distil
         from a different teacher)
    The first batch is then fed as usual by the caller.  Returns the exchange route string."""
    gstep.prepare(first_batch[0], first_batch[1])
    D.synchronize()
    route = D.init_exchange()
    log("gradient exchange: " + route)
    for m in (model_t, model):
        D.broadcast_(m.net.store.params, 0)
        D.broadcast_(m.net.store.bufs, 0)
    model_t.net.refresh_derived_in_place(need_dgrad=False)
    model.net.refresh_derived_in_place(need_dgrad=True)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return route


def stop_if_barrier_timeouts(n_local, distributed):
    """In-kernel barriers of the one-launch BN / GN backward give up after a bounded spin instead of hanging the GPU; a
    wait that gave up means wrong gradients, so training stops.  The decision is COLLECTIVE (MAX over ranks of the
    per-device counter): a rank that stopped alone would leave the others waiting in the next gradient all-reduce.
    Every rank shuts its exchange down and leaves the process group before raising."""
    n_to = D.max_over_ranks(n_local)
    if n_to != 0:
        D.shutdown_exchange()
        if distributed and torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()
        raise SystemExit("kd6d: %d in-kernel barrier waits timed out (gradients of a step are wrong); "
                         "re-run with --two_launch_norm_bwd" % n_to)
    return 0

