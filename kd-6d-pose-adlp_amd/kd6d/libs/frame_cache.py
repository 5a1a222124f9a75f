"""Device-resident frame cache (train_kd.py / test.py --frame_cache device).

The BOP / LINEMOD lists are small (a few hundred frames for one class, ~15 000 for all 13) and a run visits every frame
tens to hundreds of times; the host loader decodes the frame's PNG and one mask PNG per instance on every visit and
uploads ~2 MB per image from pageable memory.  `DeviceFrameCache` decodes every frame of a data set ONCE, through the
readers the data set itself uses (`load_image_cached`, `normalise_frame`, `get_single_bop_annotation` -- not through
`__getitem__`: no augmentation parameter is drawn and nothing is resampled while it builds), and keeps, on the device,

    frames   (n, H, W, 3) uint8, BGR as the data set yields it
    masks    (n, H, W) uint8, the merged instance image
    table_f  (n, 9 + MAX_GT*12) float32  per frame {K, rot[MAX_GT], trans[MAX_GT]}, zero-padded like PackedTargets
    table_i  (n, 1 + MAX_GT) int32       per frame {n_gt, class_ids[MAX_GT]}
    kp3d     (classes, 8, 3) float32, once per data set

plus, on the host, a copy of the two tables, every frame's `meta` dict (unchanged: evaluation reads it), its PoseAnnot
without the mask (the augmentation front-end and `projected_box` read it) and its DZI box.  Batches are then assembled
by csrc/frame_cache.hip from sampler indices (`kd6d.libs.train_libs.CachedDziLoader`).

A frame `BOP_Dataset.getitem1` would turn into None (unreadable file, or a training frame without a known object) gets
no slot; `resolve()` replaces its index the way `BOP_Dataset.__getitem__` does, so lengths and the `random` stream are
those of the host loader.  Storage (and the budget check) is sized for every list entry, since which frames are
unusable is known only after decoding.  There is no fall-back to the host path: a list that does not fit the budget, frames of
different sizes or too many instances raise.
"""
import bisect
import random
import time

import numpy as np
import torch

from .._lib import CACHE_ROW_F, CACHE_ROW_I, MAX_GT
from . import dataset as DS
from .poses import PoseAnnot

_CHUNK = 16          # frames per staging buffer / per decode batch


class _RawFrames(torch.utils.data.Dataset):
    """What the cache stores of item i of a list of BOP_Datasets: (i, frame uint8 (H,W,3), mask uint8 (H,W), meta), or
    (i, None) for a frame getitem1 would refuse.  Runs in the DataLoader workers of the build."""

    def __init__(self, parts):
        self.parts = parts
        self.starts = np.cumsum([0] + [len(p) for p in parts]).tolist()

    def __len__(self):
        return self.starts[-1]

    def __getitem__(self, i):
        p = bisect.bisect_right(self.starts, i) - 1
        ds = self.parts[p]
        path = ds.img_files[i - self.starts[p]]
        img = DS.load_image_cached(path, ds.cache)
        if img is None:
            print("image %s not found" % path)
            return i, None
        img = DS.normalise_frame(img)
        h, w = img.shape[:2]
        K, mask, class_ids, rotations, translations = DS.get_single_bop_annotation(path, ds.objID_2_clsID, ds.cache)
        if ds.training and len(class_ids) == 0:
            return i, None
        if mask is None:                       # a frame without any ground-truth entry
            mask = np.zeros((h, w), np.uint8)
        meta = {"path": path, "K": K, "width": w, "height": h, "class_ids": class_ids, "rotations": rotations,
                "translations": translations}
        return i, torch.from_numpy(np.ascontiguousarray(img[:, :, :3])), torch.from_numpy(np.ascontiguousarray(mask)), meta


def _as_list(batch):
    return batch


def _allocate(shape, dtype, device, pinned=False):
    """The ONE place the cache allocates frame storage (device arrays and the staging buffer)."""
    return torch.empty(shape, dtype=dtype, device="cpu" if pinned else device, pin_memory=pinned)


def table_rows(K, class_ids, rotations, translations):
    """One frame's rows of the annotation table, rounded and padded the way PackedTargets does it."""
    g = len(class_ids)
    if g > MAX_GT:
        raise ValueError("kd6d_ssc_assign handles at most %d instances per image" % MAX_GT)
    rf = np.zeros(CACHE_ROW_F, np.float32)
    ri = np.zeros(CACHE_ROW_I, np.int32)
    rf[0:9] = np.asarray(K, np.float64).reshape(9).astype(np.float32)
    rf[9:9 + g * 9] = np.asarray(rotations, np.float32).reshape(-1)
    rf[9 + MAX_GT * 9:9 + MAX_GT * 9 + g * 3] = np.asarray(translations, np.float32).reshape(-1)
    ri[0] = g
    ri[1:1 + g] = np.asarray(class_ids, np.int32).reshape(-1)
    return rf, ri


class DeviceFrameCache:
    def __init__(self, dataset, device, budget_bytes, num_workers=0, log=print):
        """dataset: a BOP_Dataset or a ConcatDataset of them.  budget_bytes bounds frames + masks; num_workers decode in
        parallel.  log: where the one build line goes (None: nowhere)."""
        t0 = time.time()
        self.parts = list(dataset.datasets) if hasattr(dataset, "datasets") else [dataset]
        self.device = torch.device(device)
        self.length = len(dataset)
        raw = _RawFrames(self.parts)
        assert len(raw) == self.length
        self.starts = raw.starts
        kp = self.parts[0].bbox_3d
        for p in self.parts[1:]:
            if p.bbox_3d.shape != kp.shape or not torch.equal(p.bbox_3d, kp):
                raise ValueError("frame cache: the data sets of one cache must share their 3D boxes (BBOX_FILE)")
        self.kp3d_host = kp.to(torch.float32).contiguous()
        self.slot_of = np.full(self.length, -1, np.int64)
        self.metas, self.targets, self.boxes = [], [], []
        self.frames = self.masks = None
        self.H = self.W = 0
        rows_f, rows_i = [], []
        pinned = self.device.type == "cuda"
        stage_f = stage_m = None
        first_path = None
        filled, flushed = 0, 0

        def flush():
            nonlocal filled, flushed
            if filled:
                self.frames[flushed:flushed + filled].copy_(stage_f[:filled], non_blocking=True)
                self.masks[flushed:flushed + filled].copy_(stage_m[:filled], non_blocking=True)
                if pinned:
                    torch.cuda.current_stream(self.device).synchronize()      # the staging buffer is reused
                flushed += filled
                filled = 0

        # a generator of its own: building the cache must not move torch's global RNG (the samplers seed from it)
        loader = torch.utils.data.DataLoader(raw, batch_size=_CHUNK, shuffle=False, num_workers=int(num_workers),
                                             collate_fn=_as_list, generator=torch.Generator())
        for batch in loader:
            for item in batch:
                if item[1] is None:
                    continue
                i, frame, mask, meta = item
                h, w = int(frame.shape[0]), int(frame.shape[1])
                if self.frames is None:
                    need = self.length * h * w * 4
                    if need > int(budget_bytes):
                        raise ValueError("frame cache: %d frames of %dx%d need %d bytes (%.3f GB) of device memory, "
                                         "--frame_cache_gb allows %d (%.3f GB); raise it or run with --frame_cache off"
                                         % (self.length, w, h, need, need / 2.0 ** 30, int(budget_bytes),
                                            int(budget_bytes) / 2.0 ** 30))
                    self.H, self.W, first_path = h, w, meta["path"]
                    self.frames = _allocate((self.length, h, w, 3), torch.uint8, self.device)
                    self.masks = _allocate((self.length, h, w), torch.uint8, self.device)
                    stage_f = _allocate((_CHUNK, h, w, 3), torch.uint8, self.device, pinned)
                    stage_m = _allocate((_CHUNK, h, w), torch.uint8, self.device, pinned)
                if (h, w) != (self.H, self.W):
                    raise ValueError("frame cache: all frames of one cache share one size, but %s is %dx%d and %s is %dx%d"
                                     % (first_path, self.W, self.H, meta["path"], w, h))
                if tuple(mask.shape) != (h, w):
                    raise ValueError("frame cache: the masks of %s are %dx%d, the frame is %dx%d"
                                     % (meta["path"], int(mask.shape[1]), int(mask.shape[0]), w, h))
                rf, ri = table_rows(meta["K"], meta["class_ids"], meta["rotations"], meta["translations"])
                slot = len(self.metas)
                self.slot_of[i] = slot
                stage_f[filled].copy_(frame)
                stage_m[filled].copy_(mask)
                filled += 1
                if filled == _CHUNK:
                    flush()
                rows_f.append(rf); rows_i.append(ri)
                self.metas.append(meta)
                g = len(meta["class_ids"])
                t = PoseAnnot(self.kp3d_host, torch.tensor(meta["K"], dtype=torch.float32), None,
                              torch.tensor(meta["class_ids"], dtype=torch.long),
                              torch.tensor(np.asarray(meta["rotations"], np.float32).reshape(-1, 3, 3)),
                              torch.tensor(np.asarray(meta["translations"], np.float32).reshape(-1, 3, 1)), w, h)
                self.targets.append(t)
                # the box DZI jitters (DziLoader): the projected 3D box of instance 0, the whole frame without one
                self.boxes.append(DS.projected_box(t, 0) if g else np.array([0.0, 0.0, float(w), float(h)]))
        flush()
        self.n = len(self.metas)
        if self.n == 0:
            raise ValueError("frame cache: none of the %d frames is usable" % self.length)
        self.n_invalid = self.length - self.n
        self.frames, self.masks = self.frames[:self.n], self.masks[:self.n]
        self.table_f = np.stack(rows_f)
        self.table_i = np.stack(rows_i)
        self.table_f_dev = torch.from_numpy(self.table_f).to(self.device)
        self.table_i_dev = torch.from_numpy(self.table_i).to(self.device)
        self.kp3d_dev = self.kp3d_host.to(self.device)
        self.nbytes = self.n * self.H * self.W * 4
        self.build_seconds = time.time() - t0
        if log is not None:
            log("frame cache: %d frames of %dx%d on %s, %d invalid, %d bytes (%.3f GB), built in %.1f s"
                % (self.n, self.W, self.H, self.device, self.n_invalid, self.nbytes, self.nbytes / 2.0 ** 30,
                   self.build_seconds))

    def __len__(self):
        return self.length

    def resolve(self, index):
        """Data set index -> slot.  An index without a slot is replaced as BOP_Dataset.__getitem__ replaces it: by
        random.randint over the frames of ITS list, until one is usable."""
        index = int(index)
        if not 0 <= index < self.length:
            raise IndexError("frame cache: index %d outside the data set of %d frames" % (index, self.length))
        slot = self.slot_of[index]
        if slot < 0:
            p = bisect.bisect_right(self.starts, index) - 1
            lo, cnt = self.starts[p], self.starts[p + 1] - self.starts[p]
            while slot < 0:
                slot = self.slot_of[lo + random.randint(0, cnt - 1)]
        return int(slot)

    def check_slots(self, slots):
        """The host-side validation of what goes to the device as gather indices."""
        bad = [int(s) for s in slots if not 0 <= int(s) < self.n]
        if bad:
            raise IndexError("frame cache: slots %s outside the %d cached frames" % (bad, self.n))

    def upload_slots(self, slots):
        self.check_slots(slots)
        return torch.tensor([int(s) for s in slots], dtype=torch.int32).to(self.device)

    def gather(self, slots):
        """-> (index on the device, frames (B,H,W,3) uint8, masks (B,H,W) float32): one upload, one launch."""
        from .. import ops
        index = self.upload_slots(slots)
        frames, masks = ops.cache_gather_frames(self.frames, self.masks, index)
        return index, frames, masks
