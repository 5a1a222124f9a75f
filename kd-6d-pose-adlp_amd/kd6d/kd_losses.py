"""Host orchestration of the loss side of the KD step (no arithmetic: kernel launches only).

Replaces the Python of losses/kd_loss.py:111-160 (KDPoseLoss.__call__), :40-109
(KDObjectSpaceLoss), losses/loss_libs.py:1-51 (kd_loss_2d), losses/loss.py:164-268
(prepare_targets) and postprocess/postprocess_kd.py (teacher knowledge) with one launch each and
no device->host synchronisation anywhere in the step.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import Levels, check, lib

ANCHOR_SIZES = [32, 64, 128, 256, 512]
ANCHOR_STRIDES = [8, 16, 32, 64, 128]
CAP = 32          # slots per image for teacher cells / pose candidates (one class: <= 12; the PnP kernels take <= 32)
MAX_GT = _lib.MAX_GT
PER_OBJECT_GATE_ERROR = ("--kd_per_object cannot be combined with --teacher_pnp_gate: the gate solves one pose per image "
                         "from the image's cells, a per-object gate is not implemented")


def check_gtype(gtype, kernel_losses, blur):
    """The one rule for --gtype / SamplesLoss(loss): -> None for 'sinkhorn', the KD6D_KERNEL_* code for a kernel
    distance when kernel_losses (--kd_kernel_losses, SamplesLoss(kernel_losses=True)) opts in; everything else is refused."""
    if gtype == "sinkhorn":
        return None
    if gtype in ("l1", "l2"):
        raise NotImplementedError("--gtype %s: geomloss has no such loss (geomloss.SamplesLoss knows sinkhorn, hausdorff, "
                                  "energy, gaussian and laplacian; the reference itself fails on %r)" % (gtype, gtype))
    if gtype not in _lib.KERNEL_KINDS:
        raise NotImplementedError("only --gtype sinkhorn, gaussian, laplacian and energy are implemented on the HIP path "
                                  "(got %r)" % (gtype,))
    if not kernel_losses:
        raise NotImplementedError("only --gtype sinkhorn is implemented on the HIP path by default (got %r): the kernel "
                                  "distances gaussian / laplacian / energy are opt-in, pass --kd_kernel_losses "
                                  "(cfg['KD']['KERNEL_LOSSES'], SamplesLoss(kernel_losses=True))" % (gtype,))
    if gtype != "energy" and not blur > 0:
        raise ValueError("--gtype %s needs --blur > 0 (got %r)" % (gtype, blur))
    return _lib.KERNEL_KINDS[gtype]


def positives_bound(positive_num, n_levels=_lib.MAX_SEG, instances=MAX_GT):
    """Most positive cells kd6d_ssc_assign can pick in one image: per instance the per-level shares of positive_num,
    each rounded half up, i.e. at most floor(positive_num + 0.5 * levels) (include/kd6d.h, kd6d_ssc_assign)."""
    return instances * int(float(positive_num) + 0.5 * n_levels)


POS_CAP = positives_bound(10)      # 48: slots per image for the student's positives at the reference's POSITIVE_NUM


def make_levels(batch, shapes, sizes=ANCHOR_SIZES, strides=ANCHOR_STRIDES):
    lv = Levels()
    lv.n, lv.batch = len(shapes), batch
    for i in range(_lib.MAX_SEG):
        lv.anchor_size[i] = float(sizes[i])
        lv.anchor_stride[i] = float(strides[i])
        if i < len(shapes):
            lv.h[i], lv.w[i] = shapes[i]
    return lv


class PackedTargets:
    """list[PoseAnnot] -> dense device tensors, padded to MAX_GT instances per image."""

    def __init__(self, targets, device):
        B = len(targets)
        self.batch = B
        f32 = dict(dtype=torch.float32, device=device)
        self.mask = torch.stack([t.mask.to(device=device, dtype=torch.float32) for t in targets]).contiguous()
        self.mask_h, self.mask_w = int(self.mask.shape[1]), int(self.mask.shape[2])
        self.kp3d = torch.stack([t.keypoints_3d.to(**f32) for t in targets]).contiguous()     # (B,15,8,3)
        self.K = torch.stack([t.K.to(**f32) for t in targets]).contiguous()
        self.bbox_trans = torch.stack([t.bbox_trans.to(**f32) for t in targets]).contiguous()
        cls = torch.full((B, MAX_GT), 0, dtype=torch.int32)
        ngt = torch.zeros(B, dtype=torch.int32)
        rot = torch.zeros(B, MAX_GT, 3, 3)
        tr = torch.zeros(B, MAX_GT, 3)
        same_dev = all(t.class_ids.device == torch.device(device) for t in targets) and torch.device(device).type != "cpu"
        if same_dev:
            # inputs already resident on the device: assemble there (no host round trip)
            cls, ngt, rot, tr = cls.to(device), ngt.to(device), rot.to(device), tr.to(device)
        for i, t in enumerate(targets):
            g = min(len(t.class_ids), MAX_GT)
            if len(t.class_ids) > MAX_GT:
                raise ValueError("kd6d_ssc_assign handles at most %d instances per image" % MAX_GT)
            cls[i, :g] = t.class_ids[:g].to(torch.int32)
            ngt[i] = g
            rot[i, :g] = t.rotations[:g].to(torch.float32)
            tr[i, :g] = t.translations[:g].reshape(g, 3).to(torch.float32)
        self.class_ids = cls.to(device).contiguous()
        self.n_gt = ngt.to(device).contiguous()
        self.rot = rot.to(device).contiguous()
        self.trans = tr.to(device).contiguous()
        self.frame_wh = (640.0, 480.0)        # kd_loss.py:116-117 ("not 256")
        self._pack_small()

    _SMALL_F = ("kp3d", "K", "bbox_trans", "rot", "trans")
    _SMALL_I = ("class_ids", "n_gt")

    @classmethod
    def from_packed(cls, mask, flat_f, flat_i, batch):
        """A batch whose small fields are already packed on the device (kd6d_cache_gather_targets wrote flat_f / flat_i
        in the layout of _SMALL_F / _SMALL_I): adopts the three buffers, then moves them into one block exactly as
        __init__ does.  mask (batch, h, w) float32; the class count follows from flat_f's size."""
        B = int(batch)
        assert mask.dtype == torch.float32 and mask.dim() == 3 and mask.shape[0] == B and mask.is_contiguous()
        assert flat_f.dtype == torch.float32 and flat_i.dtype == torch.int32
        up = lambda v: (v + 3) // 4 * 4
        kp = flat_f.numel() - (up(B * 9) + up(B * 6) + up(B * MAX_GT * 9) + up(B * MAX_GT * 3))
        if kp <= 0 or kp % (B * 24) or flat_i.numel() != up(B * MAX_GT) + up(B):
            raise ValueError("PackedTargets.from_packed: buffers of %d fp32 / %d int32 elements are not the packed layout "
                             "of %d images" % (flat_f.numel(), flat_i.numel(), B))
        out = object.__new__(cls)
        out.batch = B
        out.mask, out.flat_f, out.flat_i = mask, flat_f, flat_i
        out.mask_h, out.mask_w = int(mask.shape[1]), int(mask.shape[2])
        shapes = dict(kp3d=(B, kp // (B * 24), 8, 3), K=(B, 3, 3), bbox_trans=(B, 2, 3), rot=(B, MAX_GT, 3, 3),
                      trans=(B, MAX_GT, 3), class_ids=(B, MAX_GT), n_gt=(B,))
        for names, flat in ((cls._SMALL_F, flat_f), (cls._SMALL_I, flat_i)):
            off = 0
            for n in names:
                cnt = int(np.prod(shapes[n]))
                setattr(out, n, flat[off:off + cnt].view(shapes[n]))
                off += up(cnt)
        out.frame_wh = (640.0, 480.0)
        out.block = None
        out._into_block(torch.zeros(out.block_bytes(), dtype=torch.uint8, device=mask.device))
        return out

    def _pack_small(self):
        """Re-home the small per-image fields as views of one fp32 and one int32 buffer (8 tensors -> 2)."""
        for names, attr in ((self._SMALL_F, "flat_f"), (self._SMALL_I, "flat_i")):
            parts = [getattr(self, n) for n in names]
            sizes = [(p.numel() + 3) // 4 * 4 for p in parts]          # keep every view 16-byte aligned
            flat = torch.zeros(sum(sizes), dtype=parts[0].dtype, device=parts[0].device)
            off = 0
            for n, p_, sz in zip(names, parts, sizes):
                v = flat[off:off + p_.numel()].view(p_.shape)
                v.copy_(p_)
                setattr(self, n, v)
                off += sz
            setattr(self, attr, flat)
        # ... and mask, floats, ints in ONE block, so that a static copy of a batch is one device copy
        self.block = None
        self._into_block(torch.zeros(self.block_bytes(), dtype=torch.uint8, device=self.mask.device))

    def _block_layout(self):
        """Byte offsets of (mask, flat_f, flat_i) inside one block, each segment 256-byte aligned, and the total."""
        sizes = [t.numel() * t.element_size() for t in (self.mask, self.flat_f, self.flat_i)]
        offs, total = [], 0
        for sz in sizes:
            offs.append(total)
            total += (sz + 255) // 256 * 256
        return offs, sizes, total

    def _into_block(self, block):
        """Re-home mask / flat_f / flat_i as views of `block` (uint8, _block_layout()'s size); contents are copied."""
        offs, sizes, total = self._block_layout()
        assert block.dtype == torch.uint8 and block.numel() == total
        new = [block[o:o + sz].view(t.dtype).view(t.shape)
               for o, sz, t in zip(offs, sizes, (self.mask, self.flat_f, self.flat_i))]
        for n, t in zip(new, (self.mask, self.flat_f, self.flat_i)):
            n.copy_(t)
        self.mask, self.flat_f, self.flat_i = new
        self.block = block
        self._rebind()

    def block_bytes(self):
        return self._block_layout()[2]

    def rebind_block(self, block):
        """Move the batch into caller-owned storage (GraphedKDStep's hand-over blocks); contents are copied."""
        self._into_block(block)

    def clone_static(self):
        out = object.__new__(PackedTargets)
        out.__dict__.update(self.__dict__)
        out.mask = self.mask.clone()
        for names, attr in ((self._SMALL_F, "flat_f"), (self._SMALL_I, "flat_i")):
            setattr(out, attr, getattr(self, attr).clone())
        out._rebind()
        out.block = None
        out._into_block(torch.zeros(out.block_bytes(), dtype=torch.uint8, device=out.mask.device))
        return out

    def _rebind(self):
        for names, attr in ((self._SMALL_F, "flat_f"), (self._SMALL_I, "flat_i")):
            flat, off = getattr(self, attr), 0
            for n in names:
                old = getattr(self, n)
                setattr(self, n, flat[off:off + old.numel()].view(old.shape))
                off += (old.numel() + 3) // 4 * 4

    def copy_from(self, other):
        """One device copy when both sides keep their batch in one block of the same layout (every PackedTargets
        built by __init__ / clone_static does), three otherwise."""
        mine, theirs = getattr(self, "block", None), getattr(other, "block", None)
        if mine is not None and theirs is not None and mine.numel() == theirs.numel():
            mine.copy_(theirs, non_blocking=True)
            return
        self.mask.copy_(other.mask, non_blocking=True)
        self.flat_f.copy_(other.flat_f, non_blocking=True)
        self.flat_i.copy_(other.flat_i, non_blocking=True)

    def rebind_storage(self, mask, flat_f, flat_i):
        """Move the three device buffers into caller-owned storage of the same shapes (contents are copied)."""
        for new, old in ((mask, self.mask), (flat_f, self.flat_f), (flat_i, self.flat_i)):
            assert new.shape == old.shape and new.dtype == old.dtype
            new.copy_(old)
        self.mask, self.flat_f, self.flat_i = mask, flat_f, flat_i
        self.block = None
        self._rebind()


_SLOT_STARTS = {}


def _slot_starts(batch, cap, device):
    """int32 [0, cap, 2*cap, ...]: constant per (batch, cap, device), built once (it used to cost two torch launches
    inside every replayed step)."""
    key = (batch, cap, str(device))
    t = _SLOT_STARTS.get(key)
    if t is None:
        t = _SLOT_STARTS[key] = torch.arange(batch, dtype=torch.int32, device=device) * cap
    return t


def teacher_blocks(batch, per_object=False):
    """Output blocks of a teacher selection: one per image, or one per (image, ground-truth slot) with per_object."""
    return batch * (MAX_GT if per_object else 1)


def teacher_flat_sizes(batch, cap=None, per_object=False):
    """(fp32 elements, int32 elements) of the two buffers every slot array of a teacher selection is a view of: the
    ONE place the layout's sizes come from (teacher_flats, TeacherKnowledge.from_flats, the hand-over blocks of
    kd6d.graph)."""
    blocks = teacher_blocks(batch, per_object)
    n = blocks * (cap or CAP)
    return n * 48, n + (blocks + 3) // 4 * 4


def teacher_flats(batch, device, cap=None, per_object=False):
    """Caller-owned output buffers of teacher_select: fp32 and int32, teacher_flat_sizes() elements."""
    nf, ni = teacher_flat_sizes(batch, cap, per_object)
    return (torch.zeros(nf, dtype=torch.float32, device=device), torch.zeros(ni, dtype=torch.int32, device=device))


class TeacherKnowledge(dict):
    """pred_t of the reference (models/model_kd.py:83-92).  The device-side slot arrays are what the
    student step consumes; the reference-named entries are materialised (with a sync) on demand.

    per_object: the selection ran per (image, ground-truth slot) -- block o = b*MAX_GT + g holds the cells of class
    class_ids[b, g] (kd6d_teacher_select_objects), `blocks` = batch*MAX_GT of them instead of `batch`."""

    def __init__(self, t_cnt, t_kp, t_score, t_row, t_kp_norm, t_beta, cap, batch, flats=None, per_object=False):
        super().__init__()
        self.t_cnt, self.t_kp, self.t_score, self.t_row = t_cnt, t_kp, t_score, t_row
        self.t_kp_norm, self.t_beta = t_kp_norm, t_beta
        self.cap, self.batch = cap, batch
        self.per_object = bool(per_object)
        self.blocks = teacher_blocks(batch, per_object)
        self.t_start = _slot_starts(self.blocks, cap, t_cnt.device)
        self.flats = flats            # (fp32, int32) buffers all the slot arrays are views of

    @staticmethod
    def from_flats(wf, wi, batch, cap, per_object=False):
        """Slot arrays as views of one fp32 and one int32 buffer of teacher_flat_sizes() elements."""
        b = teacher_blocks(batch, per_object)
        n = b * cap
        assert (wf.numel(), wi.numel()) == teacher_flat_sizes(batch, cap, per_object), "teacher buffers of another layout"
        return TeacherKnowledge(wi[n:n + b], wf[0:n * 16].view(n, 8, 2), wf[n * 32:n * 40].view(n, 8), wi[0:n],
                                wf[n * 16:n * 32].view(n, 8, 2), wf[n * 40:n * 48].view(n, 8), cap, batch, (wf, wi),
                                per_object)

    @staticmethod
    def group_views(wf, wi, group, batch, cap, per_object=False):
        """`group` batches selected in ONE launch over group*batch images (buffers of teacher_flat_sizes(group*batch)):
        the cells of batch s are a contiguous range of every slot array (they are image-major), no copies."""
        big = TeacherKnowledge.from_flats(wf, wi, group * batch, cap, per_object)
        b = teacher_blocks(batch, per_object)
        n = b * cap
        return [TeacherKnowledge(big.t_cnt[s * b:(s + 1) * b], big.t_kp[s * n:(s + 1) * n], big.t_score[s * n:(s + 1) * n],
                                 big.t_row[s * n:(s + 1) * n], big.t_kp_norm[s * n:(s + 1) * n],
                                 big.t_beta[s * n:(s + 1) * n], cap, batch, None, per_object) for s in range(group)]

    def clone_static(self):
        """Persistent copy (own storage) that `copy_from` refreshes: the double buffer of the step pipeline."""
        wf, wi = (t.clone() for t in self.flats)
        return TeacherKnowledge.from_flats(wf, wi, self.batch, self.cap, self.per_object)

    def copy_from(self, other):
        for mine, theirs in zip(self.flats, other.flats):
            mine.copy_(theirs, non_blocking=True)
        for key in ("post_kp_2d", "post_kp_cls", "post_pos_per_img"):
            self.pop(key, None)

    def __missing__(self, key):
        if key not in ("post_kp_2d", "post_kp_cls", "post_pos_per_img"):
            raise KeyError(key)
        cnt = self.t_cnt.cpu().tolist()
        kp = torch.cat([self.t_kp[b * self.cap:b * self.cap + n] for b, n in enumerate(cnt)]) if self.blocks else self.t_kp[:0]
        sc = torch.cat([self.t_score[b * self.cap:b * self.cap + n] for b, n in enumerate(cnt)]) if self.blocks else self.t_score[:0]
        self["post_kp_2d"], self["post_kp_cls"], self["post_pos_per_img"] = kp, sc, cnt
        return dict.__getitem__(self, key)


class DeferredTeacher:
    """pred_t produced on another HIP stream (the frozen teacher's forward overlaps the student's).
    The student's loss joins that stream right before it first reads the teacher's cells."""

    def __init__(self, value, stream):
        self.value, self.stream = value, stream

    def join(self):
        torch.cuda.current_stream().wait_stream(self.stream)
        return self.value


def teacher_select(cls_t, reg_t, levels, batch, bbox_trans, th=0.1, positive_num=10, positive_lambda=1.0, cap=CAP,
                   frame_wh=(640.0, 480.0), flats=None, zeroed=False, per_object=False, class_ids=None, n_gt=None):
    """flats: optional caller-owned output buffers (teacher_flat_sizes() elements; the step pipeline keeps them inside
    its hand-over block); zeroed here unless the caller already did (zeroed=True: the teacher's step prologue,
    ops.zero_many).  per_object: one selection per (image, ground-truth slot) on the class class_ids[b, g] for
    g < n_gt[b] (both (batch, MAX_GT) / (batch,) int32 device tensors: PackedTargets.class_ids / .n_gt) instead of one
    per image on the first class that emits."""
    dev = cls_t.device
    lv = make_levels(batch, levels)
    nf, ni = teacher_flat_sizes(batch, cap, per_object)
    if flats is None:
        wf = torch.zeros(nf, dtype=torch.float32, device=dev)        # one fill for all fp32 outputs
        wi = torch.zeros(ni, dtype=torch.int32, device=dev)
    else:
        wf, wi = flats
        assert wf.numel() == nf and wi.numel() == ni
        if not zeroed:
            wf.zero_(); wi.zero_()
    tk = TeacherKnowledge.from_flats(wf, wi, batch, cap, per_object)
    P = ops._ptr
    if per_object:
        if class_ids is None or n_gt is None:
            raise ValueError("teacher_select(per_object=True) needs the targets' class_ids and n_gt")
        assert class_ids.dtype == torch.int32 and n_gt.dtype == torch.int32
        assert class_ids.numel() == batch * MAX_GT and n_gt.numel() == batch
        check(lib.kd6d_teacher_select_objects(ctypes.byref(lv), P(cls_t), P(reg_t), P(bbox_trans), P(class_ids), P(n_gt),
                                              th, float(positive_num), float(positive_lambda), cap, frame_wh[0],
                                              frame_wh[1], P(tk.t_cnt), P(tk.t_kp), P(tk.t_score), P(tk.t_row),
                                              P(tk.t_kp_norm), P(tk.t_beta), ops._stream()),
              "kd6d_teacher_select_objects")
        return tk
    check(lib.kd6d_teacher_select(ctypes.byref(lv), P(cls_t), P(reg_t), P(bbox_trans),
                                  th, float(positive_num), float(positive_lambda), cap, frame_wh[0], frame_wh[1],
                                  P(tk.t_cnt), P(tk.t_kp), P(tk.t_score), P(tk.t_row),
                                  P(tk.t_kp_norm), P(tk.t_beta), ops._stream()),
          "kd6d_teacher_select")
    return tk


class KDLoss:
    """Student-side losses of one step.  forward() launches; backward(weights) fills dcls/dreg."""

    def __init__(self, internal_K, diameters, gamma=2.0, alpha=0.25, positive_num=10, positive_lambda=1.0,
                 kd_cfg=None, cap=None):
        K = np.asarray(internal_K, np.float64).reshape(3, 3)
        self.kinv = (ctypes.c_float * 9)(*np.linalg.inv(K).reshape(-1).astype(np.float32).tolist())
        self.diameters_host = [float(d) for d in diameters]
        self.diameters = None
        self.gamma, self.alpha = float(gamma), float(alpha)
        self.positive_num, self.positive_lambda = float(positive_num), float(positive_lambda)
        kd_cfg = kd_cfg or {}
        # KERNEL_LOSSES (--kd_kernel_losses): GTYPE may also name one of geomloss' kernel distances; the KD term is
        # then kd6d_kernel_div_fwd_bwd in the Sinkhorn launch's place (self.kernel = its KD6D_KERNEL_* code)
        self.kernel = check_gtype(kd_cfg.get("GTYPE", "sinkhorn"), bool(kd_cfg.get("KERNEL_LOSSES", False)),
                                  float(kd_cfg.get("GBLUR", 0.001)))
        if kd_cfg.get("GLEVEL", "point") != "point" or int(kd_cfg.get("GnD", 2)) != 2:
            raise NotImplementedError("only --glevel point / --gnD 2 are implemented")
        self.p = float(kd_cfg.get("GP", 2.0))
        self.blur = float(kd_cfg.get("GBLUR", 0.001))
        self.scaling = float(kd_cfg.get("SCALING", 0.5))
        reach = kd_cfg.get("REACH", 0.5)
        self.reach = -1.0 if reach is None else float(reach)
        self.weighted = bool(kd_cfg.get("WEIGHTED_OT", True))
        self.detach = bool(kd_cfg.get("DETACH", False))
        # PER_OBJECT (--kd_per_object): one OT problem per (image, ground-truth slot) -- the student's positives of
        # instance g against the teacher's cells of that instance's class -- instead of one per image
        self.per_object = bool(kd_cfg.get("PER_OBJECT", False))
        if not self.weighted:
            raise NotImplementedError("unweighted OT (--weightedOT false) is not implemented on the HIP path")
        # every pick of a full image (MAX_GT instances) must fit: beyond `cap` the kernel truncates, and labels,
        # losses and gradients would silently differ from the reference's
        need = positives_bound(self.positive_num)
        self.cap = max(POS_CAP, need) if cap is None else int(cap)
        if self.cap > 64 or self.cap < need:
            raise ValueError("KDLoss: positive_num=%g can select %d cells in an image with %d instances; cap=%d %s"
                             % (self.positive_num, need, MAX_GT, self.cap,
                                "exceeds the 64 slots of kd6d_ssc_assign" if self.cap > 64 else
                                "would truncate them (include/kd6d.h, kd6d_ssc_assign)"))
        self.ctx = None
        self._ws = {}
        self._keys = {}
        # device-side sampling keys: reproducible from torch.manual_seed.  The key of a cell is a hash of (seed, step
        # counter, cell index) and train_kd.py seeds every rank alike, so the rank is mixed in: data-parallel ranks
        # must not draw the same key field every step (the reference's torch.randperm runs from one seed on every rank
        # too, but consumes the generator per ground truth of ITS shard, so its ranks decorrelate); the constant also
        # keeps (seed 0, step 0, cell 0) from hashing the all-zero state
        from .libs.distributed import get_rank
        self.seed = (torch.initial_seed() + 0x9E3779B97F4A7C15 * (get_rank() + 1)) & 0xFFFFFFFFFFFFFFFF
        self.anchor_sizes, self.anchor_strides = ANCHOR_SIZES, ANCHOR_STRIDES      # configs/ape.yaml:3-4

    def workspaces(self, batch, device):
        """The per-step accumulators / slot arrays of the loss side, (fp32, int32), persistent per batch size: the
        step prologue (PoseModuleKD._begin_step) zeroes them together with the gradient bucket."""
        key = (batch, str(device))
        ws = self._ws.get(key)
        if ws is None:
            nf, ni = self._ws_sizes(batch)
            ws = self._ws[key] = (torch.zeros(nf, dtype=torch.float32, device=device),
                                  torch.zeros(ni, dtype=torch.int32, device=device))
        return ws

    def _ws_layout(self, batch):
        """The ONE place the per-object part of the workspaces is laid out: ({name: (offset, elements)} fp32,
        {name: ...} int32, fp32 total, int32 total).  "image" is the per-image layout forward() / assign() have always
        used; per_object appends, behind it, the object-major copies xs_obj / g_xs_obj (n*16 each), alpha_obj /
        g_alpha_obj (n*8 each), loss_obj (batch*MAX_GT) and obj_start / obj_cnt / valid_obj (batch*MAX_GT each), dest (n)."""
        n, bp = batch * self.cap, (batch + 3) // 4 * 4
        nobj = batch * MAX_GT
        parts_f = [("image", 8 + bp + n * 64 + 16)]            # + the two loss sums' fixed-point workspaces
        parts_i = [("image", 3 * bp + 4 + 2 * n)]
        if self.per_object:
            parts_f += [("xs_obj", n * 16), ("g_xs_obj", n * 16), ("alpha_obj", n * 8), ("g_alpha_obj", n * 8),
                        ("loss_obj", nobj)]
            parts_i += [("obj_start", nobj), ("obj_cnt", nobj), ("valid_obj", nobj), ("dest", n)]
        out = []
        for parts in (parts_f, parts_i):
            seg, off = {}, 0
            for name, cnt in parts:
                seg[name] = (off, cnt)
                off += cnt
            out += [seg, off]
        return out[0], out[2], out[1], out[3]

    def _ws_sizes(self, batch):
        """(fp32, int32) elements of the per-step workspaces."""
        return self._ws_layout(batch)[2:]

    def assign(self, levels, batch, tgt, keys=None, prezeroed=False, step_counter=None):
        """SSC target assignment + the zeroed per-step workspaces.  Depends on the targets only, not on the student's
        output: the graphed step runs it on a side stream beside the student's forward.  prezeroed: the workspaces
        are the persistent pair of workspaces(), already zeroed by the step prologue.  keys: the sampling keys (tests
        pin them); otherwise drawn here -- on the device from (seed, step_counter[0], cell) when the caller has a
        device step counter (graph-replayable without torch's generator), else by torch.rand."""
        dev = tgt.mask.device
        rows = batch * sum(h * w for h, w in levels)
        cap = self.cap
        lv = make_levels(batch, levels, self.anchor_sizes, self.anchor_strides)
        if keys is None and step_counter is not None:
            kb = self._keys.get((rows, str(dev)))
            if kb is None:
                kb = self._keys[(rows, str(dev))] = torch.empty(rows, dtype=torch.float32, device=dev)
            keys = ops.uniform_keys(kb, step_counter, self.seed)
        elif keys is None:
            keys = torch.rand(rows, dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        labels = torch.empty(rows, **i32)
        n = batch * cap
        bp = (batch + 3) // 4 * 4
        # one zero fill per dtype for every per-step accumulator / slot array of the loss side
        if prezeroed:
            wf, wi = self.workspaces(batch, dev)
        else:
            nf, ni = self._ws_sizes(batch)
            wf = torch.zeros(nf, **f32)
            wi = torch.zeros(ni, **i32)
        pos_cnt = wi[0:batch]
        pos_row, pos_gt = wi[3 * bp + 4:3 * bp + 4 + n], wi[3 * bp + 4 + n:3 * bp + 4 + 2 * n]
        P = ops._ptr
        check(lib.kd6d_ssc_assign(ctypes.byref(lv), P(tgt.mask), tgt.mask_h, tgt.mask_w, P(tgt.kp3d), P(tgt.K),
                                  P(tgt.class_ids), P(tgt.n_gt), P(tgt.rot), P(tgt.trans), P(tgt.bbox_trans),
                                  P(keys), self.positive_num, self.positive_lambda, cap, P(labels), P(pos_cnt),
                                  P(pos_row), P(pos_gt), ops._stream()), "kd6d_ssc_assign")
        return dict(rows=rows, levels=tuple(levels), batch=batch, labels=labels, wf=wf, wi=wi, keys=keys)

    def _divergence(self, xs, alpha, start, cnt, teacher, n, loss, valid, g_xs, g_alpha):
        """The KD term's one launch over n problems (student segments start / cnt, the teacher's own), on the current
        stream: the Sinkhorn divergence, or the kernel distance self.kernel names.  Same buffers, same contract for
        both; the gradient buffers were zeroed by the step prologue (ops adds no fill to the captured step)."""
        sets = (xs, alpha, start, cnt, teacher.t_kp_norm, teacher.t_beta, teacher.t_start, teacher.t_cnt, n)
        out = (loss, valid, g_xs, g_alpha)
        if self.kernel is None:
            ops.sinkhorn_div(*sets, self.p, self.blur, self.scaling, self.reach, out=out)
        else:       # p, scaling and reach do not enter a kernel distance (geomloss ignores them alike)
            ops.kernel_div(self.kernel, *sets, self.blur, out=out)

    def forward(self, cls_s, reg_s, levels, batch, tgt, teacher, keys=None, seg_scale=None, pre=None):
        dev = cls_s.device
        rows = cls_s.shape[0]
        cap = self.cap
        lv = make_levels(batch, levels, self.anchor_sizes, self.anchor_strides)
        if self.diameters is None or self.diameters.device != dev:
            self.diameters = torch.tensor(self.diameters_host, dtype=torch.float32, device=dev)
        if pre is None or pre["rows"] != rows or pre["levels"] != tuple(levels) or pre["batch"] != batch:
            pre = self.assign(levels, batch, tgt, keys)
        labels, wf, wi = pre["labels"], pre["wf"], pre["wi"]
        n = batch * cap
        bp = (batch + 3) // 4 * 4
        pos_cnt, valid, s_start = wi[0:batch], wi[bp:bp + batch], wi[2 * bp:2 * bp + batch]
        n_valid = wi[3 * bp:3 * bp + 1]
        pos_row, pos_gt = wi[3 * bp + 4:3 * bp + 4 + n], wi[3 * bp + 4 + n:3 * bp + 4 + 2 * n]
        st = ops._stream()
        P = ops._ptr
        losses = wf[0:4]                       # cls, reg, kd, (pad)
        loss_img = wf[8:8 + batch]
        o = 8 + bp
        xs, g_reg, g_xs = (wf[o + k * n * 16:o + (k + 1) * n * 16].view(n, 8, 2) for k in range(3))
        alpha, g_alpha = (wf[o + n * 48 + k * n * 8:o + n * 48 + (k + 1) * n * 8].view(n, 8) for k in range(2))
        ws_cls, ws_reg = wf[o + n * 64:o + n * 64 + 8], wf[o + n * 64 + 8:o + n * 64 + 16]     # kd6d_scalar_ws each
        check(lib.kd6d_focal_fwd(P(cls_s), P(labels), rows, self.gamma, self.alpha, P(losses[0:1]), P(ws_cls), st),
              "kd6d_focal_fwd")
        fw, fh = tgt.frame_wh
        check(lib.kd6d_student_points(ctypes.byref(lv), P(cls_s), P(reg_s), P(pos_cnt), P(pos_row), P(pos_gt),
                                      P(tgt.class_ids), P(tgt.kp3d), P(tgt.rot), P(tgt.trans), P(tgt.bbox_trans),
                                      P(self.diameters), self.kinv, fw, fh, cap, P(xs), P(alpha), P(g_reg),
                                      P(losses[1:2]), P(ws_reg), P(s_start), st), "kd6d_student_points")
        if teacher is not None and bool(getattr(teacher, "per_object", False)) != self.per_object:
            raise ValueError("KDLoss(PER_OBJECT=%s) got a teacher selection made with per_object=%s: both sides of the "
                             "KD term must use the same mode" % (self.per_object, not self.per_object))
        if teacher is not None and self.per_object:
            # group the positives by instance -> one Sinkhorn problem per object (same kernel, batch*MAX_GT problems,
            # teacher segments at o*cap) -> mean over the valid objects -> gradients back into slot order
            nobj = batch * MAX_GT
            if teacher.t_cnt.numel() != nobj:
                raise ValueError("per-object KD: the teacher selection holds %d blocks, this batch has %d objects slots"
                                 % (teacher.t_cnt.numel(), nobj))
            seg_f, seg_i, nf, ni = self._ws_layout(batch)
            assert wf.numel() == nf and wi.numel() == ni, "workspaces of another layout (made without PER_OBJECT?)"

            def part(buf, seg, name):
                off, cnt = seg[name]
                return buf[off:off + cnt]

            xs_o, g_xs_o = (part(wf, seg_f, k).view(n, 8, 2) for k in ("xs_obj", "g_xs_obj"))
            al_o, g_al_o = (part(wf, seg_f, k).view(n, 8) for k in ("alpha_obj", "g_alpha_obj"))
            loss_obj = part(wf, seg_f, "loss_obj")
            o_start, o_cnt, o_valid, dest = (part(wi, seg_i, k) for k in ("obj_start", "obj_cnt", "valid_obj", "dest"))
            check(lib.kd6d_kd_group_objects(P(pos_cnt), P(pos_gt), P(xs), P(alpha), batch, cap, P(o_start), P(o_cnt),
                                            P(dest), P(xs_o), P(al_o), st), "kd6d_kd_group_objects")
            self._divergence(xs_o, al_o, o_start, o_cnt, teacher, nobj, loss_obj, o_valid, g_xs_o, g_al_o)
            check(lib.kd6d_kd_mean(P(loss_obj), P(o_valid), nobj, P(losses[2:3]), P(n_valid), st), "kd6d_kd_mean")
            check(lib.kd6d_kd_scatter_objects(P(pos_cnt), P(pos_gt), P(dest), P(o_valid), P(g_xs_o), P(g_al_o), batch,
                                              cap, P(g_xs), P(g_alpha), P(valid), st), "kd6d_kd_scatter_objects")
            self.obj = dict(start=o_start, cnt=o_cnt, valid=o_valid, dest=dest, loss=loss_obj, xs=xs_o, alpha=al_o,
                            g_xs=g_xs_o, g_alpha=g_al_o)
        elif teacher is not None:
            self._divergence(xs, alpha, s_start, pos_cnt, teacher, batch, loss_img, valid, g_xs, g_alpha)
            check(lib.kd6d_kd_mean(P(loss_img), P(valid), batch, P(losses[2:3]), P(n_valid), st), "kd6d_kd_mean")
        self.ctx = dict(lv=lv, cls=cls_s, reg=reg_s, labels=labels, pos_cnt=pos_cnt, pos_row=pos_row, pos_gt=pos_gt,
                        tgt=tgt, g_reg=g_reg, g_xs=g_xs, g_alpha=g_alpha, n_valid=n_valid, valid=valid,
                        rows=rows, batch=batch, xs=xs, alpha=alpha, seg_scale=seg_scale, losses=losses)
        return losses

    def backward(self, weights, dtype, dcls, dreg, dseg_scale=None, acc_stride=0):
        """weights: device fp32 tensor {d/d loss_cls, d/d loss_reg, d/d loss_kd}.  dreg must be zeroed.  dseg_scale:
        lo-plane view of the PLANAR gradient accumulators of the head's scales (int64, stride acc_stride), or None."""
        assert dseg_scale is None or (dseg_scale.dtype == torch.int64 and acc_stride > 0)
        c = self.ctx
        P = ops._ptr
        st = ops._stream()
        tgt = c["tgt"]
        fw, fh = tgt.frame_wh
        check(lib.kd6d_focal_bwd(ops.dt_code(dtype), P(c["cls"]), P(c["labels"]), c["rows"], self.gamma, self.alpha,
                                 P(weights[0:1]), P(dcls), st), "kd6d_focal_bwd")
        check(lib.kd6d_loss_backward(ctypes.byref(c["lv"]), ops.dt_code(dtype), P(c["cls"]), P(c["reg"]),
                                     P(c["pos_cnt"]), P(c["pos_row"]), P(c["pos_gt"]), P(tgt.class_ids),
                                     P(tgt.bbox_trans), P(c["g_reg"]), P(c["g_xs"]), P(c["g_alpha"]),
                                     P(c["n_valid"]), P(c["valid"]), P(weights), P(c["seg_scale"]),
                                     P(dseg_scale), int(acc_stride), fw, fh, self.cap, int(self.detach), P(dcls), P(dreg), st),
              "kd6d_loss_backward")
