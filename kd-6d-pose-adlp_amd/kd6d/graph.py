"""hipGraph replay of the whole KD step (train_kd.py:104-140 of the reference).

One step is ~350 kernel launches with static shapes, static buffer addresses and no host
synchronisation, so launching it from Python costs more host time (~6 ms) than the kernels take.
`GraphedKDStep` captures it once into two hipGraphs and replays them:

    G1: zero grads -> teacher forward + cell selection  ||  student forward -> SSC assignment +
        focal / object-space / Sinkhorn-OT losses -> backward sweep (weight gradients on a third stream)
    (eager) RCCL mean all-reduce of the flat gradient bucket, world size > 1 only
    G2: sum of squares -> fused clip + AdamW (+ bf16 shadow refresh)

Everything that changes from step to step enters through device memory: the batch is copied into
static input buffers, the OneCycle learning rate and Adam bias corrections are written by the tiny
`kd6d_set_hyper` launch (`FusedClipAdamW.advance`), the random keys of the SSC positive sampling
come from torch's graph-safe Philox generator.

`pipeline=True` additionally software-pipelines ACROSS steps: the frozen teacher does not depend on
the student's weights, so call k runs the teacher on batch k beside the student's forward/backward
on batch k-1 (whose teacher cells were produced by call k-1 and are double-buffered).  Every batch
still gets exactly one teacher forward and one student step; the losses returned by call k belong
to batch k-1 and `flush()` trains on the last pending batch.  The critical path of a call drops from
teacher + student to max(teacher, student), and the two halves fill each other's idle CUs.
"""

import contextlib
import math

import torch

from . import ops
from .group_pipeline import GroupPipeline
from .kd_losses import DeferredTeacher, PackedTargets
from .libs import distributed as D
from .libs.poses import ImageList


@contextlib.contextmanager
def _setting(obj, **values):
    """Attributes of `obj` set for the length of a `with`; what they held before comes back on the way out."""
    before = {k: getattr(obj, k, None) for k in values}
    for k, v in values.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in before.items():
            setattr(obj, k, v)


# ---- byte blocks: everything a step hands over lives in ONE uint8 tensor, so that handing it over is ONE device copy ----
def _part_bytes(part):
    if isinstance(part, int):
        return part
    shape, dtype = part
    return math.prod(shape) * torch.empty(0, dtype=dtype).element_size()


def block_layout(parts):
    """parts: a byte count or a (shape, dtype) each.  -> (offsets, total bytes), every part on a 256-byte boundary."""
    offs, total = [], 0
    for part in parts:
        offs.append(total)
        total += (_part_bytes(part) + 255) // 256 * 256
    return offs, total


def block_views(block, parts, offs):
    """The parts of block_layout() as views of `block` (uint8): raw bytes for a byte count, typed and shaped otherwise."""
    views = []
    for part, o in zip(parts, offs):
        raw = block[o:o + _part_bytes(part)]
        views.append(raw if isinstance(part, int) else raw.view(part[1]).view(part[0]))
    return views


class _KDStepBase:
    """What both replayed steps are made of: streams and weight-gradient settings, the student's step body, the gradient
    exchange, and THE capture and replay routines."""
    # ... each weight-gradient launch sized (split-K count) for CUs / this many.  Pipelined steps (a teacher forward
    # shares the device for the first 60 % of the step): CUs / 2; strictly sequential steps: CUs / 4 (4242 against 4168
    # images/s).
    WGRAD_BUDGET_DIV = {True: 2.0, False: 4.0}

    def __init__(self, teacher, student, optimizer, loss_weights, cfg_kd, warmup, exchange, teacher_stream, side_streams,
                 wgrad):
        self.teacher, self.student, self.opt = teacher, student, optimizer
        # fork/join inside the captured graph: the teacher's forward runs beside the student's, and the weight
        # gradients beside the dgrad / normalisation chain (many of these kernels fill < 256 CUs on their own)
        self.teacher_stream = torch.cuda.Stream() if teacher_stream else None
        # ... with several weight gradients in flight, each sized for a share of the CUs: the same k-loop work
        # with proportionally fewer atomic dW-tile flushes (measured: 1 -> 4 streams = +8 % on the step)
        # (WGRAD_STREAMS / WGRAD_BUDGET_DIV.  Swept on the closing state of round 1, medians of
        #  3 runs: 4 streams at CUs/4 4539 images/s, CUs/3 4566, CUs/2 4595-4640, CUs/1.5 4597, whole device 4529;
        #  3 streams 4330-4430, 5 streams 4140-4200, 6-8 streams 4340)
        snet = student.net
        snet.side_stream = torch.cuda.Stream() if side_streams else None
        snet.side_streams = ([snet.side_stream] + [torch.cuda.Stream() for _ in range(side_streams - 1)]
                             if side_streams > 1 else None)
        snet.wgrad_cu_budget, snet.wgrad_group_wgs, snet.wgrad_group_flush = wgrad
        self.w_cls, self.w_reg, self.w_kd = (float(w) for w in loss_weights)
        self._w = None                                     # the same weights as a device tensor
        self.cfg_kd = cfg_kd
        self.warmup = warmup
        self.g_step = self.g_opt = None
        self.graphs_per_step = 2
        self.images = self.tgt = self.losses = None        # the batch the student trains on
        self.t_cur = None                                  # pipelines: teacher cells of `images`
        self._nhwc = None                                  # pipelines: (current, next) packed NHWC inputs
        # data-parallel exchange schedule (kd6d/libs/distributed.py EXCHANGE_MODE): "between" the two graphs, or
        # "overlap" = two slices captured inside the single step graph, the big one beside the backbone sweep
        self.exchange = exchange or D.EXCHANGE_MODE
        assert self.exchange in ("between", "overlap")

    @classmethod
    def _wgrad_settings(cls, teacher_beside):
        """(wgrad_cu_budget, wgrad_group_wgs, wgrad_group_flush) of the student's network for a step whose first part a
        teacher forward shares the device with, or for a strictly sequential one."""
        cus = ops.device_cu_count()
        budget = int(cus / cls.WGRAD_BUDGET_DIV[bool(teacher_beside)])
        # grouped head weight gradients: one workgroup per two CUs beside a teacher forward (5284-5292 images/s against
        # 5215-5234 at one per CU and 5208-5214 at two), two per CU when the step is strictly sequential (4553 against 4467)
        # ... and where the group goes out: measured, see WgradSchedule.flush_group
        return (budget, cus // 2, "head_end") if teacher_beside else (budget, 2 * cus, "fpn_end")

    @property
    def pending(self):
        return self.pending_steps > 0

    def _overlap(self):
        return self.exchange == "overlap" and D.exchange_active()

    def _per_object(self):
        """The teacher selects its cells per (image, ground-truth slot) (PoseModuleKD.kd_per_object)."""
        return bool(getattr(self.teacher, "kd_per_object", False))

    # ---- the student's half of the body the reference's loop runs per iteration (train_kd.py:104-137) ----------
    def _student_step(self, pred_t):
        if self._w is None:
            self._w = torch.tensor([self.w_cls, self.w_reg, self.w_kd], dtype=torch.float32,
                                   device=self.student.net.device)
        # the exchange is this object's business: inside the sweep ("overlap", D.overlapped_exchange) or after the step
        # (_exchange); set around the call only, an eager step of the same module keeps its own choice
        schedule = "overlap" if self.exchange == "overlap" else "deferred"
        with _setting(self.student.net, nhwc_in=self._nhwc[0] if self._nhwc is not None else None), \
                _setting(self.student, exchange_schedule=schedule):
            losses = self.student.step_losses(self.images, self.tgt, pred_t, self._w)
        return {"loss_cls": losses[0], "loss_reg": losses[1], "loss_kd": losses[2]}

    def _exchange(self):
        if not self._overlap():            # (overlap: both slices were issued inside the step already)
            D.exchange_gradients(self.student.net.store)

    def _count_opt_step(self):
        # torch's lr schedulers count optimizer.step() calls to warn about ordering
        if hasattr(self.opt, "_opt_called"):
            self.opt._opt_called = True
        if hasattr(self.opt, "_step_count"):
            self.opt._step_count += 1

    # ---- capture ------------------------------------------------------------------------------
    def _snapshot(self):
        st, opt = self.student.net.store, self.opt
        return dict(params=st.params.clone(), bufs=st.bufs.clone(), m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                    nbt=self.student._nbt.clone(), steps=opt.steps, sc=getattr(opt, "_step_count", None))

    def _restore(self, snap):
        st, opt = self.student.net.store, self.opt
        st.params.copy_(snap["params"]); st.bufs.copy_(snap["bufs"])
        opt.exp_avg.copy_(snap["m"]); opt.exp_avg_sq.copy_(snap["v"])
        self.student._nbt.copy_(snap["nbt"])
        if st.shadow is not None:
            st.refresh_shadow()                 # bf16 copy of the restored master weights
        opt.steps = snap["steps"]
        if snap["sc"] is not None:
            opt._step_count = snap["sc"]

    def _capture_graphs(self, bodies, warmup_exchange):
        """One graph per step body (all in one pool) [+ the optimiser's], the training state as it was -> the graphs.
        warmup_exchange: the eager warm-up steps run the gradient exchange too."""
        snap = self._snapshot()                              # the warm-up steps below must not train
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                        # eager warm-up: allocates every static buffer
            for _ in range(self.warmup):
                for body in bodies:
                    body()
                    if warmup_exchange:
                        self._exchange()
                    self.opt.advance()
                    self.opt.launch(device_schedule=True)
                    self._count_opt_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # Without a gradient exchange (one rank) nothing has to happen between the reverse sweep and the optimiser:
        # ONE graph per step, and the eager kd6d_set_hyper launch moves in front of it.  With an exchange the RCCL
        # all-reduce sits between two graphs.
        self.graphs_per_step = 2 if (D.exchange_active() and not self._overlap()) else 1
        graphs, pool = [], None
        for body in bodies:
            g = torch.cuda.CUDAGraph()
            # thread-local capture mode: with a process group alive, RCCL's watchdog thread polls events concurrently
            with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                self.losses = body()
                if self.graphs_per_step == 1:
                    self.opt.launch(device_schedule=True)
            pool = g.pool()
            graphs.append(g)
        if self.graphs_per_step == 2:
            self.g_opt = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_opt, pool=pool, capture_error_mode="thread_local"):
                self.opt.launch(device_schedule=True)
        self._restore(snap)
        return graphs

    def _replay(self, graph):
        """One training step from its graph: the ONE place that knows the order."""
        if self.graphs_per_step == 1:
            self.opt.advance()                 # lr / bias corrections of THIS step, consumed at the graph's end
            graph.replay()
        else:
            graph.replay()
            self._exchange()
            self.opt.advance()
            self.g_opt.replay()
        self._count_opt_step()
        for _, bn in self.student.net.bns:     # what FusedClipAdamW.launch() does when it runs from Python: the
            bn.fold = None                     # cached eval-mode BN scale/shift belong to the previous weights
        return self.losses


class GraphedKDStep(_KDStepBase):
    WGRAD_STREAMS = 4          # weight-gradient launches kept in flight beside the dgrad / normalisation chain
    # (one knob for both step classes: the grouped step reads it here too)

    def __init__(self, teacher, student, optimizer, loss_weights=(0.1, 1.0, 5.0), cfg_kd=None, warmup=3,
                 concurrent=True, pipeline=False, exchange=None):
        nside = self.WGRAD_STREAMS if concurrent else 0
        budget, wgs, flush = self._wgrad_settings(pipeline)
        super().__init__(teacher, student, optimizer, loss_weights, cfg_kd, warmup, exchange,
                         teacher_stream=concurrent or pipeline, side_streams=nside,
                         wgrad=(budget if nside > 1 else 0, wgs, flush))
        self.pipeline = pipeline
        self.images_nxt = self.tgt_nxt = None              # pipeline: the batch the teacher looks at
        self._blocks = None                                # pipeline: [current, next] hand-over blocks
        self.primed = False                                # pipeline: the teacher has seen a batch the student has not

    @property
    def pending_steps(self):
        """Batches the pipeline holds that have not had their student step yet."""
        return int(self.primed)

    # ---- the body the reference's loop runs per iteration (train_kd.py:104-137) ----------
    def _teacher(self, images, tgt):
        out = self._nhwc[1] if (self._nhwc is not None and images is self.images_nxt) else None
        with _setting(self.teacher.net, nhwc_out=out):
            return self._teacher_launch(images, tgt)

    def _teacher_launch(self, images, tgt):
        with torch.no_grad():
            if self.teacher_stream is None:
                return self.teacher(images, targets=tgt, is_teacher=True, cfg_kd=self.cfg_kd)
            self.teacher_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.teacher_stream):
                ops.mark("teacher.start")
                pred = self.teacher(images, targets=tgt, is_teacher=True, cfg_kd=self.cfg_kd)
                ops.mark("teacher.end")
            return DeferredTeacher(pred, self.teacher_stream)

    def _forward_backward(self):
        ops.mark("step.start")              # (step_losses opens with the step's zero_grad)
        if not self.pipeline:
            return self._student_step(self._teacher(self.images, self.tgt))
        nxt = self._teacher(self.images_nxt, self.tgt_nxt)       # batch k, beside ...
        losses = self._student_step(self.t_cur)                  # ... the student step on batch k-1
        nxt = nxt.join() if isinstance(nxt, DeferredTeacher) else nxt
        # (running these hand-over copies on the teacher's stream behind the reverse sweep removes the 50 us they
        # trail the step by, but the extra mid-step dependency costs 120 us: measured, reverted)
        self._advance(nxt)
        ops.mark("step.end")
        return losses

    def _advance(self, pred_nxt):
        """k -> k+1: what the teacher just saw becomes the student's next batch."""
        if self._blocks is not None:         # everything handed over lives in one block per side: ONE copy
            self._blocks[0].copy_(self._blocks[1], non_blocking=True)
            for key in ("post_kp_2d", "post_kp_cls", "post_pos_per_img"):
                self.t_cur.pop(key, None)
            return
        self.t_cur.copy_from(pred_nxt)
        self.images.tensors.copy_(self.images_nxt.tensors, non_blocking=True)
        self.tgt.copy_from(self.tgt_nxt)

    def _make_blocks(self):
        """Re-home images, targets and teacher cells of the current / next batch in two byte blocks of identical
        layout, so that the hand-over at the end of a step is one device copy instead of six."""
        from .kd_losses import TeacherKnowledge
        dev = self.images.tensors.device
        # the image travels in the layout both networks consume (packed NHWC, 8 channels, the networks' dtype): the
        # teacher's conversion of batch k is what the student reads one replay later instead of converting it again
        snet, tnet = self.student.net, self.teacher.net
        assert snet.dtype == tnet.dtype, "teacher and student share the converted input: same precision"
        nhwc_cur = ops.image_to_nhwc(self.images.tensors, snet.dtype, 8)
        parts = [(nhwc_cur.shape, nhwc_cur.dtype), self.tgt.block_bytes()] + [(f.shape, f.dtype) for f in self.t_cur.flats]
        offs, total = block_layout(parts)
        blocks = [torch.zeros(total, dtype=torch.uint8, device=dev) for _ in range(2)]
        cur, nxt = (block_views(b, parts, offs) for b in blocks)
        cur[0].copy_(nhwc_cur)
        ops.image_to_nhwc(self.images_nxt.tensors, snet.dtype, 8, out=nxt[0])
        self._nhwc = (cur[0], nxt[0])
        for side, tgt in ((cur, self.tgt), (nxt, self.tgt_nxt)):
            tgt.rebind_block(side[1])
        cur[2].copy_(self.t_cur.flats[0]); cur[3].copy_(self.t_cur.flats[1])
        self.t_cur = TeacherKnowledge.from_flats(cur[2], cur[3], self.t_cur.batch, self.t_cur.cap, self.t_cur.per_object)
        self.teacher._teacher_flats = (nxt[2], nxt[3])     # the teacher's selection writes straight into the next block
        self._blocks = blocks

    # ---- static inputs ------------------------------------------------------------------------
    def _load(self, images, tgt):
        x = images.tensors if hasattr(images, "tensors") else images
        if self.images is None:
            self.images = ImageList(torch.empty_like(x), getattr(images, "sizes", None))
            self.tgt = tgt.clone_static()
            if self.pipeline:
                self.images_nxt = ImageList(torch.empty_like(x), getattr(images, "sizes", None))
                self.tgt_nxt = tgt.clone_static()
        dst_i, dst_t = (self.images_nxt, self.tgt_nxt) if self.pipeline else (self.images, self.tgt)
        assert x.shape == dst_i.tensors.shape, "the captured step has a static batch shape"
        assert (tgt.mask_h, tgt.mask_w) == (dst_t.mask_h, dst_t.mask_w)
        dst_i.tensors.copy_(x, non_blocking=True)
        dst_t.copy_from(tgt)

    # ---- capture ------------------------------------------------------------------------------
    def _handover(self):
        """pipeline=True: what the student reads of the hand-over (image, targets, teacher cells).  The warm-up
        iterations of a capture advance the pipeline; these are what rewinds it."""
        img = self._nhwc[0] if self._nhwc is not None else self.images.tensors
        return [img, self.tgt.mask, self.tgt.flat_f, self.tgt.flat_i, self.t_cur.flats[0], self.t_cur.flats[1]]

    def _capture(self):
        if self.pipeline and self._blocks is None:
            self._make_blocks()
        elif not self.pipeline and getattr(self.teacher, "_teacher_flats", None) is None:
            from .kd_losses import teacher_flats     # caller-owned teacher outputs: cleared by the teacher's prologue
            self.teacher._teacher_flats = teacher_flats(self.images.tensors.shape[0], self.images.tensors.device,
                                                        per_object=self._per_object())
        kept = [(t, t.clone()) for t in self._handover()] if self.pipeline else []
        self.g_step, = self._capture_graphs([self._forward_backward], warmup_exchange=True)
        for t, before in kept:
            t.copy_(before)

    # ---- public -------------------------------------------------------------------------------
    def __call__(self, images, tgt):
        """One KD step.  Returns the dict of (device, static) loss scalars -- of THIS batch, or with
        pipeline=True of the previous one (None on the priming call)."""
        if not isinstance(tgt, PackedTargets):
            tgt = PackedTargets(tgt, self.student.net.device)
        self._load(images, tgt)
        if self.pipeline and not self.primed:   # priming call: teacher only, the student starts next call
            # (eager call: fresh output buffers, not the captured step's)
            with _setting(self.teacher, _teacher_flats=None), torch.no_grad():
                pred = self.teacher(self.images_nxt, targets=self.tgt_nxt, is_teacher=True, cfg_kd=self.cfg_kd)
            if self.t_cur is None:
                self.t_cur = pred.clone_static()
            else:                               # a new pipeline after flush(): the captured step's buffers stay
                self.t_cur.copy_from(pred)
            self.images.tensors.copy_(self.images_nxt.tensors)
            if self._nhwc is not None:
                ops.image_to_nhwc(self.images_nxt.tensors, self.student.net.dtype, 8, out=self._nhwc[0])
            self.tgt.copy_from(self.tgt_nxt)
            self.primed = True
            return None
        if self.g_step is None:
            self._capture()
        return self._replay(self.g_step)

    def flush(self):
        """pipeline=True: train on the batch that is still waiting for its student step."""
        if not self.primed:
            return None
        if self.g_step is None:
            self._capture()
        out = self._replay(self.g_step)    # the teacher re-reads the same (last) batch: harmless, results unused
        self.primed = False        # a later call starts a new pipeline (teacher only) instead of repeating this batch
        return out


class _GroupSide:
    """One block of GroupedTeacherKDStep: `group` batches side by side (packed NHWC images, targets, teacher cells),
    everything a view of ONE byte buffer."""
    __slots__ = ("block", "nhwc", "tgts", "wf", "wi", "tk")


class GroupedTeacherKDStep(_KDStepBase):
    """The pipelined step with the frozen teacher run over the batches of `group` consecutive steps AT ONCE, its pass
    cut into `group` segments of equal device time, one beside every student step.

    The teacher does not depend on the student's weights, so nothing forces it to see one batch per launch: at B = 16
    crops most of its layers are a single partial round of tiles on 256 CUs (342 tiles of 128 x 128 on 512 slots in
    the head towers, 8-32 tiles in stages 4-5), and the same forward over 32 / 48 images costs 83 / 72 us per image
    instead of 104 (tools/teacher_batch_probe.py).

    Which batch sits in which of the three blocks (LOAD, PASS, CURRENT) and what a call issues is `GroupPipeline`'s
    business (kd6d/group_pipeline.py: its docstring states the rules); this class is the device side of it.  Loading a
    batch converts it into its slot of LOAD; a teacher segment is a hipGraph of its own, replayed on the teacher's
    stream; a student step is a hipGraph of its own [+ the optimiser's]; a rotation is two device copies with both
    streams joined.  The losses a call returns belong to batch k - 2 * group (None for the first 2 * group calls);
    `flush()` trains one pending batch per call without consuming a new one.
    The teacher's segments are cut where a timed trial replay (device timestamps at every layer-group
    boundary, PoseNet.cut_hook) says the pass has spent s / group of its time; the cut graphs are captured in ONE walk
    through the forward, ending one capture and beginning the next at those boundaries.

    (Measured on the way, 60-step runs of bench.py: the whole group pass inside the last student step's graph of a
    period, 5110-5230 images/s at group 2-4 against 5400 for one teacher forward per step -- the steps without a teacher
    beside them leave the device half empty and the one with it is no shorter than teacher + student back to back;
    segment s forked and JOINED inside the graph of student step s, 5540-5660 -- every step then ends with whichever
    branch is longer running alone; segments as graphs of their own on the teacher's stream, joined with the student's
    stream only at the period's end, as built here: 5780-5810.)

    What it needs from the caller is look-ahead only: 2 * group batches in flight instead of one."""

    def __init__(self, teacher, student, optimizer, loss_weights=(0.1, 1.0, 5.0), cfg_kd=None, warmup=3, group=2,
                 exchange=None):
        if int(group) < 2:
            raise ValueError("GroupedTeacherKDStep: group >= 2 (GraphedKDStep(pipeline=True) is the group of one)")
        # the student's graphs have no teacher branch of their own and the teacher's segments run beside ALL of a step,
        # not its first 60 %: the weight-gradient settings of the strictly sequential step win here too (100-step runs,
        # interleaved, group 2: 5950-5980 images/s with the pipelined settings, 6200-6220 with two workgroups per CU for
        # the grouped launch and its flush behind the FPN sweep; CUs / 4 per side-stream launch: +-0)
        super().__init__(teacher, student, optimizer, loss_weights, cfg_kd, warmup, exchange, teacher_stream=True,
                         side_streams=GraphedKDStep.WGRAD_STREAMS, wgrad=self._wgrad_settings(False))
        self.group = int(group)
        self.pipeline = True
        self.pipe = GroupPipeline(self.group, self)       # which batch is where, what a call issues
        self.g_student = self.g_teacher = None
        self._debug_skip_teacher = 0      # timing experiments only (bench.py --debug-skip-teacher): 1 = no teacher segment
        # is replayed, 2 = every second one
        self.sides = None                 # [current, pass, load]
        self._img_big = self._tgt_big = None
        self._geom = None
        self.segment_ms = None            # the trial replay's time per segment

    @property
    def pending_steps(self):
        return self.pipe.pending_steps

    @property
    def teacher_passes(self):
        """Completed group passes (bench.py reports them)."""
        return self.pipe.teacher_passes

    # ---- blocks ---------------------------------------------------------------------------------
    def _build_sides(self, x, tgt):
        from .kd_losses import CAP, TeacherKnowledge, teacher_flat_sizes
        T = self.group
        B, _, H, W = x.shape
        if T * B * H * W >= 1 << 24:
            # the convolution entry points take < 2^24 rows per launch (kd6d_conv2d_fwd: "grid too large"); the group
            # pass's first layer has group * B * H * W of them
            raise ValueError("GroupedTeacherKDStep: group %d x %d images of %dx%d = %d input pixels per teacher pass, the "
                             "convolution launches take < 2^24 rows: use group <= %d"
                             % (T, B, H, W, T * B * H * W, ((1 << 24) - 1) // (B * H * W)))
        dev = x.device
        snet, tnet = self.student.net, self.teacher.net
        assert snet.dtype == tnet.dtype, "teacher and student share the converted input: same precision"
        per_object = self._per_object()
        wf_n, wi_n = teacher_flat_sizes(T * B, CAP, per_object)      # one selection over the group's T * B images
        # the group's images, a target block per slot, the two buffers of the teacher's cells
        parts = ([((T * B * H * W, 8), snet.dtype)] + [tgt.block_bytes()] * T
                 + [((wf_n,), torch.float32), ((wi_n,), torch.int32)])
        offs, total = block_layout(parts)
        sides = []
        for _ in range(3):
            sd = _GroupSide()
            sd.block = torch.zeros(total, dtype=torch.uint8, device=dev)
            sd.nhwc, *tgt_bytes, sd.wf, sd.wi = block_views(sd.block, parts, offs)
            sd.tgts = []
            for raw in tgt_bytes:
                t = tgt.clone_static()
                t.rebind_block(raw)
                sd.tgts.append(t)
            # the cells of slot s: a contiguous range of every slot array (they are image-major), no copies
            sd.tk = TeacherKnowledge.group_views(sd.wf, sd.wi, T, B, CAP, per_object)
            sides.append(sd)
        self.sides = sides
        self._geom = (B, H, W)
        self.images = ImageList(torch.empty(1, dtype=x.dtype, device=dev).expand(B, 3, H, W),
                                getattr(self, "_sizes", None))                    # shape donor: the step reads `nhwc`
        self._img_big = ImageList(torch.empty(1, dtype=x.dtype, device=dev).expand(T * B, 3, H, W), None)
        big = object.__new__(PackedTargets)                                       # what the teacher reads of the targets
        big.bbox_trans = torch.zeros((T * B,) + tuple(tgt.bbox_trans.shape[1:]), dtype=torch.float32, device=dev)
        big.frame_wh = tgt.frame_wh
        if per_object:
            # the per-object selection reads every image's classes and instance count
            big.class_ids = torch.zeros((T * B,) + tuple(tgt.class_ids.shape[1:]), dtype=torch.int32, device=dev)
            big.n_gt = torch.zeros(T * B, dtype=torch.int32, device=dev)
        if self._gate_reads_targets():
            # the teacher PnP gate also reads every image's intrinsics and 3D boxes
            big.K = torch.zeros((T * B,) + tuple(tgt.K.shape[1:]), dtype=torch.float32, device=dev)
            big.kp3d = torch.zeros((T * B,) + tuple(tgt.kp3d.shape[1:]), dtype=torch.float32, device=dev)
        self._tgt_big = big

    def _gate_reads_targets(self):
        """The teacher's PnP gate on (PoseModuleKD.teacher_pnp_gate): the group pass reads K and kp3d too."""
        return bool(getattr(self.teacher, "teacher_pnp_gate", False))

    def _slot_rows(self, s):
        B, H, W = self._geom
        return slice(s * B * H * W, (s + 1) * B * H * W)

    # ---- GroupPipeline's interface: the blocks ---------------------------------------------------
    def load_slot(self, s, images, tgt):
        x = images.tensors if hasattr(images, "tensors") else images
        B, H, W = self._geom
        assert tuple(x.shape) == (B, 3, H, W), "the captured step has a static batch shape"
        L = self.sides[2]
        assert (tgt.mask_h, tgt.mask_w) == (L.tgts[s].mask_h, L.tgts[s].mask_w)
        # (on the student's stream, between two replays.  On a stream of its own -- the conversion is 15 us of a chain
        #  that bounds the step -- the step got 10-25 % SLOWER: 4640-5280 against 5780-5810 images/s at group 2-6)
        ops.image_to_nhwc(x.contiguous(), self.student.net.dtype, 8, out=L.nhwc[self._slot_rows(s)])
        L.tgts[s].copy_from(tgt)

    def rotate_blocks(self, pass_valid, n_loaded):
        main, ts = torch.cuda.current_stream(), self.teacher_stream
        C, P, L = self.sides
        # a partial load block (a drain before `group` batches arrived): the free slots repeat slot 0, so that the
        # group pass and a capture's warm-up steps see valid inputs everywhere
        for s in range(n_loaded, self.group) if n_loaded else ():
            L.nhwc[self._slot_rows(s)].copy_(L.nhwc[self._slot_rows(0)], non_blocking=True)
            L.tgts[s].copy_from(L.tgts[0])
        main.wait_stream(ts)
        if pass_valid:
            C.block.copy_(P.block, non_blocking=True)
        if n_loaded:
            P.block.copy_(L.block, non_blocking=True)
        ts.wait_stream(main)

    # ---- the teacher's pass over the pass block ----------------------------------------------------------
    def _teacher_forward(self):
        """Python walk through the group pass (current stream = the teacher's); its cells land in the block's flats."""
        T = self.group
        B = self._geom[0]
        P, tnet = self.sides[1], self.teacher.net
        ops.mark("teacher.start")
        gate = self._gate_reads_targets()
        for s in range(T):
            self._tgt_big.bbox_trans[s * B:(s + 1) * B].copy_(P.tgts[s].bbox_trans, non_blocking=True)
            if hasattr(self._tgt_big, "class_ids"):
                self._tgt_big.class_ids[s * B:(s + 1) * B].copy_(P.tgts[s].class_ids, non_blocking=True)
                self._tgt_big.n_gt[s * B:(s + 1) * B].copy_(P.tgts[s].n_gt, non_blocking=True)
            if gate:
                self._tgt_big.K[s * B:(s + 1) * B].copy_(P.tgts[s].K, non_blocking=True)
                self._tgt_big.kp3d[s * B:(s + 1) * B].copy_(P.tgts[s].kp3d, non_blocking=True)
        with _setting(tnet, nhwc_in=P.nhwc), _setting(self.teacher, _teacher_flats=(P.wf, P.wi)):
            self.teacher(self._img_big, targets=self._tgt_big, is_teacher=True, cfg_kd=self.cfg_kd)
        ops.mark("teacher.end")

    def _time_cuts(self):
        """Where to cut the pass: a trial graph of the whole pass with a device timestamp at every layer-group boundary
        (PoseNet.cut_hook), replayed twice; cut k goes to the boundary closest to k / group of the total time."""
        import ctypes
        from ._lib import check, lib
        T, ts, tnet = self.group, self.teacher_stream, self.teacher.net
        tbuf = torch.zeros(1024, dtype=torch.int64, device=self.sides[1].block.device)
        count = [0]

        def stamp():
            assert count[0] < tbuf.numel()
            check(lib.kd6d_mark(ctypes.c_void_p(tbuf.data_ptr() + 8 * count[0]), ops._stream()), "kd6d_mark")
            count[0] += 1

        with torch.no_grad(), torch.cuda.stream(ts):
            self._teacher_forward()                       # eager: allocates every static buffer of this batch size
            ts.synchronize()
            trial = torch.cuda.CUDAGraph()
            with torch.cuda.graph(trial, stream=ts, capture_error_mode="thread_local"):
                stamp()
                with _setting(tnet, cut_hook=stamp):
                    self._teacher_forward()
                stamp()
            trial.replay(); trial.replay()
            ts.synchronize()
        t = tbuf[:count[0]].cpu().tolist()
        rel = [(v - t[0]) * 1e-5 for v in t[1:]]          # ms after the start; rel[i] = end of layer group i, rel[-1] = end
        total, nhook = rel[-1], len(rel) - 1
        assert nhook >= T - 1, "the teacher's forward passes fewer cut points than segments"
        cuts, last = [], -1
        for k in range(1, T):
            cand = range(last + 1, nhook - (T - 1 - k))
            i = min(cand, key=lambda j: abs(rel[j] - k * total / T))
            cuts.append(i); last = i
        edges = [0.0] + [rel[i] for i in cuts] + [total]
        self.segment_ms = [edges[i + 1] - edges[i] for i in range(T)]
        del trial
        return cuts

    def _capture_teacher(self):
        """The pass over the pass block as `group` graphs, captured in ONE walk through the forward: the hook ends the
        running capture at a cut and begins the next graph's."""
        T, ts, tnet = self.group, self.teacher_stream, self.teacher.net
        torch.cuda.synchronize()
        cuts = self._time_cuts()
        graphs = [torch.cuda.CUDAGraph() for _ in range(T)]
        pool = torch.cuda.graph_pool_handle()
        state = {"hook": 0, "g": 0}

        def switch():
            g = state["g"]
            if g < T - 1 and state["hook"] == cuts[g]:
                graphs[g].capture_end()
                state["g"] = g + 1
                graphs[g + 1].capture_begin(pool=pool, capture_error_mode="thread_local")
            state["hook"] += 1

        torch.cuda.synchronize()
        with torch.no_grad(), torch.cuda.stream(ts):
            graphs[0].capture_begin(pool=pool, capture_error_mode="thread_local")
            try:
                with _setting(tnet, cut_hook=switch):
                    self._teacher_forward()
            finally:
                graphs[state["g"]].capture_end()
        assert state["g"] == T - 1, "the teacher's forward passed fewer cut points than segments"
        torch.cuda.synchronize()
        self.g_teacher = graphs

    def replay_teacher_segment(self, i):
        if self.g_teacher is None:
            self._capture_teacher()
        if self._debug_skip_teacher == 1 or (self._debug_skip_teacher == 2 and i % 2 == 1):
            return
        with torch.cuda.stream(self.teacher_stream):
            self.g_teacher[i].replay()

    # ---- the student's step on one slot of the current block ----------------------------------------------
    def _student_body(self, s):
        C = self.sides[0]
        ops.mark("step.start")
        self.tgt, self.t_cur = C.tgts[s], C.tk[s]
        self._nhwc = (C.nhwc[self._slot_rows(s)], None)
        losses = self._student_step(self.t_cur)
        ops.mark("step.end")
        return losses

    def ensure_captured(self):
        """The `group` student graphs (one per slot of the current block; the blocks are only read)."""
        if self.g_student is not None:
            return
        torch.cuda.synchronize()
        # (no gradient exchange in the warm-up: these steps are thrown away with the snapshot, and no RCCL communicator
        #  may come to life before the graphs exist -- see prepare())
        bodies = [lambda s=s: self._student_body(s) for s in range(self.group)]
        self.g_student = self._capture_graphs(bodies, warmup_exchange=False)
        self.g_step = self.g_student[0]

    def replay_student(self, s):
        return self._replay(self.g_student[s])

    # ---- public -------------------------------------------------------------------------------------
    def __call__(self, images, tgt):
        """One call = one batch in.  Returns the (device, static) loss scalars of batch k - 2 * group, None while the
        pipeline fills (the first 2 * group calls)."""
        return self.pipe.feed(images, self._prepare(images, tgt))

    def _prepare(self, images, tgt):
        if not isinstance(tgt, PackedTargets):
            tgt = PackedTargets(tgt, self.student.net.device)
        if self.sides is None:
            self._sizes = getattr(images, "sizes", None)
            self._build_sides(images.tensors if hasattr(images, "tensors") else images, tgt)
        return tgt

    def prepare(self, images, tgt):
        """Capture every graph NOW from a sample batch, leaving the pipeline empty and the training state untouched.

        For data-parallel runs: call it BEFORE the first RCCL communicator of the process is created (before
        kd6d.libs.distributed.init_exchange() and before any torch.distributed collective on the device).  Measured in the
        one-rank rehearsal: graphs instantiated after ncclCommInitRank has run replay 18 % slower in this launch mode
        (5115-5180 against 6216-6290 images/s; destroying the communicator again does not bring it back, creating it after
        the capture costs nothing; which stream the teacher replays on, the number of weight-gradient streams or the
        communicator's channel count make no difference).  Without prepare() the graphs are captured by the first calls
        that need them, as before."""
        tgt = self._prepare(images, tgt)
        if self.g_student is not None and self.g_teacher is not None:
            return
        self.pipe.prime(images, tgt)
        torch.cuda.synchronize()

    def flush(self):
        """Train on ONE batch that is still waiting for its student step, without consuming a new one; None when
        nothing is pending.  (Call until it returns None to drain the pipeline; a later __call__ starts a new one.)"""
        return self.pipe.flush()
