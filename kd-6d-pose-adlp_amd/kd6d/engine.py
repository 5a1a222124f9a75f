"""Static executor of the pose network on the kd6d C ABI.

One `PoseNet` = backbone (darknet53 | darknet_tiny | darknet_tiny_h) + FPN + PoseHead laid out
for MI355X: packed NHWC activations, the head run over ALL pyramid levels in one launch per layer,
parameters / gradients / Adam state in single flat fp32 buffers (one fused optimiser launch, one
RCCL all-reduce bucket), a bf16 shadow of the parameters for the bf16 MFMA path, and a hand-written
reverse sweep instead of an autograd tape (the graph is static).

Reference being replaced: models/model.py:455-487 (PoseModule.__init__), backbone/darknet*.py,
models/model.py:40-103 (FPN), :370-451 (PoseHead).  Parameter NAMES and logical shapes follow the
reference state_dict; storage is KRSC with channels padded to multiples of 8.
"""
import math
from collections import namedtuple

import torch

from . import ops
from .ops import ACT_LEAKY, ACT_NONE, ACT_RELU
from .wgrad_sched import WgradSchedule

ANCHOR_SIZES = [32, 64, 128, 256, 512]
ANCHOR_STRIDES = [8, 16, 32, 64, 128]
TINY_CHANNELS = {
    "darknet_tiny": [[16], [32], [16, 128, 16, 128], [32, 256, 32, 256], [64, 512, 64, 512, 128]],
    "darknet_tiny_h": [[8], [16], [8, 64, 8, 64], [16, 128, 16, 128], [32, 256, 32, 256, 64]],
}
BACKBONE_CFG = {  # arguments/argument.py:59-68
    "darknet53": ([0, 0, 256, 512, 1024], 256),
    "darknet_tiny": ([0, 0, 128, 128], 256),
    "darknet_tiny_h": ([0, 0, 64, 64], 128),
}


BN_EPS, BN_MOMENTUM = 1e-5, 0.1      # every BatchNorm of the reference (torch defaults)


def _pad8(c):
    return (c + 7) // 8 * 8


# ----------------------------------------------------------------------------------------
# the training tape (PoseNet.tape): what the forward walk of the backbone leaves for the reverse sweep, in forward
# order.  `is_block`: the record counts as a block for WgradSchedule.tail_start (a DarkUnit is one block).
# ----------------------------------------------------------------------------------------
class BlockRec(namedtuple("BlockRec", "block x raw batch levels pooled")):
    """One ConvBlock: its input x (what the weight gradient reads), the fp32 convolution output raw, the geometry key
    (batch, levels), and pooled = (h, w) of the convolution output when BatchNorm ran fused with MaxPool2d(2,2)."""
    __slots__ = ()
    is_block = True


class UnitRec(namedtuple("UnitRec", "conv1 conv2")):
    """One DarkUnit: the BlockRecs of its two blocks."""
    __slots__ = ()
    is_block = True


class PoolRec(namedtuple("PoolRec", "stage x batch h w")):
    """The separate MaxPool2d(2,2) behind stage `stage` (0-based) of a darknet-tiny backbone and its input."""
    __slots__ = ()
    is_block = False


class Marker(namedtuple("Marker", "kind stage")):
    """End of stage `stage`: kind "stage" (Darknet-53) or "pooled" (darknet-tiny, the pool fused into the last block)."""
    __slots__ = ()
    is_block = False


# the arguments every train-mode BatchNorm launch ends with, and the block's slice of the zeroed arena
BNArgs = namedtuple("BNArgs", "gamma beta eps momentum running_mean running_var save_mean save_invstd act")
BlockScratch = namedtuple("BlockScratch", "ssum ssq mean invstd w1 w2 barrier stats")
# a block whose BatchNorm + LeakyReLU the NEXT block's convolution applies while it loads its input
Pending = namedtuple("Pending", "block raw sums bn")


# ----------------------------------------------------------------------------------------
# flat parameter store
# ----------------------------------------------------------------------------------------
class Entry:
    __slots__ = ("name", "kind", "shape", "store_shape", "offset", "numel", "trainable", "region", "det", "slab", "parts")

    def __init__(self, name, kind, shape, store_shape, trainable):
        self.name, self.kind, self.shape, self.store_shape = name, kind, tuple(shape), tuple(store_shape)
        self.numel = int(math.prod(store_shape))
        self.trainable = trainable
        self.offset = -1
        self.region = None
        self.det = False        # its gradient is summed in the fixed-point accumulator image (ParamStore.gacc)
        self.slab = None        # ... or arrives as partial images in this fp32 (parts, numel) slab (per-layer weight gradients)
        self.parts = 0


class ParamStore:
    """Flat fp32 buffers.  Regions: 'train' (optimised), 'frozen' (registered-but-unused parameters
    such as backbone.output.* and head.scales.4 of a 4-level student: the reference never gives them
    a gradient, so AdamW never touches them), 'buf' (BN running stats)."""

    ALIGN = 8

    def __init__(self):
        self.entries = {}
        self.order = []
        self.device = torch.device("cpu")
        self.finalized = False

    def add(self, name, kind, shape, store_shape=None, trainable=True, region=None):
        assert not self.finalized and name not in self.entries
        e = Entry(name, kind, shape, store_shape or shape, trainable)
        e.region = region or ("train" if trainable else "frozen")
        self.entries[name] = e
        self.order.append(e)
        return e

    def finalize(self):
        sizes = {"train": 0, "frozen": 0, "buf": 0}
        for e in self.order:
            e.offset = sizes[e.region]
            sizes[e.region] += (e.numel + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.sizes = sizes
        self.n_train = sizes["train"]
        n_par = sizes["train"] + sizes["frozen"]
        self.params = torch.zeros(max(n_par, 8), dtype=torch.float32)
        self.bufs = torch.zeros(max(sizes["buf"], 8), dtype=torch.float32)
        self.grads = None
        self.gacc = None
        self._resolve_plans = {}
        self.shadow = None
        self.finalized = True

    def base(self, e):
        return e.offset + (self.n_train if e.region == "frozen" else 0)

    def storage(self, e, which="params"):
        """1-D view of the entry inside a flat buffer."""
        if e.region == "buf":
            return self.bufs[e.offset:e.offset + e.numel]
        flat = getattr(self, which)
        b = self.base(e)
        return flat[b:b + e.numel]

    def logical_view(self, e, which="params"):
        """View with the reference's logical shape (OIHW for convs) sharing the flat storage."""
        s = self.storage(e, which)
        if e.kind == "conv":
            co, ci, kh, kw = e.shape
            cop, _, _, cip = e.store_shape
            return s.view(cop, kh, kw, cip)[:co, :, :, :ci].permute(0, 3, 1, 2)
        return s.view(e.store_shape)[tuple(slice(0, d) for d in e.shape)]

    def to(self, device):
        self.device = torch.device(device)
        self.params = self.params.to(device)
        self.bufs = self.bufs.to(device)
        if self.grads is not None:
            self.grads = self.grads.to(device)
        if self.gacc is not None:
            self.gacc = self.gacc.to(device)
        for e in self.order:
            e.slab = None
        self._resolve_plans = {}
        if self.shadow is not None:
            self.shadow = self.shadow.to(device)

    def ensure_grads(self):
        if self.grads is None:
            self.grads = torch.zeros(max(self.n_train, 8), dtype=torch.float32, device=self.params.device)
        if self.gacc is None:
            # Fixed-point accumulator image of the gradient bucket (csrc/kd6d_det.h, include/kd6d.h "reproducible
            # reductions"): PLANAR, the lo words of all elements then the hi words.  Every gradient that is a sum over
            # workgroups (per-layer weight gradients, bias gradients, GroupNorm gains / shifts, the head's scales) is
            # added here with integer atomics -- bitwise reproducible -- and resolve_grads() turns the touched regions
            # into fp32 gradients once per step, leaving them zero for the next one.
            self.gacc = torch.zeros(2 * self.acc_stride, dtype=torch.int64, device=self.params.device)

    @property
    def acc_stride(self):
        """Distance (int64 words) between the lo and the hi word of a gradient accumulator."""
        return max(self.n_train, 8)

    def acc(self, e):
        """lo-plane view of the entry's gradient accumulators (pass with acc_stride to the kd6d entry points); marks
        the entry for resolve_grads()."""
        assert e.region == "train"
        self.ensure_grads()
        if not e.det:
            e.det = True
            self._resolve_plans = {}
        b = self.base(e)
        return self.gacc[b:b + e.numel]

    def slab(self, e, parts):
        """fp32 (parts, numel) slab the per-layer weight-gradient launch of entry e stores its partial images into; marks
        the entry for resolve_grads().  One slab per entry, kept for the life of the store (recorded graphs hold it)."""
        assert e.region == "train" and not e.det
        if e.slab is None or e.slab.shape[0] < parts:
            assert not torch.cuda.is_current_stream_capturing(), "ParamStore.slab: allocation inside a graph capture"
            e.slab = torch.empty(parts, e.numel, dtype=torch.float32, device=self.params.device)
            e.parts = 0
        if e.parts != parts:            # another geometry / budget than the last launch: the region table changes
            assert not torch.cuda.is_current_stream_capturing(), \
                "ParamStore.slab: a new split count inside a graph capture (run one eager warm-up step first)"
            e.parts = parts
            self._resolve_plans = {}
        return e.slab[:parts]

    def resolve_grads(self, lo=0, hi=None):
        """grads[lo:hi] += the gradients that were summed across workgroups, for every marked entry in that range:
        fixed-point accumulators (cleared) and partial-image slabs (left as they are; added in the fixed association
        include/kd6d.h states).  One launch
        (kd6d_grad_acc_resolve); the region table is built on first use -- outside any stream capture."""
        hi = self.n_train if hi is None else hi
        plan = self._resolve_plans.get((lo, hi))
        if plan is None:
            assert not torch.cuda.is_current_stream_capturing(), \
                "ParamStore.resolve_grads: first use of a new set of accumulated gradients inside a graph capture " \
                "(run one eager warm-up step first)"
            regs = []           # [first, count, parts, slab address]
            for e in self.order:
                if e.region != "train" or not (lo <= self.base(e) < hi):
                    continue
                b, n = self.base(e), e.numel
                if e.slab is not None and e.parts > 0:
                    regs.append([b, n, e.parts, e.slab.data_ptr()])
                elif e.det:
                    if regs and regs[-1][2] == 0 and regs[-1][0] + regs[-1][1] == b:
                        regs[-1][1] += n
                    else:
                        regs.append([b, n, 0, 0])
            desc, blk = [], 0
            for b, n, parts, ptr in regs:
                desc += [b, n, blk, parts, ptr]
                per = 1024 // (ops.lib.kd6d_grad_acc_resolve_part_groups(parts) if parts else 1)     # elements per workgroup
                blk += (n + per - 1) // per
            plan = (torch.tensor(desc or [0] * 5, dtype=torch.int64, device=self.params.device), len(regs), blk)
            self._resolve_plans[(lo, hi)] = plan
        desc, n_regions, blocks = plan
        if n_regions == 0:
            return
        ops.check(ops.lib.kd6d_grad_acc_resolve(ops._ptr(desc), n_regions, blocks, ops._ptr(self.gacc), self.acc_stride,
                                                ops._ptr(self.grads), ops._stream()), "kd6d_grad_acc_resolve")

    def ensure_shadow(self):
        if self.shadow is None:
            self.shadow = torch.empty(self.params.numel(), dtype=torch.bfloat16, device=self.params.device)
        return self.shadow

    def refresh_shadow(self):
        sh = self.ensure_shadow()
        ops.check(ops.lib.kd6d_cast_f32_to_bf16(ops._ptr(self.params), ops._ptr(sh), self.params.numel(),
                                                ops._stream()), "kd6d_cast_f32_to_bf16")


# ----------------------------------------------------------------------------------------
# layers
# ----------------------------------------------------------------------------------------
class Conv:
    """conv2d (+ optional bias) over 1..5 packed levels.  Weight entry is KRSC-stored."""

    def __init__(self, net, name, cin, cout, k, stride=1, bias=True, trainable=True):
        self.net, self.name = net, name
        self.cin, self.cout, self.k, self.stride = cin, cout, k, stride
        self.cin_p, self.cout_p = _pad8(cin), _pad8(cout)
        st = net.store
        self.w = st.add(name + ".weight", "conv", (cout, cin, k, k), (self.cout_p, k, k, self.cin_p), trainable)
        self.b = st.add(name + ".bias", "vec", (cout,), (self.cout_p,), trainable) if bias else None
        self.geoms = {}
        self._fusable = {}
        self._parts = {}
        self.wt_off = None     # offset inside the dgrad-packed weight buffer
        net.convs.append(self)

    def geom(self, batch, levels):
        key = (batch, tuple(levels))
        g = self.geoms.get(key)
        if g is None:
            g = ops.Geom(batch, self.cin_p, self.cout_p, self.k, self.stride, self.k // 2, list(levels))
            self.geoms[key] = g
        return g

    # pointers into the flat buffers ------------------------------------------------------
    def weight(self):
        st = self.net.store
        src = st.params if self.net.dtype == torch.float32 else st.shadow
        b = st.base(self.w)
        return src[b:b + self.w.numel]

    def bias(self):
        return None if self.b is None else self.net.store.storage(self.b)

    def weight_t(self):
        return self.net.wt[self.wt_off:self.wt_off + self.w.numel]

    def flops(self, g):
        """Algorithmic FLOPs of one pass (2*MAC on the reference's logical channel counts)."""
        return 2 * g.rows_out * self.cout * self.k * self.k * self.cin

    def fwd(self, x, batch, levels, out=None, scale=None, shift=None, act=ACT_NONE, residual=None,
            seg_scale=None, out_f32=False, stats=None, stats_groups=0):
        g = self.geom(batch, levels)
        if shift is None:
            shift = self.bias()
        return ops.conv2d_fwd(g, x, self.weight(), out=out, ch_scale=scale, ch_shift=shift, act=act,
                              residual=residual, seg_scale=seg_scale, out_f32=out_f32, flops=self.flops(g),
                              stats=stats, stats_groups=stats_groups, workspace=self.net.workspace()), g

    def norm_fusable(self, batch, levels, kind, groups=0):
        """Does this layer take the conv + normalisation + activation launch (kd6d_conv2d_fwd_norm)?  Cached per
        geometry and value of the `conv.fuse_norm` option."""
        key = (batch, tuple(levels), kind, groups, self.net.dtype, ops.get_option("conv.fuse_norm"))
        ok = self._fusable.get(key)
        if ok is None:
            ok = self._fusable[key] = ops.conv_norm_fusable(self.geom(batch, levels), self.net.dtype, kind, groups)
        return ok

    def fwd_norm(self, x, batch, levels, y, kind, gamma, beta, act, raw_out=None, groups=0, stats=None, **bn):
        """conv (+ bias) -> normalisation -> activation in one launch; stats / counters live in the per-step zeroed arena."""
        g = self.geom(batch, levels)
        net = self.net
        if stats is None:
            stats = net.scratch(self.name + ".fstats", ops.conv_norm_stats_floats(g, kind, groups))
        counters = net.scratch(self.name + ".fctr", ops.conv_norm_counter_words(g, kind))
        return ops.conv2d_fwd_norm(g, x, self.weight(), y, kind, gamma, beta, stats, counters, act, raw_out=raw_out,
                                   bias=self.bias(), groups=groups, flops=self.flops(g), **bn), g

    def wgrad_slab(self, g, dtype, cu_budget):
        """The slab this layer's weight-gradient launch stores its partial images into (ParamStore.slab)."""
        key = (id(g), dtype, cu_budget, ops.get_option("wgrad.small"))
        parts = self._parts.get(key)
        if parts is None:
            parts = self._parts[key] = ops.conv2d_wgrad_parts(g, dtype, self.b is not None, cu_budget)
        return self.net.store.slab(self.w, parts)

    def stem_slab(self, g, dtype):
        """The slab of the fused pooled-BatchNorm backward + weight gradient (ops.bn_pool_bwd_wgrad), or None when that
        launch does not take this geometry (or option stem.fused = 0).  Sized for WgradSchedule.budget(), the budget of
        the separate launch it stands in for: the fused launch splits the pixels as that one does (csrc/conv_plan.h,
        stem_bwd_rule)."""
        budget = self.net.wgrad.budget()
        key = (id(g), dtype, "stem", budget, ops.get_option("stem.fused"))
        parts = self._parts.get(key)
        if parts is None:
            parts = self._parts[key] = ops.bn_pool_bwd_wgrad_parts(g, dtype, budget) if self.b is None else 0
        return self.net.store.slab(self.w, parts) if parts else None

    def bwd(self, x, dy, batch, levels, need_dx=True, dx=None, accumulate=False, need_dw=True):
        """wgrad (+ bias grad) where the network's WgradSchedule puts it, then dgrad."""
        g = self.geom(batch, levels)
        if need_dw:
            self.net.wgrad.submit(self, g, x, dy)
        if not need_dx:
            return None
        return ops.conv2d_dgrad(g, dy, self.weight_t(), dx=dx, accumulate=accumulate, flops=self.flops(g))


class BatchNorm:
    def __init__(self, net, name, c, trainable=True):
        st = net.store
        self.net, self.c = net, c
        self.gamma = st.add(name + ".weight", "vec", (c,), (c,), trainable)
        self.beta = st.add(name + ".bias", "vec", (c,), (c,), trainable)
        self.rm = st.add(name + ".running_mean", "vec", (c,), (c,), False, region="buf")
        self.rv = st.add(name + ".running_var", "vec", (c,), (c,), False, region="buf")
        self.nbt_index = len(net.bns)
        net.bns.append((name, self))
        self.fold = None

    def folded(self):
        """eval-mode scale/shift (computed once per weight load; torch ops = plumbing)."""
        if self.fold is None:
            st = self.net.store
            scale = st.storage(self.gamma) * torch.rsqrt(st.storage(self.rv) + BN_EPS)
            shift = st.storage(self.beta) - st.storage(self.rm) * scale
            self.fold = (scale.contiguous(), shift.contiguous())
        return self.fold


class ConvBlock:
    """conv(no bias) + BN + LeakyReLU(0.1)  (backbone/common.py:250-324)."""
    # up to 256 workgroups adding into one channel; beyond that a separate pass wins
    FUSE_STATS_MAX_ROWS = 1 << 15

    @staticmethod
    def bwd_replicas(rows):
        """Replica rows of the backward reduction's accumulators (kd6d.h): from 64 workgroups up."""
        return 8 if rows >= (1 << 14) else 1

    def _scratch_sizes(self, rows):
        """THE layout of the block's slice of the per-step zeroed arena, in fp32 slots and in order (BlockScratch): the
        {sum, sumsq} accumulators of the batch statistics, saved mean / invstd, the backward's R replica rows of two
        accumulator sums, its barrier words.  An accumulator (kd6d_acc, kd6d.h) takes ACC_FLOATS slots."""
        c, A, R = self.conv.cout_p, ops.ACC_FLOATS, self.bwd_replicas(rows)
        return (A * c, A * c, c, c, A * R * c, A * R * c, ops.BARRIER_WORDS)

    def scratch_floats(self, rows):
        return sum(self._scratch_sizes(rows))

    def scratch_views(self, rows):
        """The named views of that slice for a convolution output of `rows` rows; `stats` is ssum and ssq as the one
        {sum, sumsq} tensor the convolution epilogue takes."""
        hit = self._views.get(rows)
        if hit is None or hit[0] is not self.net.scratch_buf:       # first use, or the arena moved (PoseNet.to)
            sizes = self._scratch_sizes(rows)
            s = self.net.scratch(self.name, sum(sizes))
            views, o = [], 0
            for n in sizes:
                views.append(s[o:o + n])
                o += n
            hit = self._views[rows] = (self.net.scratch_buf, BlockScratch(*views, stats=s[0:sizes[0] + sizes[1]]))
        return hit[1]

    def __init__(self, net, name, cin, cout, k, stride=1):
        self.net, self.name = net, name
        self.conv = Conv(net, name + ".conv", cin, cout, k, stride, bias=False)
        self.bn = BatchNorm(net, name + ".bn", self.conv.cout_p)
        self._views = {}        # rows -> (the arena they were cut from, BlockScratch)
        assert self.conv.cout_p == cout, "BN channels must already be a multiple of 8"

    def fwd_eval(self, x, batch, levels, residual=None):
        sc, sh = self.bn.folded()
        y, g = self.conv.fwd(x, batch, levels, scale=sc, shift=sh, act=ACT_LEAKY, residual=residual)
        return y, g.levels_out

    def _train_ctx(self, batch, levels):
        """(geometry, arena views, BatchNorm argument bundle) of a training forward."""
        st, bn = self.net.store, self.bn
        geom = self.conv.geom(batch, levels)
        sv = self.scratch_views(geom.rows_out)
        return geom, sv, BNArgs(st.storage(bn.gamma), st.storage(bn.beta), BN_EPS, BN_MOMENTUM, st.storage(bn.rm),
                                st.storage(bn.rv), sv.mean, sv.invstd, ACT_LEAKY)

    def fwd_train(self, x, batch, levels, tape, pool=False, residual=None):
        """-> (z, levels of z); one BlockRec on the tape.
        residual: a tensor of the output's shape and dtype added after the activation (the DarkUnit's identity,
        backbone/darknet53.py:54-58; kd6d_bn_train_fwd_res); only on the separate normalise launch (no pooling or fusion).
        pool=True: the block is followed by MaxPool2d(2,2) (darknet.py:94-97); normalisation, activation and
        pooling run as one kernel and only the pooled tensor is stored (csrc/norm_ops.hip, bn_pool_*)."""
        net = self.net
        geom, sv, bn = self._train_ctx(batch, levels)
        # the pre-BN tensor stays fp32 (also in bf16 mode): (x - mean) must not cancel bf16 rounding
        raw = net.buf(self.name + ".raw", (geom.rows_out, self.conv.cout_p), torch.float32)
        if residual is not None:
            assert not pool and not net.fuse_norm_on(), \
                "ConvBlock.fwd_train: the residual add runs only on the separate normalise launch"
        if not pool and net.fuse_norm_on() and self.conv.norm_fusable(batch, levels, ops.NORM_BATCH):
            # conv -> batch statistics -> normalise + LeakyReLU as ONE launch (grid barrier in the epilogue)
            z = net.buf(self.name + ".z", raw.shape, net.dtype)
            self.conv.fwd_norm(x, batch, levels, z, ops.NORM_BATCH, bn.gamma, bn.beta, bn.act, raw_out=raw, eps=bn.eps,
                               momentum=bn.momentum, running_mean=bn.running_mean, running_var=bn.running_var,
                               save_mean=bn.save_mean, save_invstd=bn.save_invstd)
            tape.append(BlockRec(self, x, raw, batch, tuple(levels), None))
            return z, geom.levels_out
        # batch statistics come out of the conv epilogue; for the long, narrow first layers (hundreds of
        # workgroups would add into the same 8..64 addresses) a separate reduction pass is cheaper
        fused = geom.rows_out <= self.FUSE_STATS_MAX_ROWS
        self.conv.fwd(x, batch, levels, out_f32=True, out=raw, stats=sv.stats if fused else None, stats_groups=0)
        if not fused:
            ops.colstats(raw, sv.ssum, sv.ssq)
        return self._normalise(x, raw, geom, sv, bn, tape, pool, residual)

    def fwd_train_on_load(self, x, batch, levels, tape, pending, defer, pool=False):
        """The transform-on-load path (kd6d_conv2d_fwd_block) -> (z, levels of z, Pending or None).
        pending: the previous block's record when ITS normalisation was deferred to this convolution (x is None then).
        defer=True: this block's BatchNorm + LeakyReLU is NOT launched here -- the next block of the stage applies it
        while it loads its input; z is None and the Pending record for that block is returned."""
        net = self.net
        geom, sv, bn = self._train_ctx(batch, levels)
        c = self.conv.cout_p
        raw = net.buf(self.name + ".raw", (geom.rows_out, c), torch.float32)
        bn_in = z_in = None
        if pending is not None:
            bn_in = dict(pending.bn._asdict(), sums=pending.sums, replicas=ops.BN_REPLICAS)
            z_in = net.buf(pending.block.name + ".z", pending.raw.shape, net.dtype)     # written by this launch
            x = pending.raw
        if defer:          # the consumer adds the replica rows
            stats, reps = net.scratch(self.name + ".sums", ops.BN_REPLICAS * 2 * c * ops.ACC_FLOATS), ops.BN_REPLICAS
        else:              # bn_train_fwd / bn_pool_train_fwd read plain {sum, sumsq}
            stats, reps = sv.stats, 1
        fused = defer or geom.rows_out <= self.FUSE_STATS_MAX_ROWS
        ops.conv2d_fwd_block(geom, x, self.conv.weight(), raw, stats=stats if fused else None, stats_replicas=reps,
                             bn_in=bn_in, z_out=z_in, flops=self.conv.flops(geom))
        if pending is not None:
            x = z_in           # what the weight gradient reads
        if defer:
            tape.append(BlockRec(self, x, raw, batch, tuple(levels), None))
            return None, geom.levels_out, Pending(self, raw, stats, bn)
        if not fused:
            ops.colstats(raw, sv.ssum, sv.ssq)
        return self._normalise(x, raw, geom, sv, bn, tape, pool, None) + (None,)

    def _normalise(self, x, raw, geom, sv, bn, tape, pool, residual):
        """The normalise launch behind the convolution (pooled, with the residual, or plain) and the tape record."""
        net, batch, levels = self.net, geom.batch, tuple(geom.levels_in)
        if pool:
            (h, w), = geom.levels_out
            z = net.buf(self.name + ".zpool", (batch * (h // 2) * (w // 2), self.conv.cout_p), net.dtype)
            ops.bn_pool_train_fwd(raw, z, batch, h, w, sv.ssum, sv.ssq, *bn)
            tape.append(BlockRec(self, x, raw, batch, levels, (h, w)))
            return z, [(h // 2, w // 2)]
        z = net.buf(self.name + ".z", raw.shape, net.dtype)
        if residual is not None:
            ops.bn_train_fwd_res(raw, residual, z, sv.ssum, sv.ssq, *bn)
        else:
            ops.bn_train_fwd(raw, z, sv.ssum, sv.ssq, *bn)
        tape.append(BlockRec(self, x, raw, batch, levels, None))
        return z, geom.levels_out

    def bwd(self, rec, dz, need_dx=True, dx=None, accumulate=False):
        net, st = self.net, self.net.store
        x, raw, pooled = rec.x, rec.raw, rec.pooled
        R = self.bwd_replicas(raw.shape[0])
        sv = self.scratch_views(raw.shape[0])       # the barrier words were zeroed with the arena at the start of the step
        gamma, beta = st.storage(self.bn.gamma), st.storage(self.bn.beta)
        dgamma, dbeta = st.storage(self.bn.gamma, "grads"), st.storage(self.bn.beta, "grads")
        if pooled is not None and not need_dx and x.dtype == torch.bfloat16:
            # nothing but the weight gradient reads the gradient of the convolution output: formed in LDS, never stored
            g = self.conv.geom(rec.batch, rec.levels)
            slab = self.conv.stem_slab(g, x.dtype)
            if slab is not None:
                ops.bn_pool_train_bwd_reduce(raw, dz, rec.batch, pooled[0], pooled[1], sv.mean, sv.invstd, gamma, beta,
                                             ACT_LEAKY, sv.w1, sv.w2, replicas=R)
                ops.bn_pool_bwd_wgrad(g, x, raw, dz, sv.mean, sv.invstd, gamma, beta, ACT_LEAKY, sv.w1, sv.w2, dgamma, dbeta,
                                      slab, replicas=R, flops=self.conv.flops(g), cu_budget=net.wgrad.budget())
                return None
        draw = net.buf(self.name + ".draw", raw.shape, net.dtype)
        if pooled is not None:                  # dz is the gradient of the pooled output
            ops.bn_pool_train_bwd(raw, dz, draw, rec.batch, pooled[0], pooled[1], sv.mean, sv.invstd, gamma, beta,
                                  ACT_LEAKY, sv.w1, sv.w2, dgamma, dbeta, replicas=R, counter=sv.barrier)
        else:
            ops.bn_train_bwd(raw, dz, draw, sv.mean, sv.invstd, gamma, beta, ACT_LEAKY, sv.w1, sv.w2, dgamma, dbeta,
                             replicas=R, counter=sv.barrier)
        return self.conv.bwd(x, draw, rec.batch, rec.levels, need_dx=need_dx, dx=dx, accumulate=accumulate)


class GroupNormReLU:
    def __init__(self, net, name, c, groups=32):
        st = net.store
        self.net, self.name, self.c, self.groups = net, name, c, groups
        self.gamma = st.add(name + ".weight", "vec", (c,), (c,), True)
        self.beta = st.add(name + ".bias", "vec", (c,), (c,), True)

    def stats(self, batch, levels):
        """{sum, sumsq} per (level, image, group) in the per-step zeroed scratch arena; filled by the
        epilogue of the conv that produces this layer's input."""
        return self.net.scratch(self.name + ".stats", len(levels) * batch * self.groups * 2 * ops.ACC_FLOATS)

    def fwd(self, x, batch, levels, out=None):
        net, st = self.net, self.net.store
        hw = [h * w for (h, w) in levels]
        if out is None:
            out = net.buf(self.name + ".y", x.shape)
        ops.gn_relu_fwd(x, out, hw, batch, self.groups, st.storage(self.gamma), st.storage(self.beta), 1e-5,
                        self.stats(batch, levels), flags=ops.GN_STATS_READY)
        return out

    def fwd_fused(self, conv, x, batch, levels, out, raw_out=None):
        """conv -> GroupNorm -> ReLU as one launch (the conv's epilogue); the statistics land where bwd expects them."""
        st = self.net.store
        conv.fwd_norm(x, batch, levels, out, ops.NORM_GROUP, st.storage(self.gamma), st.storage(self.beta), ACT_RELU,
                      raw_out=raw_out, groups=self.groups, eps=1e-5, stats=self.stats(batch, levels))
        return out

    def bwd_item(self, x, dz, batch, levels, dx):
        """The argument tuple of ops.gn_relu_bwd / gn_relu_bwd_pair for this layer."""
        net, st = self.net, self.net.store
        gsum = net.scratch(self.name + ".gsum", ops.gn_bwd_workspace_floats(len(levels), batch, self.groups))
        return (x, dz, dx, st.storage(self.gamma), st.storage(self.beta), self.stats(batch, levels), gsum,
                st.acc(self.gamma), st.acc(self.beta))

    def bwd(self, x, dz, batch, levels, dx):
        hw = [h * w for (h, w) in levels]
        x, dz, dx, gamma, beta, stats, gsum, dgamma, dbeta = self.bwd_item(x, dz, batch, levels, dx)
        ops.gn_relu_bwd(x, dz, dx, hw, batch, self.groups, gamma, beta, stats, gsum, dgamma, dbeta,
                        self.net.store.acc_stride, flags=ops.GN_WS_ZEROED)
        return dx


# ----------------------------------------------------------------------------------------
# the network
# ----------------------------------------------------------------------------------------
class PoseNet:
    def __init__(self, arch, dtype=torch.bfloat16, n_class=16, n_conv=4, prior=0.01):
        assert arch in BACKBONE_CFG, "Unsupported backbone %r" % (arch,)
        self.arch, self.dtype = arch, dtype
        self.store = ParamStore()
        self.convs, self.bns = [], []
        self._bufs, self._scratch_off, self._scratch_size, self.scratch_buf = {}, {}, 0, None
        self.wt = None
        self.training = True
        self.in_hw = None
        self.levels, self.batch = None, None
        # ---- the knobs of the reverse sweep's weight-gradient schedule (wgrad_sched.py reads them when it needs them;
        # GraphedKDStep / GroupedTeacherKDStep and bench.py set them) ----
        self.side_stream = None        # set (e.g. by GraphedKDStep) to run weight gradients concurrently
        self.side_streams = None       # optional list: consecutive weight gradients rotate over these streams
        self.wgrad_cu_budget = 0       # CUs each forked weight gradient aims to fill (0 = the device)
        # the weight gradients of the head and FPN output convolutions as ONE grouped launch per step
        # (csrc/conv_wgrad_group.hip); created on first use, bf16 only.  wgrad_group_wgs: workgroups of that launch
        # (0 = one per two CUs).  Measured on the step (images/s, 64 / 128 / 256 workgroups): pipelined 4831 / 4828 /
        # 4788, strictly sequential 4050 / 4164 / 4241 -- GraphedKDStep asks for one per CU in sequential mode
        self.use_wgrad_group = True
        self.wgrad_group_wgs = 0
        self.wgrad_group_flush = "head_end"     # or "fpn_end" (GraphedKDStep picks by launch mode)
        self.wgrad = WgradSchedule(self, ops)   # ... and its transient state
        # set by GraphedKDStep around its own calls only: the packed NHWC input to use instead of converting `images`
        # (nhwc_in), or where to put the conversion (nhwc_out)
        self.nhwc_in = self.nhwc_out = None
        # GroupedTeacherKDStep: called at layer-group boundaries of an eval-mode forward (the places where the frozen
        # teacher's pass over several steps' batches may be cut into per-step graph segments)
        self.cut_hook = None
        self.grad_hook = None           # called by backward() when the FPN + head gradients have been issued
        self.resolve_hi = None          # backward() resolves the accumulated gradients of [0, resolve_hi) at its end (None: all)
        self.fuse_pool = True           # BN + act + maxpool as one kernel (training)
        # conv + normalisation + activation as one launch (kd6d_conv2d_fwd_norm: in-kernel barrier in the conv epilogue).
        # Measured on the step, interleaved runs on one box (profiles/README.md round 3): the frozen teacher's towers
        # fused (the fp32 pre-normalisation tensor is then not even stored) +0.4 ... +1.1 % on config 2 but -1.8 % on
        # config 4's shard and -1.2 % on full frames; the student's towers fused -3 %, its BatchNorm blocks -1.2 %.  A
        # workgroup that waits at a barrier keeps its LDS and wave slots while the other stream's kernels could use them:
        # a kernel boundary is the cheaper barrier when two streams share the device.  Off (None = off); the entry point,
        # its tests and the residency argument (csrc/kd6d_barrier.h) stay for single-stream callers.
        self.fuse_norm = None
        # inside a stage of the student's backbone a block's BatchNorm + LeakyReLU can be applied by the NEXT block's
        # convolution while it loads its input (kd6d_conv2d_fwd_block): up to 10 of the 15 normalise launches (and the 3
        # separate statistics passes of stage 3) leave the forward chain without any wait inside a kernel.  Measured
        # (interleaved runs on one box, round 3): 0 -> 5192 / 5212 images/s, 1 -> 5151 / 5172, 2 -> 5187: the
        # register-staged kernel that can transform on load gives back what the removed launches save (the 3x3 layers
        # leave the LDS-DMA kernels and re-read the fp32 tensor once per tap).  Off by default; kept, tested, for
        # layer mixes where the normalise launches weigh more.
        self.bn_on_load = 0            # 0 off | 1 where the next block is a 1x1 convolution | 2 every in-stage transition
        # cls / pose tower layers as one launch (training): 0 = off, 1 = forward and data gradients, 2 = forward only
        self.pair_towers = 1
        feat, oc = BACKBONE_CFG[arch]
        self.out_channel = oc
        self.n_levels = 5 if arch == "darknet53" else 4
        self.n_cls = n_class - 1
        st = self.store
        # ---- backbone ----
        if arch == "darknet53":
            self.init_block = ConvBlock(self, "backbone.features.init_block", 3, 32, 3)
            self.stages = []
            cin = 32
            for i, (c, n) in enumerate(zip([64, 128, 256, 512, 1024], [2, 3, 9, 9, 5])):
                units = []
                for j in range(n):
                    nm = "backbone.features.stage%d.unit%d" % (i + 1, j + 1)
                    if j == 0:
                        units.append(("down", ConvBlock(self, nm, cin, c, 3, 2)))
                    else:
                        units.append(("res", ConvBlock(self, nm + ".conv1", cin, c // 2, 1),
                                      ConvBlock(self, nm + ".conv2", c // 2, c, 3)))
                    cin = c
                self.stages.append(units)
            st.add("backbone.output.weight", "vec", (1000, 1024), (1000, 1024), False)
            st.add("backbone.output.bias", "vec", (1000,), (1000,), False)
        else:
            self.stages = []
            cin = 3
            chans = TINY_CHANNELS[arch]
            for i, per_stage in enumerate(chans):
                units = []
                for j, c in enumerate(per_stage):
                    pointwise = len(per_stage) > 1 and (j % 2 == 0)     # darknet.py:92 with odd_pointwise
                    units.append(ConvBlock(self, "backbone.features.stage%d.unit%d" % (i + 1, j + 1), cin, c,
                                           1 if pointwise else 3))
                    cin = c
                self.stages.append(units)
            st.add("backbone.output.final_conv.weight", "vec", (1000, cin, 1, 1), (1000, cin, 1, 1), False)
            st.add("backbone.output.final_conv.bias", "vec", (1000,), (1000,), False)
        # ---- FPN ----
        self.inner, self.outc = {}, {}
        for i, c in enumerate(feat):
            if c == 0:
                continue
            self.inner[i] = Conv(self, "fpn.inner_convs.%d" % i, c, oc, 1)
            self.outc[i] = Conv(self, "fpn.out_convs.%d" % i, oc, oc, 3)
        self.p6 = Conv(self, "fpn.top_blocks.p6", feat[-1], oc, 3, 2)
        self.p7 = Conv(self, "fpn.top_blocks.p7", oc, oc, 3, 2)
        # ---- head ----
        self.cls_tower, self.pose_tower = [], []
        for t, tower in (("cls_tower", self.cls_tower), ("pose_tower", self.pose_tower)):
            for i in range(n_conv):
                tower.append((Conv(self, "head.%s.%d" % (t, 3 * i), oc, oc, 3),
                              GroupNormReLU(self, "head.%s.%d" % (t, 3 * i + 1), oc)))
        self.cls_logits = Conv(self, "head.cls_logits", oc, self.n_cls, 3)
        self.pose_pred = Conv(self, "head.pose_pred", oc, self.n_cls * 16, 3)
        self.scales = st.add("head.scales", "vec", (8,), (8,), True)          # slots 0..n_levels-1 used
        for l in range(5):
            if l >= self.n_levels:
                st.add("head.scales.%d.scale" % l, "vec", (1,), (1,), False)
        self.prior = prior
        st.finalize()
        self.reset_parameters()

    # ---- parameters ----------------------------------------------------------------------
    def named_logical(self):
        """(reference name, logical-shape view) for every state_dict tensor except the anchors."""
        st = self.store
        out = []
        for e in st.order:
            if e.name == "head.scales":
                for l in range(self.n_levels):
                    out.append(("head.scales.%d.scale" % l, st.storage(e)[l:l + 1], True))
                continue
            out.append((e.name, st.logical_view(e), e.region != "buf"))
        return out

    def reset_parameters(self, seed=None):
        """Reference initialisation (darknet*.py:_init_params, model.py:22-37,420-433)."""
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        st = self.store
        for e in st.order:
            v = st.logical_view(e) if e.name != "head.scales" else st.storage(e)
            if e.name == "head.scales" or e.name.endswith(".scale"):
                v.fill_(1.0)
            elif e.name.endswith("running_var"):
                v.fill_(1.0)
            elif e.name.endswith("running_mean"):
                v.zero_()
            elif e.kind == "conv":
                fan_in = e.shape[1] * e.shape[2] * e.shape[3]
                if e.name.startswith("head."):
                    v.copy_(torch.randn(e.shape, generator=g) * 0.01)
                else:
                    a = 1.0 if e.name.startswith("fpn.") else 0.0
                    bound = math.sqrt(2.0 / (1 + a * a)) * math.sqrt(3.0 / fan_in)
                    v.copy_((torch.rand(e.shape, generator=g) * 2 - 1) * bound)
            elif e.name.endswith("bn.weight") or (e.name.startswith("head.") and e.name.endswith(".weight")):
                v.fill_(1.0)          # BN / GN gamma
            elif e.name == "head.cls_logits.bias":
                v.fill_(-math.log((1 - self.prior) / self.prior))
            elif e.name.startswith("backbone.output"):
                v.copy_(torch.randn(e.shape, generator=g) * 0.01 if len(e.shape) > 1 else torch.zeros(e.shape))
            else:
                v.zero_()
        self.invalidate()

    def invalidate(self):
        for _, bn in self.bns:
            bn.fold = None
        self._weights_dirty = True

    def refresh_derived_in_place(self, need_dgrad=False):
        """The master weights / buffers changed BEHIND recorded hipGraphs (a parameter broadcast after the step was
        captured: train_kd.py's graphs-first start of a data-parallel run): recompute everything the recorded kernels read
        that is derived from them INTO THE BUFFERS THEY WERE RECORDED WITH -- the bf16 shadow, the dgrad packing and the
        eval-mode BatchNorm folds.  (invalidate() would free the fold tensors whose addresses the graphs hold.)"""
        st = self.store
        for _, bn in self.bns:
            if bn.fold is not None:
                scale = st.storage(bn.gamma) * torch.rsqrt(st.storage(bn.rv) + BN_EPS)
                bn.fold[0].copy_(scale)
                bn.fold[1].copy_(st.storage(bn.beta) - st.storage(bn.rm) * scale)
        self._weights_dirty = True
        self.prepare_weights(need_dgrad=need_dgrad and self.wt is not None)

    def to(self, device):
        self.store.to(device)
        self._bufs.clear()
        self.scratch_buf = None
        self.wt = None
        self.invalidate()
        return self

    @property
    def device(self):
        return self.store.params.device

    # ---- workspaces ----------------------------------------------------------------------
    def buf(self, name, shape, dtype=None):
        dtype = dtype or self.dtype
        key = (name, tuple(shape), dtype)
        b = self._bufs.get(key)
        if b is None:
            b = torch.empty(tuple(shape), dtype=dtype, device=self.device)
            self._bufs[key] = b
        return b

    SCRATCH_FLOATS = 1 << 22
    WORKSPACE_BYTES = 64 << 20      # split-K partial slabs (fp32) of the few-tile / long-K layers

    def fuse_norm_on(self):
        return False if self.fuse_norm is None else bool(self.fuse_norm)

    def workspace(self):
        ws = self._bufs.get("__workspace__")
        if ws is None:
            ws = torch.empty(self.WORKSPACE_BYTES // 4, dtype=torch.float32, device=self.device)
            self._bufs["__workspace__"] = ws
        return ws

    def scratch(self, name, n):
        """fp32 slice of the per-step scratch arena (zeroed once per step by the training forward)."""
        off = self._scratch_off.get((name, n))          # per (name, size): the same net may run several batch sizes
        if off is None:
            off = self._scratch_size
            self._scratch_off[(name, n)] = off
            self._scratch_size += (n + 7) // 8 * 8
            assert self._scratch_size <= self.SCRATCH_FLOATS, "scratch arena too small"
        if self.scratch_buf is None:
            self.scratch_buf = torch.zeros(self.SCRATCH_FLOATS, dtype=torch.float32, device=self.device)
        return self.scratch_buf[off:off + n]

    def prepare_weights(self, need_dgrad):
        """bf16 shadow + dgrad packing (one launch each) whenever the master weights changed."""
        st = self.store
        if self.dtype == torch.bfloat16 and (self._weights_dirty or st.shadow is None):
            st.refresh_shadow()
        if need_dgrad:
            if self.wt is None:
                off, blk, desc = 0, 0, []
                self._dgrad_layers = [c for c in self.convs if c.w.trainable]
                for c in self._dgrad_layers:
                    c.wt_off = off
                    desc += [st.base(c.w), off, c.cout_p, c.cin_p, c.k, blk]
                    off += c.w.numel
                    blk += (c.w.numel + 2047) // 2048
                self.wt = torch.empty(off, dtype=self.dtype, device=self.device)
                self._dgrad_desc = torch.tensor(desc, dtype=torch.int32, device=self.device)
                self._dgrad_blocks = blk
            src = st.params if self.dtype == torch.float32 else st.shadow
            ops.pack_dgrad_weights(src, self.wt, self._dgrad_desc, len(self._dgrad_layers), self._dgrad_blocks)
        self._weights_dirty = False

    # ---- forward ---------------------------------------------------------------------------
    def _cut(self):
        if self.cut_hook is not None and not self.training:
            self.cut_hook()

    def _backbone53(self, x, B, lv):
        if self.training:
            # training (the teacher recipe): every block is conv (+ fused statistics) -> normalise launch; the
            # transform-on-load and conv + normalisation fusions have no residual path
            assert not self.fuse_norm_on() and not self.bn_on_load, \
                "darknet53 training runs without fuse_norm and bn_on_load"
            tape = self.tape
            x, lv = self.init_block.fwd_train(x, B, lv, tape)
            feats = []
            for i, units in enumerate(self.stages):
                for u in units:
                    if u[0] == "down":
                        x, lv = u[1].fwd_train(x, B, lv, tape)
                    else:
                        x, lv = self.unit_fwd_train(u, x, B, lv)
                tape.append(Marker("stage", i))
                feats.append((x, lv))
            return feats
        x, lv = self.init_block.fwd_eval(x, B, lv)
        self._cut()
        feats = []
        for units in self.stages:
            for u in units:
                if u[0] == "down":
                    x, lv = u[1].fwd_eval(x, B, lv)
                else:
                    h, _ = u[1].fwd_eval(x, B, lv)
                    x, lv = u[2].fwd_eval(h, B, lv, residual=x)
                self._cut()
            feats.append((x, lv))
        return feats

    def unit_fwd_train(self, u, x, B, lv):
        """DarkUnit ("res", conv1 block, conv2 block) in training mode: conv2(conv1(x)) + x with the add behind conv2's
        LeakyReLU (backbone/darknet53.py:54-58); one UnitRec on the tape."""
        recs = []
        h, _ = u[1].fwd_train(x, B, lv, recs)
        y, lv = u[2].fwd_train(h, B, lv, recs, residual=x)
        self.tape.append(UnitRec(*recs))
        return y, lv

    def unit_bwd(self, rec, grad):
        """Backward of a UnitRec: grad (the gradient of the unit's output) becomes, in place, the gradient of its input,
        d_out + conv1's data gradient."""
        rec1, rec2 = rec.conv1, rec.conv2
        d_mid = rec2.block.bwd(rec2, grad, dx=self.buf(rec2.block.name + ".dx", rec2.x.shape))
        # written over d_out: on this stream conv2's BatchNorm backward has already consumed d_out, and the forked
        # weight gradients read only x and draw
        rec1.block.bwd(rec1, d_mid, dx=grad, accumulate=True)
        return grad

    def _backbone_tiny(self, x, B, lv):
        feats = []
        n = len(self.stages)
        for i, units in enumerate(self.stages):
            if self.training and self.fuse_pool:
                pending = None
                for j, u in enumerate(units):
                    last = j == len(units) - 1
                    # inside a stage the next block applies this block's BatchNorm + LeakyReLU while loading its input
                    # (one launch per block instead of conv [+ statistics] + normalise): stages 3-5; the first two
                    # stages are single blocks
                    nxt_pointwise = (not last) and units[j + 1].conv.k == 1
                    defer = self.bn_on_load == 2 and not last or (self.bn_on_load == 1 and nxt_pointwise)
                    pool = i != n - 1 and last
                    if pending is None and not defer:
                        x, lv = u.fwd_train(x, B, lv, self.tape, pool=pool)
                    else:
                        x, lv, pending = u.fwd_train_on_load(x, B, lv, self.tape, pending, defer, pool=pool)
                if i != n - 1:
                    self.tape.append(Marker("pooled", i))
                feats.append((x, lv))
                continue
            for u in units:
                x, lv = u.fwd_train(x, B, lv, self.tape) if self.training else u.fwd_eval(x, B, lv)
            if i != n - 1:
                (h, w) = lv[0]
                y = self.buf("pool%d" % i, (B * (h // 2) * (w // 2), x.shape[1]))
                ops.maxpool2_fwd(x, y, B, h, w)
                if self.training:
                    self.tape.append(PoolRec(i, x, B, h, w))
                x, lv = y, [(h // 2, w // 2)]
            feats.append((x, lv))
        # darknet.py:125-135: out4 = stage5(stage4(out3))
        return [feats[0], feats[1], feats[2], feats[4]]

    def scratch_region(self):
        """The part of the statistics arena a step has to zero (None until a first forward has sized it)."""
        if self.scratch_buf is None or self._scratch_size == 0:
            return None
        return self.scratch_buf[:max(self._scratch_size, 8)]

    def forward(self, images, scratch_zeroed=False):
        """images (B,3,H,W) fp32 NCHW on device -> packed logits cls (rows,16) fp32, reg (rows,240) fp32.
        scratch_zeroed: the caller's step prologue (ops.zero_many) already cleared scratch_region()."""
        B, _, H, W = images.shape
        self.prepare_weights(need_dgrad=self.training)
        self.tape = []
        if self.scratch_buf is not None and not scratch_zeroed:
            # one memset per step: every atomically accumulated statistic lives here (only the part in use)
            self.scratch_buf[:max(self._scratch_size, 8)].zero_()
        if self.nhwc_in is not None:        # GraphedKDStep: the frozen teacher converted this batch one replay earlier
            x = self.nhwc_in
            assert x.shape == (B * H * W, 8) and x.dtype == self.dtype
        else:
            out = self.nhwc_out if self.nhwc_out is not None else self.buf("input", (B * H * W, 8))
            assert out.shape == (B * H * W, 8) and out.dtype == self.dtype
            x = ops.image_to_nhwc(images.contiguous(), self.dtype, 8, out=out)
        feats = self._backbone53(x, B, [(H, W)]) if self.arch == "darknet53" else self._backbone_tiny(x, B, [(H, W)])
        ops.mark("%s.fwd.backbone.end" % ("teacher" if not self.training else "student"))
        oc = self.out_channel
        idxs = sorted(self.inner.keys())
        top = idxs[-1]
        levels = [feats[i][1][0] for i in idxs]
        h6 = ((levels[-1][0] + 1) // 2, (levels[-1][1] + 1) // 2)
        h7 = ((h6[0] + 1) // 2, (h6[1] + 1) // 2)
        levels_all = levels + [h6, h7]
        row0, r = [], 0
        for (h, w) in levels_all:
            row0.append(r)
            r += B * h * w
        head_in = self.buf("head_in", (r, oc))
        self.levels, self.rows, self.level_row0, self.batch = levels_all, r, row0, B
        self.in_hw = (H, W)

        def slot(li):
            h, w = levels_all[li]
            return head_in[row0[li]:row0[li] + B * h * w]

        inner_prev = None
        self.fpn_ctx = {}
        for pos in range(len(idxs) - 1, -1, -1):
            i = idxs[pos]
            f, lv = feats[i]
            h, w = lv[0]
            if inner_prev is None:
                inner, _ = self.inner[i].fwd(f, B, lv, out=self.buf("inner%d" % i, (B * h * w, oc)))
            else:
                lat, _ = self.inner[i].fwd(f, B, lv, out=self.buf("lat%d" % i, (B * h * w, oc)))
                inner = ops.upsample2_add(lat, inner_prev, self.buf("inner%d" % i, (B * h * w, oc)), B, h, w)
            self.outc[i].fwd(inner, B, lv, out=slot(pos))
            self.fpn_ctx[i] = (f, lv, inner)
            inner_prev = inner
            self._cut()
        ftop, lvtop = feats[top]
        p6, _ = self.p6.fwd(ftop, B, lvtop, out=slot(len(idxs)))
        p6r = ops.eltwise(ops.ELT_RELU, p6, None, self.buf("p6_relu", p6.shape))
        self.p7.fwd(p6r, B, [h6], out=slot(len(idxs) + 1))
        self.p6_ctx = (ftop, lvtop, p6, p6r, h6)
        ops.mark("%s.fwd.fpn.end" % ("teacher" if not self.training else "student"))
        # ---- head over all levels at once ----
        self.head_ctx = {}
        outs = {}
        towers = (("cls", self.cls_tower, self.cls_logits), ("pose", self.pose_tower, self.pose_pred))
        # A group of towers goes through a layer together.  Training with pair_towers: both -- the two convolutions of a
        # layer have identical geometry and go out as one launch (ops.conv_pair: 228 tiles of 192x128 instead of
        # 2 x 170 tiles of 128x128).  Otherwise (the frozen teacher among them) tower by tower.
        groups = [towers] if self.training and self.pair_towers else [towers[:1], towers[1:]]
        for group in groups:
            xs = {tname: head_in for tname, _, _ in group}
            saved = {tname: [] for tname, _, _ in group}
            for li in range(len(self.cls_tower)):
                raws = {}
                fuse = self.fuse_norm_on() and all(tower[li][0].norm_fusable(B, levels_all, ops.NORM_GROUP, tower[li][1].groups)
                                                   for _, tower, _ in group)
                with ops.conv_pair(enabled=len(group) == 2):
                    for tname, tower, _ in group:
                        conv, gn = tower[li]
                        # a fused eval-mode layer (the frozen teacher): the fp32 pre-normalisation tensor is not even stored
                        raws[tname] = self.buf("%s.raw%d" % (tname, li), (r, oc), torch.float32) \
                            if self.training or not fuse else None
                        if fuse:
                            gn.fwd_fused(conv, xs[tname], B, levels_all, self.buf("%s.act%d" % (tname, li), (r, oc)),
                                         raw_out=raws[tname])
                        else:
                            conv.fwd(xs[tname], B, levels_all, out_f32=True, out=raws[tname],
                                     stats=gn.stats(B, levels_all), stats_groups=gn.groups)
                for tname, tower, _ in group:
                    y = self.buf("%s.act%d" % (tname, li), (r, oc))
                    if not fuse:
                        tower[li][1].fwd(raws[tname], B, levels_all, out=y)
                    saved[tname].append((xs[tname], raws[tname]))
                    xs[tname] = y
                self._cut()
            for tname, _, final in group:
                seg = self.store.storage(self.scales) if tname == "pose" else None
                outs[tname], _ = final.fwd(xs[tname], B, levels_all, seg_scale=seg, out_f32=True,
                                           out=self.buf("%s.logits" % tname, (r, final.cout_p), torch.float32))
                self.head_ctx[tname] = (saved[tname], xs[tname])
        return outs["cls"], outs["pose"]

    # ---- backward (student only) -------------------------------------------------------------
    def backward(self, dcls, dreg):
        """dcls (rows,16), dreg (rows,240) in self.dtype: gradients w.r.t. the UNSCALED head outputs
        (the Scale module's factor is already folded into dreg by kd6d_loss_backward)."""
        assert self.training
        B, lv_all, r, oc = self.batch, self.levels, self.rows, self.out_channel
        self.wgrad.begin()
        d_head_in = self.buf("d_head_in", (r, oc))
        towers = (("cls", self.cls_tower, self.cls_logits, dcls), ("pose", self.pose_tower, self.pose_pred, dreg))
        hw = [h * w for (h, w) in lv_all]
        first = True            # layer 0: the towers add into d_head_in one after the other, the first not accumulating
        for group in ([towers] if self.pair_towers else [towers[:1], towers[1:]]):
            dxs = {}
            for tname, _, final, dlog in group:
                dxs[tname] = final.bwd(self.head_ctx[tname][1], dlog, B, lv_all, dx=self.buf("%s.dact" % tname, (r, oc)))
            for li in range(len(self.cls_tower) - 1, -1, -1):
                draws, items = {}, []
                for tname, tower, _, _ in group:
                    draws[tname] = self.buf("%s.draw%d" % (tname, li), (r, oc))
                    items.append((tower[li][1], self.head_ctx[tname][0][li][1], dxs[tname], B, lv_all, draws[tname]))
                if len(group) == 2:
                    # the two GroupNorm backwards of the layer as one launch (170 four-wave workgroups each: alone they
                    # are latency-bound and, back to back on one stream, the second waited for the first)
                    ops.gn_relu_bwd_pair([gn.bwd_item(*a) for gn, *a in items], hw, B, items[0][0].groups,
                                         self.store.acc_stride, flags=ops.GN_WS_ZEROED)
                else:
                    (gn, *a), = items
                    gn.bwd(*a)
                # the data gradients of a pair as one launch (never layer 0's: they add into the same tensor); the
                # weight gradients go where the WgradSchedule puts them as usual
                with ops.conv_pair(enabled=self.pair_towers == 1 and li > 0):
                    for tname, tower, _, _ in group:
                        x_in = self.head_ctx[tname][0][li][0]
                        if li > 0:
                            dxs[tname] = tower[li][0].bwd(x_in, draws[tname], B, lv_all,
                                                          dx=self.buf("%s.dact" % tname, (r, oc)))
                        else:
                            tower[0][0].bwd(x_in, draws[tname], B, lv_all, dx=d_head_in, accumulate=not first)
                            first = False
        row0 = self.level_row0
        ops.mark("student.bwd.head.end")

        def dslot(li):
            h, w = lv_all[li]
            return d_head_in[row0[li]:row0[li] + B * h * w]

        idxs = sorted(self.inner.keys())
        n_l = len(idxs)
        # d_head_in is complete: the FPN output convolutions' weight gradients (x = the top-down sums kept by the
        # forward, dy = the level slices of d_head_in) join the head's group, which then goes out as one launch pair
        # here or behind the FPN sweep (WgradSchedule.flush_group)
        grouped_out = set()
        for pos, i in enumerate(idxs):
            f, lv, inner = self.fpn_ctx[i]
            if self.wgrad.try_group(self.outc[i], self.outc[i].geom(B, lv), inner, dslot(pos)):
                grouped_out.add(i)
        self.wgrad.close_group_section()
        self.wgrad.flush_group("head_end")
        # P7 = conv(relu(P6)); P6 = conv(top feature)
        ftop, lvtop, p6, p6r, h6 = self.p6_ctx
        d_p6r = self.p7.bwd(p6r, dslot(n_l + 1), B, [h6], dx=self.buf("d_p6r", p6.shape))
        d_p6 = ops.eltwise(ops.ELT_RELU_BWD, p6, d_p6r, self.buf("d_p6a", p6.shape))
        d_p6 = ops.eltwise(ops.ELT_ADD, d_p6, dslot(n_l), self.buf("d_p6", p6.shape))
        dfeat = {}
        top = idxs[-1]
        dfeat[top] = self.p6.bwd(ftop, d_p6, B, lvtop, dx=self.buf("dfeat%d" % top, ftop.shape))
        d_inner_up = None
        for pos in range(n_l):
            i = idxs[pos]
            f, lv, inner = self.fpn_ctx[i]
            h, w = lv[0]
            d_inner = self.buf("d_inner%d" % i, inner.shape)
            if d_inner_up is not None:
                ops.sumpool2(d_inner_up[0], d_inner, B, d_inner_up[1], d_inner_up[2])
                self.outc[i].bwd(inner, dslot(pos), B, lv, dx=d_inner, accumulate=True, need_dw=i not in grouped_out)
            else:
                self.outc[i].bwd(inner, dslot(pos), B, lv, dx=d_inner, need_dw=i not in grouped_out)
            if i == top:
                self.inner[i].bwd(f, d_inner, B, lv, dx=dfeat[top], accumulate=True)
            else:
                dfeat[i] = self.inner[i].bwd(f, d_inner, B, lv, dx=self.buf("dfeat%d" % i, f.shape))
            d_inner_up = (d_inner, h, w)
        ops.mark("student.bwd.fpn.end")
        self.wgrad.flush_group("fpn_end")
        if self.grad_hook is not None:
            # every gradient outside the backbone has been issued (on this stream or on the weight-gradient streams):
            # a data-parallel caller starts their exchange here, beside the backbone sweep
            self.wgrad.flush_list()
            self.grad_hook()
        if self.arch == "darknet53":
            self._backbone53_bwd(dfeat)
        else:
            self._backbone_tiny_bwd(dfeat[top], dfeat.get(2))
        self.wgrad.finish()
        # every accumulated gradient (per-layer weight / bias gradients, GroupNorm gains and shifts, the head's scales)
        # -> fp32, accumulators cleared for the next step: one launch.  A caller that resolved the FPN + head part
        # early (grad_hook, the overlapped exchange) sets resolve_hi to where that part begins.
        self.store.resolve_grads(0, self.resolve_hi)
        return None

    def _backbone53_bwd(self, dfeat):
        """Reverse sweep of Darknet-53's backbone over the training tape.  dfeat: stage index (2, 3, 4) -> the FPN's
        gradient of that stage's output; the stage-3 / stage-4 ones are added by the data gradient of the next stage's
        down-sampling block (accumulate=True into the FPN's buffer)."""
        tape = self.tape
        grad = dfeat[len(self.stages) - 1]
        tail_at = self.wgrad.tail_start(tape)
        for i_rec in range(len(tape) - 1, -1, -1):
            rec = tape[i_rec]
            if i_rec == tail_at:
                self.wgrad.enter_tail()
            if isinstance(rec, Marker):
                continue
            if isinstance(rec, UnitRec):
                grad = self.unit_bwd(rec, grad)
                continue
            if i_rec == 0:                      # the init block: no gradient of the image
                rec.block.bwd(rec, grad, need_dx=False)
                continue
            prev = tape[i_rec - 1]
            if isinstance(prev, Marker) and prev.stage in dfeat:
                # the first block of the stage after a feature the FPN reads: its data gradient adds into the FPN's
                grad = rec.block.bwd(rec, grad, dx=dfeat[prev.stage], accumulate=True)
            else:
                grad = rec.block.bwd(rec, grad, dx=self.buf(rec.block.name + ".dx", rec.x.shape))

    def _backbone_tiny_bwd(self, grad, dfeat2):
        """Reverse sweep of a darknet-tiny backbone over the training tape.  grad: the FPN's gradient of out4 (after
        stage 5); dfeat2: of out3 (the pooled output of stage 3), added when the sweep reaches it."""
        tape = self.tape
        tail_at = self.wgrad.tail_start(tape)
        for i_rec in range(len(tape) - 1, -1, -1):
            rec = tape[i_rec]
            if i_rec == tail_at:
                self.wgrad.enter_tail()
            if isinstance(rec, BlockRec):
                need_dx = i_rec > 0
                grad = rec.block.bwd(rec, grad, need_dx=need_dx,
                                     dx=self.buf(rec.block.name + ".dx", rec.x.shape) if need_dx else None)
                continue
            if rec.stage == 2 and dfeat2 is not None:   # out3: behind the pool of stage 3, separate or inside its last block
                grad = ops.eltwise(ops.ELT_ADD, grad, dfeat2, self.buf("d_out3", grad.shape))
            if isinstance(rec, PoolRec):
                grad = ops.maxpool2_bwd(rec.x, grad, self.buf("dpool%d" % rec.stage, rec.x.shape), rec.batch, rec.h, rec.w)
