"""Thin Python wrappers over the C ABI: tensors in, tensors out, no arithmetic here.

All activations are "packed NHWC": a 2-D tensor (rows, C) whose rows are the pixels of
one or several pyramid levels laid out level-major, then image, then row-major (y, x).
"""
import ctypes

import torch

from . import _lib
from ._lib import ACT_LEAKY, ACT_NONE, ACT_RELU, GN_STATS_READY, GN_WS_ZEROED, ConvGeom, check, lib  # noqa: F401


def dt_code(dtype):
    if dtype == torch.bfloat16:
        return _lib.KD6D_BF16
    if dtype == torch.float32:
        return _lib.KD6D_F32
    raise TypeError("kd6d supports bfloat16 and float32 activations, got %s" % dtype)


def granule(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "kd6d ops need contiguous device tensors"
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- reproducible reductions (include/kd6d.h): statistics and workspaces are kd6d_acc, 16 bytes each ----------
ACC_FLOATS = 4                       # fp32 slots one accumulator takes in an fp32 arena
ACC_ACT, ACC_GRAD = _lib.ACC_ACT, _lib.ACC_GRAD


def acc_zeros(n, device):
    """n zeroed accumulators as an fp32 tensor (the engine keeps them inside its per-step zeroed fp32 arena)."""
    return torch.zeros(n * ACC_FLOATS, dtype=torch.float32, device=device)


def acc_read(acc, n, kind, out=None, accumulate=False, clear=False):
    """fp32 values of n interleaved accumulators (kd6d_acc_read): tests, debugging, stand-alone callers."""
    assert acc.is_contiguous() and acc.numel() * acc.element_size() >= n * 16
    if out is None:
        assert not accumulate
        out = torch.empty(n, dtype=torch.float32, device=acc.device)
    check(lib.kd6d_acc_read(_ptr(acc), n, kind, _ptr(out), int(accumulate), int(clear), _stream()), "kd6d_acc_read")
    return out


def planar_acc(n, device):
    """A stand-alone PLANAR gradient accumulator array for n elements: int64 (2 * n), lo plane then hi plane; pass
    acc[:n] with stride n to conv2d_wgrad / gn_relu_bwd / loss_backward."""
    return torch.zeros(2 * n, dtype=torch.int64, device=device)


def planar_acc_value(acc):
    """fp32 value of a stand-alone planar accumulator array made by planar_acc (torch arithmetic: test helper; the
    engine resolves its gradient bucket with kd6d_grad_acc_resolve)."""
    n = acc.numel() // 2
    lo, hi = acc[:n].double(), acc[n:].double()
    return (hi * 2.0 ** (47 - ACC_GRAD) + lo * 2.0 ** (-ACC_GRAD)).float()


# ---- optional per-launch timing (bench.py roofline leg): HIP events on the launch stream ----------
_prof = None


def profile_begin():
    global _prof
    _prof = []


def profile_end():
    """-> list of (kind, algorithmic_flops, milliseconds, tag) for every bracketed launch."""
    global _prof
    rec, _prof = _prof, None
    torch.cuda.synchronize()
    return [(k, f, e0.elapsed_time(e1), t) for (k, f, e0, e1, t) in rec]


_pair_deferred = None      # inside a conv_pair bracket while profiling: (kind, flops, tag) of the recorded launches


class _Timed:
    __slots__ = ("kind", "flops", "e0", "tag", "n0")

    def __init__(self, kind, flops, tag=None):
        self.kind, self.flops, self.e0, self.tag, self.n0 = kind, flops, None, tag, 0

    def __enter__(self):
        if _prof is not None:
            if _pair_deferred is not None:
                self.n0 = lib.kd6d_conv2d_pair_pending()
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if self.e0 is not None:
            if _pair_deferred is not None and lib.kd6d_conv2d_pair_pending() > self.n0:
                _pair_deferred.append((self.kind, self.flops, self.tag))     # launched (and timed) when the bracket closes
                return
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _prof.append((self.kind, self.flops, self.e0, e1, self.tag))


class Geom:
    """Forward-sense geometry of one conv layer over 1..5 pyramid levels."""

    def __init__(self, batch, cin, cout, ksize, stride, pad, levels):
        assert 1 <= len(levels) <= _lib.MAX_SEG
        self.batch, self.cin, self.cout = batch, cin, cout
        self.ksize, self.stride, self.pad = ksize, stride, pad
        self.levels_in = [tuple(l) for l in levels]
        self.levels_out = [((h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1)
                           for (h, w) in self.levels_in]
        g = ConvGeom()
        g.nseg, g.batch, g.cin, g.cout = len(levels), batch, cin, cout
        g.ksize, g.stride, g.pad = ksize, stride, pad
        rin = rout = 0
        for s, ((h, w), (ho, wo)) in enumerate(zip(self.levels_in, self.levels_out)):
            g.seg[s].in_h, g.seg[s].in_w, g.seg[s].out_h, g.seg[s].out_w = h, w, ho, wo
            g.seg[s].in_row0, g.seg[s].out_row0 = rin, rout
            rin += batch * h * w
            rout += batch * ho * wo
        self.rows_in, self.rows_out = rin, rout
        self.c = g

    @property
    def ref(self):
        return ctypes.byref(self.c)


def conv2d_fwd(geom, x, w, out=None, ch_scale=None, ch_shift=None, act=ACT_NONE, residual=None,
               seg_scale=None, out_f32=False, flops=0, stats=None, stats_groups=0, workspace=None):
    assert x.shape == (geom.rows_in, geom.cin), (x.shape, geom.rows_in, geom.cin)
    assert w.dtype == x.dtype and w.numel() == geom.cout * geom.ksize * geom.ksize * geom.cin
    odt = torch.float32 if out_f32 else x.dtype
    if out is None:
        out = torch.empty((geom.rows_out, geom.cout), dtype=odt, device=x.device)
    assert out.shape == (geom.rows_out, geom.cout) and out.dtype == odt
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == odt
    for v in (ch_scale, ch_shift):
        assert v is None or (v.dtype == torch.float32 and v.numel() >= geom.cout)
    assert seg_scale is None or (seg_scale.dtype == torch.float32 and seg_scale.numel() >= len(geom.levels_in))
    with _Timed("conv_fwd", flops, geom):
        check(lib.kd6d_conv2d_fwd(geom.ref, dt_code(x.dtype), _ptr(x), _ptr(w), _ptr(out), _ptr(ch_scale),
                                  _ptr(ch_shift), act, _ptr(residual), _ptr(seg_scale), int(out_f32),
                                  _ptr(stats), int(stats_groups), _ptr(workspace),
                                  0 if workspace is None else workspace.numel() * workspace.element_size(),
                                  _stream()), "kd6d_conv2d_fwd")
    return out


NORM_GROUP, NORM_BATCH = _lib.NORM_GROUP, _lib.NORM_BATCH


def conv_norm_fusable(geom, dtype, kind, groups=0):
    """kd6d_conv2d_fwd_norm_fusable: does this layer take the conv + normalisation + activation launch?"""
    return bool(lib.kd6d_conv2d_fwd_norm_fusable(geom.ref, dt_code(dtype), int(kind), int(groups)))


def conv_norm_counter_words(geom, kind):
    """32-bit words of the pre-zeroed barrier counters of conv2d_fwd_norm (kd6d.h)."""
    return BARRIER_WORDS if kind == NORM_BATCH else len(geom.levels_in) * geom.batch * _lib.NORM_MAX_CTILES


def conv_norm_stats_floats(geom, kind, groups=0):
    """fp32 slots of the fused launch's statistics accumulators."""
    if kind == NORM_BATCH:
        return _lib.BN_FUSED_REPLICAS * 2 * geom.cout * ACC_FLOATS
    return len(geom.levels_in) * geom.batch * groups * 2 * ACC_FLOATS


def conv2d_fwd_norm(geom, x, w, y, kind, gamma, beta, stats, counters, act, raw_out=None, bias=None, groups=0, eps=1e-5,
                    momentum=0.1, running_mean=None, running_var=None, save_mean=None, save_invstd=None, flops=0):
    """conv (+ bias) -> GroupNorm / train-mode BatchNorm -> activation as ONE launch (kd6d_conv2d_fwd_norm).
    y: (rows_out, cout) in x.dtype; raw_out: optional fp32 pre-normalisation tensor for the backward pass;
    stats / counters: pre-zeroed (conv_norm_stats_floats / conv_norm_counter_words)."""
    assert x.shape == (geom.rows_in, geom.cin) and w.dtype == x.dtype
    assert y.shape == (geom.rows_out, geom.cout) and y.dtype == x.dtype
    assert raw_out is None or (raw_out.shape == y.shape and raw_out.dtype == torch.float32)
    assert stats.dtype == torch.float32 and stats.numel() >= conv_norm_stats_floats(geom, kind, groups)   # accumulators
    assert counters.numel() >= conv_norm_counter_words(geom, kind) and counters.element_size() == 4
    n = _lib.ConvNorm()
    n.kind, n.groups, n.act, n.eps, n.momentum = int(kind), int(groups), int(act), float(eps), float(momentum)
    for name, t in (("gamma", gamma), ("beta", beta), ("y", y), ("stats", stats), ("counters", counters),
                    ("running_mean", running_mean), ("running_var", running_var), ("save_mean", save_mean),
                    ("save_invstd", save_invstd)):
        assert t is None or (t.is_cuda and t.is_contiguous())
        setattr(n, name, t.data_ptr() if t is not None else None)
    with _Timed("conv_fwd", flops, geom):
        check(lib.kd6d_conv2d_fwd_norm(geom.ref, dt_code(x.dtype), _ptr(x), _ptr(w), _ptr(raw_out), _ptr(bias),
                                       ctypes.byref(n), _stream()), "kd6d_conv2d_fwd_norm")
    return y


BN_REPLICAS = _lib.BN_FUSED_REPLICAS


def conv2d_fwd_block(geom, x, w, y_raw, stats=None, stats_replicas=1, bn_in=None, z_out=None, flops=0):
    """kd6d_conv2d_fwd_block: the convolution of a train-mode ConvBlock -> fp32 y_raw + its batch sums (stats:
    stats_replicas rows of {sum, sumsq}, pre-zeroed).  bn_in: dict(sums, replicas, gamma, beta, act, eps, momentum,
    running_mean, running_var, save_mean, save_invstd) -- then x is the PREVIOUS block's fp32 conv output, normalised and
    activated while loaded, and z_out receives that activation (what this layer's weight gradient reads)."""
    assert y_raw.shape == (geom.rows_out, geom.cout) and y_raw.dtype == torch.float32
    assert stats is None or (stats.dtype == torch.float32 and stats.numel() >= stats_replicas * 2 * geom.cout * ACC_FLOATS)
    bn = None
    if bn_in is not None:
        assert x.shape == (geom.rows_in, geom.cin) and x.dtype == torch.float32
        assert z_out is None or (z_out.shape == x.shape and z_out.dtype == w.dtype)
        bn = _lib.BnIn()
        bn.replicas, bn.act = int(bn_in["replicas"]), int(bn_in["act"])
        bn.eps, bn.momentum = float(bn_in.get("eps", 1e-5)), float(bn_in.get("momentum", 0.1))
        assert bn_in["sums"].numel() >= bn.replicas * 2 * geom.cin * ACC_FLOATS
        for name in ("sums", "gamma", "beta", "running_mean", "running_var", "save_mean", "save_invstd"):
            t = bn_in.get(name)
            assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32)
            setattr(bn, name, t.data_ptr() if t is not None else None)
    else:
        assert x.shape == (geom.rows_in, geom.cin) and x.dtype == w.dtype and z_out is None
    with _Timed("conv_fwd", flops, geom):
        check(lib.kd6d_conv2d_fwd_block(geom.ref, dt_code(w.dtype), _ptr(x), ctypes.byref(bn) if bn is not None else None,
                                        _ptr(z_out), _ptr(w), _ptr(y_raw), _ptr(stats), int(stats_replicas), _stream()),
              "kd6d_conv2d_fwd_block")
    return y_raw


def conv2d_dgrad(geom, dy, wt, dx=None, accumulate=False, flops=0):
    assert dy.shape == (geom.rows_out, geom.cout), (dy.shape, geom.rows_out, geom.cout)
    assert wt.dtype == dy.dtype and wt.numel() == geom.cout * geom.ksize * geom.ksize * geom.cin
    if dx is None:
        assert not accumulate
        dx = torch.empty((geom.rows_in, geom.cin), dtype=dy.dtype, device=dy.device)
    assert dx.shape == (geom.rows_in, geom.cin) and dx.dtype == dy.dtype
    with _Timed("conv_dgrad", flops, geom):
        check(lib.kd6d_conv2d_dgrad(geom.ref, dt_code(dy.dtype), _ptr(dy), _ptr(wt), _ptr(dx),
                                    int(accumulate), _stream()), "kd6d_conv2d_dgrad")
    return dx


def conv2d_wgrad_parts(geom, dtype, with_bias=False, cu_budget=0):
    """Number of partial dW images kd6d_conv2d_wgrad writes for this geometry / budget (kd6d_conv2d_wgrad_parts)."""
    n = int(lib.kd6d_conv2d_wgrad_parts(geom.ref, dt_code(dtype), int(with_bias), int(cu_budget)))
    if n < 1:
        check(n, "kd6d_conv2d_wgrad_parts")
    return n


def conv2d_wgrad(geom, x, dy, dw_slab, flops=0, dbias=None, acc_stride=0, cu_budget=0):
    """dw_slab: fp32 (parts, cout*k*k*cin) -- every pixel split stores its partial dW image (conv2d_wgrad_parts of them);
    the caller adds them in order (ParamStore.resolve_grads / kd6d_grad_acc_resolve).  dbias: lo-plane view of PLANAR
    gradient accumulators (int64; the hi word of element i sits acc_stride words behind its lo word)."""
    assert x.shape == (geom.rows_in, geom.cin) and dy.shape == (geom.rows_out, geom.cout)
    assert x.dtype == dy.dtype and dw_slab.dtype == torch.float32 and dw_slab.is_contiguous()
    assert dw_slab.numel() % (geom.cout * geom.ksize * geom.ksize * geom.cin) == 0
    with _Timed("conv_wgrad", flops, geom):
        assert dbias is None or (dbias.dtype == torch.int64 and dbias.numel() >= geom.cout and acc_stride > 0)
        check(lib.kd6d_conv2d_wgrad(geom.ref, dt_code(x.dtype), _ptr(x), _ptr(dy), _ptr(dw_slab), dw_slab.numel(),
                                    _ptr(dbias), int(acc_stride), int(cu_budget), _stream()), "kd6d_conv2d_wgrad")
    return dw_slab


def conv2d_wgrad_list(calls):
    """Several conv2d_wgrad calls behind one point of the current stream (kd6d_conv2d_wgrad_list): the bf16 calls of the
    transposing kernel family as list launches of up to four, side by side inside one kernel; every slab and bias
    accumulator gets the bits its own conv2d_wgrad call gives.  calls: dicts with conv2d_wgrad's arguments (geom, x, dy,
    dw_slab, flops, dbias, acc_stride, cu_budget).  While per-launch events are recorded (the instrumented eager steps)
    the calls go out one by one, so that every layer keeps its own entry."""
    if _prof is not None or len(calls) == 1:
        for c in calls:
            conv2d_wgrad(c["geom"], c["x"], c["dy"], c["dw_slab"], flops=c.get("flops", 0), dbias=c.get("dbias"),
                         acc_stride=c.get("acc_stride", 0), cu_budget=c.get("cu_budget", 0))
        return
    arr = (_lib.WgradCall * len(calls))()
    for a, c in zip(arr, calls):
        geom, x, dy, slab, dbias = c["geom"], c["x"], c["dy"], c["dw_slab"], c.get("dbias")
        acc_stride = c.get("acc_stride", 0)
        assert x.shape == (geom.rows_in, geom.cin) and dy.shape == (geom.rows_out, geom.cout)
        assert x.dtype == dy.dtype and slab.dtype == torch.float32 and slab.is_contiguous()
        assert slab.numel() % (geom.cout * geom.ksize * geom.ksize * geom.cin) == 0
        assert dbias is None or (dbias.dtype == torch.int64 and dbias.numel() >= geom.cout and acc_stride > 0)
        a.g, a.dtype = ctypes.pointer(geom.c), dt_code(x.dtype)
        a.x, a.dy, a.dw_slab, a.slab_floats = _ptr(x).value, _ptr(dy).value, _ptr(slab).value, slab.numel()
        a.dbias_acc = None if dbias is None else _ptr(dbias).value
        a.acc_hi_stride, a.cu_budget = int(acc_stride), int(c.get("cu_budget", 0))
    check(lib.kd6d_conv2d_wgrad_list(arr, len(calls), _stream()), "kd6d_conv2d_wgrad_list")


def conv2d_wgrad_f32(geom, x, dy, with_bias=False, cu_budget=0):
    """Stand-alone weight gradient -> fp32 tensors (dw, dbias | None): slab and bias accumulators made, filled and
    reduced here (torch arithmetic on the device: tests and tools; the engine resolves with kd6d_grad_acc_resolve).
    The parts are added one after the other, which is NOT the association of kd6d_grad_acc_resolve (include/kd6d.h:
    groups of four running sums): the same value up to the rounding of an fp32 sum, other bits from four parts on."""
    nw = geom.cout * geom.ksize * geom.ksize * geom.cin
    parts = conv2d_wgrad_parts(geom, x.dtype, with_bias, cu_budget)
    slab = torch.empty(parts, nw, dtype=torch.float32, device=x.device)
    acc = planar_acc(geom.cout, x.device) if with_bias else None
    conv2d_wgrad(geom, x, dy, slab, dbias=acc[:geom.cout] if with_bias else None, acc_stride=geom.cout,
                 cu_budget=cu_budget)
    dw = slab[0].clone()
    for k in range(1, parts):              # in part order (see the docstring)
        dw += slab[k]
    return dw, (planar_acc_value(acc) if with_bias else None)


def set_option(name, value):
    """kd6d_set_option (include/kd6d.h): pin a kernel family for the calls that follow; tests and benches only."""
    check(lib.kd6d_set_option(name.encode(), int(value)))


def get_option(name):
    v = ctypes.c_longlong(0)
    check(lib.kd6d_get_option(name.encode(), ctypes.byref(v)))
    return int(v.value)


class option:
    """`with ops.option("conv.smallc", 1): ...` -- the option is put back on exit."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def zero_many(tensors, counter=None):
    """kd6d_zero_regions: zero every tensor of `tensors` (contiguous device tensors, None entries skipped) and add 1
    to each element of the int64 tensor `counter`, as one launch on the current stream."""
    lst = _lib.ZeroList()
    n = 0
    for t in tensors:
        if t is None or t.numel() == 0:
            continue
        assert t.is_contiguous() and n < _lib.MAX_ZERO
        lst.ptr[n] = t.data_ptr()
        lst.bytes[n] = t.numel() * t.element_size()
        n += 1
    lst.n = n
    if counter is not None:
        assert counter.dtype == torch.int64 and counter.is_contiguous()
    check(lib.kd6d_zero_regions(ctypes.byref(lst), _ptr(counter) if counter is not None else None,
                                counter.numel() if counter is not None else 0, _stream()), "kd6d_zero_regions")


def uniform_keys(out, counter, seed):
    """kd6d_uniform_keys: out (fp32, device) <- uniform [0, 1) keys of (seed, counter[0], index)."""
    assert out.dtype == torch.float32 and counter.dtype == torch.int64
    check(lib.kd6d_uniform_keys(_ptr(out), out.numel(), _ptr(counter), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
          "kd6d_uniform_keys")
    return out


def device_cu_count():
    n = lib.kd6d_device_cu_count()
    if n <= 0:
        raise RuntimeError("kd6d_device_cu_count failed: %s" % lib.kd6d_last_error().decode())
    return n


_marks = None          # (int64 tensor, {name: slot}) while a timeline is being recorded (tools/step_timeline.py)


def mark(name):
    """Device timestamp into the slot registered for `name`; no-op unless marks_begin() was called."""
    if _marks is None:
        return
    buf, slots = _marks
    idx = slots.setdefault(name, len(slots))
    assert idx < buf.numel(), "too many marks"
    check(lib.kd6d_mark(ctypes.c_void_p(buf.data_ptr() + 8 * idx), _stream()), "kd6d_mark")


def marks_begin(device, n=64):
    global _marks
    _marks = (torch.zeros(n, dtype=torch.int64, device=device), {})
    return _marks


def marks_end():
    global _marks
    m, _marks = _marks, None
    return m


def pack_dgrad_weights(w_base, wt_base, desc_dev, n_layers, total_blocks):
    check(lib.kd6d_pack_dgrad_weights(dt_code(w_base.dtype), _ptr(w_base), _ptr(wt_base), _ptr(desc_dev),
                                      n_layers, total_blocks, _stream()), "kd6d_pack_dgrad_weights")


def colstats(x, sum_, sumsq=None):
    """sum_ / sumsq: C accumulators each (acc_zeros(C) or slices of the zeroed arena), class ACC_ACT."""
    rows, c = x.shape
    assert sum_.numel() >= c * ACC_FLOATS and (sumsq is None or sumsq.numel() >= c * ACC_FLOATS)
    check(lib.kd6d_colstats(dt_code(x.dtype), _ptr(x), rows, c, _ptr(sum_), _ptr(sumsq), _stream()),
          "kd6d_colstats")


def _xf32(x, act_dtype):
    """1 when the pre-normalisation tensor is fp32 but activations are bf16."""
    return int(x.dtype == torch.float32 and act_dtype == torch.bfloat16)


def bn_train_fwd(x, y, sum_, sumsq, gamma, beta, eps, momentum, running_mean, running_var,
                 save_mean, save_invstd, act):
    rows, c = x.shape
    check(lib.kd6d_bn_train_fwd(dt_code(y.dtype), _xf32(x, y.dtype), _ptr(x), _ptr(y), rows, c, _ptr(sum_), _ptr(sumsq),
                                _ptr(gamma), _ptr(beta), eps, momentum, _ptr(running_mean),
                                _ptr(running_var), _ptr(save_mean), _ptr(save_invstd), act, _stream()),
          "kd6d_bn_train_fwd")
    return y


def bn_train_fwd_res(x, residual, y, sum_, sumsq, gamma, beta, eps, momentum, running_mean, running_var,
                     save_mean, save_invstd, act):
    """bn_train_fwd with the DarkUnit's identity: y = act(bn(x)) + residual (residual: y's dtype and shape)."""
    rows, c = x.shape
    assert residual.shape == y.shape and residual.dtype == y.dtype
    check(lib.kd6d_bn_train_fwd_res(dt_code(y.dtype), _xf32(x, y.dtype), _ptr(x), _ptr(residual), _ptr(y), rows, c,
                                    _ptr(sum_), _ptr(sumsq), _ptr(gamma), _ptr(beta), eps, momentum,
                                    _ptr(running_mean), _ptr(running_var), _ptr(save_mean), _ptr(save_invstd), act,
                                    _stream()),
          "kd6d_bn_train_fwd_res")
    return y


BARRIER_WORDS = 32          # KD6D_BARRIER_WORDS: pre-zeroed 32-bit words of an in-kernel barrier (kd6d.h)


def bn_train_bwd(x, dz, dx, mean, invstd, gamma, beta, act, ws_sum_dy, ws_sum_dy_xhat, dgamma, dbeta, replicas=1,
                 counter=None):
    """ws_sum_dy / ws_sum_dy_xhat: `replicas` rows of C accumulators each, pre-zeroed (kd6d.h).  counter: BARRIER_WORDS
    pre-zeroed 32-bit words -> the one-launch backward (in-kernel barrier) when the tensor fits; None -> reduce + apply."""
    rows, c = x.shape
    assert ws_sum_dy.numel() >= replicas * c * ACC_FLOATS and ws_sum_dy_xhat.numel() >= replicas * c * ACC_FLOATS
    assert counter is None or counter.numel() >= BARRIER_WORDS
    check(lib.kd6d_bn_train_bwd(dt_code(dz.dtype), _xf32(x, dz.dtype), _ptr(x), _ptr(dz), _ptr(dx), rows, c, _ptr(mean),
                                _ptr(invstd), _ptr(gamma), _ptr(beta), act, _ptr(ws_sum_dy), _ptr(ws_sum_dy_xhat),
                                _ptr(counter), _ptr(dgamma), _ptr(dbeta), replicas, _stream()), "kd6d_bn_train_bwd")
    return dx


class conv_pair:
    """`with ops.conv_pair(): convA(...); convB(...)` -- two independent, identically shaped 3x3 convolutions
    (forward or data gradient) as one launch (kd6d_conv2d_pair_begin/_end in kd6d.h).  The two convolutions run
    when the block closes: nothing inside it may consume their results."""

    def __init__(self, enabled=True):
        self.enabled = enabled

    def __enter__(self):
        global _pair_deferred
        if self.enabled:
            check(lib.kd6d_conv2d_pair_begin(), "kd6d_conv2d_pair_begin")
            if _prof is not None:
                _pair_deferred = []
        return self

    def __exit__(self, *exc):
        global _pair_deferred
        if self.enabled:
            deferred, _pair_deferred = _pair_deferred, None
            if deferred:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            check(lib.kd6d_conv2d_pair_end(), "kd6d_conv2d_pair_end")
            if deferred:       # one launch: its duration against the work of both convolutions
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                _prof.append((deferred[0][0], sum(d[1] for d in deferred), e0, e1, deferred[0][2]))
        return False


def bn_pool_train_fwd(x, y, batch, h, w, sum_, sumsq, gamma, beta, eps, momentum, running_mean, running_var,
                      save_mean, save_invstd, act):
    """BN(train) + act + MaxPool2d(2,2): x (batch*h*w, C) conv output -> y (batch*h/2*w/2, C) pooled."""
    rows, c = x.shape
    assert rows == batch * h * w and tuple(y.shape) == (batch * (h // 2) * (w // 2), c)
    check(lib.kd6d_bn_pool_train_fwd(dt_code(y.dtype), _xf32(x, y.dtype), _ptr(x), _ptr(y), batch, h, w, c,
                                     _ptr(sum_), _ptr(sumsq), _ptr(gamma), _ptr(beta), eps, momentum,
                                     _ptr(running_mean), _ptr(running_var), _ptr(save_mean), _ptr(save_invstd), act,
                                     _stream()), "kd6d_bn_pool_train_fwd")
    return y


def bn_pool_train_bwd(x, dy, dx, batch, h, w, mean, invstd, gamma, beta, act, ws_sum_dy, ws_sum_dy_xhat, dgamma,
                      dbeta, replicas=1, counter=None):
    """dy: gradient of the POOLED output; dx: gradient of the conv output x (same rows as x, dtype of dy);
    counter as in bn_train_bwd."""
    rows, c = x.shape
    assert rows == batch * h * w and tuple(dy.shape) == (batch * (h // 2) * (w // 2), c) and dx.shape == x.shape
    assert ws_sum_dy.numel() >= replicas * c * ACC_FLOATS and ws_sum_dy_xhat.numel() >= replicas * c * ACC_FLOATS
    assert counter is None or counter.numel() >= BARRIER_WORDS
    check(lib.kd6d_bn_pool_train_bwd(dt_code(dy.dtype), _xf32(x, dy.dtype), _ptr(x), _ptr(dy), _ptr(dx), batch, h, w,
                                     c, _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), act, _ptr(ws_sum_dy),
                                     _ptr(ws_sum_dy_xhat), _ptr(counter), _ptr(dgamma), _ptr(dbeta), replicas,
                                     _stream()), "kd6d_bn_pool_train_bwd")
    return dx


def bn_pool_train_bwd_reduce(x, dy, batch, h, w, mean, invstd, gamma, beta, act, ws_sum_dy, ws_sum_dy_xhat, replicas=1):
    """The reduction pass of bn_pool_train_bwd alone: the two sums into `replicas` rows (bn_pool_bwd_wgrad finishes)."""
    rows, c = x.shape
    assert rows == batch * h * w and tuple(dy.shape) == (batch * (h // 2) * (w // 2), c)
    assert ws_sum_dy.numel() >= replicas * c * ACC_FLOATS and ws_sum_dy_xhat.numel() >= replicas * c * ACC_FLOATS
    check(lib.kd6d_bn_pool_train_bwd_reduce(dt_code(dy.dtype), _xf32(x, dy.dtype), _ptr(x), _ptr(dy), batch, h, w, c,
                                            _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(beta), act, _ptr(ws_sum_dy),
                                            _ptr(ws_sum_dy_xhat), replicas, _stream()), "kd6d_bn_pool_train_bwd_reduce")


def bn_pool_bwd_wgrad_parts(geom, dtype, cu_budget=0):
    """Partial dW images kd6d_bn_pool_bwd_wgrad writes for this geometry / budget; 0: the fused launch does not take it."""
    n = int(lib.kd6d_bn_pool_bwd_wgrad_parts(geom.ref, dt_code(dtype), int(cu_budget)))
    if n < 0:
        check(n, "kd6d_bn_pool_bwd_wgrad_parts")
    return n


def bn_pool_bwd_wgrad(geom, x, raw, dz, mean, invstd, gamma, beta, act, ws_sum_dy, ws_sum_dy_xhat, dgamma, dbeta, dw_slab,
                      replicas=1, flops=0, cu_budget=0):
    """Apply pass of the pooled BatchNorm backward + weight gradient of the convolution in front, one launch, for a block
    whose input needs no gradient.  x: the block's input (rows, cin); raw: fp32 conv output (rows, cout); dz: gradient of
    the pooled output; the sums as bn_pool_train_bwd_reduce left them; dw_slab: fp32 (bn_pool_bwd_wgrad_parts, cout*9*cin)."""
    assert geom.ksize == 3 and x.shape == (geom.rows_in, geom.cin) and raw.shape == (geom.rows_out, geom.cout)
    assert raw.dtype == torch.float32 and x.dtype == dz.dtype and dz.numel() * 4 == raw.numel()
    assert dw_slab.dtype == torch.float32 and dw_slab.is_contiguous()
    assert ws_sum_dy.numel() >= replicas * geom.cout * ACC_FLOATS and ws_sum_dy_xhat.numel() >= replicas * geom.cout * ACC_FLOATS
    with _Timed("conv_wgrad", flops, geom):
        check(lib.kd6d_bn_pool_bwd_wgrad(geom.ref, dt_code(x.dtype), _ptr(x), _ptr(raw), _ptr(dz), _ptr(mean), _ptr(invstd),
                                         _ptr(gamma), _ptr(beta), act, _ptr(ws_sum_dy), _ptr(ws_sum_dy_xhat), replicas,
                                         _ptr(dgamma), _ptr(dbeta), _ptr(dw_slab), dw_slab.numel(), int(cu_budget),
                                         _stream()), "kd6d_bn_pool_bwd_wgrad")
    return dw_slab


def _hw_array(level_hw):
    arr = (ctypes.c_int32 * len(level_hw))(*[int(v) for v in level_hw])
    return arr


def gn_relu_fwd(x, y, level_hw, batch, groups, gamma, beta, eps, stats, flags=0):
    rows, c = x.shape
    assert rows == batch * sum(level_hw)
    assert stats.numel() >= len(level_hw) * batch * groups * 2 * ACC_FLOATS
    check(lib.kd6d_gn_relu_fwd(dt_code(y.dtype), _xf32(x, y.dtype), _ptr(x), _ptr(y), _hw_array(level_hw), len(level_hw),
                               batch, c, groups, _ptr(gamma), _ptr(beta), eps, _ptr(stats), flags, _stream()),
          "kd6d_gn_relu_fwd")
    return y


def gn_bwd_workspace_floats(n_levels, batch, groups):
    """fp32 slots of kd6d_gn_relu_bwd's workspace: the group-sum accumulators plus one barrier counter per (level, image)
    (the launchers' copy of the layout: csrc/norm_plan.h, gn_bwd_workspace; tests/test_norm_plan_host.py ties the two)."""
    return 2 * n_levels * batch * groups * ACC_FLOATS + n_levels * batch


def gn_relu_bwd(x, dz, dx, level_hw, batch, groups, gamma, beta, stats, gsum_ws, dgamma, dbeta, acc_stride=0, eps=1e-5,
                flags=0):
    """dgamma / dbeta: lo-plane views of PLANAR gradient accumulators with stride acc_stride (ParamStore.acc /
    planar_acc), or None."""
    rows, c = x.shape
    assert rows == batch * sum(level_hw)
    assert gsum_ws.numel() >= gn_bwd_workspace_floats(len(level_hw), batch, groups), "gsum_ws too small (kd6d.h)"
    assert all(t is None or t.dtype == torch.int64 for t in (dgamma, dbeta))
    check(lib.kd6d_gn_relu_bwd(dt_code(dz.dtype), _xf32(x, dz.dtype), _ptr(x), _ptr(dz), _ptr(dx), _hw_array(level_hw),
                               len(level_hw), batch, c, groups, _ptr(gamma), _ptr(beta), eps, _ptr(stats),
                               _ptr(gsum_ws), _ptr(dgamma), _ptr(dbeta), int(acc_stride), flags, _stream()),
          "kd6d_gn_relu_bwd")
    return dx


def gn_relu_bwd_pair(items, level_hw, batch, groups, acc_stride, eps=1e-5, flags=0):
    """Two gn_relu_bwd of identical geometry as one launch (kd6d_gn_relu_bwd_pair).  items: two tuples
    (x, dz, dx, gamma, beta, stats, gsum_ws, dgamma, dbeta); dgamma / dbeta as in gn_relu_bwd."""
    assert len(items) == 2
    packed = []
    for (x, dz, dx, gamma, beta, stats, gsum_ws, dgamma, dbeta) in items:
        rows, c = x.shape
        assert rows == batch * sum(level_hw) and x.shape == items[0][0].shape and dz.dtype == items[0][1].dtype
        assert gsum_ws.numel() >= gn_bwd_workspace_floats(len(level_hw), batch, groups), "gsum_ws too small (kd6d.h)"
        it = _lib.GnItem()
        for name, t in zip(("x", "dz", "dx", "gamma", "beta", "stats", "gsum_ws", "dgamma", "dbeta"),
                           (x, dz, dx, gamma, beta, stats, gsum_ws, dgamma, dbeta)):
            assert t is None or (t.is_cuda and t.is_contiguous())
            setattr(it, name, t.data_ptr() if t is not None else None)
        packed.append(it)
    x0, dz0 = items[0][0], items[0][1]
    check(lib.kd6d_gn_relu_bwd_pair(dt_code(dz0.dtype), _xf32(x0, dz0.dtype), ctypes.byref(packed[0]),
                                    ctypes.byref(packed[1]), _hw_array(level_hw), len(level_hw), batch, x0.shape[1],
                                    groups, eps, int(acc_stride), flags, _stream()), "kd6d_gn_relu_bwd_pair")


def maxpool2_fwd(x, y, b, h, w):
    c = x.shape[-1]
    check(lib.kd6d_maxpool2_fwd(dt_code(x.dtype), _ptr(x), _ptr(y), b, h, w, c, _stream()),
          "kd6d_maxpool2_fwd")
    return y


def maxpool2_bwd(x, dy, dx, b, h, w, accumulate=False):
    c = x.shape[-1]
    check(lib.kd6d_maxpool2_bwd(dt_code(x.dtype), _ptr(x), _ptr(dy), _ptr(dx), b, h, w, c,
                                int(accumulate), _stream()), "kd6d_maxpool2_bwd")
    return dx


def upsample2_add(fine, coarse, out, b, h, w):
    c = fine.shape[-1]
    check(lib.kd6d_upsample2_add(dt_code(fine.dtype), _ptr(fine), _ptr(coarse), _ptr(out), b, h, w, c,
                                 _stream()), "kd6d_upsample2_add")
    return out


def sumpool2(dfine, dcoarse, b, h, w, accumulate=False):
    c = dfine.shape[-1]
    check(lib.kd6d_sumpool2(dt_code(dfine.dtype), _ptr(dfine), _ptr(dcoarse), b, h, w, c,
                            int(accumulate), _stream()), "kd6d_sumpool2")
    return dcoarse


ELT_RELU, ELT_RELU_BWD, ELT_ADD = 0, 1, 2


def eltwise(mode, x, dy, y):
    check(lib.kd6d_eltwise(dt_code(x.dtype), mode, _ptr(x), _ptr(dy), _ptr(y), x.numel(), _stream()),
          "kd6d_eltwise")
    return y


def image_to_nhwc(img, dtype, cpad=8, out=None):
    b, c, h, w = img.shape
    assert img.dtype == torch.float32
    if out is None:
        out = torch.empty((b * h * w, cpad), dtype=dtype, device=img.device)
    check(lib.kd6d_image_to_nhwc(dt_code(dtype), _ptr(img), _ptr(out), b, c, h, w, cpad, _stream()),
          "kd6d_image_to_nhwc")
    return out


def _small_set_div(launch, name, xs, alpha, s_start, s_cnt, yt, beta, t_start, t_cnt, n_images, loss_kp, out):
    """One small-set launch (include/kd6d.h, "the small-set launch contract"): xs (P,8,2), alpha (P,8), yt (M,8,2),
    beta (M,8); problem b owns student rows [s_start[b], s_start[b]+s_cnt[b]) and teacher rows likewise (int32 device
    arrays).  -> loss_img (B), valid_img (B) int32, grad_xs (P,8,2), grad_alpha (P,8); loss_kp: optional (B,8) fp32 output
    of the eight per-keypoint values.  out: these four as the caller's buffers, used as they are (the kernel does not
    write the gradient rows of skipped problems: the caller has zeroed them); otherwise allocated here, gradients zeroed.
    launch(inputs, outputs) makes the C call with the entry point's own arguments between the two groups."""
    if out is None:
        dev = xs.device
        out = (torch.empty(n_images, dtype=torch.float32, device=dev), torch.empty(n_images, dtype=torch.int32, device=dev),
               torch.zeros_like(xs), torch.zeros_like(alpha))
    loss, valid, gx, ga = out
    check(launch((_ptr(xs), _ptr(alpha), _ptr(s_start), _ptr(s_cnt), _ptr(yt), _ptr(beta), _ptr(t_start), _ptr(t_cnt),
                  n_images), (_ptr(loss), _ptr(valid), _ptr(loss_kp), _ptr(gx), _ptr(ga), _stream())), name)
    return out


def sinkhorn_div(xs, alpha, s_start, s_cnt, yt, beta, t_start, t_cnt, n_images, p, blur, scaling, reach, loss_kp=None,
                 out=None):
    """Debiased Sinkhorn divergence per problem (csrc/sinkhorn.hip); arguments and results: _small_set_div."""
    reach = -1.0 if reach is None else reach
    return _small_set_div(lambda ins, outs: lib.kd6d_sinkhorn_div_fwd_bwd(*ins, p, blur, scaling, reach, *outs),
                          "kd6d_sinkhorn_div_fwd_bwd", xs, alpha, s_start, s_cnt, yt, beta, t_start, t_cnt, n_images,
                          loss_kp, out)


def kernel_kind(kind):
    """'gaussian' | 'laplacian' | 'energy' (or the KD6D_KERNEL_* code itself) -> the code."""
    from ._lib import KERNEL_KINDS
    if isinstance(kind, str):
        if kind not in KERNEL_KINDS:
            raise ValueError("kernel loss %r: expected one of %s" % (kind, sorted(KERNEL_KINDS)))
        return KERNEL_KINDS[kind]
    return int(kind)


def kernel_div(kind, xs, alpha, s_start, s_cnt, yt, beta, t_start, t_cnt, n_images, blur, loss_kp=None, out=None):
    """Kernel distance (gaussian / laplacian / energy MMD, csrc/kernel_loss.hip) per problem; arguments and results:
    _small_set_div."""
    code = kernel_kind(kind)
    return _small_set_div(lambda ins, outs: lib.kd6d_kernel_div_fwd_bwd(code, *ins, blur, *outs),
                          "kd6d_kernel_div_fwd_bwd", xs, alpha, s_start, s_cnt, yt, beta, t_start, t_cnt, n_images,
                          loss_kp, out)


def kernel_dense(kind, x, alpha, y, beta, blur=0.05):
    """Kernel distance between two weighted point sets of any size: x (N,D), alpha (N), y (M,D), beta (M), D in
    {2,4,8,16} (kd6d_kernel_dense_fwd_bwd).  Returns loss (1,), dL/dx (N,D), dL/dalpha (N)."""
    N, D = x.shape
    M = y.shape[0]
    dev = x.device
    assert x.dtype == torch.float32 and y.shape == (M, D) and alpha.shape == (N,) and beta.shape == (M,)
    nws = int(lib.kd6d_kernel_dense_workspace_floats(N, M, D))
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    gx = torch.empty_like(x)
    ga = torch.empty_like(alpha)
    check(lib.kd6d_kernel_dense_fwd_bwd(kernel_kind(kind), _ptr(x), _ptr(alpha), _ptr(y), _ptr(beta), N, M, D, blur,
                                        _ptr(ws), nws, _ptr(loss), _ptr(gx), _ptr(ga), _stream()),
          "kd6d_kernel_dense_fwd_bwd")
    return loss, gx, ga


def pnp_workspace(n_problems, iters, device):
    """Scratch of kd6d_pnp_ransac / kd6d_teacher_pnp_gate (any contents): keep one per shape across calls."""
    return torch.empty(max(int(lib.kd6d_pnp_workspace_floats(n_problems, iters)), 1), dtype=torch.float32, device=device)


def pnp_ransac(kp, cnt, box, K, reproj_err=5.0, iters=300, seed=0, workspace=None):
    """Batched PnP-RANSAC (csrc/pnp.hip).  kp (P*cap, 8, 2) px, cnt (P,) int32 cells per problem, box (P, 8, 3),
    K (P, 3, 3).  -> ok (P,) int32, R (P, 3, 3), T (P, 3), n_inliers (P,) int32 (device tensors, no synchronisation)."""
    P = cnt.numel()
    cap = kp.shape[0] // max(P, 1)
    dev = kp.device
    if workspace is None:
        workspace = pnp_workspace(P, iters, dev)
    ok = torch.empty(P, dtype=torch.int32, device=dev)
    n_inl = torch.empty(P, dtype=torch.int32, device=dev)
    R = torch.empty(P, 3, 3, dtype=torch.float32, device=dev)
    T = torch.empty(P, 3, dtype=torch.float32, device=dev)
    check(lib.kd6d_pnp_ransac(P, cap, _ptr(cnt), _ptr(kp), _ptr(box), _ptr(K), float(reproj_err), int(iters), int(seed),
                              _ptr(ok), _ptr(R), _ptr(T), _ptr(n_inl), _ptr(workspace), workspace.numel(), _stream()),
          "kd6d_pnp_ransac")
    return ok, R, T, n_inl


def teacher_pnp_gate(cls, n_cls, threshold, t_row, t_cnt, t_kp, cap, kp3d, K, reproj_err=5.0, iters=300, seed=0,
                     workspace=None):
    """In place on t_cnt (kd6d_teacher_select's slot arrays): images whose pose cannot be solved lose their cells.
    kp3d (B, n_class_rows, 8, 3), K (B, 3, 3); no synchronisation (capturable)."""
    B = t_cnt.numel()
    if workspace is None:
        workspace = pnp_workspace(B, iters, t_cnt.device)
    check(lib.kd6d_teacher_pnp_gate(_ptr(cls), int(n_cls), float(threshold), _ptr(t_row), _ptr(t_cnt), _ptr(t_kp), cap,
                                    B, _ptr(kp3d), int(kp3d.shape[1]), _ptr(K), float(reproj_err), int(iters),
                                    int(seed), _ptr(workspace), workspace.numel(), _stream()),
          "kd6d_teacher_pnp_gate")


def pose_remap(inst_img, inst_cls, src_K, src_R, src_T, box, dst_K, M_resize, M_ssr=None, pose_out=None, ok_out=None):
    """The two pose remaps of the augmentation chain for every instance of a batch in one launch (csrc/pnp.hip,
    kd6d/libs/pnp.py::remap_pose chained as augment.draw_params chains it).  inst_img, inst_cls (n,) int32; src_K
    (n_images, 3, 3), src_R (n, 3, 3), src_T (n, 3) float64; box (n_class, 8, 3) float32; M_resize, M_ssr (n_images, 2, 3)
    float64 (M_ssr None: no second stage) -- device tensors; dst_K: 9 numbers on the host.
    -> pose (n, 2, 12) fp32 = per stage {R 9, T 3}, ok (n, 2) int32 (device tensors, no synchronisation)."""
    n = inst_img.numel()
    dev = box.device
    assert inst_img.dtype == torch.int32 and inst_cls.dtype == torch.int32 and inst_cls.numel() == n
    assert box.dtype == torch.float32 and box.dim() == 3 and tuple(box.shape[1:]) == (8, 3)
    n_images, n_class = src_K.numel() // 9, box.shape[0]
    for t, m in ((src_K, n_images * 9), (src_R, n * 9), (src_T, n * 3), (M_resize, n_images * 6), (M_ssr, n_images * 6)):
        assert t is None or (t.dtype == torch.float64 and t.numel() == m), "pose_remap: float64 (%d) expected" % m
    pose = torch.empty(n, 2, 12, dtype=torch.float32, device=dev) if pose_out is None else pose_out
    ok = torch.empty(n, 2, dtype=torch.int32, device=dev) if ok_out is None else ok_out
    assert pose.dtype == torch.float32 and pose.numel() >= n * 24 and ok.dtype == torch.int32 and ok.numel() >= n * 2
    if n == 0:
        return pose, ok
    kd = (ctypes.c_double * 9)(*[float(v) for v in (dst_K.reshape(-1).tolist() if hasattr(dst_K, "reshape") else dst_K)])
    check(lib.kd6d_pose_remap(n, n_images, n_class, _ptr(inst_img), _ptr(inst_cls), _ptr(src_K), _ptr(src_R), _ptr(src_T),
                              _ptr(box), kd, _ptr(M_resize), _ptr(M_ssr), _ptr(pose), _ptr(ok), _stream()),
          "kd6d_pose_remap")
    return pose, ok


def pose_errors(verts, voff, vcnt, vidx, K, Rg, Tg, Rp, Tp, sym, max_v=None, want_nn=False, validate=True):
    """Mean 3D / 2D-reprojection error of P (ground truth, prediction) pairs in one launch (csrc/pose_err.hip,
    evaluate.py::compute_pose_diff).  verts (Nv, 3) fp32 pool; voff, vcnt, sym (P,) int32; vidx (P, max_v) int32 relative
    to voff, or None (vertices 0 ... vcnt-1; max_v then has to be given); K, Rg, Rp (P, 3, 3), Tg, Tp (P, 3) fp32.
    -> err (P, 2) [, nn (P, max_v) int32] (device tensors, no synchronisation).
    validate: check on the device that every index stays inside the pool and read the verdict back (ONE
    synchronisation; the kernel itself cannot know the pool's size).  Callers that built the index arrays themselves and
    replay the launch in a captured graph pass False."""
    P = voff.numel()
    dev = verts.device
    if vidx is not None:
        assert vidx.dtype == torch.int32 and vidx.dim() == 2 and vidx.shape[0] == P
        max_v = vidx.shape[1] if max_v is None else max_v
        assert vidx.shape[1] == max_v
    assert max_v is not None, "pose_errors: max_v is needed without an index table"
    assert verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3
    for t in (voff, vcnt, sym):
        assert t.dtype == torch.int32 and t.numel() == P
    for t, n in ((K, 9), (Rg, 9), (Rp, 9), (Tg, 3), (Tp, 3)):
        assert t.dtype == torch.float32 and t.numel() == P * n
    if validate and P > 0:
        Nv = verts.shape[0]
        cnt = vcnt.long()
        bad = (voff < 0) | (cnt < 1) | (cnt > max_v)
        if vidx is None:
            bad = bad | (voff.long() + cnt > Nv)
        else:
            used = torch.arange(max_v, device=dev)[None, :] < cnt[:, None]
            at = voff.long()[:, None] + vidx.long()
            bad = bad | (used & ((vidx < 0) | (at >= Nv))).any(dim=1)
        if bool(bad.any()):
            raise ValueError("pose_errors: problem %d points outside the vertex pool of %d vertices (or its vcnt is "
                             "outside 1 ... %d)" % (int(torch.nonzero(bad)[0]), Nv, max_v))
    err = torch.empty(P, 2, dtype=torch.float32, device=dev)
    nn = torch.empty(P, max_v, dtype=torch.int32, device=dev) if want_nn else None
    if P == 0:
        return (err, nn) if want_nn else err
    check(lib.kd6d_pose_errors(P, int(max_v), _ptr(verts), _ptr(voff), _ptr(vcnt), _ptr(vidx), _ptr(K), _ptr(Rg),
                               _ptr(Tg), _ptr(Rp), _ptr(Tp), _ptr(sym), _ptr(err), _ptr(nn), _stream()),
          "kd6d_pose_errors")
    return (err, nn) if want_nn else err


def bop_errors(verts, voff, vcnt, syms, soff, scnt, K, Rg, Tg, Rp, Tp, validate=True, max_scnt=None):
    """MSSD / MSPD of P (ground truth, prediction) pairs in one call (csrc/bop_err.hip; the float64 definition is
    kd6d.libs.bop_metrics.bop_errors_host).  verts (Nv, 3) fp32 vertex pool; syms (Ns, 12) fp32 symmetry pool (R
    row-major, then t); voff, vcnt, soff, scnt (P,) int32: problem p scores every vertex voff[p] ... voff[p] + vcnt[p] - 1
    under the symmetries soff[p] ... soff[p] + scnt[p] - 1 (scnt[p] <= 0: the identity alone; vcnt[p] <= 0: err = 0);
    K, Rg, Rp (P, 3, 3), Tg, Tp (P, 3) fp32.  -> err (P, 2) = (mssd, mspd), a device tensor.
    validate: check on the device that every vertex and symmetry index stays inside its pool and read the verdict back
    (ONE synchronisation, which also yields the largest scnt; the kernel cannot know the pools' sizes).  Callers that
    built the index arrays themselves and replay the call in a captured graph pass False and max_scnt (the largest
    scnt[p], which sizes the workspace; without it it is read back from scnt)."""
    P = voff.numel()
    dev = verts.device
    assert verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3
    assert syms.dtype == torch.float32 and syms.numel() % 12 == 0
    for t in (voff, vcnt, soff, scnt):
        assert t.dtype == torch.int32 and t.numel() == P
    for t, n in ((K, 9), (Rg, 9), (Rp, 9), (Tg, 3), (Tp, 3)):
        assert t.dtype == torch.float32 and t.numel() == P * n
    err = torch.empty(P, 2, dtype=torch.float32, device=dev)
    if P == 0:
        return err
    if validate:
        Nv, Ns = verts.shape[0], syms.numel() // 12
        vc, sc = vcnt.long().clamp(min=0), scnt.long().clamp(min=0)
        bad_v = (vc > 0) & ((voff < 0) | (voff.long() + vc > Nv))
        bad_s = (sc > 0) & ((soff < 0) | (soff.long() + sc > Ns))
        verdict = torch.stack([bad_v.any().long(), bad_s.any().long(), sc.max()]).tolist()     # the one synchronisation
        if verdict[0]:
            raise ValueError("bop_errors: problem %d points outside the vertex pool of %d vertices"
                             % (int(torch.nonzero(bad_v)[0]), Nv))
        if verdict[1]:
            raise ValueError("bop_errors: problem %d points outside the symmetry pool of %d transforms"
                             % (int(torch.nonzero(bad_s)[0]), Ns))
        assert max_scnt is None or max_scnt >= verdict[2], "bop_errors: max_scnt=%d < largest scnt %d" % (max_scnt, verdict[2])
        max_scnt = verdict[2] if max_scnt is None else max_scnt
    elif max_scnt is None:
        max_scnt = int(scnt.max())
    if syms.numel() == 0:             # every problem is identity only: the pool is never read, but the ABI takes no NULL
        syms = torch.zeros(1, 12, dtype=torch.float32, device=dev)
    nws = int(lib.kd6d_bop_errors_workspace_floats(P, int(max_scnt)))
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    check(lib.kd6d_bop_errors(P, _ptr(verts), _ptr(voff), _ptr(vcnt), _ptr(syms), _ptr(soff), _ptr(scnt), _ptr(K),
                              _ptr(Rg), _ptr(Tg), _ptr(Rp), _ptr(Tp), _ptr(ws), nws, _ptr(err), _stream()),
          "kd6d_bop_errors")
    return err


VSD_MAX_TAU = 16                     # taus one kd6d_bop_vsd call takes


def _mesh_items_check(verts, faces, voff, vcnt, foff, fcnt):
    """The device-side index check of render_depth / bop_vsd -> (items that leave a pool, items with a face index
    outside [0, vcnt)) as bool tensors; no synchronisation here.  A face index is relative to its item's voff, so the
    bound depends on the item: the largest and smallest index of a face range come from a sparse table (range
    maximum in log2(Nf) levels), every item at once."""
    Nv, Nf = verts.shape[0], faces.shape[0]
    vc, fc = vcnt.long(), fcnt.long()
    bad = (voff < 0) | (vc < 1) | (voff.long() + vc > Nv) | (foff < 0) | (fc < 1) | (foff.long() + fc > Nf)
    if Nf == 0:
        return bad, torch.zeros_like(bad)
    hi = [faces.max(dim=1).values.long()]
    lo = [-faces.min(dim=1).values.long()]
    while 2 << (len(hi) - 1) <= Nf:
        h = 1 << (len(hi) - 1)
        hi.append(torch.maximum(hi[-1][:-h], hi[-1][h:]))
        lo.append(torch.maximum(lo[-1][:-h], lo[-1][h:]))
    start = torch.where(bad, torch.zeros_like(fc), foff.long())
    length = torch.where(bad, torch.ones_like(fc), fc)
    level = torch.floor(torch.log2(length.double())).long()
    level = torch.where((2 ** (level + 1)) <= length, level + 1, level)       # guard the rounding of log2
    level = torch.where((2 ** level) > length, level - 1, level)
    top, low = torch.zeros_like(fc), torch.zeros_like(fc)
    for k in range(len(hi)):
        at = level == k
        i0 = torch.where(at, start, torch.zeros_like(start)).clamp(max=hi[k].numel() - 1)
        i1 = torch.where(at, start + length - (1 << k), torch.zeros_like(start)).clamp(0, hi[k].numel() - 1)
        top = torch.where(at, torch.maximum(hi[k][i0], hi[k][i1]), top)
        low = torch.where(at, torch.maximum(lo[k][i0], lo[k][i1]), low)
    return bad, ~bad & ((top >= vc) | (low > 0))


def _mesh_items_assert(who, verts, faces, voff, vcnt, foff, fcnt, n):
    assert verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3
    assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
    for t in (voff, vcnt, foff, fcnt):
        assert t.dtype == torch.int32 and t.numel() == n, "%s: four int32 arrays of %d items" % (who, n)


def render_depth(verts, faces, voff, vcnt, foff, fcnt, K, R, T, height, width, validate=True):
    """Depth maps of n (mesh, pose, camera) triples in one call (csrc/bop_vsd.hip; the float64 definition and the
    rasteriser contract are kd6d.libs.bop_metrics.render_depth_host).  verts (Nv, 3) fp32 vertex pool, faces (Nf, 3)
    int32 face pool whose indices are relative to the item's voff; voff, vcnt, foff, fcnt (n,) int32; K, R (n, 3, 3),
    T (n, 3) fp32.  -> (n, height, width) fp32: the camera-frame z of the nearest surface, 0 = background.
    validate: check on the device that every offset, count and face index stays inside its pool and read the verdict
    back (ONE synchronisation); nothing is launched when it fails."""
    n = voff.numel()
    dev = verts.device
    _mesh_items_assert("render_depth", verts, faces, voff, vcnt, foff, fcnt, n)
    for t, k in ((K, 9), (R, 9), (T, 3)):
        assert t.dtype == torch.float32 and t.numel() == n * k
    out = torch.empty(n, int(height), int(width), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if validate:
        bad, bad_face = _mesh_items_check(verts, faces, voff, vcnt, foff, fcnt)
        verdict = torch.stack([bad.any(), bad_face.any()]).tolist()                    # the one synchronisation
        if verdict[0]:
            raise ValueError("render_depth: item %d points outside the pools of %d vertices and %d faces"
                             % (int(torch.nonzero(bad)[0]), verts.shape[0], faces.shape[0]))
        if verdict[1]:
            raise ValueError("render_depth: item %d has a face index outside its vcnt vertices"
                             % int(torch.nonzero(bad_face)[0]))
    nws = int(lib.kd6d_bop_vsd_workspace_ints(n))
    ws = torch.empty(nws, dtype=torch.int32, device=dev)
    check(lib.kd6d_render_depth(n, _ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], _ptr(voff), _ptr(vcnt),
                                _ptr(foff), _ptr(fcnt), _ptr(K), _ptr(R), _ptr(T), int(height), int(width), _ptr(ws),
                                nws, _ptr(out), _stream()), "kd6d_render_depth")
    return out


def bop_vsd(verts, faces, voff, vcnt, foff, fcnt, K, Rg, Tg, Rp, Tp, diameter, frame, depth, delta, taus,
            validate=True):
    """BOP's VSD of P (ground truth, estimate) pairs in one call (csrc/bop_vsd.hip; the float64 definition is
    kd6d.libs.bop_metrics.vsd_errors_host).  Pools and index arrays as render_depth; K, Rg, Rp (P, 3, 3), Tg, Tp
    (P, 3), diameter (P,) fp32; frame (P,) int32 = the problem's image in depth (n_img, H, W) fp32 (the vertices' unit,
    0 = missing); delta: the visibility tolerance; taus: up to 16 floats (a host sequence).
    -> counts (P, 2 + n_tau) int32 = (n_u, n_inter, cost_k ...), err (P, n_tau) fp32 = cost_k / n_u (1 when n_u == 0):
    device tensors.
    validate: check on the device that every offset, count, face index and frame index stays inside its pool and read
    the verdict back (ONE synchronisation); nothing is launched when it fails.  Callers that built the index arrays
    themselves and replay the call in a captured graph pass False."""
    P = voff.numel()
    dev = verts.device
    taus = [float(t) for t in taus]
    assert 1 <= len(taus) <= VSD_MAX_TAU, "bop_vsd: %d taus (1 ... %d)" % (len(taus), VSD_MAX_TAU)
    _mesh_items_assert("bop_vsd", verts, faces, voff, vcnt, foff, fcnt, P)
    for t, k in ((K, 9), (Rg, 9), (Rp, 9), (Tg, 3), (Tp, 3), (diameter, 1)):
        assert t.dtype == torch.float32 and t.numel() == P * k
    assert frame.dtype == torch.int32 and frame.numel() == P
    assert depth.dtype == torch.float32 and depth.dim() == 3
    n_img, H, W = depth.shape
    counts = torch.empty(P, 2 + len(taus), dtype=torch.int32, device=dev)
    err = torch.empty(P, len(taus), dtype=torch.float32, device=dev)
    if P == 0:
        return counts, err
    if validate:
        bad, bad_face = _mesh_items_check(verts, faces, voff, vcnt, foff, fcnt)
        bad_frame = (frame < 0) | (frame >= n_img)
        verdict = torch.stack([bad.any(), bad_face.any(), bad_frame.any()]).tolist()   # the one synchronisation
        if verdict[0]:
            raise ValueError("bop_vsd: problem %d points outside the pools of %d vertices and %d faces"
                             % (int(torch.nonzero(bad)[0]), verts.shape[0], faces.shape[0]))
        if verdict[1]:
            raise ValueError("bop_vsd: problem %d has a face index outside its vcnt vertices"
                             % int(torch.nonzero(bad_face)[0]))
        if verdict[2]:
            raise ValueError("bop_vsd: problem %d points outside the depth pool of %d images"
                             % (int(torch.nonzero(bad_frame)[0]), n_img))
    nws = int(lib.kd6d_bop_vsd_workspace_ints(P))
    ws = torch.empty(nws, dtype=torch.int32, device=dev)
    tau_c = (ctypes.c_float * len(taus))(*taus)
    check(lib.kd6d_bop_vsd(P, _ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], _ptr(voff), _ptr(vcnt),
                           _ptr(foff), _ptr(fcnt), _ptr(K), _ptr(Rg), _ptr(Tg), _ptr(Rp), _ptr(Tp), _ptr(diameter),
                           _ptr(frame), _ptr(depth), int(n_img), int(H), int(W), float(delta), tau_c, len(taus),
                           _ptr(ws), nws, _ptr(counts), _ptr(err), _stream()), "kd6d_bop_vsd")
    return counts, err


RENDER_MAX_SLOTS = 4                 # KD6D_MAX_GT: objects one rendered frame shows
RENDER_MAX_FACES = 1 << 28           # faces of one item (the owner id keeps 28 bits for the face)


def render_frames(verts, faces, vcol, voff, vcnt, foff, fcnt, item_frame, item_slot, R, T, K, light, ambient, bg_index,
                  backgrounds, height, width, want_depth=False, out=None, validate=True):
    """Shaded colour frames with their visible-instance masks in one call (csrc/render_frames.hip; the float64
    definition is kd6d.libs.render.render_frames_host).  verts (Nv, 3) fp32, faces (Nf, 3) int32 relative to the item's
    voff, vcol (Nv, 3) uint8 RGB; per item voff, vcnt, foff, fcnt, item_frame, item_slot (n_items,) int32, R
    (n_items, 3, 3), T (n_items, 3) fp32; per frame K (n, 3, 3), light (n, 3), ambient (n,) fp32, bg_index (n,) int32;
    backgrounds (n_bg, height, width, 3) uint8 (BGR, copied as they are).
    -> frames (n, height, width, 3) uint8 BGR, masks (n, height, width) uint8 (0 = background, slot + 1 = the object that
    owns the pixel), depth (n, height, width) fp32 or None (want_depth).  out: (frames, masks, depth or None) to write into.
    validate: check on the device that every offset, count, face index, frame, slot and background index stays in its
    range and that no two items claim one (frame, slot), and read the verdict back (ONE synchronisation); nothing is
    launched when it fails."""
    n = K.numel() // 9
    n_items = voff.numel()
    dev = K.device
    H, W = int(height), int(width)
    _mesh_items_assert("render_frames", verts, faces, voff, vcnt, foff, fcnt, n_items)
    assert vcol.dtype == torch.uint8 and vcol.shape == verts.shape, "render_frames: vcol is (Nv, 3) uint8"
    for t in (item_frame, item_slot):
        assert t.dtype == torch.int32 and t.numel() == n_items
    for t, k, m in ((R, 9, n_items), (T, 3, n_items), (K, 9, n), (light, 3, n), (ambient, 1, n)):
        assert t.dtype == torch.float32 and t.numel() == m * k and t.is_contiguous()
    assert bg_index.dtype == torch.int32 and bg_index.numel() == n
    assert backgrounds.dtype == torch.uint8 and backgrounds.dim() == 4 and tuple(backgrounds.shape[1:]) == (H, W, 3) and \
        backgrounds.is_contiguous(), "render_frames: backgrounds is (n_bg, %d, %d, 3) uint8" % (H, W)
    n_bg = backgrounds.shape[0]
    if out is None:
        out = (torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev), torch.empty(n, H, W, dtype=torch.uint8, device=dev),
               torch.empty(n, H, W, dtype=torch.float32, device=dev) if want_depth else None)
    frames, masks, depth = out
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (n, H, W, 3) and frames.is_contiguous()
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (n, H, W) and masks.is_contiguous()
    assert depth is None or (depth.dtype == torch.float32 and tuple(depth.shape) == (n, H, W) and depth.is_contiguous())
    if n == 0:
        return frames, masks, depth
    if validate:
        checks = [(bg_index < 0) | (bg_index >= n_bg)]
        if n_items:
            bad, bad_face = _mesh_items_check(verts, faces, voff, vcnt, foff, fcnt)
            bad_fs = (item_frame < 0) | (item_frame >= n) | (item_slot < 0) | (item_slot >= RENDER_MAX_SLOTS)
            key = (item_frame.long() * RENDER_MAX_SLOTS + item_slot.long()).clamp(0, n * RENDER_MAX_SLOTS - 1)
            twice = torch.zeros(n * RENDER_MAX_SLOTS, dtype=torch.int32, device=dev).index_add_(0, key, (~bad_fs).int()) > 1
            checks += [bad | (fcnt >= RENDER_MAX_FACES), bad_face, bad_fs, twice]
        verdict = torch.stack([c.any() for c in checks]).tolist()                      # the one synchronisation
        if verdict[0]:
            raise ValueError("render_frames: frame %d points outside the pool of %d backgrounds"
                             % (int(torch.nonzero(checks[0])[0]), n_bg))
        if n_items and verdict[1]:
            raise ValueError("render_frames: item %d points outside the pools of %d vertices and %d faces"
                             % (int(torch.nonzero(checks[1])[0]), verts.shape[0], faces.shape[0]))
        if n_items and verdict[2]:
            raise ValueError("render_frames: item %d has a face index outside its vcnt vertices"
                             % int(torch.nonzero(checks[2])[0]))
        if n_items and verdict[3]:
            raise ValueError("render_frames: item %d has a frame outside [0, %d) or a slot outside [0, %d)"
                             % (int(torch.nonzero(checks[3])[0]), n, RENDER_MAX_SLOTS))
        if n_items and verdict[4]:
            at = int(torch.nonzero(checks[4])[0])
            raise ValueError("render_frames: two items claim slot %d of frame %d" % (at % RENDER_MAX_SLOTS, at // RENDER_MAX_SLOTS))
    nws = int(lib.kd6d_render_frames_workspace_ints(n, n_items))
    ws = torch.empty(nws, dtype=torch.int32, device=dev)
    check(lib.kd6d_render_frames(n, n_items, _ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], _ptr(vcol),
                                 _ptr(voff), _ptr(vcnt), _ptr(foff), _ptr(fcnt), _ptr(item_frame), _ptr(item_slot),
                                 _ptr(R), _ptr(T), _ptr(K), _ptr(light), _ptr(ambient), _ptr(bg_index),
                                 _ptr(backgrounds), int(n_bg), H, W, _ptr(ws), nws, _ptr(frames), _ptr(masks),
                                 _ptr(depth) if depth is not None else None, _stream()), "kd6d_render_frames")
    return frames, masks, depth


def sinkhorn_dense(x, alpha, y, beta, blur=0.05, scaling=0.5, reach=0.5, diameter=None, p=2.0):
    """Debiased (unbalanced) Sinkhorn divergence between two LARGE weighted point sets: x (N,D), alpha (N),
    y (M,D), beta (M), D in {2,4,8,16} -- losses/kd_loss.py:26-30 / loss_libs.py:47 with a dense grid of local
    predictions (BASELINE config 5).  Returns loss (1,), dS/dx (N,D), dS/dalpha (N).
    diameter=None reproduces geomloss' default: it is measured on the device and read back (one sync, like
    the reference's `.item()`); pass a float (geomloss' diameter= argument) to stay asynchronous."""
    N, D = x.shape
    M = y.shape[0]
    dev = x.device
    assert x.dtype == torch.float32 and y.shape == (M, D) and alpha.shape == (N,) and beta.shape == (M,)
    nws = int(lib.kd6d_sinkhorn_dense_workspace_floats(N, M, D))
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    if diameter is None:
        d = torch.empty(1, dtype=torch.float32, device=dev)
        check(lib.kd6d_sinkhorn_dense_diameter(_ptr(x), _ptr(y), N, M, D, _ptr(ws), _ptr(d), _stream()),
              "kd6d_sinkhorn_dense_diameter")
        diameter = float(d.item())
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    gx = torch.empty_like(x)
    ga = torch.empty_like(alpha)
    check(lib.kd6d_sinkhorn_dense_fwd_bwd(_ptr(x), _ptr(alpha), _ptr(y), _ptr(beta), N, M, D, p, blur, scaling,
                                          reach if reach is not None else -1.0, float(max(diameter, 1e-12)), _ptr(ws), nws,
                                          _ptr(loss), _ptr(gx), _ptr(ga), _stream()), "kd6d_sinkhorn_dense_fwd_bwd")
    return loss, gx, ga


# ---- grouped weight gradient (csrc/conv_wgrad_group.hip) -----------------------------------------------------
def wgrad_group_supported(geom, dtype):
    return bool(lib.kd6d_wgrad_group_supported(geom.ref, dt_code(dtype)))


class WgradGroup:
    """The weight gradients of several layers as one launch pair.  add() collects (geometry, x, dy, dw, dbias);
    launch() plans the work list on first use (or when the tensors or their geometry changed), keeps the plan and the
    partial-tile slab on the device, and enqueues the two kernels on the current stream.  The collected tensors
    must stay alive and unchanged until the launch has run (the engine's per-layer buffers are static)."""

    def __init__(self, n_workgroups):
        self.n_workgroups = int(n_workgroups)
        self.items, self.flops = [], 0
        # one (plan, slab, info, tensors) per distinct set of tensors, kept for the life of the group: a captured
        # hipGraph replays the device pointers of the plan it was captured with, so a later eager launch with other
        # buffers (another batch size on the same network) must not free or overwrite it
        self._plans = {}

    def add(self, geom, x, dy, dw, dbias=None, flops=0):
        assert x.shape == (geom.rows_in, geom.cin) and dy.shape == (geom.rows_out, geom.cout)
        assert x.dtype == dy.dtype == torch.bfloat16 and dw.dtype == torch.float32
        assert dw.numel() == geom.cout * geom.ksize * geom.ksize * geom.cin
        assert dbias is None or (dbias.dtype == torch.float32 and dbias.numel() >= geom.cout)
        self.items.append((geom, x, dy, dw, dbias))
        self.flops += flops

    def __len__(self):
        return len(self.items)

    def _build(self, device):
        # the plan travels host -> device with a pageable copy and the slab is allocated: neither may happen inside a
        # stream capture (the engine's eager warm-up steps run the same launch first, so the capture finds the plan)
        assert not torch.cuda.is_current_stream_capturing(), \
            "WgradGroup: first launch of a new tensor set inside a graph capture (run one eager warm-up step first)"
        n = len(self.items)
        arr = (_lib.WgradItem * n)()
        for i, (g, x, dy, dw, db) in enumerate(self.items):
            ctypes.memmove(ctypes.byref(arr[i].geom), ctypes.byref(g.c), ctypes.sizeof(_lib.ConvGeom))
            arr[i].x, arr[i].dy, arr[i].dw = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
            arr[i].dbias = db.data_ptr() if db is not None else None
        info = (ctypes.c_int32 * 4)()
        nbytes = lib.kd6d_wgrad_group_plan(arr, n, _lib.KD6D_BF16, self.n_workgroups, None, 0, info)
        if nbytes < 0:
            check(int(nbytes), "kd6d_wgrad_group_plan")
        host = torch.zeros(int(nbytes), dtype=torch.uint8)
        rc = lib.kd6d_wgrad_group_plan(arr, n, _lib.KD6D_BF16, self.n_workgroups, ctypes.c_void_p(host.data_ptr()),
                                       int(nbytes), info)
        if rc < 0:
            check(int(rc), "kd6d_wgrad_group_plan")
        slab_floats = int(info[2]) + (int(info[3]) << 31)
        # allocated on the default stream: the caching allocator then never hands the blocks to another stream's
        # tensors while a side stream (where the launch runs) still uses them
        with torch.cuda.stream(torch.cuda.default_stream(device)):
            plan = host.to(device)
            slab = torch.empty(slab_floats, dtype=torch.float32, device=device)
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream(device))
        return dict(plan=plan, slab=slab, info=(int(info[0]), int(info[1])), keep=list(self.items))

    def launch(self):
        """Enqueue on the current stream; clears the collected items."""
        if not self.items:
            return
        # the plan holds the pointers AND the geometry (levels, channels, kernel size): both are the key, so the same
        # buffers under other levels of the same row total get a plan of their own
        key = (self.n_workgroups,) + tuple(
            (x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), bytes(g.c))
            for g, x, dy, dw, db in self.items)
        ent = self._plans.get(key)
        if ent is None:
            ent = self._plans[key] = self._build(self.items[0][1].device)
        with _Timed("conv_wgrad", self.flops, self.items[0][0]):
            check(lib.kd6d_wgrad_group_launch(_ptr(ent["plan"]), ent["info"][0], ent["info"][1], _ptr(ent["slab"]),
                                              _stream()), "kd6d_wgrad_group_launch")
        self.items, self.flops = [], 0


# ---- device-resident frame cache (csrc/frame_cache.hip; kd6d/libs/frame_cache.py) ---------------------------------
def cache_target_sizes(batch, kp_elems):
    """(fp32, int32) elements of the packed small fields of a PackedTargets of `batch` images: kd6d_cache_gather_targets'
    outputs, the layout of PackedTargets._SMALL_F / _SMALL_I (every field rounded up to 4 elements)."""
    up = lambda v: (v + 3) // 4 * 4
    g = _lib.MAX_GT
    return (up(batch * kp_elems) + up(batch * 9) + up(batch * 6) + up(batch * g * 9) + up(batch * g * 3),
            up(batch * g) + up(batch))


def cache_gather_frames(frames, masks, index, frames_out=None, masks_out=None):
    """frames (n,H,W,3) uint8, masks (n,H,W) uint8, index (B) int32, all on the device -> (frames[index] uint8,
    masks[index] as float32).  frames_out / masks_out: optional caller-owned outputs (contiguous views are fine)."""
    assert frames.dtype == torch.uint8 and masks.dtype == torch.uint8 and index.dtype == torch.int32
    n, H, W, C = frames.shape
    assert C == 3 and tuple(masks.shape) == (n, H, W)
    B = int(index.numel())
    if frames_out is None:
        frames_out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=frames.device)
    if masks_out is None:
        masks_out = torch.empty((B, H, W), dtype=torch.float32, device=frames.device)
    assert tuple(frames_out.shape) == (B, H, W, 3) and frames_out.dtype == torch.uint8
    assert tuple(masks_out.shape) == (B, H, W) and masks_out.dtype == torch.float32
    check(lib.kd6d_cache_gather_frames(_ptr(frames), _ptr(masks), n, H, W, _ptr(index), B, _ptr(frames_out),
                                       _ptr(masks_out), _stream()), "kd6d_cache_gather_frames")
    return frames_out, masks_out


def cache_gather_targets(table_f, table_i, kp3d, index, bbox_trans, flat_f=None, flat_i=None):
    """Annotation table rows `index` + the crop launch's bbox_trans (B,2,3) -> (flat_f, flat_i) of a PackedTargets."""
    n = int(table_f.shape[0])
    assert table_f.dtype == torch.float32 and tuple(table_f.shape) == (n, _lib.CACHE_ROW_F)
    assert table_i.dtype == torch.int32 and tuple(table_i.shape) == (n, _lib.CACHE_ROW_I)
    assert kp3d.dtype == torch.float32 and index.dtype == torch.int32
    B = int(index.numel())
    assert bbox_trans.dtype == torch.float32 and bbox_trans.numel() == B * 6
    nf, ni = cache_target_sizes(B, int(kp3d.numel()))
    if flat_f is None:
        flat_f = torch.empty(nf, dtype=torch.float32, device=table_f.device)
    if flat_i is None:
        flat_i = torch.empty(ni, dtype=torch.int32, device=table_f.device)
    assert flat_f.numel() == nf and flat_i.numel() == ni
    check(lib.kd6d_cache_gather_targets(_ptr(table_f), _ptr(table_i), _ptr(kp3d), int(kp3d.numel()), n, _ptr(index), B,
                                        _ptr(bbox_trans), _ptr(flat_f), _ptr(flat_i), _stream()),
          "kd6d_cache_gather_targets")
    return flat_f, flat_i
