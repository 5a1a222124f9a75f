"""A recording stand-in for kd6d.ops inside kd6d.engine, for CPU tests of the forward and reverse walk of PoseNet.

`Ledger` takes every launch the engine issues -- with the tensors and scalars it is handed, the stream it is issued on --
and runs nothing; streams are recording stand-ins too.  A real PoseNet of any backbone then walks small CPU tensors, so
the code under test is the engine's own: ConvBlock, the head and FPN walks, both backbone sweeps, WgradSchedule.

  events   (kind, ...) in issue order: ("launch", name, stream), ("wgrad", stream, calls), ("group", stream, n),
           ("wait", waiter, other), ("pair", enabled) / ("pair_end", enabled), ("mark", name), and whatever a test appends
           itself (hook, tail, cut, resolve)
  calls    (event index, name, args, kwargs) of every launch and weight gradient, the tensors as they were handed over
  writes   (event index, span) of the tensor each launch writes
  born     slab data_ptr -> event index at which its layer's Conv.bwd built the weight-gradient call"""
import contextlib

import pytest
import torch

from kd6d import engine, ops as real_ops

# position (or keyword) of the tensor a launch WRITES; everything else it is handed is read
WRITES = {"image_to_nhwc": "out", "conv2d_fwd": "out", "conv2d_fwd_block": 3, "conv2d_fwd_norm": 3, "conv2d_dgrad": "dx",
          "eltwise": 3, "upsample2_add": 2, "sumpool2": 1, "maxpool2_fwd": 1, "maxpool2_bwd": 2, "gn_relu_fwd": 1,
          "bn_train_fwd": 1, "bn_train_fwd_res": 2, "bn_pool_train_fwd": 1, "bn_train_bwd": 2, "bn_pool_train_bwd": 2,
          "gn_relu_bwd": 2}
# what the engine asks of ops without launching anything: handed through to the real module
PASS = ("get_option", "set_option", "option", "wgrad_group_supported", "gn_bwd_workspace_floats", "conv_norm_stats_floats",
        "conv_norm_counter_words")


def span(t):
    return (t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size(),
            t.untyped_storage().data_ptr() + (t.storage_offset() + t.numel()) * t.element_size())


def overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


class Stream:
    def __init__(self, ledger, name):
        self.ledger, self.name = ledger, name

    def wait_stream(self, other):
        self.ledger.events.append(("wait", self.name, other.name))


class _Lib:
    """kd6d.ops.lib for the few entry points the engine calls directly (the shadow cast, the gradient resolve)."""

    def __init__(self, ledger):
        self._ledger = ledger

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a: self._ledger._launch("lib." + name, a, {}) or 0


class Ledger:
    """Stands in for kd6d.ops inside kd6d.engine."""

    def __init__(self):
        self.events = []            # (kind, ...) in issue order
        self.calls = []             # (event index, name, args, kwargs)
        self.writes = []            # (event index, span)
        self.current = "main"
        self.main = Stream(self, "main")
        self.born = {}              # slab data_ptr -> event index at which its layer's Conv.bwd built the call
        self.fusable = False        # what conv_norm_fusable answers
        self.stem_parts = 0         # what bn_pool_bwd_wgrad_parts answers (0: the stem goes through Conv.bwd)
        self.lib = _Lib(self)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        val = getattr(real_ops, name)
        if not callable(val) or isinstance(val, type) and name == "Geom" or name in PASS:
            return val
        return lambda *a, **k: self._launch(name, a, k)

    # ---- sizes and switches the engine asks for (no device) ----
    def device_cu_count(self):
        return 256

    def conv2d_wgrad_parts(self, *a, **k):
        return 2

    def bn_pool_bwd_wgrad_parts(self, *a, **k):
        return self.stem_parts

    def conv_norm_fusable(self, *a, **k):
        return self.fusable

    def check(self, *a, **k):
        return None

    def _ptr(self, t):
        return t

    def _stream(self):
        return self.current

    def mark(self, name):
        self.events.append(("mark", name))

    @contextlib.contextmanager
    def conv_pair(self, enabled=True):
        self.events.append(("pair", bool(enabled)))
        try:
            yield
        finally:
            self.events.append(("pair_end", bool(enabled)))

    def WgradGroup(self, wgs):
        ledger = self

        class Group(list):
            n_workgroups = wgs

            def add(self, g, x, dy, dw, dbias, flops=0):
                self.append((x, dy))
                ledger.calls.append((len(ledger.events), "group.add", (g, x, dy, dw, dbias), dict(flops=flops)))

            def launch(self):
                ledger.events.append(("group", ledger.current, len(self)))
                del self[:]
        return Group()

    def _launch(self, name, a, k):
        idx = len(self.events)
        out = None
        w = WRITES.get(name)
        if isinstance(w, str):
            out = k.get(w)
        elif w is not None and w < len(a):
            out = a[w]
        if name == "conv2d_fwd" and out is None:        # an eval-mode block: the launcher allocates its output
            geom, x = a[0], a[1]
            out = torch.empty((geom.rows_out, geom.cout), dtype=torch.float32 if k.get("out_f32") else x.dtype)
            k = dict(k, out=out)
        self.events.append(("launch", name, self.current))
        self.calls.append((idx, name, a, k))
        if torch.is_tensor(out):
            self.writes.append((idx, span(out)))
        return out

    def conv2d_wgrad(self, geom, x, dy, slab, flops=0, dbias=None, acc_stride=0, cu_budget=0):
        call = dict(geom=geom, x=x, dy=dy, dw_slab=slab, flops=flops, dbias=dbias, acc_stride=acc_stride, cu_budget=cu_budget)
        self.calls.append((len(self.events), "conv2d_wgrad", (), call))
        self.events.append(("wgrad", self.current, [call]))

    def conv2d_wgrad_list(self, calls):
        for call in calls:
            self.calls.append((len(self.events), "conv2d_wgrad", (), call))
        self.events.append(("wgrad", self.current, list(calls)))


def install(monkeypatch, led):
    """Put `led` in the place of kd6d.ops inside kd6d.engine, and recording stand-ins in the place of torch's streams."""
    monkeypatch.setattr(engine, "ops", led)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: led.main)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)

    @contextlib.contextmanager
    def on(stream):
        old, led.current = led.current, stream.name
        try:
            yield
        finally:
            led.current = old
    monkeypatch.setattr(torch.cuda, "stream", on)
    slab = engine.Conv.wgrad_slab

    def wgrad_slab(self, g, dtype, cu_budget):
        s = slab(self, g, dtype, cu_budget)
        led.born[s.data_ptr()] = len(led.events)
        return s
    monkeypatch.setattr(engine.Conv, "wgrad_slab", wgrad_slab)
    return led


def host_only(net):
    """Keep a network's walk off the weights: no bf16 shadow, no dgrad packing, no resolve (none of them is under test)."""
    net.store.ensure_grads()
    net.store.resolve_grads = lambda *a, **k: engine.ops.events.append(("resolve",))
    net.prepare_weights = lambda **k: None
    for conv in net.convs:
        conv.weight = conv.weight_t = conv.bias = lambda: None
    return net


@pytest.fixture
def ledger(monkeypatch):
    return install(monkeypatch, Ledger())
