"""CPU: the host-side pieces of the replayed steps (kd6d/graph.py, kd6d/libs/distributed.py), each on its own with recording
stand-ins and no device object:
  * the byte-block layout both pipelines cut their hand-over blocks with (block_layout / block_views);
  * the ONE replay routine: advance -> replay with one graph per step, replay -> exchange -> advance -> optimiser graph with two;
  * the ONE capture routine: which warm-up runs the exchange, one pool, the optimiser's graph only when there are two per step,
    the training state put back;
  * the overlapped gradient exchange around PoseNet.backward (D.overlapped_exchange)."""
from types import SimpleNamespace as NS

import pytest
import torch

from kd6d import graph as G
from kd6d.libs import distributed as D


# ---- 1. block layout ------------------------------------------------------------------------------------------------------
def _check_layout(parts, nbytes):
    offs, total = G.block_layout(parts)
    aligned = [(n + 255) // 256 * 256 for n in nbytes]
    assert len(offs) == len(parts) and all(o % 256 == 0 for o in offs)
    assert total == sum(aligned)
    for i, (o, n) in enumerate(zip(offs, nbytes)):                  # no two parts overlap, none leaves the block
        assert o + n <= (offs[i + 1] if i + 1 < len(offs) else total)
    return offs, total


def test_block_layout_edge_sizes():
    sizes = [1, 255, 256, 257, 0]
    offs, total = _check_layout(sizes, sizes)
    assert (offs, total) == ([0, 256, 512, 768, 1280], 1280)
    block = torch.zeros(total, dtype=torch.uint8)
    views = G.block_views(block, sizes, offs)
    assert [v.numel() for v in views] == sizes and all(v.dtype == torch.uint8 for v in views)
    for i, v in enumerate(views):
        v.fill_(i + 1)
    want = torch.zeros(total, dtype=torch.uint8)
    for i, (o, n) in enumerate(zip(offs, sizes)):
        want[o:o + n] = i + 1
    assert torch.equal(block, want)                                  # every view writes its own bytes, nothing else


def test_block_layout_realistic_set_matches_the_former_arithmetic():
    """B = 2 at 64 x 64: the packed NHWC-8 bf16 image, a target block of 33000 bytes, and the two buffers of the teacher's
    cells (teacher_flat_sizes(2, 32): 3072 floats, 68 ints).  Expected numbers from the formula both former copies used,
    offset += (bytes + 255) // 256 * 256: 131072 | 33000 -> 33024 | 12288 | 272 -> 512."""
    from kd6d.kd_losses import teacher_flat_sizes
    nf, ni = teacher_flat_sizes(2, 32)
    assert (nf, ni) == (3072, 68)
    parts = [((2 * 64 * 64, 8), torch.bfloat16), 33000, ((nf,), torch.float32), ((ni,), torch.int32)]
    offs, total = _check_layout(parts, [131072, 33000, 12288, 272])
    assert (offs, total) == ([0, 131072, 164096, 176384], 176896)
    block = torch.zeros(total, dtype=torch.uint8)
    nhwc, tgt, wf, wi = G.block_views(block, parts, offs)
    assert (nhwc.dtype, tuple(nhwc.shape)) == (torch.bfloat16, (8192, 8))
    assert (tgt.dtype, tuple(tgt.shape)) == (torch.uint8, (33000,))
    assert (wf.dtype, tuple(wf.shape)) == (torch.float32, (3072,))
    assert (wi.dtype, tuple(wi.shape)) == (torch.int32, (68,))
    base = block.data_ptr()
    assert [v.data_ptr() - base for v in (nhwc, tgt, wf, wi)] == offs          # views alias the block
    wi.fill_(-1)
    assert int((block != 0).sum()) == 272 and bool((block[176384:176384 + 272] == 255).all())
    # the grouped step's block: `group` target blocks in a row, each on its own boundary
    T = 3
    parts = [((T * 8192, 8), torch.bfloat16)] + [33000] * T + [((T * nf,), torch.float32), ((T * ni,), torch.int32)]
    offs, total = G.block_layout(parts)
    o_tgt = T * 131072
    o_wf = o_tgt + T * 33024
    o_wi = o_wf + T * 12288
    assert offs == [0] + [o_tgt + s * 33024 for s in range(T)] + [o_wf, o_wi]
    assert total == o_wi + (T * 272 + 255) // 256 * 256


# ---- stand-ins for the step classes ---------------------------------------------------------------------------------------
class Opt:
    def __init__(self, log):
        self.log, self.steps, self._step_count, self._opt_called = log, 0, 0, False
        self.exp_avg, self.exp_avg_sq = torch.zeros(4), torch.zeros(4)

    def advance(self):
        self.steps += 1
        self.log.append("advance")

    def launch(self, device_schedule=False):
        assert device_schedule
        self.exp_avg += 1.0
        self.exp_avg_sq += 1.0
        self.log.append("opt")


class Graph:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def replay(self):
        self.log.append("replay(%s)" % self.name)


def _student(n_bn=3):
    store = NS(params=torch.arange(4.0), bufs=torch.ones(2), shadow=None)
    net = NS(store=store, bns=[("bn%d" % i, NS(fold="stale")) for i in range(n_bn)], device="cpu")
    return NS(net=net, _nbt=torch.zeros(n_bn, dtype=torch.long))


def _step(log, exchange="between"):
    """A real _KDStepBase: without a teacher stream and side streams its constructor touches no device."""
    return G._KDStepBase(None, _student(), Opt(log), (0.1, 1.0, 5.0), None, 2, exchange, teacher_stream=False,
                         side_streams=0, wgrad=(0, 512, "fpn_end"))


@pytest.fixture
def exchange_log(monkeypatch):
    log = []
    monkeypatch.setattr(D, "exchange_active", lambda: True)
    monkeypatch.setattr(D, "exchange_gradients", lambda store: log.append("exchange"))
    return log


# ---- 2. replay order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, want", [(1, ["advance", "replay(step)"]),
                                     (2, ["replay(step)", "exchange", "advance", "replay(opt)"])])
def test_replay_order(exchange_log, n, want):
    log = exchange_log
    st = _step(log)
    st.graphs_per_step, st.g_opt, st.losses = n, Graph(log, "opt"), {"loss_cls": 1}
    assert st._replay(Graph(log, "step")) is st.losses
    assert log == want
    assert st.opt._step_count == 1 and st.opt._opt_called                    # the step count hook ran
    assert all(bn.fold is None for _, bn in st.student.net.bns)               # every cached BN fold is dropped


def test_replay_overlap_runs_no_exchange_between_graphs(exchange_log):
    st = _step(exchange_log, exchange="overlap")
    st.graphs_per_step, st.losses = 1, {}
    st._replay(Graph(exchange_log, "step"))
    assert exchange_log == ["advance", "replay(step)"]
    st._exchange()                                                            # both slices went out inside the step
    assert "exchange" not in exchange_log


# ---- 3. capture -----------------------------------------------------------------------------------------------------------
class _Cuda:
    """torch.cuda, as far as the capture routine reaches it."""

    def __init__(self, monkeypatch, log):
        self.pools = []
        cuda = self

        class Stream:
            def wait_stream(self, other):
                pass

        class CUDAGraph(Graph):
            def __init__(self):
                super().__init__(log, "g%d" % len(cuda.pools))

            def pool(self):
                return "pool-of-first"

        class ctx:
            def __init__(self, *a, **k):
                pass

            def __enter__(self):
                return self

            def __exit__(self, *exc):
                return False

        class graph(ctx):
            def __init__(self, g, pool=None, capture_error_mode=None):
                assert capture_error_mode == "thread_local"
                cuda.pools.append(pool)
                self.g = g

            def __enter__(self):
                log.append("capture_begin")

            def __exit__(self, *exc):
                log.append("capture_end")
                return False

        for name, obj in (("Stream", Stream), ("CUDAGraph", CUDAGraph), ("graph", graph), ("stream", ctx),
                          ("current_stream", Stream), ("synchronize", lambda: None)):
            monkeypatch.setattr(torch.cuda, name, obj)


@pytest.mark.parametrize("active", [False, True])
@pytest.mark.parametrize("warmup_exchange", [False, True])
def test_capture_routine(monkeypatch, exchange_log, active, warmup_exchange):
    log = exchange_log
    monkeypatch.setattr(D, "exchange_active", lambda: active)
    cuda = _Cuda(monkeypatch, log)
    st = _step(log)
    store, opt = st.student.net.store, st.opt

    def body(name):
        def run():
            store.params.add_(1.0)                    # a step trains ...
            st.student._nbt.add_(1)
            log.append(name)
            return {"from": name}
        return run

    graphs = st._capture_graphs([body("a"), body("b")], warmup_exchange=warmup_exchange)
    per_body = (["exchange"] if warmup_exchange else []) + ["advance", "opt"]
    warm = (["a"] + per_body + ["b"] + per_body) * 2                                     # warmup = 2
    n = 2 if active else 1
    cap = []
    for name in ("a", "b"):
        cap += ["capture_begin", name] + (["opt"] if n == 1 else []) + ["capture_end"]
    if n == 2:
        cap += ["capture_begin", "opt", "capture_end"]
    assert log == warm + cap
    assert st.graphs_per_step == n and len(graphs) == 2 and (st.g_opt is not None) == (n == 2)
    assert cuda.pools == [None] + ["pool-of-first"] * (len(graphs) + n - 2)              # ONE pool
    assert st.losses == {"from": "b"}
    # ... and the capture does not: parameters, buffers, moments, counters are the ones from before
    assert torch.equal(store.params, torch.arange(4.0)) and torch.equal(opt.exp_avg, torch.zeros(4))
    assert torch.equal(opt.exp_avg_sq, torch.zeros(4)) and int(st.student._nbt.sum()) == 0
    assert (opt.steps, opt._step_count) == (0, 0)


def test_grouped_step_warms_up_without_an_exchange(monkeypatch, exchange_log):
    """No RCCL communicator may come to life before the graphs exist: the grouped step's warm-up steps run no exchange,
    the plain step's do."""
    log = exchange_log
    _Cuda(monkeypatch, log)
    monkeypatch.setattr(G.ops, "device_cu_count", lambda: 256)
    student = _student()
    gs = G.GroupedTeacherKDStep(None, student, Opt(log), group=2, warmup=1)
    assert (student.net.wgrad_cu_budget, student.net.wgrad_group_wgs, student.net.wgrad_group_flush) == (64, 512, "fpn_end")
    gs._student_body = lambda s: log.append("body%d" % s)
    gs.ensure_captured()
    assert "exchange" not in log and log[:6] == ["body0", "advance", "opt", "body1", "advance", "opt"]
    assert gs.graphs_per_step == 2 and len(gs.g_student) == 2 and gs.g_step is gs.g_student[0]
    del log[:]
    gs.ensure_captured()
    assert log == []                                                          # captured once
    assert gs.replay_student(1) is gs.losses and log == ["replay(g1)", "exchange", "advance", "replay(g2)"]

    del log[:]
    student = _student()
    ps = G.GraphedKDStep(None, student, Opt(log), warmup=1, pipeline=False)
    assert (student.net.wgrad_cu_budget, student.net.wgrad_group_wgs, student.net.wgrad_group_flush) == (64, 512, "fpn_end")
    assert len(student.net.side_streams) == G.GraphedKDStep.WGRAD_STREAMS and ps.teacher_stream is not None
    ps.teacher = NS(_teacher_flats=("f", "i"))
    ps.images = NS(tensors=torch.zeros(2, 3, 8, 8))
    ps._forward_backward = lambda: log.append("body")
    ps._capture()
    assert log[:4] == ["body", "exchange", "advance", "opt"] and not ps.pending and ps.pending_steps == 0
    piped = G.GraphedKDStep(None, _student(), Opt(log), pipeline=True)
    assert (piped.student.net.wgrad_cu_budget, piped.student.net.wgrad_group_wgs,
            piped.student.net.wgrad_group_flush) == (128, 128, "head_end")


# ---- 4. the overlapped exchange -------------------------------------------------------------------------------------------
class _NamedStream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_stream(self, other):
        self.log.append(("wait", self.name, other.name))


def _overlap_fixture(monkeypatch):
    log = []
    state = {"current": _NamedStream(log, "main")}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: state["current"])

    class on_stream:
        def __init__(self, s):
            self.s = s

        def __enter__(self):
            self.prev, state["current"] = state["current"], self.s

        def __exit__(self, *exc):
            state["current"] = self.prev
            return False

    monkeypatch.setattr(torch.cuda, "stream", on_stream)
    monkeypatch.setattr(D, "exchange_slice", lambda store, lo, hi: log.append(("exchange", state["current"].name, lo, hi)))
    sides = [_NamedStream(log, "w0"), _NamedStream(log, "w1")]
    store = NS(n_train=1000, resolve_grads=lambda lo, hi: log.append(("resolve", state["current"].name, lo, hi)))
    net = NS(store=store, wgrad=NS(streams=lambda: list(sides)), grad_hook=None, resolve_hi=None)
    return log, net, _NamedStream(log, "comm")


def test_overlapped_exchange_order_and_bounds(monkeypatch):
    log, net, comm = _overlap_fixture(monkeypatch)
    with D.overlapped_exchange(net, comm, 300):
        assert callable(net.grad_hook) and net.resolve_hi == 300             # installed inside the `with` ...
        log.append("fpn+head swept")
        net.grad_hook()
        log.append("backbone swept")
        assert log[-6:-1] == [("wait", "comm", "main"), ("wait", "comm", "w0"), ("wait", "comm", "w1"),
                              ("resolve", "comm", 300, 1000), ("exchange", "comm", 300, 1000)]
        log.append("student.bwd.end")
    assert net.grad_hook is None and net.resolve_hi is None                   # ... and only there
    assert log == ["fpn+head swept", ("wait", "comm", "main"), ("wait", "comm", "w0"), ("wait", "comm", "w1"),
                   ("resolve", "comm", 300, 1000), ("exchange", "comm", 300, 1000), "backbone swept", "student.bwd.end",
                   ("wait", "main", "comm"), ("exchange", "main", 0, 300)]


def test_overlapped_exchange_removes_the_hook_on_an_exception(monkeypatch):
    log, net, comm = _overlap_fixture(monkeypatch)
    with pytest.raises(ZeroDivisionError):
        with D.overlapped_exchange(net, comm, 300):
            assert net.grad_hook is not None
            1 / 0
    assert net.grad_hook is None and net.resolve_hi is None
    assert log == []                                                          # no tail exchange behind a failed sweep


def test_setting_puts_back_what_was_there():
    obj = NS(a=1, b=None)
    with pytest.raises(KeyError):
        with G._setting(obj, a=2, b="x", c=3):
            assert (obj.a, obj.b, obj.c) == (2, "x", 3)
            raise KeyError("boom")
    assert (obj.a, obj.b, obj.c) == (1, None, None)
