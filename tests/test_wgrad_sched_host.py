"""CPU: the reverse sweep's weight-gradient scheduler (kd6d/wgrad_sched.py) on its own, with stand-in convolutions,
streams and launchers.  Checked: the decision table of submit() (group / list / one fork / in line), the round-robin
order of the forks over 1 and 4 streams, the flush points of the lists, begin() after an aborted sweep, streams() and
budget() for the three stream configurations, finish()'s joins, which of the two points launches the group, and that
wgrad_group_wgs is read when the first sweep begins."""
import contextlib
from types import SimpleNamespace as NS

import pytest
import torch

from kd6d.wgrad_sched import WgradSchedule

BF16, F32 = NS(dtype=torch.bfloat16), NS(dtype=torch.float32)


class Stream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_stream(self, other):
        self.log.append(("wait", self.name, other.name))


class Ops:
    """The launchers the scheduler reaches: every call lands in `log` with the stream it is issued on."""

    def __init__(self, log):
        self.log, self.current, self.list_option, self.unsupported = log, "main", 0, set()

    def get_option(self, name):
        assert name == "wgrad.list"
        return self.list_option

    def device_cu_count(self):
        return 256

    def wgrad_group_supported(self, geom, dtype):
        return geom not in self.unsupported

    def WgradGroup(self, wgs):
        ops = self
        ops.log.append(("group_new", wgs))

        class Group(list):
            def add(self, geom, x, dy, dw, dbias, flops=0):
                self.append((geom, dw, dbias, flops))

            def launch(self):
                ops.log.append(("group", ops.current, [g for g, _, _, _ in self]))
                del self[:]
        return Group()

    def conv2d_wgrad(self, geom, x, dy, slab, flops=0, dbias=None, acc_stride=0, cu_budget=0):
        self.log.append(("wgrad", self.current, [geom], cu_budget))
        assert (slab, flops, dbias, acc_stride) == ("slab:%s:%d" % (geom, cu_budget), 100, "acc:b", 7)

    def conv2d_wgrad_list(self, calls):
        self.log.append(("wgrad", self.current, [c["geom"] for c in calls], calls[0]["cu_budget"]))
        for c in calls:
            assert sorted(c) == ["acc_stride", "cu_budget", "dbias", "dw_slab", "dy", "flops", "geom", "x"]
            assert c["dw_slab"] == "slab:%s:%d" % (c["geom"], c["cu_budget"]) and c["dbias"] == "acc:b"

    def mark(self, name):
        pass


class Conv:
    w, b = "w", "b"

    def __init__(self, log):
        self.log, self.born = log, {}

    def flops(self, geom):
        return 100

    def wgrad_slab(self, geom, dtype, cu_budget):
        self.born[geom] = len(self.log)
        return "slab:%s:%d" % (geom, cu_budget)


@pytest.fixture
def rig(monkeypatch):
    """(scheduler, net, ops, conv, log) with `n` side streams: rig(0) none, rig(1) side_stream only, rig(4) the list."""
    def make(n, dtype=torch.bfloat16):
        log = []
        ops = Ops(log)
        main = Stream(log, "main")
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: main)

        @contextlib.contextmanager
        def on(stream):
            old, ops.current = ops.current, stream.name
            try:
                yield
            finally:
                ops.current = old
        monkeypatch.setattr(torch.cuda, "stream", on)
        store = NS(storage=lambda e, which: "%s:%s" % (which, e), acc=lambda e: "acc:%s" % e, acc_stride=7)
        sides = [Stream(log, "s%d" % i) for i in range(n)]
        net = NS(dtype=dtype, store=store, side_stream=sides[0] if n else None, side_streams=sides if n > 1 else None,
                 wgrad_cu_budget=64, use_wgrad_group=True, wgrad_group_wgs=0, wgrad_group_flush="head_end")
        return WgradSchedule(net, ops), net, ops, Conv(log), log
    return make


def _launches(log):
    return [e for e in log if e[0] in ("wgrad", "group")]


# ---- the decision table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [0, 1, 4])
@pytest.mark.parametrize("list_option", [0, 1, 3])
def test_submit_decision_table(rig, n_streams, list_option):
    s, net, ops, conv, log = rig(n_streams)
    ops.list_option = list_option
    ops.unsupported = {"odd"}
    s.begin()
    # grouped section open, bf16, a geometry the grouped kernel takes: the group -- nothing is launched, no stream taken
    s.submit(conv, "g0", BF16, BF16)
    assert _launches(log) == [] and len(s.group) == 1 and s.pending == [] and s.rr == 0
    assert s.group[0] == ("g0", "grads:w", "grads:b", 100)
    # ... an unsupported geometry or fp32 tensors inside the section, and everything behind it: per layer
    per_layer = [("odd", BF16), ("f32", F32)]
    for geom, x in per_layer:
        s.submit(conv, geom, x, x)
    s.close_group_section()
    s.submit(conv, "g1", BF16, BF16)
    assert len(s.group) == 1
    names = ["odd", "f32", "g1"]
    if n_streams and list_option > 1:
        assert _launches(log) == [("wgrad", "s1" if n_streams > 1 else "s0", names, 64)]          # one list of three
        s.enter_tail()
        s.submit(conv, "t", BF16, BF16)                                                            # the tail: one fork
        assert _launches(log)[1:] == [("wgrad", "s2" if n_streams > 1 else "s0", ["t"], 64)]
    elif n_streams:
        want = ["s1", "s2", "s3"] if n_streams > 1 else ["s0"] * 3
        assert _launches(log) == [("wgrad", st, [g], 64) for st, g in zip(want, names)]            # one fork each
        assert [e for e in log if e[0] == "wait"] == [("wait", st, "main") for st in want]
    else:
        assert _launches(log) == [("wgrad", "main", [g], 0) for g in names]                        # in line, budget 0
        assert not [e for e in log if e[0] == "wait"]
    assert s.pending == []


def test_group_needs_bf16_network_and_the_knob(rig):
    for dtype, use, want in ((torch.float32, True, False), (torch.bfloat16, False, False), (torch.bfloat16, True, True)):
        s, net, ops, conv, log = rig(4, dtype)
        net.use_wgrad_group = use
        s.begin()
        assert (s.group is not None) == want == s.grouping
        assert s.try_group(conv, "g", BF16, BF16) == want
        s.close_group_section()
        assert not s.try_group(conv, "g", BF16, BF16)


# ---- round robin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 4])
def test_round_robin_over_lists_single_forks_and_the_group(rig, n_streams):
    s, net, ops, conv, log = rig(n_streams)
    ops.list_option = 2
    s.begin()
    s.submit(conv, "h0", BF16, BF16)
    assert s.try_group(conv, "o0", BF16, BF16)
    s.close_group_section()
    s.flush_group("head_end")                  # fork 1: the group
    s.submit(conv, "a", BF16, BF16)
    rr = s.rr
    s.submit(conv, "b", BF16, BF16)            # fork 2: [a, b]; `a` took no stream while it waited
    assert s.rr == (rr + 1) % n_streams
    s.submit(conv, "c", BF16, BF16)
    s.enter_tail()                             # fork 3: [c]
    s.submit(conv, "d", BF16, BF16)            # fork 4
    s.submit(conv, "e", BF16, BF16)            # fork 5
    s.finish()
    name = (lambda k: "s%d" % (k % 4)) if n_streams == 4 else (lambda k: "s0")
    assert _launches(log) == [("group", name(1), ["h0", "o0"]), ("wgrad", name(2), ["a", "b"], 64),
                              ("wgrad", name(3), ["c"], 64), ("wgrad", name(4), ["d"], 64), ("wgrad", name(5), ["e"], 64)]
    # every fork: the side stream waits for the chain's stream, then the launch
    forks = [i for i, e in enumerate(log) if e[0] == "wait" and e[2] == "main"]
    assert [log[i][1] for i in forks] == [name(k) for k in range(1, 6)]
    assert all(log[i + 1][0] in ("wgrad", "group") and log[i + 1][1] == log[i][1] for i in forks)
    # the slab is taken when the layer is reached, not at the flush
    assert conv.born["a"] <= conv.born["b"] < next(i for i, e in enumerate(log) if e[0] == "wgrad")


# ---- flushing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [2, 3, 4])
def test_lists_flush_at_the_option_value_and_the_remainder_on_request(rig, value):
    s, net, ops, conv, log = rig(4)
    net.use_wgrad_group = False
    ops.list_option = value
    flushes = []
    flush = s.flush_list

    def counted():
        flushes.append(len(s.pending))
        flush()
    s.flush_list = counted                      # (as tests/test_wgrad_list_step_gpu.py counts forks)
    s.begin()
    n = 2 * value + 1
    for k in range(n):
        s.submit(conv, "l%d" % k, BF16, BF16)
        assert len(_launches(log)) == (k + 1) // value, "a list goes out exactly when it is full"
    assert len(s.pending) == 1 and flushes == [value, value]
    s.flush_list()                              # the remainder
    s.flush_list()                              # nothing left: no fork
    assert [len(e[2]) for e in _launches(log)] == [value, value, 1] and s.pending == []
    assert [g for e in _launches(log) for g in e[2]] == ["l%d" % k for k in range(n)]
    assert len([e for e in log if e[0] == "wait"]) == 3
    # enter_tail(): what is pending first, then single forks whatever the option says; finish() ends the tail
    s.submit(conv, "p", BF16, BF16)
    s.enter_tail()
    assert flushes[-1] == 1 and _launches(log)[-1][2] == ["p"] and s.list_limit() == 0
    s.submit(conv, "q", BF16, BF16)
    s.submit(conv, "r", BF16, BF16)
    assert [e[2] for e in _launches(log)[-2:]] == [["q"], ["r"]] and s.pending == []
    s.finish()
    assert flushes[-1] == 0 and s.list_limit() == value


def test_begin_after_an_aborted_sweep_leaves_nothing_pending(rig):
    s, net, ops, conv, log = rig(4)
    net.use_wgrad_group = False
    ops.list_option = 4
    s.begin()
    s.submit(conv, "a", BF16, BF16)             # the sweep raised behind this layer: one call pending
    assert len(s.pending) == 1
    s.begin()
    assert s.pending == []
    s.enter_tail()                              # ... or inside its tail
    assert s.list_limit() == 0
    s.begin()
    assert not s.tail and s.list_limit() == 4
    s.finish()
    assert _launches(log) == [], "a call of the aborted sweep was launched by the next one"


# ---- streams, joins, budget -----------------------------------------------------------------------------------------
def test_streams_budget_and_finish_for_the_three_configurations(rig):
    for n in (0, 1, 4):
        s, net, ops, conv, log = rig(n)
        assert [st.name for st in s.streams()] == ["s%d" % i for i in range(n)]
        assert s.budget() == (64 if n else 0)
        net.wgrad_cu_budget = 32                # read from the net when asked, not copied
        assert s.budget() == (32 if n else 0)
        s.begin()
        s.finish()
        assert [e for e in log if e[0] == "wait"] == [("wait", "main", "s%d" % i) for i in range(n)]     # once per stream
    s, net, ops, conv, log = rig(1)
    net.side_streams = []                       # an empty list is no list
    assert [st.name for st in s.streams()] == ["s0"]


# ---- the group: which point launches, and its size ----------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [0, 4])
@pytest.mark.parametrize("point", ["head_end", "fpn_end"])
def test_the_group_goes_out_at_the_point_the_knob_names(rig, point, n_streams):
    s, net, ops, conv, log = rig(n_streams)
    net.wgrad_group_flush = point
    s.begin()
    s.submit(conv, "h", BF16, BF16)
    s.close_group_section()
    s.flush_group("head_end")
    assert len(_launches(log)) == (point == "head_end")
    s.flush_group("fpn_end")
    assert _launches(log) == [("group", "s1" if n_streams else "main", ["h"])]
    s.flush_group(point)                        # empty: no launch, no fork
    assert len(_launches(log)) == 1 and len([e for e in log if e[0] == "wait"]) == (1 if n_streams else 0)


def test_group_size_is_read_at_the_first_begin(rig):
    s, net, ops, conv, log = rig(4)
    assert log == []                            # nothing is created with the scheduler
    net.wgrad_group_wgs = 96                    # (bench.py sets it after the step object is built)
    s.begin()
    net.wgrad_group_wgs = 512
    s.begin()
    assert [e for e in log if e[0] == "group_new"] == [("group_new", 96)]
    s, net, ops, conv, log = rig(4)
    s.begin()
    assert log == [("group_new", 128)]          # 0: one workgroup per two CUs
