"""CPU: where the reverse sweep launches its per-layer weight gradients under option wgrad.list, with the device work
replaced by a ledger (kd6d.engine's `ops` records every launch with the tensors it reads and writes; streams are
recording stand-ins).  A real PoseNet of either backbone runs a real forward + backward walk on small CPU tensors, so the
code under test is Conv.bwd, WgradSchedule, the flush points of PoseNet.backward and of both backbone sweeps
(unit_bwd included).  For wgrad.list = 0, 2, 3 and 4:
  * every layer's weight gradient is issued exactly once;
  * after the launch that produces its dy, before the final join, and -- the FPN / head part -- before grad_hook;
  * nothing writes a buffer a pending call reads between the point its layer was reached and its launch;
  * the number of forks is what the option implies."""
import pytest
import torch

from kd6d import engine, ops as real_ops
from walk_ledger import Stream, ledger, overlap as _overlap, span as _span  # noqa: F401  (ledger: the fixture)


def _sweep(led, arch, value, hook=True):
    """One forward + backward walk; returns (events of the backward, index of the hook event, net)."""
    net = engine.PoseNet(arch, dtype=torch.bfloat16)
    net.training = True
    net.side_streams = [Stream(led, "side%d" % i) for i in range(4)]
    net.side_stream = net.side_streams[0]
    net.wgrad_cu_budget = 64
    net.store.ensure_grads()
    net.store.resolve_grads = lambda *a, **k: led.events.append(("resolve",))
    net.prepare_weights = lambda **k: None
    net.weight_of = None
    for conv in net.convs:
        conv_ = conv[1] if isinstance(conv, tuple) else conv
        conv_.weight = lambda: None
        conv_.weight_t = lambda: None
        conv_.bias = lambda: None
    enter_tail = net.wgrad.enter_tail

    def tail():
        led.events.append(("tail",))
        enter_tail()
    net.wgrad.enter_tail = tail
    B, H = 1, 64
    with real_ops.option("wgrad.list", value):
        net.forward(torch.zeros(B, 3, H, H))
        start = len(led.events)
        if hook:
            net.grad_hook = lambda: led.events.append(("hook",))
        dcls = torch.zeros(net.rows, 16, dtype=torch.bfloat16)
        dreg = torch.zeros(net.rows, 240, dtype=torch.bfloat16)
        net.backward(dcls, dreg)
    return start, net, (dcls, dreg)


def _layers(net):
    return [c[1] if isinstance(c, tuple) else c for c in net.convs]


@pytest.mark.parametrize("arch", ["darknet_tiny_h", "darknet53"])
def test_sweep_issues_every_weight_gradient_once_and_in_time(ledger, arch):
    led = ledger
    sections = {}
    for value in (0, 2, 3, 4):
        del led.events[:], led.writes[:]
        led.born.clear()
        start, net, douts = _sweep(led, arch, value)
        ev = led.events
        joins = [i for i, e in enumerate(ev) if e[0] == "wait" and e[1] == "main" and i > start]
        hook = next(i for i, e in enumerate(ev) if e == ("hook",))
        assert joins and hook < joins[0]
        seen = {}
        for i, e in enumerate(ev):
            if e[0] != "wgrad":
                continue
            assert e[1] != "main", "a weight gradient on the chain's stream"
            assert i < joins[0], "a weight gradient behind the final join"
            assert len(e[2]) <= max(value, 1), "a fork carries more calls than the option allows"
            for c in e[2]:
                key = c["dw_slab"].data_ptr()
                assert key not in seen, "a layer's weight gradient issued twice"
                seen[key] = i
                born = led.born[key]
                assert start <= born <= i
                for t in (c["x"], c["dy"]):
                    sp = _span(t)
                    assert not any(born <= w < i and _overlap(sp, s) for w, s in led.writes), \
                        "a buffer a pending call reads is written before its launch (wgrad.list=%d)" % value
                # dy was produced before the layer was reached (the head's logit gradients come from the caller)
                sp = _span(c["dy"])
                made = [w for w, s in led.writes if start <= w < born and _overlap(sp, s)]
                assert made or any(_overlap(sp, _span(d)) for d in douts), "dy has no producer in the sweep"
        # every convolution of the network: either in the grouped launch or issued here, exactly once
        grouped = sum(e[2] for e in ev if e[0] == "group")
        assert len(seen) + grouped == len(_layers(net)), (len(seen), grouped, len(_layers(net)))
        # the FPN / head part is out before the hook: no call born before the hook is launched behind it
        for key, i in seen.items():
            if led.born[key] < hook:
                assert i < hook, "an FPN weight gradient behind grad_hook"
        # a fork = a side stream waiting for the chain.  What the option implies, exactly: the layers in front of the hook
        # (FPN, P6 / P7) in lists of `value` with the remainder flushed at the hook, the backbone's layers in front of the
        # tail the same with the remainder flushed where the tail begins, one fork per layer inside the tail, and one
        # fork for the grouped head launch
        tail = next(i for i, e in enumerate(ev) if e == ("tail",))
        assert hook < tail < joins[0]
        born = sorted(led.born[k] for k in seen)
        n_fpn = sum(1 for b in born if b < hook)
        n_pre = sum(1 for b in born if hook < b < tail)
        n_tail = sum(1 for b in born if b > tail)
        assert n_fpn >= 2 and n_pre >= 5 and n_tail >= net.wgrad.WGRAD_LIST_TAIL_BLOCKS, (n_fpn, n_pre, n_tail)
        sections.setdefault(arch, (n_fpn, n_pre, n_tail))
        assert sections[arch] == (n_fpn, n_pre, n_tail), "the option changed which section a layer belongs to"
        v = max(value, 1)
        want = []
        for n in (n_fpn, n_pre):
            want += [v] * (n // v) + ([n % v] if n % v else [])
        want += [1] * n_tail
        got = [len(e[2]) for e in ev if e[0] == "wgrad"]
        assert got == want, "wgrad.list=%d: calls per fork %s, the option implies %s" % (value, got, want)
        groups = sum(1 for e in ev if e[0] == "group" and e[1] != "main")
        assert groups == 1
        forks = sum(1 for i, e in enumerate(ev) if e[0] == "wait" and e[1] != "main" and i > start)
        assert forks == len(want) + groups, (value, forks, want)


def test_no_side_stream_no_list(ledger):
    """Eager path without a side stream: the option changes nothing, every weight gradient runs on the chain's stream."""
    led = ledger
    net = engine.PoseNet("darknet_tiny_h", dtype=torch.bfloat16)
    assert net.wgrad.list_limit() == 0
    net.side_stream = Stream(led, "side0")
    with real_ops.option("wgrad.list", 4):
        assert net.wgrad.list_limit() == 4
        net.wgrad.tail = True
        assert net.wgrad.list_limit() == 0
    with real_ops.option("wgrad.list", 1):
        net.wgrad.tail = False
        assert net.wgrad.list_limit() == 0
