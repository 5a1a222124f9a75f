"""kd6d_conv2d_wgrad_list against kd6d_conv2d_wgrad, bit for bit: the transposing-weight-gradient rows of
tests/conv_variant_cases.py (the smallest ragged shapes the planner sends to each of the four variants, the
declined-though-forced fallbacks included) and one more two-level geometry, with and without a bias gradient, at two
cu_budget values, in lists of 1, 2, 3, 4 and 6 calls that put the entry with the largest LDS first, last and in the
middle.  Every call runs once on its own and once inside the list, into separately zeroed slabs and accumulators:
torch.equal on every slab (guard floats behind it included) and accumulator.  Lists with a call the list kernel does
not take (a narrow-family row, fp32 rows) must give the single launches' bits too, and one list of integer-valued
calls is compared exactly with a float64 reference, so that the test does not only stand on the old path."""
import pytest
import torch

import conv_plan_lib as P
import conv_variant_cases as C
from util_pack import pack_levels

pytestmark = pytest.mark.gpu

GUARD = 1024               # floats behind every slab
SENTINEL = -12345.0
BUDGETS = (0, 16)

TR = {}                    # variant BN -> rows
for _r in C.ROWS:
    if _r.list == "wgrad_tr":
        TR.setdefault(_r.variant[0], []).append(_r)
TWO_LEVEL = C.Row("two-level", "wgrad_tr", (128, 2, 2, 0, 0, 0), "wgrad", "bf16", {}, (2, 40, 72, 3, 1, [(11, 9), (6, 5)]), (0,), "")
SMALL = next(r for r in C.ROWS if r.list == "wgrad_small")
F32 = next(r for r in C.ROWS if r.list == "wgrad" and r.variant[0] == 64)

# lists by variant BN (128 has the largest LDS): first, last, in the middle; "2L" = the extra two-level geometry; (64, i)
# = the i-th of the four BN = 64 rows (three declined-though-forced fallbacks and the regular one; rows 2 and 3 are the
# 1x1 shapes of the table).  Every row of TR is in at least one list of several entries (test_every_row_is_listed).
LISTS = {
    "1": [128], "1b": [16], "1-1x1": [(64, 3)],
    "2-big-first": [128, 16], "2-big-last": [32, "2L"], "2-1x1": [(64, 2), (64, 3)],
    "3-big-middle": [64, 128, 32], "3-big-first": ["2L", 16, 64], "3-1x1-big-last": [(64, 3), (64, 2), 128],
    "4-big-last": [16, 32, 64, 128], "4-big-first": [128, 64, 32, 16], "4-big-middle": [32, "2L", 128, 16],
    "4-all-64": [(64, 0), (64, 1), (64, 2), (64, 3)], "4-1x1-big-middle": [(64, 2), 128, (64, 3), (64, 1)],
    "6": [64, 16, 128, 32, "2L", 64], "6-every-64": [(64, 3), "2L", (64, 2), (64, 1), 16, (64, 0)],
}


def _ops():
    from kd6d import ops
    return ops


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return P.build_lib(tmp_path_factory.mktemp("wgrad_list_gpu"))


def _rows(keys):
    """The rows of a list: (BN, i) names the i-th row of a variant; a bare BN takes the variant's rows in turn."""
    used, rows = {}, []
    for k in keys:
        if k == "2L":
            rows.append(TWO_LEVEL)
        elif isinstance(k, tuple):
            rows.append(TR[k[0]][k[1]])
        else:
            i = used.get(k, 0)
            used[k] = i + 1
            rows.append(TR[k][i % len(TR[k])])
    return rows


class Call:
    """One weight-gradient call with its own zeroed slab (+ guard floats) and bias accumulator."""

    def __init__(self, ops, row, dev, bias, budget, integer=False):
        B, cin, cout, k, stride, levels = row.case
        self.row, self.budget = row, budget
        self.dtype = C.TORCH_DTYPE[row.dtype]
        self.geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
        inp = C.integer_inputs(row) if integer else C.random_inputs(row)
        self.x = pack_levels(inp["xs"], self.dtype).to(dev)
        self.dy = pack_levels(inp["dys"], self.dtype).to(dev)
        self.nw = cout * k * k * cin
        self.parts = ops.conv2d_wgrad_parts(self.geom, self.dtype, bias, budget)
        self.bias, self.dev = bias, dev

    def fresh(self, ops):
        buf = torch.zeros(self.parts * self.nw + GUARD, dtype=torch.float32, device=self.dev)
        buf[self.parts * self.nw:] = SENTINEL
        acc = ops.planar_acc(self.geom.cout, self.dev) if self.bias else None
        return buf, acc

    def args(self, buf, acc):
        return dict(geom=self.geom, x=self.x, dy=self.dy, dw_slab=buf[:self.parts * self.nw], flops=0,
                    dbias=None if acc is None else acc[:self.geom.cout], acc_stride=self.geom.cout, cu_budget=self.budget)


def _both_ways(ops, calls):
    """[(slab + guard, acc)] of the single launches and of the list."""
    single = [c.fresh(ops) for c in calls]
    for c, (buf, acc) in zip(calls, single):
        a = c.args(buf, acc)
        ops.conv2d_wgrad(a["geom"], a["x"], a["dy"], a["dw_slab"], dbias=a["dbias"], acc_stride=a["acc_stride"],
                         cu_budget=a["cu_budget"])
    listed = [c.fresh(ops) for c in calls]
    ops.conv2d_wgrad_list([c.args(buf, acc) for c, (buf, acc) in zip(calls, listed)])
    torch.cuda.synchronize()
    return single, listed


def _same_bits(calls, single, listed):
    for i, (c, (b0, a0), (b1, a1)) in enumerate(zip(calls, single, listed)):
        what = "call %d (%s, bias %d, cu_budget %d)" % (i, c.row.id, c.bias, c.budget)
        n = c.parts * c.nw
        assert (b1[n:] == SENTINEL).all() and (b0[n:] == SENTINEL).all(), what + ": wrote behind its slab"
        assert torch.equal(b0, b1), what + ": the slab differs from the single launch's"
        assert b1[:n].abs().sum().item() > 0, what + ": nothing written"
        if c.bias:
            assert torch.equal(a0, a1), what + ": the bias accumulator differs"
            assert (a1 != 0).any(), what + ": no bias gradient"


def _check_planned(planner, ops, calls, in_force):
    """The host planner, at this device's CU count and under the options in force, sends every call where its row says."""
    for c in calls:
        row = c.row._replace(options=dict(in_force))
        name, v, plan = C.planned(planner, row, ops.device_cu_count(), c.budget)
        assert (name, v) == (c.row.list, c.row.variant), "%s: the planner would launch %s %s" % (c.row.id, name, v)


def test_every_row_is_listed():
    """Every transposing-weight-gradient row of the variant table runs inside a list of several entries."""
    multi = {r.id for keys in LISTS.values() if len(keys) > 1 for r in _rows(keys)}
    want = {r.id for rows in TR.values() for r in rows}
    assert len(want) == 7 and sorted(len(v) for v in TR.values()) == [1, 1, 1, 4]
    assert want <= multi, sorted(want - multi)
    assert any(r.case[3] == 1 for r in TR[64][2:]) and all(r.case[3] == 1 for r in TR[64][2:])      # the 1x1 shapes


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("bias", (False, True))
@pytest.mark.parametrize("name", list(LISTS))
def test_list_gives_the_single_launches_bits(gpu_device, planner, name, bias, budget):
    ops = _ops()
    calls = [Call(ops, r, gpu_device, bias, budget) for r in _rows(LISTS[name])]
    _check_planned(planner, ops, calls, {})
    single, listed = _both_ways(ops, calls)
    _same_bits(calls, single, listed)
    assert ops.lib.kd6d_barrier_timeouts() == 0


@pytest.mark.parametrize("pos", (0, 2, 4))
def test_list_with_calls_the_list_kernel_does_not_take(gpu_device, planner, pos):
    """A narrow-family row (option wgrad.small = 1, as the variant table runs it; no bias: that family takes none) and an
    fp32 row with a bias gradient among four listable calls."""
    ops = _ops()
    with ops.option("wgrad.small", 1):
        calls = [Call(ops, r, gpu_device, True, 16) for r in _rows([16, 128, 32, 64])]
        extra = [Call(ops, SMALL, gpu_device, False, 16), Call(ops, F32, gpu_device, True, 0)]
        _check_planned(planner, ops, calls + extra, {"wgrad.small": 1})
        calls[pos:pos] = extra
        single, listed = _both_ways(ops, calls)
    _same_bits(calls, single, listed)


def test_integer_list_is_exact(gpu_device):
    """Small integers: every partial sum is exact in fp32, so the parts add up to the float64 reference exactly."""
    ops = _ops()
    rows = _rows([16, 32, 64, 128])
    calls = [Call(ops, r, gpu_device, True, 16, integer=True) for r in rows]
    listed = [c.fresh(ops) for c in calls]
    ops.conv2d_wgrad_list([c.args(buf, acc) for c, (buf, acc) in zip(calls, listed)])
    torch.cuda.synchronize()
    for c, (buf, acc) in zip(calls, listed):
        B, cin, cout, k, stride, levels = c.row.case
        dw = buf[:c.parts * c.nw].view(c.parts, c.nw).double().sum(0).view(cout, k, k, cin).permute(0, 3, 1, 2).cpu()
        assert torch.equal(dw, C.integer_reference(c.row)), c.row.id
        db = torch.stack([dy.double().sum((0, 2, 3)) for dy in C.integer_inputs(c.row)["dys"]]).sum(0)
        assert torch.equal(ops.planar_acc_value(acc).double().cpu(), db), c.row.id + ": bias gradient"
