"""The grouped weight gradient (csrc/conv_wgrad_group.hip through ops.WgradGroup) at every tile variant and loader edge:
one test per launch of tests/wgrad_group_cases.py (tests/test_wgrad_group_cases_host.py proves on the CPU, through the
real planner, what the launches reach).  Every test runs its group

  on small integers    dW (from 5) and dbias (from 7) equal conv2d_weight / the column sums in fp64 bit for bit; a second
                       launch of the same group onto the same outputs -- a plan-cache hit -- leaves 5 + 2 * the sums;
  on Gaussian inputs   under the tolerance of test_wgrad_group_matches_torch, twice from identical outputs with bitwise
                       equal results: the summation order is FIXED (ordered partial tiles, one ordered sum per element,
                       no atomics), so two executions of a launch may not differ in a single bit.

x and dY are views in the middle of larger allocations whose other rows are NaN: a fetch outside the tensor that the
buffer descriptor does not answer with zeros poisons the result.  dW and dbias are views inside buffers filled with a
sentinel, which must come back bit-identical: the reduce kernel writes no channel beyond cout.  The integer results of a
case are the same tensor at every workgroup count.  test_plan_cache_keeps_geometry_apart covers the launcher's cache."""
import pytest
import torch

import wgrad_group_cases as C
from util_pack import pack_levels, unpack_levels

pytestmark = pytest.mark.gpu

GUARD_ROWS = 136          # NaN pixel rows either side of x / dY: more than a step (64 positions) plus its look-back and -ahead
GUARD_FLOATS = 1024       # sentinel floats either side of dW / dbias (a multiple of 4: the views stay 16-byte aligned)
SENTINEL = -123456.75
NAN = float("nan")

_integer_results = {}     # case name -> (workgroup count, [(dW, dbias)]) of the first launch that ran: the same at every count


def _ops():
    from kd6d import ops
    return ops


def _guarded_input(levels_nchw, dev):
    """(whole allocation, the packed (rows, C) tensor as a view in its middle); NaN around it."""
    packed = pack_levels(levels_nchw, torch.bfloat16)
    buf = torch.full((packed.shape[0] + 2 * GUARD_ROWS, packed.shape[1]), NAN, dtype=torch.bfloat16, device=dev)
    view = buf[GUARD_ROWS:GUARD_ROWS + packed.shape[0]]
    view.copy_(packed)
    return buf, view


def _guarded_output(shape, extra, dev):
    """(whole allocation, the view handed to the kernel, its `shape` part): sentinel everywhere; the view is `extra`
    elements longer than the part the kernel may write."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + extra + 2 * GUARD_FLOATS,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[GUARD_FLOATS:GUARD_FLOATS + n + extra], buf[GUARD_FLOATS:GUARD_FLOATS + n].view(shape)


def _sentinels_intact(buf, n, what):
    bits = buf.cpu().view(torch.int32)
    want = torch.tensor([SENTINEL]).view(torch.int32)[0]
    keep = torch.ones(bits.numel(), dtype=torch.bool)
    keep[GUARD_FLOATS:GUARD_FLOATS + n] = False
    bad = ((bits != want) & keep).nonzero()
    assert len(bad) == 0, "%s: %d elements outside the result were written, first at offset %d" % (
        what, len(bad), int(bad[0]) - GUARD_FLOATS)


class _Launch:
    """The tensors of one case on the device, and the group that runs them."""

    def __init__(self, ops, case, n_workgroups, inputs, dev):
        self.case = case
        self.group = ops.WgradGroup(n_workgroups)
        self.items = []
        for (cin, cout, k, bias), inp in zip(case.items, inputs):
            geom = ops.Geom(case.B, cin, cout, k, 1, k // 2, case.levels)
            assert ops.wgrad_group_supported(geom, torch.bfloat16)
            xbuf, x = _guarded_input(inp["xs"], dev)
            dybuf, dy = _guarded_input(inp["dys"], dev)
            dwbuf, dwv, dw = _guarded_output((cout, k, k, cin), 0, dev)
            dbbuf, dbv, db = _guarded_output((cout,), 24, dev) if bias else (None, None, None)
            self.items.append(dict(geom=geom, xbuf=xbuf, x=x, dybuf=dybuf, dy=dy, dwbuf=dwbuf, dwv=dwv, dw=dw, dbbuf=dbbuf,
                                   dbv=dbv, db=db))

    def reset(self, dw0, db0):
        for it in self.items:
            it["dw"].fill_(dw0)
            if it["db"] is not None:
                it["db"].fill_(db0)

    def run(self):
        """One launch pair; [(dW, dbias or None)] on the host, once the sentinels are seen untouched."""
        for it in self.items:
            self.group.add(it["geom"], it["x"], it["dy"], it["dwv"], it["dbv"])
        assert len(self.group) == len(self.items)
        self.group.launch()
        torch.cuda.synchronize()
        assert len(self.group) == 0
        out = []
        for i, it in enumerate(self.items):
            _sentinels_intact(it["dwbuf"], it["dw"].numel(), "%s item %d dW" % (self.case.name, i))
            if it["db"] is not None:
                _sentinels_intact(it["dbbuf"], it["db"].numel(), "%s item %d dbias" % (self.case.name, i))
            out.append((it["dw"].cpu().clone(), None if it["db"] is None else it["db"].cpu().clone()))
        return out


@pytest.mark.parametrize("name,n_workgroups", C.LAUNCHES)
def test_wgrad_group_case(gpu_device, name, n_workgroups):
    ops, case = _ops(), C.BY_NAME[name]
    what = "%s at %d workgroups" % (name, n_workgroups)

    # ---- integers: exact, and exact again on top of the first result through the cached plan
    run = _Launch(ops, case, n_workgroups, C.integer_inputs(case), gpu_device)
    ref = C.integer_reference(case)
    run.reset(C.DW0, C.DB0)
    first = run.run()
    for times, got in ((1, first), (2, run.run())):
        for i, ((dw, db), (rdw, rdb)) in enumerate(zip(got, ref)):
            C.check_integer(dw, C.DW0 + times * rdw, "%s, launch %d, item %d dW (cout, ky, kx, cin)" % (what, times, i))
            if db is not None:
                C.check_integer(db, C.DB0 + times * rdb, "%s, launch %d, item %d dbias" % (what, times, i))
    assert len(run.group._plans) == 1, "the second launch of the same tensors planned again"
    n0, seen = _integer_results.setdefault(name, (n_workgroups, first))
    for i, ((dw, db), (sdw, sdb)) in enumerate(zip(first, seen)):
        assert torch.equal(dw, sdw) and (db is None or torch.equal(db, sdb)), "%s: item %d differs from %d workgroups" % (what, i, n0)

    # ---- Gaussian inputs on fresh outputs, twice from the same initial values
    run = _Launch(ops, case, n_workgroups, C.random_inputs(case), gpu_device)
    ref = C.random_reference(case)
    run.reset(0.25, 0.5)
    got = run.run()
    worst = 0.0
    for i, ((dw, db), (rdw, rdb)) in enumerate(zip(got, ref)):
        worst = max(worst, C.random_error(dw - 0.25, rdw), 0.0 if db is None else C.random_error(db - 0.5, rdb))
    print("%s: largest error of the random pass = %.2e of the tolerance" % (what, worst))
    for i, ((dw, db), (rdw, rdb)) in enumerate(zip(got, ref)):
        C.check_random(dw - 0.25, rdw, "%s, random pass, item %d dW" % (what, i))
        if db is not None:
            C.check_random(db - 0.5, rdb, "%s, random pass, item %d dbias" % (what, i))
    run.reset(0.25, 0.5)
    for i, ((dw, db), (dw2, db2)) in enumerate(zip(got, run.run())):
        assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)), "%s: two executions differ, item %d" % (what, i)
    assert len(run.group._plans) == 1
    assert ops.lib.kd6d_barrier_timeouts() == 0


def test_plan_cache_keeps_geometry_apart(gpu_device):
    """One group, one set of buffers, three geometries of 32 pixel rows per image in turn: every launch computes ITS
    geometry's gradient.  (A plan cache keyed on the pointers and the row total alone replays the first plan.)"""
    ops, dev = _ops(), gpu_device
    B, cin, cout, k = 2, 128, 16, 3
    g = torch.Generator().manual_seed(4242)
    x = torch.randint(-3, 4, (B * 32, cin), generator=g).float()
    dy = torch.randint(-3, 4, (B * 32, cout), generator=g).float()
    xd, dyd = x.to(dev, torch.bfloat16), dy.to(dev, torch.bfloat16)
    dw = torch.empty(cout, k, k, cin, device=dev)
    db = torch.empty(cout, device=dev)
    group = ops.WgradGroup(8)
    item = (cin, cout, k, True)
    refs = []
    for levels in ([(4, 8)], [(8, 4)], [(4, 4), (4, 4)], [(4, 8)]):
        rdw, rdb = C.reference_item(item, unpack_levels(x, B, levels), unpack_levels(dy, B, levels))
        assert all(not torch.equal(rdw, other) for lv, other in refs if lv != levels)      # the geometries do differ
        refs.append((levels, rdw))
        dw.fill_(C.DW0)
        db.fill_(C.DB0)
        group.add(ops.Geom(B, cin, cout, k, 1, 1, levels), xd, dyd, dw, db)
        group.launch()
        torch.cuda.synchronize()
        assert len(group) == 0
        C.check_integer(dw.cpu(), C.DW0 + rdw, "levels %s, dW (cout, ky, kx, cin)" % levels)
        C.check_integer(db.cpu(), C.DB0 + rdb, "levels %s, dbias" % levels)
    assert len(group._plans) == 3           # ... and the first geometry, asked for again, found its plan
