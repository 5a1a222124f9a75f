"""Every compiled convolution kernel variant, once, against an exact reference: one test per row of
tests/conv_variant_cases.py (tests/test_conv_variant_cases_host.py proves on the CPU that the rows cover every entry of
every KD6D_CONV_*_TILES list of csrc/conv_plan.h).  A test pins the row's options, FAILS when the planner -- the same
header, built for the host, asked at this device's CU count -- would launch another kernel than the row declares, and
then runs the row's entry point twice: on small integers, where the fp32 result is exact in any summation order and
is compared with torch.equal, and on Gaussian inputs under the tolerances of the parity tests of test_kernels_gpu.py.
Forward and data gradient write into the leading rows of a NaN-filled buffer: nothing may stay NaN inside and nothing
may be written behind the last row."""
import pytest
import torch

import conv_plan_lib as P
import conv_variant_cases as C
from util_pack import pack_levels, unpack_levels, w_to_dgrad, w_to_krsc

pytestmark = pytest.mark.gpu

GUARD_ROWS = 300          # more than the tallest tile (256 pixels) behind the last destination row
NAN = float("nan")


def _ops():
    from kd6d import ops
    return ops


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return P.build_lib(tmp_path_factory.mktemp("conv_variants_gpu"))


@pytest.fixture
def pin():
    """pin(name, value): kd6d_set_option for the rest of this test."""
    ops, old = _ops(), []

    def set_(name, value):
        old.append((name, ops.get_option(name)))
        ops.set_option(name, value)
    yield set_
    while old:
        ops.set_option(*old.pop())


def _guarded(rows, cols, dtype, dev, fill=None):
    """(the whole buffer, its leading `rows` rows): NaN everywhere, or `fill` in the leading rows."""
    buf = torch.full((rows + GUARD_ROWS, cols), NAN, dtype=dtype, device=dev)
    if fill is not None:
        buf[:rows] = fill
    return buf, buf[:rows]


def _landed(buf, rows, what):
    """The destination rows on the host, once the guard rows are seen untouched and no destination element is left unwritten."""
    got = buf.float().cpu()
    assert torch.isnan(got[rows:]).all(), "%s: wrote behind the last destination row" % what
    holes = torch.isnan(got[:rows]).nonzero()
    assert len(holes) == 0, "%s: %d destination elements never written, first %s" % (what, len(holes), holes[0].tolist())
    return got[:rows]


def _run_fwd(ops, planner, row, dev, ncu):
    B, cin, cout, k, stride, levels = row.case
    dtype = C.TORCH_DTYPE[row.dtype]
    name, v, plan = C.planned(planner, row, ncu)
    assert (name, v) == (row.list, row.variant), "the planner would launch %s %s" % (name, v)
    geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    rows = geom.rows_out
    splitk = row.list == "splitk"

    def call(xp, wp, what, **kw):
        ws = torch.full((C.splitk_ws_floats(row),), NAN, device=dev) if splitk else None
        buf, out = _guarded(rows, cout, torch.float32 if kw.get("out_f32") else dtype, dev)
        ops.conv2d_fwd(geom, xp, wp, out=out, workspace=ws, **kw)
        torch.cuda.synchronize()
        if splitk:        # exactly the planned number of slabs was written
            n = plan.nsplit * rows * cout
            assert not torch.isnan(ws[:n]).any() and torch.isnan(ws[n:]).all(), "%s: not %d split-K slabs" % (what, plan.nsplit)
        return unpack_levels(_landed(buf, rows, what), B, geom.levels_out)

    inp = C.integer_inputs(row)
    got = call(pack_levels(inp["xs"], dtype).to(dev), w_to_krsc(inp["w"], dtype).to(dev), "integer", out_f32=True)
    for li, (g, r) in enumerate(zip(got, C.integer_reference(row))):
        C.check_integer(g, r, torch.float32, "integer pass, level %d (B, cout, h, w)" % li)

    inp, ref = C.random_inputs(row), C.random_reference(row)
    xp, wp = pack_levels(inp["xs"], dtype).to(dev), w_to_krsc(inp["w"], dtype).to(dev)
    for li, (g, r) in enumerate(zip(call(xp, wp, "random", out_f32=True), ref)):
        C.check_random(g, r, dtype, False, "random pass, level %d" % li)

    # scale, shift, leaky ReLU and a residual fused behind the tile, stored in the activation dtype
    epi = C.epilogue_inputs(row)
    got = call(xp, wp, "epilogue", ch_scale=epi["scale"].to(dev), ch_shift=epi["shift"].to(dev), act=1,
               residual=pack_levels(epi["res"], dtype).to(dev))
    for li, (g, r) in enumerate(zip(got, C.epilogue_reference(ref, epi))):
        C.check_random(g, r, dtype, True, "epilogue, level %d" % li)

    # the fused per-channel statistics, where they stay on this variant: sums over the stored fp32 result
    if cout % 4 == 0 and C.planned(planner, row, ncu, stats=1)[:2] == (row.list, row.variant):
        stats = ops.acc_zeros(2 * cout, dev)
        buf, out = _guarded(rows, cout, torch.float32, dev)
        ops.conv2d_fwd(geom, xp, wp, out=out, ch_shift=epi["shift"].to(dev), out_f32=True, stats=stats, stats_groups=0)
        torch.cuda.synchronize()
        y = _landed(buf, rows, "statistics")
        st = ops.acc_read(stats, 2 * cout, ops.ACC_ACT).cpu().double()
        want = torch.cat([y.double().sum(0), (y.double() ** 2).sum(0)])
        torch.testing.assert_close(st, want, rtol=1e-4, atol=1e-4 * max(float(want.abs().max()), 1.0))
        for li, (g, r) in enumerate(zip(unpack_levels(y, B, geom.levels_out), ref)):
            C.check_random(g, r + epi["shift"].view(1, -1, 1, 1), dtype, False, "statistics call, level %d" % li)


def _run_dgrad(ops, planner, row, dev, ncu):
    B, cin, cout, k, stride, levels = row.case
    dtype = C.TORCH_DTYPE[row.dtype]
    name, v, plan = C.planned(planner, row, ncu)
    assert (name, v) == (row.list, row.variant), "the planner would launch %s %s" % (name, v)
    geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    rows = geom.rows_in
    for what, inp, ref in (("integer", C.integer_inputs(row), C.integer_reference(row)),
                           ("random", C.random_inputs(row), C.random_reference(row))):
        dyp, wt = pack_levels(inp["dys"], dtype).to(dev), w_to_dgrad(inp["w"], dtype).to(dev)
        buf, dx = _guarded(rows, cin, dtype, dev)
        ops.conv2d_dgrad(geom, dyp, wt, dx=dx)
        buf_acc, dx_acc = _guarded(rows, cin, dtype, dev, fill=pack_levels(inp["dx0"], dtype).to(dev))
        ops.conv2d_dgrad(geom, dyp, wt, dx=dx_acc, accumulate=True)
        torch.cuda.synchronize()
        got = unpack_levels(_landed(buf, rows, what), B, levels)
        got_acc = unpack_levels(_landed(buf_acc, rows, what + ", accumulate"), B, levels)
        for li, (g, ga, r, d0) in enumerate(zip(got, got_acc, ref, inp["dx0"])):
            if what == "integer":
                C.check_integer(g, r, dtype, "integer pass, level %d (B, cin, h, w)" % li)
                C.check_integer(ga, r + d0.double(), dtype, "integer pass onto dx0, level %d (B, cin, h, w)" % li)
            else:
                C.check_random(g, r, dtype, True, "random pass, level %d" % li)
                C.check_random(ga, r + d0, dtype, True, "random pass onto dx0, level %d" % li)


def _run_wgrad(ops, planner, row, dev, ncu):
    B, cin, cout, k, stride, levels = row.case
    dtype = C.TORCH_DTYPE[row.dtype]
    geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    passes = []
    for inp, exact in ((C.integer_inputs(row), True), (C.random_inputs(row), False)):
        ref = C.integer_reference(row) if exact else C.random_reference(row)
        passes.append((pack_levels(inp["xs"], dtype).to(dev), pack_levels(inp["dys"], dtype).to(dev), ref, exact))
    for budget in row.budgets:
        name, v, plan = C.planned(planner, row, ncu, budget)
        assert (name, v) == (row.list, row.variant), "cu_budget %d: the planner would launch %s %s" % (budget, name, v)
        assert ops.conv2d_wgrad_parts(geom, dtype, False, budget) == plan.parts, budget
        for xp, dyp, ref, exact in passes:
            dw, _ = ops.conv2d_wgrad_f32(geom, xp, dyp, cu_budget=budget)
            torch.cuda.synchronize()
            got = dw.view(cout, k, k, cin).cpu().permute(0, 3, 1, 2)
            if exact:
                C.check_integer(got, ref, torch.float32, "integer pass, cu_budget %d (cout, cin, ky, kx)" % budget)
            else:
                C.check_random_wgrad(got, ref, "random pass, cu_budget %d" % budget)


@pytest.mark.parametrize("rid", [r.id for r in C.ROWS])
def test_conv_variant(gpu_device, planner, pin, rid):
    ops = _ops()
    row = C.BY_ID[rid]
    for name, value in row.options.items():
        pin(name, value)
    run = {"fwd": _run_fwd, "dgrad": _run_dgrad, "wgrad": _run_wgrad}[row.kind]
    run(ops, planner, row, gpu_device, ops.device_cu_count())
    torch.cuda.synchronize()
    assert ops.lib.kd6d_barrier_timeouts() == 0
