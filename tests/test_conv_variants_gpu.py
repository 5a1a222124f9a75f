"""Every compiled convolution kernel variant, once, against an exact reference: one test per row of
tests/conv_variant_cases.py (tests/test_conv_variant_cases_host.py proves on the CPU that the rows cover every entry of
every KD6D_CONV_*_TILES list of csrc/conv_plan.h).  A test pins the row's options, FAILS when the planner -- the same
header, built for the host, asked at this device's CU count -- would launch another kernel than the row declares, and
then runs the row's entry point twice: on small integers, where the fp32 result is exact in any summation order and
is compared with torch.equal, and on Gaussian inputs under the tolerances of the parity tests of test_kernels_gpu.py.
Forward and data gradient write into the leading rows of a NaN-filled buffer: nothing may stay NaN inside and nothing
may be written behind the last row.

The fused statistics are compared to the word: on narrow integers every accumulator's two int64 words must be the integer
sum of the fp64 reference times 2^32, per channel in every forward row and per (level, image, group) in the fwd_gstats rows
of STAT_ROWS, for the fp32 and for the bf16 store.  The fused instantiations have their rows there too: fwd_norm
(kd6d_conv2d_fwd_norm, GroupNorm and BatchNorm, with and without raw_out), fwd_block (replica rows, NORM = true) and fwd_xf
(BatchNorm on load, XF = true)."""
import pytest
import torch
import torch.nn.functional as F

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
               residual=pack_levels(epi["res"], dtype).to(dev), seg_scale=epi["seg_scale"].to(dev))
    for li, (g, r) in enumerate(zip(got, C.epilogue_reference(ref, epi))):
        C.check_random(g, r, dtype, True, "epilogue, level %d" % li)

    # the fused per-channel statistics: every forward variant but split-K (splitk_rule: no statistics) keeps them on the
    # same kernel.  To the word on narrow integers, for the fp32 and the bf16 store; on Gaussian inputs under a tolerance
    if not splitk:
        assert cout % 4 == 0
        name, v, _ = C.planned(planner, row, ncu, stats=1)
        assert (name, v) == (row.list, row.variant), "with statistics the planner would launch %s %s" % (name, v)
        _exact_stats(ops, row, geom, dev, 0, torch.float32)
        if dtype == torch.bfloat16:
            _exact_stats(ops, row, geom, dev, 0, torch.bfloat16)
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


def _words(stats, replicas=1):
    """The accumulators as [lo, hi] int64 words, replica rows added as integers (never through kd6d_acc_read: fp32)."""
    w = stats.view(torch.int64).cpu().view(replicas, -1, 2)
    return w.sum(0).tolist(), w


def _exact_stats(ops, row, geom, dev, groups, stored):
    """kd6d_conv2d_fwd on narrow integers with a shift, stored as `stored`: the result and every statistic exact."""
    B, cin, cout, k, stride, levels = row.case
    dtype = C.TORCH_DTYPE[row.dtype]
    what = "exact %s statistics, stored %s" % ("group" if groups else "per-channel", stored)
    inp, ref = C.narrow_inputs(row), C.narrow_reference(row)
    n = 2 * cout if groups == 0 else len(levels) * B * groups * 2
    stats = ops.acc_zeros(n, dev)
    buf, out = _guarded(geom.rows_out, cout, stored, dev)
    ops.conv2d_fwd(geom, pack_levels(inp["xs"], dtype).to(dev), w_to_krsc(inp["w"], dtype).to(dev), out=out,
                   ch_shift=inp["shift"].to(dev), out_f32=stored == torch.float32, stats=stats, stats_groups=groups)
    torch.cuda.synchronize()
    y = _landed(buf, geom.rows_out, what)
    for li, (g, r) in enumerate(zip(unpack_levels(y, B, geom.levels_out), ref)):
        C.check_integer(g, r, stored, "%s, level %d" % (what, li))
    rows = C.packed_rows(ref)
    C.check_stat_words(_words(stats)[0], C.channel_sums(rows) if groups == 0 else C.group_sums(rows, row, groups), what)


def _random_fwd(row):
    return C._random_inputs(C._key(row.case), "fwd", row.dtype), C._random_reference(C._key(row.case), "fwd", row.dtype)


def _run_gstats(ops, planner, row, dev, ncu):
    B, cin, cout, k, stride, levels = row.case
    dtype, G = C.TORCH_DTYPE[row.dtype], row.extra["groups"]
    name, v, plan = C.planned_stat(planner, row, ncu)
    assert (name, v) == (row.list, row.variant), "the planner would launch %s %s" % (name, v)
    geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    if "refused" in row.note:      # conv_plan.h stats_followup_ok: refused before anything is launched
        from kd6d._lib import Kd6dError
        inp = C.narrow_inputs(row)
        stats = ops.acc_zeros(len(levels) * B * G * 2, dev)
        buf, out = _guarded(geom.rows_out, cout, torch.float32, dev)
        with pytest.raises(Kd6dError, match="to divide 256"):
            ops.conv2d_fwd(geom, pack_levels(inp["xs"], dtype).to(dev), w_to_krsc(inp["w"], dtype).to(dev), out=out, out_f32=True,
                           stats=stats, stats_groups=G)
        torch.cuda.synchronize()
        assert torch.isnan(buf).all() and not stats.view(torch.int64).any(), "a refused call launched something"
        return
    _exact_stats(ops, row, geom, dev, G, torch.float32)
    if dtype == torch.bfloat16:
        _exact_stats(ops, row, geom, dev, G, torch.bfloat16)
    if row.list == "halo" and row.variant in C.HALO_TWINS:         # the twins have no forward row: per-channel sums here
        q = P.plan_conv(planner, P.Layer(*row.case), "fwd", P.BF16, stats=1, ncu=ncu, **C.plan_options(row))
        assert (q.family, q.BP, q.BC, q.WP, q.WC, q.HMAX, q.PDB) == (P.HALO,) + row.variant
        _exact_stats(ops, row, geom, dev, 0, torch.float32)
        _exact_stats(ops, row, geom, dev, 0, torch.bfloat16)
    # Gaussian inputs: the statistics against the sums of the tensor the call stored
    inp, ref = _random_fwd(row)
    shift = C.epilogue_inputs(row)["shift"]
    stats = ops.acc_zeros(len(levels) * B * G * 2, dev)
    buf, out = _guarded(geom.rows_out, cout, torch.float32, dev)
    ops.conv2d_fwd(geom, pack_levels(inp["xs"], dtype).to(dev), w_to_krsc(inp["w"], dtype).to(dev), out=out,
                   ch_shift=shift.to(dev), out_f32=True, stats=stats, stats_groups=G)
    torch.cuda.synchronize()
    y = _landed(buf, geom.rows_out, "random group statistics")
    C.check_stat_values(_words(stats)[0], C.group_sums(y, row, G), "random group statistics")
    for li, (g, r) in enumerate(zip(unpack_levels(y, B, geom.levels_out), ref)):
        C.check_random(g, r + shift.view(1, -1, 1, 1), dtype, False, "group-statistics call, level %d" % li)


def _run_norm(ops, planner, row, dev, ncu):
    """kd6d_conv2d_fwd_norm on narrow integers: raw_out and the statistics exact, the normalised result, save_mean,
    save_invstd and the running statistics against fp64 from the exact tensor (tolerances of test_conv_fwd_norm_group /
    _batch).  One launch with and one without raw_out."""
    B, cin, cout, k, stride, levels = row.case
    dtype, G, group = C.TORCH_DTYPE[row.dtype], row.extra["groups"], row.extra["norm"] == "group"
    name, v, plan = C.planned_stat(planner, row, ncu)
    assert (name, v) == (row.list, row.variant), "the planner would launch %s %s" % (name, v)
    geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    kind = ops.NORM_GROUP if group else ops.NORM_BATCH
    assert ops.conv_norm_fusable(geom, dtype, kind, G), "not a fused launch on this device"
    inp = C.narrow_inputs(row)
    gen = torch.Generator().manual_seed(cout + B)
    gamma, beta = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.2
    rm0, rv0 = torch.randn(cout, generator=gen) * 0.1, torch.rand(cout, generator=gen) + 0.5
    bias = inp["shift"] if group else None                           # (a ConvBlock's convolution has no bias)
    raws = [r if group else r - inp["shift"].double().view(1, -1, 1, 1) for r in C.narrow_reference(row)]
    rows = C.packed_rows(raws)
    if group:
        want = [F.relu(F.group_norm(r, G, gamma.double(), beta.double(), 1e-5)) for r in raws]
        sums = C.group_sums(rows, row, G)
    else:
        flat = rows.t().reshape(1, cout, -1, 1)
        rm, rv = rm0.double().clone(), rv0.double().clone()
        ybn = F.leaky_relu(F.batch_norm(flat, rm, rv, gamma.double(), beta.double(), True, 0.1, 1e-5), 0.1)
        want = unpack_levels(ybn.reshape(cout, -1).t(), B, geom.levels_out)
        sums = C.channel_sums(rows)
    xp, wk = pack_levels(inp["xs"], dtype).to(dev), w_to_krsc(inp["w"], dtype).to(dev)
    for with_raw in (True, False):
        what = "%s, %s raw_out" % (row.extra["norm"], "with" if with_raw else "without")
        stats = torch.zeros(ops.conv_norm_stats_floats(geom, kind, G), device=dev)
        ctr = torch.zeros(ops.conv_norm_counter_words(geom, kind), dtype=torch.int32, device=dev)
        ybuf, y = _guarded(geom.rows_out, cout, dtype, dev)
        rbuf, raw_out = _guarded(geom.rows_out, cout, torch.float32, dev)
        rmd, rvd = rm0.to(dev), rv0.to(dev)
        mean, invstd = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
        kw = dict(groups=G, bias=bias.to(dev)) if group else dict(running_mean=rmd, running_var=rvd, save_mean=mean, save_invstd=invstd)
        ops.conv2d_fwd_norm(geom, xp, wk, y, kind, gamma.to(dev), beta.to(dev), stats, ctr, ops.ACT_RELU if group else ops.ACT_LEAKY,
                            raw_out=raw_out if with_raw else None, **kw)
        torch.cuda.synchronize()
        assert ops.lib.kd6d_barrier_timeouts() == 0
        if with_raw:
            for li, (g, r) in enumerate(zip(unpack_levels(_landed(rbuf, geom.rows_out, what), B, geom.levels_out), raws)):
                C.check_integer(g, r, torch.float32, "%s: raw_out, level %d" % (what, li))
        else:
            assert torch.isnan(rbuf).all(), "%s: raw_out written although not passed" % what
        C.check_stat_words(_words(stats, 1 if group else ops.BN_REPLICAS)[0], sums, what)
        for li, (g, r) in enumerate(zip(unpack_levels(_landed(ybuf, geom.rows_out, what), B, geom.levels_out), want)):
            torch.testing.assert_close(g.double(), r.double(), msg=lambda m: "%s: y, level %d: %s" % (what, li, m), **C.tol(dtype, True))
        if not group:
            m_ref, v_ref = rows.mean(0), rows.var(0, unbiased=False)
            torch.testing.assert_close(mean.cpu().double(), m_ref, rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(invstd.cpu().double(), torch.rsqrt(v_ref + 1e-5), rtol=1e-3, atol=1e-4)
            torch.testing.assert_close(rmd.cpu().double(), rm, rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(rvd.cpu().double(), rv, rtol=1e-3, atol=1e-4)


def _run_block(ops, planner, row, dev, ncu):
    """kd6d_conv2d_fwd_block(bn = NULL) with replica rows: the NORM = true instantiation of the row's tile."""
    B, cin, cout, k, stride, levels = row.case
    dtype, R = C.TORCH_DTYPE[row.dtype], row.extra["replicas"]
    name, v, plan = C.planned_stat(planner, row, ncu)
    assert (name, v) == (row.list, row.variant), "the planner would launch %s %s" % (name, v)
    geom = ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    inp = C.narrow_inputs(row)
    raws = [r - inp["shift"].double().view(1, -1, 1, 1) for r in C.narrow_reference(row)]
    rnd, rnd_ref = _random_fwd(row)
    for what, src, ref in (("integer", inp, raws), ("random", rnd, rnd_ref)):
        stats = ops.acc_zeros(R * 2 * cout, dev)
        buf, out = _guarded(geom.rows_out, cout, torch.float32, dev)
        ops.conv2d_fwd_block(geom, pack_levels(src["xs"], dtype).to(dev), w_to_krsc(src["w"], dtype).to(dev), out, stats=stats,
                             stats_replicas=R)
        torch.cuda.synchronize()
        y = _landed(buf, geom.rows_out, what)
        total, per_replica = _words(stats, R)
        if what == "integer":
            for li, (g, r) in enumerate(zip(unpack_levels(y, B, geom.levels_out), ref)):
                C.check_integer(g, r, torch.float32, "integer pass, level %d" % li)
            C.check_stat_words(total, C.channel_sums(C.packed_rows(ref)), "replica rows added")
            # workgroup b adds to row b % R: with R workgroups or more every replica row holds a part of the sums of squares
            if plan.grid_x >= R:
                assert all(bool(per_replica[r, cout:].any()) for r in range(R)), "a replica row stayed empty"
        else:
            for li, (g, r) in enumerate(zip(unpack_levels(y, B, geom.levels_out), ref)):
                C.check_random(g, r, dtype, False, "random pass, level %d" % li)
            C.check_stat_values(total, C.channel_sums(y), "random pass, replica rows added")


def _run_xf(ops, planner, row, dev, ncu):
    """kd6d_conv2d_fwd_block with bn given (XF = true): block A, a 1x1 convolution of 8 channels on narrow integers, is exact
    in its output and its batch sums; block B normalises and activates A's output while it loads it."""
    B, cin, cout, k, stride, levels = row.case
    dtype, R = C.TORCH_DTYPE[row.dtype], row.extra["replicas"]
    name, v, plan = C.planned_stat(planner, row, ncu)
    assert (name, v) == (row.list, row.variant), "the planner would launch %s %s" % (name, v)
    arow = row._replace(case=(B, 8, cin, 1, 1, levels))
    ga, gb = ops.Geom(B, 8, cin, 1, 1, 0, levels), ops.Geom(B, cin, cout, k, stride, k // 2, levels)
    ainp = C.narrow_inputs(arow)
    araw = [r - ainp["shift"].double().view(1, -1, 1, 1) for r in C.narrow_reference(arow)]
    raw_a = torch.empty(ga.rows_out, cin, device=dev)
    sums_a = ops.acc_zeros(R * 2 * cin, dev)
    ops.conv2d_fwd_block(ga, pack_levels(ainp["xs"], dtype).to(dev), w_to_krsc(ainp["w"], dtype).to(dev), raw_a, stats=sums_a,
                         stats_replicas=R)
    torch.cuda.synchronize()
    arows = C.packed_rows(araw)
    assert torch.equal(raw_a.cpu(), arows.float()), "block A is not exact"
    C.check_stat_words(_words(sums_a, R)[0], C.channel_sums(arows), "block A")
    gen = torch.Generator().manual_seed(cin + 3 * cout)
    gamma, beta = torch.rand(cin, generator=gen) + 0.5, torch.randn(cin, generator=gen) * 0.2
    rm0, rv0 = torch.randn(cin, generator=gen) * 0.1, torch.rand(cin, generator=gen) + 0.5
    w = _random_fwd(row)[0]["w"]
    rmd, rvd = rm0.to(dev), rv0.to(dev)
    mean, invstd = torch.empty(cin, device=dev), torch.empty(cin, device=dev)
    z = torch.full((ga.rows_out, cin), 7.0, dtype=dtype, device=dev)
    buf, raw_b = _guarded(gb.rows_out, cout, torch.float32, dev)
    sums_b = ops.acc_zeros(R * 2 * cout, dev)
    ops.conv2d_fwd_block(gb, raw_a, w_to_krsc(w, dtype).to(dev), raw_b, stats=sums_b, stats_replicas=R, z_out=z,
                         bn_in=dict(sums=sums_a, replicas=R, gamma=gamma.to(dev), beta=beta.to(dev), act=ops.ACT_LEAKY, eps=1e-5,
                                    momentum=0.1, running_mean=rmd, running_var=rvd, save_mean=mean, save_invstd=invstd))
    torch.cuda.synchronize()
    # A's BatchNorm + LeakyReLU in fp64 from the exact tensor
    rm, rv = rm0.double().clone(), rv0.double().clone()
    zr = F.leaky_relu(F.batch_norm(arows.t().reshape(1, cin, -1, 1), rm, rv, gamma.double(), beta.double(), True, 0.1, 1e-5), 0.1)
    zs = z.float().cpu()
    torch.testing.assert_close(zs.double(), zr.reshape(cin, -1).t(), msg=lambda m: "z_out: %s" % m, **C.tol(dtype, True))
    torch.testing.assert_close(mean.cpu().double(), arows.mean(0), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(invstd.cpu().double(), torch.rsqrt(arows.var(0, unbiased=False) + 1e-5), rtol=1e-3, atol=1e-4)
    torch.testing.assert_close(rmd.cpu().double(), rm, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(rvd.cpu().double(), rv, rtol=1e-3, atol=1e-4)
    # B's raw output: the convolution of z_out AS STORED; its batch sums: the sums of the tensor it stored
    y = _landed(buf, gb.rows_out, "block B")
    for li, (g, zl) in enumerate(zip(unpack_levels(y, B, gb.levels_out), unpack_levels(zs, B, levels))):
        want = F.conv2d(zl.double(), w.double(), stride=stride, padding=k // 2)
        torch.testing.assert_close(g.double(), want, msg=lambda m: "block B, level %d: %s" % (li, m), **C.tol(dtype, False))
    C.check_stat_values(_words(sums_b, R)[0], C.channel_sums(y), "block B, replica rows added")


RUN = {"fwd": _run_fwd, "dgrad": _run_dgrad, "wgrad": _run_wgrad, "fwd_gstats": _run_gstats, "fwd_norm": _run_norm,
       "fwd_block": _run_block, "fwd_xf": _run_xf}


@pytest.mark.parametrize("rid", [r.id for r in C.ROWS + C.STAT_ROWS])
def test_conv_variant(gpu_device, planner, pin, rid):
    ops = _ops()
    row = C.BY_ID[rid]
    for name, value in row.options.items():
        pin(name, value)
    run = RUN[row.kind]
    run(ops, planner, row, gpu_device, ops.device_cu_count())
    torch.cuda.synchronize()
    assert ops.lib.kd6d_barrier_timeouts() == 0
