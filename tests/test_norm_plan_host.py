"""CPU: the launch rules of csrc/norm_ops.hip -- accepted channel counts, grids, dynamic LDS bytes, the one-launch
decisions of the BN / GN backwards, the GN backward workspace -- built for the host with g++ from the SAME header the
launchers include (csrc/norm_plan.h through tests/norm_plan_host.cpp)."""
import ctypes

import pytest

import norm_plan_lib

LL = ctypes.c_longlong
DTYPES = [("bf16", 8), ("f32", 4)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return norm_plan_lib.build_lib(tmp_path_factory.mktemp("norm_plan"))


def _bn_plan(L, items, pooled=0, resident=768, counter=1, enabled=1, max_granules=1 << 40):
    out = (ctypes.c_int * 3)()
    L.np_bn_onepass_plan(items, pooled, resident, counter, enabled, max_granules, out)
    return bool(out[0]), out[1], out[2]


def _gn_plan(L, C, eg, levels, resident, factor):
    out = (ctypes.c_int * 3)()
    L.np_gn_onepass_plan(C, eg, (ctypes.c_int32 * len(levels))(*levels), len(levels), resident, factor, out)
    return out[0], out[1], bool(out[2])


def _ceil(a, b):
    return -(-a // b)


def _accepted(L, eg, rule):
    return [C for C in range(1, eg * 256 + 1) if getattr(L, rule)(C, eg)]


def test_constants_and_channel_rules(plan):
    assert plan.k == {"threads": 256, "flush_lds": 16384, "bn_hold": 4, "pool_hold": 2, "gn_hold": 8, "bn_blocks": 512,
                      "colstats_cap": 128, "bn_reduce_cap": 512, "gn_bwd_max_c": 512}
    assert plan.np_granule_width(1) == 8 and plan.np_granule_width(0) == 4
    for _, eg in DTYPES:
        ok = _accepted(plan, eg, "np_channels_ok")
        assert ok == [eg * d for d in (1, 2, 4, 8, 16, 32, 64, 128, 256)]           # C/eg divides 256
        assert _accepted(plan, eg, "np_colstats_channels_ok") == list(range(eg, eg * 256 + 1, eg))
        for C in (0, -eg, eg * 256 + eg, eg * 512):
            assert not plan.np_channels_ok(C, eg) and not plan.np_colstats_channels_ok(C, eg)
    assert all(plan.np_colstats_channels_ok(C, 8) and not plan.np_channels_ok(C, 8) for C in (40, 120, 240))


def test_grids(plan):
    for n, want in ((0, 1), (1, 1), (256, 1), (257, 2), (2048 * 256, 2048), (2048 * 256 + 1, 2048), (1 << 40, 2048)):
        assert plan.np_grid_for(n) == want
    # 8 granules per thread unpooled, 2 windows per thread pooled, at most 512 workgroups
    for n in (1, 2048, 2049, 512 * 2048, 512 * 2048 + 1, 1 << 33):
        assert plan.np_bn_bwd_reduce_grid(n) == min(max(_ceil(n, 256 * 8), 1), 512)
        assert plan.np_bn_pool_bwd_reduce_grid(n) == min(max(_ceil(n, 256 * 2), 1), 512)
    # colstats: 8 passes of 256 // cgs rows per workgroup, at most 128 workgroups
    for cgs in (1, 5, 15, 16, 30, 256):
        for rows in (1, 8 * (256 // cgs), 8 * (256 // cgs) + 1, 10 ** 7):
            assert plan.np_colstats_grid(rows, cgs) == min(_ceil(rows, 8 * (256 // cgs)), 128)


def _flush_nparts(C, eg):
    """block_channel_flush, read off the kernel: partial sums per channel (`pre`: DPP rotations leave one per 16-lane row)"""
    cgs = C // eg
    return 16 if (cgs < 16 and 16 % cgs == 0) else 256 // cgs


def _flush_need(C, eg, nacc):
    """fp32 slots [nparts][nacc * C], or nacc * C two-word LDS accumulators beyond 16 partials"""
    nparts = _flush_nparts(C, eg)
    return nacc * C * 16 if nparts > 16 else nparts * nacc * C * 4


def test_lds_need_of_every_accepted_channel_count_fits_what_is_launched(plan):
    flush = plan.k["flush_lds"]
    slot_max = acc_max = 0
    for _, eg in DTYPES:
        for C in _accepted(plan, eg, "np_colstats_channels_ok"):      # a superset of what the BN / GN entry points accept
            for nacc in (1, 2):
                need = plan.np_flush_lds_bytes(C, eg, nacc)
                assert need == _flush_need(C, eg, nacc), (C, eg, nacc)
                assert 0 < need <= flush, (C, eg, nacc, need)
                if _flush_nparts(C, eg) > 16:
                    acc_max = max(acc_max, need)
                else:
                    slot_max = max(slot_max, need)
        for C in _accepted(plan, eg, "np_channels_ok"):
            # BN backward apply: the unpooled launcher passes exactly the need, the pooled one kFlushLdsBytes
            assert plan.np_bn_apply_lds_bytes(C) == 2 * C * 4 <= flush
            # BN one-launch kernels: the flush, then the totals in the same space; launched with kFlushLdsBytes
            one = plan.np_bn_onepass_lds_bytes(C, eg)
            assert one == max(_flush_need(C, eg, 2), 2 * C * 4) <= flush
            # GN backward (reduce and one-pass): red[4 * C] 64-bit words, launched with kFlushLdsBytes
            gn = plan.np_gn_bwd_lds_bytes(C)
            assert gn == 32 * C
            assert (gn <= flush) == (C <= 512) == (C <= plan.k["gn_bwd_max_c"]), C
    assert slot_max == 256 * 8 * 2 * 4 == flush        # 256 threads x 2 sums x 8 channels, fp32 slots
    assert acc_max == 32 * 120                         # C = 120 (bf16): 17 partials per channel, two accumulators each


def test_bn_one_launch_rule_matches_the_header_wording(plan):
    """include/kd6d.h: "512 workgroups x 4 granules per thread", default limit bn.onepass_max granules."""
    full = 512 * 256 * 4
    assert _bn_plan(plan, 1) == (True, 1, 1)
    assert _bn_plan(plan, full) == (True, 512, 4)
    assert _bn_plan(plan, full + 1) == (False, 0, 0)
    for resident, cap in ((768, 512), (100, 75), (683, 512), (682, 511), (1, 0), (0, 0), (-256, 0)):
        for n in (1, 511, 512, 513, 65536, 65537, 131072, 75 * 1024, 75 * 1024 + 1, full - 1, full, full + 1):
            for mx in (65536, 1 << 40):
                taken, grid, per = _bn_plan(plan, n, resident=resident, max_granules=mx)
                assert taken == (cap > 0 and n <= cap * 256 * 4 and n <= mx), (resident, n, mx)
                if taken:
                    assert grid == min(_ceil(n, 512), cap) and per == _ceil(n, grid * 256)
                    assert 1 <= per <= 4 and grid * 256 * per >= n
    # no device (query failed), no counter, option bn.onepass = 0, nothing to do
    assert not _bn_plan(plan, 4096, resident=0)[0]
    assert not _bn_plan(plan, 4096, counter=0)[0]
    assert not _bn_plan(plan, 4096, enabled=0)[0]
    assert not _bn_plan(plan, 0)[0] and not _bn_plan(plan, -5)[0]
    assert _bn_plan(plan, 4096) == (True, 8, 2)


def test_bn_one_launch_rule_pooled(plan):
    """work item = 2x2 window: 2 windows per thread at most, one while the device has room, 4 input granules each"""
    full = 512 * 256 * 2
    assert _bn_plan(plan, full, pooled=1) == (True, 512, 2)
    assert _bn_plan(plan, full + 1, pooled=1) == (False, 0, 0)
    for n in (1, 255, 256, 257, 16384, 16385, 512 * 256, 512 * 256 + 1, full):
        for mx in (65536, 1 << 40):
            taken, grid, per = _bn_plan(plan, n, pooled=1, max_granules=mx)
            assert taken == (n <= full and n * 4 <= mx), (n, mx)
            if taken:
                assert grid == min(_ceil(n, 256), 512) and per == _ceil(n, grid * 256) and per <= 2
    assert _bn_plan(plan, 16384, pooled=1, max_granules=65536)[0] and not _bn_plan(plan, 16385, pooled=1, max_granules=65536)[0]
    assert not _bn_plan(plan, 1024, pooled=1, resident=0)[0] and not _bn_plan(plan, 1024, pooled=1, counter=0)[0]
    assert not _bn_plan(plan, 1024, pooled=1, enabled=0)[0]


def test_gn_one_pass_plan(plan):
    levels = [32 * 32, 16 * 16, 8 * 8, 3 * 3, 1]
    for cgs, chunk in ((1, 128), (8, 128), (16, 128), (32, 64), (64, 32), (128, 16), (256, 8)):
        for _, eg in DTYPES:
            siblings = 32 * 32 // chunk                       # of the 32x32 level, the largest
            for factor in (2, 4):
                assert _gn_plan(plan, cgs * eg, eg, levels, siblings * factor, factor) == (chunk, siblings, True)
                assert _gn_plan(plan, cgs * eg, eg, levels, siblings * factor - 1, factor) == (chunk, siblings, False)
            assert _gn_plan(plan, cgs * eg, eg, levels, 0, 2) == (chunk, siblings, False)      # query failed
    assert _gn_plan(plan, 256, 8, [6 * 6, 3 * 3, 1], 2, 2) == (64, 1, True)
    assert _gn_plan(plan, 256, 8, [65], 4, 2) == (64, 2, True)            # a ragged last chunk is a sibling too


@pytest.mark.parametrize("levels,batch,groups", [(1, 1, 1), (5, 16, 32), (3, 2, 32), (5, 128, 32), (2, 7, 64), (8, 3, 4)])
def test_gn_backward_workspace_layout_matches_the_python_copy(plan, levels, batch, groups):
    from kd6d import ops
    out = (LL * 3)()
    plan.np_gn_bwd_workspace(levels, batch, groups, out)
    sums, counters, total = out
    assert total == ops.gn_bwd_workspace_floats(levels, batch, groups) * 4
    assert counters == sums == 2 * levels * batch * groups * 16          # the counters start behind that many kd6d_acc
    assert counters == (ops.gn_bwd_workspace_floats(levels, batch, groups) - levels * batch) * 4
    assert total - counters == 4 * levels * batch                        # one 32-bit counter per (level, image)
