"""CPU: what tests/test_norm_kernels_gpu.py relies on, proved without a GPU.

  coverage     the tables of tests/norm_cases.py hold every channel class csrc/norm_plan.h accepts (the header built for
               the host, tests/norm_plan_lib.py), every class of block_channel_flush, and long rows that exceed their grid
               caps ACCORDING TO THE PLANNER; the GroupNorm rows satisfy the entry points' rules
  exactness    on every row marked exact each fp64 intermediate of the kernels' arithmetic survives a round trip through
               fp32, and the absolute running sums stay below 2^24 units
  references   the hand-written references agree with torch autograd in fp64
  comparisons  each one rejects a wrong result built on the CPU (one word off by a unit, a replica row left out, a tie
               routed to the last maximum, a group boundary shifted by a channel, the last row dropped, a write behind the
               last row) -- this stands in for mutating kernels on the GPU"""
import ctypes
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import norm_cases as N
import norm_plan_lib
from test_kernels_gpu import _tol


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return norm_plan_lib.build_lib(tmp_path_factory.mktemp("norm_cases"))


def _ceil(a, b):
    return -(-a // b)


def _nparts(cgs):
    """block_channel_flush: (`pre`, partial sums per channel)"""
    pre = cgs < 16 and 16 % cgs == 0
    return pre, 16 if pre else 256 // cgs


def _bn_plan(L, items, pooled):
    out = (ctypes.c_int * 3)()
    L.np_bn_onepass_plan(items, pooled, 768, 1, 1, 65536, out)       # 3 workgroups per CU x 256 CUs, the default limit
    return bool(out[0])


# ---- coverage ---------------------------------------------------------------------------------------------------------
def test_batchnorm_table_holds_every_accepted_channel_class(plan):
    for dtype, xf32 in N.COMBOS:
        eg = N.EG[dtype]
        accepted = [C for C in range(1, eg * 256 + 1) if plan.np_channels_ok(C, eg)]
        assert len(accepted) == 9
        mine = [r for r in N.BN_ROWS if (r.dtype, r.xf32) == (dtype, xf32)]
        assert sorted({r.C for r in mine}) == accepted
        for C in accepted:
            of_c = [r for r in mine if r.C == C]
            assert {64, 77} <= {r.rows for r in of_c}
            assert {r.act for r in of_c} == {N.ACT_NONE, N.ACT_RELU, N.ACT_LEAKY}
            assert {r.fill for r in of_c} == {"zero", "ints", "none"}
    assert {r.replicas for r in N.BN_ROWS} == {1, 3, 8, 9, 64}
    assert any(r.dtype == "bf16" and r.C == 2048 for r in N.BN_ROWS) and any(r.dtype == "f32" and r.C == 4 for r in N.BN_ROWS)
    names = [r.name for r in N.BN_ROWS + [N.BN_LONG]] + [r.name for r in N.POOL_BN_ROWS + [N.POOL_BN_LONG]]
    assert len(names) == len(set(names))
    for r in N.BN_ROWS + N.POOL_BN_ROWS:
        assert (r.mode == "tol") == (r.act == N.ACT_LEAKY), r.name
        rows = r.rows if isinstance(r, N.BnRow) else r.B * r.H * r.W
        assert r.mode != "exact" or (rows & (rows - 1) == 0 and rows <= 4096), r.name


def test_every_flush_class_is_in_a_table(plan):
    seen = {(N.EG[r.dtype], r.C // N.EG[r.dtype]) for r in N.BN_ROWS} | {(N.EG[r.dtype], r.C // N.EG[r.dtype]) for r in N.COLSTATS_ROWS}
    for eg in (8, 4):
        cgs_seen = {c for e, c in seen if e == eg}
        assert {1, 2, 4, 8} <= cgs_seen                                             # `pre`: 4, 3, 2, 1 DPP rotations
        assert {_nparts(c)[1] for c in cgs_seen if not _nparts(c)[0]} >= {16, 8, 4, 2, 1}      # slots
        lds = [c for c in cgs_seen if _nparts(c)[1] > 16]
        assert len(lds) >= 2, "LDS-accumulator classes (more than 16 partials per channel)"
        for c in cgs_seen:                                                          # the planner agrees on the class
            pre, nparts = _nparts(c)
            want = 2 * c * eg * 16 if nparts > 16 else nparts * 2 * c * eg * 4
            assert plan.np_flush_lds_bytes(c * eg, eg, 2) == want
            assert plan.np_colstats_channels_ok(c * eg, eg)
    assert any(256 % c and _nparts(c)[1] <= 16 for e, c in seen), "a slot class with idle threads (cgs 30)"
    assert {r.sumsq for r in N.COLSTATS_ROWS} == {True, False} and any(r.rows == 1 for r in N.COLSTATS_ROWS)


def test_long_rows_exceed_their_caps_according_to_the_planner(plan):
    r = N.BN_LONG
    ngran = r.rows * r.C // N.EG[r.dtype]
    assert _ceil(ngran, 4) > 2048 * 256 and plan.np_grid_for(_ceil(ngran, 4)) == 2048           # forward, backward apply
    assert ngran > 2048 * 256 * 4 and (r.rows - 77) * r.C // N.EG[r.dtype] == 2048 * 256 * 4     # the smallest such power of two + 77
    assert ngran > 512 * 256 * 8 and plan.np_bn_bwd_reduce_grid(ngran) == plan.k["bn_reduce_cap"] == 512
    assert not _bn_plan(plan, ngran, 0)
    c = [x for x in N.COLSTATS_ROWS if "long" in x.note]
    assert len(c) == 1
    cgs = c[0].C // N.EG[c[0].dtype]
    assert c[0].rows > 128 * 8 * (256 // cgs) and plan.np_colstats_grid(c[0].rows, cgs) == plan.k["colstats_cap"] == 128
    p = N.POOL_BN_LONG
    items = p.B * (p.H // 2) * (p.W // 2) * p.C // N.EG[p.dtype]
    assert items == 589824 > 2048 * 256 and plan.np_grid_for(items) == 2048
    assert items > 512 * 256 * 2 and plan.np_bn_pool_bwd_reduce_grid(items) == 512
    assert not _bn_plan(plan, items, 1)
    long_pool = [x for x in N.POOL_ROWS if "long" in x.note]
    assert len(long_pool) == 1
    q = long_pool[0]
    assert plan.np_grid_for(q.B * (q.H // 2) * (q.W // 2) * q.C // N.EG[q.dtype]) == 2048
    assert q.B * (q.H // 2) * (q.W // 2) * q.C // N.EG[q.dtype] > 2048 * 256
    # every other row is short enough for the one-launch backwards the GPU test expects (counter[0] > 0)
    for r in N.BN_ROWS:
        assert _bn_plan(plan, r.rows * r.C // N.EG[r.dtype], 0), r.name
    for r in N.POOL_BN_ROWS:
        assert _bn_plan(plan, r.B * (r.H // 2) * (r.W // 2) * r.C // N.EG[r.dtype], 1), r.name


def test_pooled_rows_and_pool_rows():
    for dtype, xf32 in N.COMBOS:
        mine = [r for r in N.POOL_BN_ROWS if (r.dtype, r.xf32) == (dtype, xf32)]
        assert {r.C for r in mine} == {N.EG[dtype], N.EG[dtype] << 4, N.EG[dtype] << 8}
        for C in {r.C for r in mine}:
            assert {(r.B, r.H, r.W) for r in mine if r.C == C} == {(1, 2, 2), (3, 4, 2), (2, 6, 10)}
    assert {r.act for r in N.POOL_BN_ROWS} == {N.ACT_NONE, N.ACT_RELU, N.ACT_LEAKY}
    assert any((r.H, r.W) == (2, 2) for r in N.POOL_ROWS) and any(r.C == N.EG[r.dtype] for r in N.POOL_ROWS)
    assert any((r.C // N.EG[r.dtype]) & (r.C // N.EG[r.dtype] - 1) for r in N.POOL_ROWS)           # cgs no power of two
    assert N.POOL_ODD.H % 2 == 1 and N.POOL_ODD.W % 2 == 1
    assert {(r.dtype, r.Cpad) for r in N.IMAGE_ROWS} == {("bf16", 8), ("bf16", 16), ("f32", 8), ("f32", 16)}
    assert any(r.Cimg == r.Cpad for r in N.IMAGE_ROWS) and all(r.B * r.H * r.W > 256 for r in N.IMAGE_ROWS)


def test_groupnorm_rows_satisfy_the_entry_points_rules(plan):
    names = [r.name for r in N.GN_ROWS]
    assert len(names) == len(set(names))
    for r in N.GN_ROWS:
        eg, cpg = N.EG[r.dtype], r.C // r.G
        assert r.C % r.G == 0 and 1 <= r.G <= 64 and plan.np_channels_ok(r.C, eg), r.name
        assert cpg * 2 >= eg, r.name
        assert cpg != 2 or r.dtype == "f32", r.name
        assert 1 <= len(r.levels) <= 5 and r.batch >= 1
        assert r.backward == (r.C <= plan.k["gn_bwd_max_c"]), r.name
    has = lambda f: any(f(r) for r in N.GN_ROWS)
    assert has(lambda r: r.C // r.G == 2 and r.G == 32) and has(lambda r: r.C // r.G == 2 and r.G == 64)
    assert has(lambda r: r.dtype == "bf16" and r.C // r.G == 4 and r.G == 32) and has(lambda r: r.dtype == "bf16" and r.C // r.G == 4 and r.G == 64)
    assert has(lambda r: r.dtype == "bf16" and r.C == 64 and r.backward)            # cgs 8: no fold
    assert has(lambda r: r.dtype == "bf16" and r.C == 512 and r.backward) and has(lambda r: (r.dtype, r.C, r.G) == ("bf16", 8, 2))
    assert has(lambda r: r.G == 1) and has(lambda r: r.C == 2048 and not r.backward)
    assert has(lambda r: len(r.levels) == 5 and 1 in r.levels) and has(lambda r: r.levels == (1,))
    assert has(lambda r: r.levels == (127, 128, 129)) and has(lambda r: r.batch == 1 and r.backward)
    assert has(lambda r: r.xf32)


# ---- exactness --------------------------------------------------------------------------------------------------------
def _survives_fp32(t):
    return torch.equal(t.float().double(), t)


def _check_bn_exactness(ref, mode, dtype, what):
    a1, a2 = ref["abs_sums"]
    assert float(a1.max()) < 2 ** 24 and float(a2.max()) < 2 ** 24, what      # running sums in units of 1 and of 1/4
    assert ref["min_pre"] >= 1.0 / 16, what                                    # the activation's branch is never in doubt
    keys = ("xhat", "pre", "d", "d_xhat", "s1", "s2", "sc", "sh") + (("k1", "k2", "t1", "t2", "t3", "dx") if mode == "exact" else ())
    for k in keys:
        assert _survives_fp32(ref["steps"][k]), (what, k)
    # dgamma / dbeta: det_value converts hi = S * 2^5 through fp32
    assert all(abs(Fraction(s) * 32) < 2 ** 24 and (Fraction(s) * 32).denominator == 1 for s in ref["sums"]), what


@pytest.mark.parametrize("row", [r for r in N.BN_ROWS + [N.BN_LONG] if r.mode != "tol"], ids=lambda r: r.name)
def test_batchnorm_rows_marked_exact_are_exact_in_fp32(row):
    inp = N.bn_inputs(row.rows, row.C)
    ref = N.bn_backward_ref(inp["x"], inp["dz"], inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], row.act)
    _check_bn_exactness(ref, row.mode, row.dtype, row.name)
    s1, s2 = N.column_sums(inp["x"])
    assert max(s2) < 2 ** 24
    fill = N.prefill(row.C, row.fill)
    if fill[0] is not None:               # += onto integers: still representable
        assert _survives_fp32(fill[0].double() + ref["s2"]) and _survives_fp32(fill[1].double() + ref["s1"])


@pytest.mark.parametrize("row", [r for r in N.POOL_BN_ROWS + [N.POOL_BN_LONG] if r.mode != "tol"], ids=lambda r: r.name)
def test_pooled_rows_marked_exact_are_exact_in_fp32(row):
    inp = N.pool_bn_inputs(row.B, row.H, row.W, row.C)
    ref = N.pool_bn_backward_ref(row, inp)
    _check_bn_exactness(ref, row.mode, row.dtype, row.name)
    # the activations the argmax compares are exact in the stored dtype: rounding cannot create or break a tie
    sc = inp["gamma"] * inp["invstd"]
    a = N.act_fwd(inp["x"].double() * sc + (inp["beta"] - inp["mean"] * sc), row.act)
    assert torch.equal(a.to(N.TORCH_DTYPE[row.dtype]).double(), a)


@pytest.mark.parametrize("row", N.GN_ROWS, ids=lambda r: r.name)
def test_groupnorm_rows_keep_their_margin_and_exact_sums(row):
    case = N.gn_case(row)
    ref = case["ref"]
    assert ref["margin"] > 1e-2                                   # the ReLU mask of the fp32 kernel is the fp64 one
    assert all(isinstance(v, int) and abs(v) < 2 ** 24 for v in ref["stats"])
    # dbeta and the first group sum: integers / half integers far below 2^24 units
    assert torch.equal(ref["dbeta"], ref["dbeta"].round()) and float(ref["dbeta"].abs().max()) < 2 ** 19
    first = ref["gsum"][0::2]
    assert all(float(2 * v).is_integer() and abs(v) < 2 ** 19 for v in first)
    # the words a host builds for STATS_READY are the ones an exact kernel leaves
    N.check_stat_words(N.words_of(ref["stats"]), ref["stats"], row.name)


# ---- references against torch autograd ----------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [N.ACT_NONE, N.ACT_LEAKY, N.ACT_RELU])
def test_batchnorm_reference_agrees_with_autograd(act):
    g = torch.Generator().manual_seed(act)
    rows, C = 77, 12
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * 2 + 0.5
    dz = torch.randn(rows, C, generator=g, dtype=torch.float64)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * torch.tensor([1.0, -1.0] * (C // 2), dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    t = F.batch_norm(xr, rm, rv, gr, br, True, 0.1, N.EPS)
    y = t if act == N.ACT_NONE else F.leaky_relu(t, 0.1) if act == N.ACT_LEAKY else F.relu(t)
    y.backward(dz)
    fwd = N.bn_forward_ref(x, gamma, beta, act)
    tight = dict(rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(fwd["y"], y.detach(), **tight)
    torch.testing.assert_close(fwd["running_mean"], rm, **tight)
    torch.testing.assert_close(fwd["running_var"], rv, **tight)
    bwd = N.bn_backward_ref(x, dz, fwd["mean"], fwd["invstd"], gamma, beta, act, exact=False)
    torch.testing.assert_close(bwd["dx"], xr.grad, **tight)
    torch.testing.assert_close(bwd["s2"], gr.grad, **tight)
    torch.testing.assert_close(bwd["s1"], br.grad, **tight)


def test_exact_and_fp64_sums_of_the_batchnorm_reference_agree():
    inp = N.bn_inputs(77, 24)
    args = [inp[k] for k in ("x", "dz", "mean", "invstd", "gamma", "beta")]
    for act in (N.ACT_NONE, N.ACT_RELU):
        a, b = N.bn_backward_ref(*args, act), N.bn_backward_ref(*args, act, exact=False, chunk=10)
        assert [float(v) for v in a["sums"]] == b["sums"] and torch.equal(a["dx"], b["dx"])


def test_groupnorm_reference_agrees_with_autograd():
    g = torch.Generator().manual_seed(3)
    levels, B, C, G = (6, 1, 4), 2, 12, 3
    rows = B * sum(levels)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * 1.5 + 0.2
    dz = torch.randn(rows, C, generator=g, dtype=torch.float64)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5) * torch.tensor([1.0, -1.0] * (C // 2), dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    ref = N.gn_ref(x, dz, gamma, beta, levels, B, G)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    r0 = 0
    for hw in levels:
        xr = x[r0:r0 + B * hw].reshape(B, hw, C).permute(0, 2, 1).clone().requires_grad_(True)       # (B, C, hw)
        y = F.relu(F.group_norm(xr, G, gr, br, N.EPS))
        y.backward(dz[r0:r0 + B * hw].reshape(B, hw, C).permute(0, 2, 1))
        torch.testing.assert_close(ref["y"][r0:r0 + B * hw].reshape(B, hw, C).permute(0, 2, 1), y.detach(), rtol=1e-9, atol=1e-9)
        torch.testing.assert_close(ref["dx"][r0:r0 + B * hw].reshape(B, hw, C).permute(0, 2, 1), xr.grad, rtol=1e-8, atol=1e-8)
        r0 += B * hw
    torch.testing.assert_close(ref["dgamma"], gr.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(ref["dbeta"], br.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(N.gn_pre(x, gamma, beta, levels, B, G).clamp_min(0), ref["y"], rtol=1e-12, atol=1e-12)


def test_pool_references_agree_with_torch_on_tie_free_inputs():
    g = torch.Generator().manual_seed(9)
    B, H, W, C = 2, 6, 10, 5
    x = torch.randperm(B * H * W * C, generator=g).double().reshape(B, H, W, C)        # no two values equal
    dy = torch.randn(B, H // 2, W // 2, C, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    y.backward(dy.permute(0, 3, 1, 2))
    best, arg = N.first_max(x)
    assert torch.equal(best, y.detach().permute(0, 2, 3, 1))
    assert torch.equal(N.route(arg, dy), xr.grad.permute(0, 2, 3, 1))
    b2, a2 = N.last_max(x)                                      # without ties both rules are the same
    assert torch.equal(b2, best) and torch.equal(a2, arg)
    odd = torch.randperm(2 * 7 * 5 * 3, generator=g).double().reshape(2, 7, 5, 3)
    assert torch.equal(N.first_max(odd)[0], F.max_pool2d(odd.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
    c = torch.randn(B, H // 2, W // 2, C, generator=g, dtype=torch.float64)
    assert torch.equal(N.upsample_ref(c), F.interpolate(c.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1))
    torch.testing.assert_close(N.sumpool_ref(x), F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 4, rtol=1e-12, atol=0)
    # the adjoint pair: <upsample(c), x> == <c, sumpool(x)>
    torch.testing.assert_close((N.upsample_ref(c) * x).sum(), (c * N.sumpool_ref(x)).sum(), rtol=1e-12, atol=0)


def test_first_maximum_in_row_major_window_order():
    a = torch.zeros(1, 2, 2, 4)
    a[0, :, :, 1] = torch.tensor([[1.0, 2.0], [2.0, 0.0]])        # taps 1 and 2 tie
    a[0, :, :, 2] = torch.tensor([[0.0, 0.0], [3.0, 3.0]])        # taps 2 and 3 tie
    a[0, :, :, 3] = torch.tensor([[0.0, 0.0], [0.0, 5.0]])
    assert N.first_max(a)[1].reshape(-1).tolist() == [0, 1, 2, 3]
    assert N.last_max(a)[1].reshape(-1).tolist() == [3, 2, 3, 3]
    img = torch.arange(2 * 3 * 2 * 2).float().reshape(2, 3, 2, 2)
    assert torch.equal(N.image_ref(img, 8).reshape(2, 2, 2, 8)[1, 1, 0, :4], torch.tensor([img[1, 0, 1, 0], img[1, 1, 1, 0], img[1, 2, 1, 0], 0.0]))


# ---- the comparisons reject wrong results -----------------------------------------------------------------------------
def _rejects(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_word_comparison_rejects_one_unit_and_takes_fractions():
    sums = [5, -3, Fraction(7, 4), Fraction(-9, 2), 0, 3 << 20]
    for unit in (N.UNIT_ACT, N.UNIT_GRAD):
        words = N.words_of(sums, unit)
        N.check_stat_words(words, sums, "good", unit)
        N.check_stat_words(words, [float(s) for s in sums], "floats that hold the sums exactly", unit)
        for i in range(len(sums)):
            for part, delta in ((0, 1), (0, -1), (1, 1)):
                bad = [list(w) for w in words]
                bad[i][part] += delta
                _rejects(N.check_stat_words, bad, sums, "off by one unit", unit)
        # any split of the same total over the two words is the same accumulator
        moved = [[lo + (1 << 47), hi - 1] for lo, hi in words]
        N.check_stat_words(moved, sums, "carry not normalised", unit)
    _rejects(N.check_stat_words, N.words_of(sums, 32), sums, "wrong unit", 52)
    _rejects(N.words_of, [Fraction(1, 3)], 52)


def test_comparisons_reject_a_missing_replica_row_and_a_dropped_last_row():
    row = next(r for r in N.BN_ROWS if r.replicas == 3)
    inp = N.bn_inputs(row.rows, row.C)
    args = [inp[k] for k in ("mean", "invstd", "gamma", "beta")]
    ref = N.bn_backward_ref(inp["x"], inp["dz"], *args, row.act)
    # what a correct kernel leaves: block b of 256 rows adds its sums into replica row b % 3
    R, C = row.replicas, row.C
    acc = torch.zeros(R, 2 * C, 2, dtype=torch.int64)
    for b, lo in enumerate(range(0, row.rows, 256)):
        part = N.bn_backward_ref(inp["x"][lo:lo + 256], inp["dz"][lo:lo + 256], *args, row.act)
        acc[b % R] += torch.tensor(N.words_of(part["sums"], N.UNIT_GRAD))
    split = lambda t: (t[:, :C].contiguous(), t[:, C:].contiguous())              # the two workspaces
    w1, w2 = split(acc)
    good = N.total_words(w1, R) + N.total_words(w2, R)
    N.check_stat_words(good, ref["sums"], "all replica rows", N.UNIT_GRAD)
    for r in range(R):
        keep = [k for k in range(R) if k != r]
        _rejects(N.check_stat_words, N.total_words(w1[keep], R - 1) + N.total_words(w2[keep], R - 1), ref["sums"], "row %d left out" % r,
                 N.UNIT_GRAD)
    short = N.bn_backward_ref(inp["x"][:-1], inp["dz"][:-1], *args, row.act)
    _rejects(N.check_stat_words, N.words_of(short["sums"], N.UNIT_GRAD), ref["sums"], "last row dropped", N.UNIT_GRAD)
    s1, s2 = N.column_sums(inp["x"])
    t1, t2 = N.column_sums(inp["x"][:-1])
    _rejects(N.check_stat_words, N.words_of(t1 + t2), s1 + s2, "colstats: last row dropped")
    # dx: bit comparison against a result whose sums missed the last row
    wrong = N.bn_backward_ref(inp["x"], inp["dz"], *args, row.act)["dx"] + (short["s1"] - ref["s1"]) / row.rows * inp["gamma"] * inp["invstd"]
    dtype = N.TORCH_DTYPE[row.dtype]
    N.check_equal(ref["dx"].to(dtype).float(), ref["dx"], dtype, "good")
    _rejects(N.check_equal, wrong.to(dtype).float(), ref["dx"], dtype, "k1 from a short sum")
    _rejects(N.check_sums_close, N.words_of([2 * s for s in ref["sums"]], N.UNIT_GRAD), ref["sums"], N.UNIT_GRAD, "twice the sums")
    N.check_sums_close(N.words_of(ref["sums"], N.UNIT_GRAD), [float(s) for s in ref["sums"]], N.UNIT_GRAD, "good")


def test_comparisons_reject_a_tie_routed_to_the_last_maximum():
    row = next(r for r in N.POOL_BN_ROWS if (r.B, r.H, r.W) == (2, 6, 10) and r.mode == "sums" and r.dtype == "bf16")
    inp = N.pool_bn_inputs(row.B, row.H, row.W, row.C)
    good = N.pool_bn_backward_ref(row, inp)
    pick_last = lambda *args: N.last_max(N.pool_bn_acts(*args))
    bad = N.pool_bn_backward_ref(row, inp, argmax=pick_last)
    dtype = N.TORCH_DTYPE[row.dtype]
    # tied taps of a channel hold the same x, so the two sums cannot tell the rules apart: dx is what checks the rule
    assert bad["sums"] == good["sums"]
    _rejects(N.check_equal, bad["dx"].to(dtype).float(), good["dx"], dtype, "last maximum")
    with pytest.raises(AssertionError):
        torch.testing.assert_close(bad["dx"], good["dx"], **_tol(dtype, stored=True))      # far outside the "sums" rows' tolerance too
    p = N.pool_inputs(2, 6, 10, 24)
    x, dy = p["x"].float(), p["dy"].float()
    first, last = N.route(N.first_max(x)[1], dy), N.route(N.last_max(x)[1], dy)
    assert torch.equal(N.first_max(x)[0], N.last_max(x)[0]) and not torch.equal(first, last)      # integer x: ties everywhere
    _rejects(N.check_equal, last, first.double(), torch.float32, "maxpool2_bwd with the last maximum")


def test_comparisons_reject_a_shifted_group_boundary():
    for row in (N.GN_ROWS[0], N.GN_ROWS[2]):                      # cpg 2 (fp32) and a straddled granule (bf16)
        case = N.gn_case(row)
        good = case["ref"]
        bad = N.gn_ref(case["x"], case["dz"], case["gamma"], case["beta"], row.levels, row.batch, row.G, boundary_shift=1)
        _rejects(N.check_stat_words, N.words_of(bad["stats"]), good["stats"], "group boundary off by one channel")
        _rejects(N.check_stat_words, N.words_of(bad["gsum"][0::2], N.UNIT_GRAD), good["gsum"][0::2], "group sums", N.UNIT_GRAD)
        # dbeta is a per-channel sum: a wrong mask (here: of the wrong group's statistics) moves it
        _rejects(N.check_stat_words, N.words_of(bad["dbeta"].tolist(), N.UNIT_GRAD), good["dbeta"].tolist(), "dbeta", N.UNIT_GRAD)


def test_guarded_buffers_reject_holes_and_writes_behind_the_last_row():
    rows, C = 5, 8
    buf = torch.full((rows + N.GUARD_ROWS, C), N.NAN)
    buf[:rows] = 1.0
    assert torch.equal(N.landed(buf, rows), torch.ones(rows, C))
    behind = buf.clone()
    behind[rows, 0] = 0.0
    _rejects(N.landed, behind, rows, "write behind the last row")
    hole = buf.clone()
    hole[rows - 1, C - 1] = N.NAN
    _rejects(N.landed, hole, rows, "last row's last element never written")
    planar = torch.arange(12)
    assert N.planar_words(planar, 1, 3, 6) == [[1, 7], [2, 8], [3, 9]]
    assert N.total_words(torch.tensor([[1, 2, 3, 4], [10, 20, 30, 40]]), 2) == [[11, 22], [33, 44]]
