"""CPU: the table of tests/conv_variant_cases.py (the rows of tests/test_conv_variants_gpu.py) against the host build of
csrc/conv_plan.h -- every compiled variant of every KD6D_CONV_*_TILES list has a row per direction, every row plans the
variant it declares whatever the device size, the integer pass is exact for every row, the table stays small, and the two
comparisons reject the results a broken tile kernel would give.  The same for the fused statistics and the fused forms
(STAT_ROWS): every statistic-taking variant has its exact per-channel and group-statistics rows, every fused
instantiation its row, the group-statistics LDS table of every row fits, and the word comparison rejects the sums a
broken epilogue would leave."""
import collections

import pytest
import torch
import torch.nn.functional as F

import conv_plan_lib as P
import conv_variant_cases as C

CU_COUNTS = (64, 256, 304)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return P.build_lib(tmp_path_factory.mktemp("conv_variants"))


planned = C.planned


def missing_variants(lib, rows):
    """'list variant direction dtype' of every compiled variant that no row of `rows` plans (at 256 CUs)."""
    have = set()
    for r in rows:
        name, v, _ = planned(lib, r, 256, r.budgets[0])
        have.add((name, v, r.kind, r.dtype))
    have |= {("halo", v, kind, "bf16") for v in C.HALO_TWINS for kind in ("fwd", "dgrad")}
    missing = []
    for name in C.DIRECTIONS:
        for v in P.variants(lib, name):
            for kind in C.DIRECTIONS[name]:
                for dtype in C.DTYPES[name]:
                    if (name, v, kind, dtype) not in have:
                        missing.append("%s %s %s %s" % (name, "x".join(str(x) for x in v), kind, dtype))
    return missing


def test_every_compiled_variant_has_a_row_per_direction(lib):
    # (the ninth list, halo_norm, has forward launches of its own kind only: test_statistics_rows_cover_every_variant)
    assert set(C.DIRECTIONS) == set(C.DTYPES) == set(P.LISTS) - {"halo_norm"}
    assert missing_variants(lib, C.ROWS) == []
    # the five twins are variants of the list, taken on trust by name: test_conv_halo_two_per_cu_variants runs them
    assert len(C.HALO_TWINS) == 5 and set(C.HALO_TWINS) <= set(P.variants(lib, "halo"))
    assert not any(r.list == "halo" and r.variant in C.HALO_TWINS for r in C.ROWS)
    # the check is live: without any one variant's rows it names exactly that variant
    for name, v, kind, dtype in (("halo", (256, 128, 4, 2, 81, 1), "fwd", "bf16"), ("igemm", (128, 128, 2, 2, 0, 0), "dgrad", "f32"),
                                 ("splitk", (128, 64, 2, 2, 3, 0), "fwd", "bf16"), ("wgrad_small", (2, 2, 1, 0, 0, 0), "wgrad", "bf16")):
        rest = [r for r in C.ROWS if (r.list, r.variant, r.kind, r.dtype) != (name, v, kind, dtype)]
        assert len(rest) < len(C.ROWS)
        assert missing_variants(lib, rest) == ["%s %s %s %s" % (name, "x".join(str(x) for x in v), kind, dtype)]


def test_every_row_plans_its_declared_variant_on_any_device_size(lib):
    assert len({r.id for r in C.ROWS}) == len(C.ROWS)
    for r in C.ROWS:
        assert r.kind in C.DIRECTIONS[r.list] and r.dtype in C.DTYPES[r.list], r.id
        plans = []
        for ncu in CU_COUNTS:
            for budget in r.budgets:
                name, v, p = planned(lib, r, ncu, budget)
                assert (name, v) == (r.list, r.variant), (r.id, ncu, budget, name, v)
                plans.append(p)
        if r.kind != "wgrad":       # the whole launch, not only the kernel, is the same on every device size
            assert all(p == plans[0] for p in plans), r.id
        assert r.budgets == (0,) or r.list == "wgrad_small", r.id
        assert ("fallback" in r.note) == (r.list == "wgrad_tr" and r.options.get("wgrad.small") == 1
                                          or r.list == "halo" and r.variant[4] == 81 and r.options["conv.halo"] in C.HALO_FALLBACK_81), r.id


def test_the_shapes_reach_the_tails_and_regimes_they_are_there_for(lib):
    by_list = {}
    for r in C.ROWS:
        by_list.setdefault(r.list, []).append(r)
    for name, rows in by_list.items():
        multi = [r for r in rows if len(r.case[5]) > 1]
        assert multi or name == "wgrad_small", name                 # (the narrow weight gradient takes one level only)
    ragged, tail = set(), set()
    for r in C.ROWS:
        if r.kind == "wgrad":
            continue
        M, N, K = C.gemm(r)
        _, _, p = planned(lib, r, 256)
        key = (r.list, r.variant, r.kind, r.dtype)
        ragged |= {key} if M % p.BP else set()
        tail |= {key} if N % p.BC else set()
    every = {(r.list, r.variant, r.kind, r.dtype) for r in C.ROWS if r.kind != "wgrad"}
    assert ragged == every and tail == every, (every - ragged, every - tail)      # a ragged last pixel tile, a channel tail
    for name in ("igemm", "glds", "splitk"):
        assert any(r.case[4] == 2 for r in by_list[name]) and any(r.case[3] == 1 for r in by_list[name]), name
        assert any(C.gemm(r)[2] // r.case[3] ** 2 % 64 for r in by_list[name]) or name == "splitk", name     # tap-straddling k-steps
    for v in P.variants(lib, "igemm") + P.variants(lib, "glds"):
        name = "glds" if v[4] else "igemm"
        assert any(C.gemm(r)[0] > r.variant[0] for r in by_list[name] if r.variant == v), v      # more than one pixel tile
    # split-K: a short last split, one k-step per split
    sk = {r.id: planned(lib, r, 256)[2] for r in by_list["splitk"]}
    assert {p.nsplit for p in sk.values()} >= {4, 5, 12, 15} and any(p.nk_split == 1 for p in sk.values())
    assert any(p.nsplit * p.nk_split > -(-C.gemm(C.BY_ID[i])[2] // 64) for i, p in sk.items())
    # narrow weight gradient: persistent workgroups looping over tiles with a short last tile; one workgroup per CU
    ws = [(r, planned(lib, r, 256, b)[2]) for r in by_list["wgrad_small"] for b in r.budgets]
    assert any(p.grid_x < p.ntiles and p.tiles_per_img * p.R > r.case[5][0][0] for r, p in ws)
    assert any(p.R == 1 and p.lds > 80 * 1024 for r, p in ws) and any(r.case[5][0][1] == 256 for r, p in ws)
    # the halo maps sit on both edges of each HMAX
    assert {max(w for _, w in r.case[5]) for r in by_list["halo"]} >= {33, 64, 65, 80}


def test_integer_pass_is_exact_and_the_table_stays_small():
    work, seen = {}, set()
    for r in C.ROWS:
        splits = 16 if r.list == "splitk" else 1
        assert 9 * (C.reduction_length(r) + splits) < 2 ** 24, r.id
        assert C.reference_flops(r) <= 1e9, r.id
        assert C.largest_tensor_bytes(r) <= 64 << 20, r.id
        # a reference is computed once per case and direction (integer pass), and per dtype on top (random pass)
        work[(C._key(r.case), r.kind)] = work[(C._key(r.case), r.kind, r.dtype)] = C.reference_flops(r)
        if C._key(r.case) in seen or C.gemm(r)[0] > 4096:               # (the inputs of the wide maps: same generator)
            continue
        seen.add(C._key(r.case))
        inp = C.integer_inputs(r)
        for t in inp["xs"] + inp["dys"] + inp["dx0"] + [inp["w"]]:
            assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max() <= 3
            assert torch.equal(t, t.to(torch.bfloat16).float())
        w = inp["w"]
        assert (w != 0).any(dim=1).all() and (w != 0).any(dim=0).all(), r.id       # no tap or channel is zero throughout
        for t in inp["xs"] + inp["dys"]:
            assert (t != 0).flatten(2).any(dim=2).any(dim=0).all(), r.id
    assert sum(work.values()) < 15e9


# ---- the comparisons reject what a broken kernel would store --------------------------------------------------------
TINY = ["igemm-64x16x4x1x0x0-fwd-bf16-halo=0,smallc=0,tile=0-b2c24n12k3s1_9x7_4x3",
        "glds-64x64x2x2x4x0-fwd-bf16-halo=0,smallc=0,tile=3-b2c24n72k3s1_9x7_4x3",
        "smallc-2x2x0x0x0x0-fwd-bf16-smallc=1-b2c16n24k3s1_9x7_5x3"]


def _perturbations(row, inp, ref):
    """level-0 results of four broken kernels: (name, tensor like ref[0])."""
    B, cin, cout, k, stride, levels = row.case
    x, w = inp["xs"][0].double(), inp["w"].double()
    good = ref[0].double()
    w_tap = w.clone()
    w_tap[:, :, k - 1, k - 1] = 0                                   # one tap dropped
    yield "tap", F.conv2d(x, w_tap, stride=stride, padding=k // 2)
    col = good.clone()
    col[:, cout - 1] = 0                                            # the last column of the last channel tile zeroed
    yield "column", col
    rows = good.permute(0, 2, 3, 1).reshape(-1, cout).clone()
    rows[-1] = rows[-2]                                             # the last pixel row taken from the row before
    yield "row", rows.reshape(B, good.shape[2], good.shape[3], cout).permute(0, 3, 1, 2)
    half = cin // 2                                                 # one split's partial sum missing
    yield "split", good - F.conv2d(x[:, half:], w[:, half:], stride=stride, padding=k // 2)


@pytest.mark.parametrize("rid", TINY)
def test_comparisons_reject_broken_results(rid):
    row = C.BY_ID[rid]
    assert C.reference_flops(row) < 5e6
    dtype = C.TORCH_DTYPE[row.dtype]
    for name, inp, ref in (("integer", C.integer_inputs(row), C.integer_reference(row)),
                           ("random", C.random_inputs(row), C.random_reference(row))):
        def check(got):
            if name == "integer":
                C.check_integer(got.float(), ref[0], torch.float32, rid)
                C.check_integer(C.round_to(got.float(), torch.bfloat16), ref[0], torch.bfloat16, rid)
            else:
                C.check_random(got.float(), ref[0], dtype, False, rid)
        check(ref[0].clone())                                        # the reference itself passes
        n = 0
        for what, broken in _perturbations(row, inp, ref):
            assert broken.shape == ref[0].shape
            with pytest.raises(AssertionError):
                if name == "integer":
                    C.check_integer(broken.float(), ref[0], torch.float32, what)
                else:
                    C.check_random(broken.float(), ref[0], dtype, False, what)
            if name == "integer":                                    # ... and where the kernel stores bf16
                with pytest.raises(AssertionError):
                    C.check_integer(C.round_to(broken.float(), torch.bfloat16), ref[0], torch.bfloat16, what)
            n += 1
        assert n == 4


def test_weight_gradient_comparison_rejects_a_missing_tile():
    row = C.BY_ID["wgrad_small-1x4x3x0x0x0-wgrad-bf16-small=1-b1c8n64k3s1_40x13-cu0_1_16"]
    for inp, exact in ((C.integer_inputs(row), True), (C.random_inputs(row), False)):
        ref = C.reference(row, inp, torch.float64)
        # the short last tile (map rows 36 ... 39) lost
        got = torch.nn.grad.conv2d_weight(inp["xs"][0][:, :, :36].double(), ref.shape, inp["dys"][0][:, :, :36].double(), padding=1)
        with pytest.raises(AssertionError):
            (C.check_integer(got.float(), ref) if exact else C.check_random_wgrad(got.float(), ref.float()))
        (C.check_integer(ref.float(), ref) if exact else C.check_random_wgrad(ref.float(), ref.float()))


# ---- fused statistics and fused forms (STAT_ROWS) ----------------------------------------------------------------------
STATS_LISTS = ("igemm", "glds", "halo", "smallc")            # + splitk, which takes no statistics by rule (has_stats)


def _dt(r):
    return P.BF16 if r.dtype == "bf16" else P.F32


def missing_stat_variants(lib, rows, stat_rows):
    """What the statistics coverage lacks: 'kind list variant dtype' strings (at 256 CUs)."""
    fwd = [r for r in rows if r.kind == "fwd"]
    chan = {(r.list, r.variant, r.dtype) for r in fwd if r.list != "splitk" and planned(lib, r, 256, stats=1)[:2] == (r.list, r.variant)}
    have = {}
    for r in stat_rows:
        name, v, p = C.planned_stat(lib, r, 256)
        kind = r.kind + ("/" + r.extra["norm"] if r.kind == "fwd_norm" else "")
        if r.kind == "fwd_gstats" and (not any(summed for _, _, summed in C.level_rows(r)) or r.note):
            continue                        # (the refused row and the resident-patch fallback stand for no tile)
        have.setdefault(kind, set()).add((name, v, r.dtype))
    # the twins' per-channel sums run inside their group-statistics rows
    chan |= {k for k in have.get("fwd_gstats", ()) if k[0] == "halo" and k[1] in C.HALO_TWINS}
    missing = []

    def need(kind, got, name, v, dtype):
        if (name, v, dtype) not in got:
            missing.append("%s %s %s %s" % (kind, name, "x".join(str(x) for x in v), dtype))
    for name in STATS_LISTS:
        for v in P.variants(lib, name):
            for dtype in C.DTYPES[name]:
                need("channel", chan, name, v, dtype)
                if name != "smallc":                                   # smallc_rule: no group statistics
                    need("fwd_gstats", have.get("fwd_gstats", ()), name, v, dtype)
    for v in P.variants(lib, "halo_norm"):
        for norm in ("group", "batch"):
            need("fwd_norm/" + norm, have.get("fwd_norm/" + norm, ()), "halo_norm", v, "bf16")
    for v in P.variants(lib, "igemm"):
        for dtype in ("bf16", "f32"):
            need("fwd_block", have.get("fwd_block", ()), "igemm", v, dtype)
            need("fwd_xf", have.get("fwd_xf", ()), "igemm", v, dtype)
    for dtype in ("bf16", "f32"):
        for norm in ("group", "batch"):
            if not any(k[0] == "igemm" and k[2] == dtype for k in have.get("fwd_norm/" + norm, ())):
                missing.append("fwd_norm/%s igemm any %s" % (norm, dtype))
    return missing


def test_statistics_rows_cover_every_variant(lib):
    assert missing_stat_variants(lib, C.ROWS, C.STAT_ROWS) == []
    assert all(r.kind in C.STAT_KINDS for r in C.STAT_ROWS) and len({r.id for r in C.STAT_ROWS}) == len(C.STAT_ROWS)
    # no silent skip: every forward row of the statistic-taking lists keeps its variant with statistics, and has cout % 4 == 0
    for r in C.ROWS:
        if r.kind == "fwd" and r.list != "splitk":
            assert r.list in STATS_LISTS and r.case[2] % 4 == 0, r.id
            for ncu in CU_COUNTS:
                assert planned(lib, r, ncu, stats=1)[:2] == (r.list, r.variant), r.id
    # split-K takes no statistics (splitk_rule: has_stats), the resident-patch kernel no group statistics (smallc_rule)
    for r in C.ROWS:
        if r.kind == "fwd" and r.list == "splitk":
            assert planned(lib, r, 256, stats=1)[0] != "splitk", r.id
        if r.kind == "fwd" and r.list == "smallc":
            p = P.plan_conv(lib, P.Layer(*r.case), "fwd", P.BF16, stats=1, groups=r.case[2] // 4, **C.plan_options(r))
            assert p.family != P.SMALLC, r.id
    fallback = [r for r in C.STAT_ROWS if "fallback" in r.note]
    assert len(fallback) == 1 and fallback[0].options == {"conv.smallc": 1}
    assert P.plan_conv(lib, P.Layer(*fallback[0].case), "fwd", P.BF16, stats=1, **C.plan_options(fallback[0])).family == P.SMALLC
    assert len([r for r in C.STAT_ROWS if "refused" in r.note]) == 1
    # the follow-up's rule as norm_plan.h states it: whole 16-byte granules, a granule count that divides 256
    for cout, groups, f32, ok in ((128, 32, 1, 1), (128, 32, 0, 1), (256, 32, 0, 1), (12, 3, 1, 0), (24, 6, 0, 0), (136, 34, 1, 0),
                                 (64, 16, 0, 1), (16, 4, 0, 1), (8, 2, 0, 1), (12, 3, 0, 0), (8, 2, 1, 1)):
        assert lib.cp_stats_followup_ok(cout, groups, f32) == ok, (cout, groups, f32)
    # the check is live: without the rows of one variant and kind it names exactly that
    for kind, name, v, dtype in (("fwd_gstats", "halo", (192, 128, 4, 2, 65, 1), "bf16"), ("fwd_gstats", "igemm", (256, 32, 4, 1, 0, 0), "f32"),
                                 ("fwd_norm", "halo_norm", (128, 128, 4, 2, 81, 1), "bf16"), ("fwd_block", "igemm", (64, 16, 4, 1, 0, 0), "bf16"),
                                 ("fwd_xf", "igemm", (128, 128, 2, 2, 0, 0), "f32"), ("fwd_gstats", "glds", (64, 64, 2, 2, 6, 0), "bf16")):
        rest = [r for r in C.STAT_ROWS if (r.kind, r.list, r.variant, r.dtype) != (kind, name, v, dtype)]
        assert len(rest) < len(C.STAT_ROWS)
        miss = missing_stat_variants(lib, C.ROWS, rest)
        assert miss and all(m.split()[0].startswith(kind) and m.split()[1:] == [name, "x".join(str(x) for x in v), dtype] for m in miss), miss
    rest = [r for r in C.ROWS if (r.list, r.variant, r.kind) != ("smallc", (2, 4, 0, 0, 0, 0), "fwd")]
    assert missing_stat_variants(lib, rest, C.STAT_ROWS) == ["channel smallc 2x4x0x0x0x0 bf16"]
    twin = [r for r in C.STAT_ROWS if (r.list, r.variant) != ("halo", (64, 64, 4, 2, 33, 0))]
    assert missing_stat_variants(lib, C.ROWS, twin) == ["channel halo 64x64x4x2x33x0 bf16", "fwd_gstats halo 64x64x4x2x33x0 bf16"]


def test_statistics_rows_plan_what_they_declare_and_their_table_fits(lib):
    for r in C.STAT_ROWS:
        plans = []
        for ncu in CU_COUNTS:
            name, v, p = C.planned_stat(lib, r, ncu)
            assert (name, v) == (r.list, r.variant), (r.id, ncu, name, v)
            plans.append(p)
        assert all(p == plans[0] for p in plans), r.id
        if r.kind == "fwd_norm":
            assert C.fusable(lib, r) == 1, r.id
            assert all(summed for _, _, summed in C.level_rows(r)) or r.extra["norm"] == "batch", r.id
        G = r.extra.get("groups", 0)
        if G:
            assert lib.cp_stats_groups_ok(r.case[2], G) == 1 and r.case[2] // G in (4, 8), r.id
            t = P.stats_table(lib, P.Layer(*r.case), _dt(r), G, norm=int(r.kind == "fwd_norm"), **C.plan_options(r))
            assert t.fits == 1 and t.tile_keys <= t.room and t.bytes <= t.lds == plans[1].lds, (r.id, t)
            for m0, hw, summed in C.level_rows(r):
                assert summed == (not lib.cp_stats_level_skipped(hw, m0)), r.id
        if r.kind == "fwd_gstats":
            # a skipped level goes to the follow-up launch, for the fp32 and for the bf16 store: stats_followup_ok, or the
            # row records the refusal
            skipped = any(not summed for _, _, summed in C.level_rows(r))
            taken = all(lib.cp_stats_followup_ok(r.case[2], G, f32) for f32 in ((1, 0) if r.dtype == "bf16" else (1,)))
            assert ("refused" in r.note) == (skipped and not taken), r.id
        if r.kind == "fwd_xf":
            assert r.case[4] == 1 and r.case[3] in (1, 3), r.id
        assert C.reference_flops(r._replace(kind="fwd")) <= 1e9 and C.largest_tensor_bytes(r._replace(kind="fwd")) <= 64 << 20, r.id


def test_group_statistics_table_bound(lib):
    """conv_plan.h stats_table_fits: a tile's table [key][group] must fit the kernel's dead staging memory together with the
    staged entries; nkeys counts skipped levels too, so 1 x 1 levels at a large batch overflow it.  The entry points refuse
    such a launch; no GPU row comes near (previous test)."""
    for batch, fits in ((61, 1), (62, 1), (63, 0), (200, 0)):
        # fp32, 128 channels: 64 x 64 tiles, 32 KB of LDS: (32768 - 512 - 16) / 512 = 62 keys; a 64-row tile of the 1 x 1 level
        # holds min(batch, 64) keys
        t = P.stats_table(lib, P.Layer(batch, 8, 128, 3, 1, [(1, 1)]), P.F32, 32)
        assert (t.room, t.tile_keys, t.fits) == (62, min(batch, 64), fits), (batch, t)
        assert (t.bytes <= t.lds) == bool(fits)
    # ... the same behind summed levels, and on the halo kernel's 128 x 128 twin
    assert P.stats_table(lib, P.Layer(64, 8, 128, 3, 1, [(4, 4), (1, 1)]), P.F32, 32).fits == 0
    t = P.stats_table(lib, P.Layer(128, 128, 128, 3, 1, [(4, 4), (1, 1)]), P.BF16, 32, halo=12)
    assert t.fits == 0 and t.tile_keys == 128 and t.bytes > t.lds
    # (a fused GroupNorm launch has whole levels only, 16 pixels or more per key: at most BP / 16 + 1 keys, which always fit)
    t = P.stats_table(lib, P.Layer(128, 128, 128, 3, 1, [(4, 4), (16, 1)]), P.BF16, 32, norm=1, halo=12)
    assert t.fits == 1 and t.tile_keys <= 128 // 16 + 1 < t.room
    # the step's tower pyramids stay far inside it
    for batch in (2, 16, 32):
        for c in (128, 256):
            t = P.stats_table(lib, P.Layer(batch, c, c, 3, 1, [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]), P.BF16, 32)
            assert t.fits == 1 and t.tile_keys <= 40 < t.room, (batch, c, t)


def edges_of(lib, r):
    """The edges of the group-statistics epilogue that the launch of row r reaches, computed from its plan at 256 CUs."""
    _, _, p = C.planned_stat(lib, r, 256)
    B, cout, G = r.case[0], r.case[2], r.extra["groups"]
    cpg = cout // G
    lv = C.level_rows(r)
    M = C.gemm(r._replace(kind="fwd"))[0]
    keys = C.row_keys(r).tolist()
    level_of = lambda m: keys[m] // B
    f = {"cpg%d" % cpg}
    if (cout % p.BC) and (cout % p.BC) // cpg < p.BC // cpg:
        f.add(C.TAIL)
    if any(not s for _, _, s in lv) and any(s for _, _, s in lv):
        f.add(C.MIXED[0])
    if M % p.BP and M % 16:
        f.add(C.MIXED[1])
    if M % p.BP and M > p.BP:
        f.add(C.SHORT)
    for m0 in range(0, M, p.BP):
        last = min(m0 + p.BP, M) - 1
        if len({keys[m] for m in range(m0, last + 1, 16) if lv[level_of(m)][2]}) >= 2:
            f.add(C.KEYS)
        if len({level_of(m) for m in range(m0, last + 1, 16) if lv[level_of(m)][2]}) >= 2:
            f.add(C.LEVELS)
    return f


def test_group_statistics_rows_reach_the_edges_they_are_there_for(lib):
    fam = {}
    for r in C.STAT_ROWS:
        if r.kind != "fwd_gstats":
            continue
        got = edges_of(lib, r)
        # every row reaches what it declares, whatever the other rows do
        assert set(r.why) - {"N <= 64", "N > 64"} <= got, (r.id, set(r.why) - got)
        assert any(s for _, _, s in C.level_rows(r)), r.id    # (the 256- and 192-pixel tiles too: maps with H * W % 16 == 0)
        if not r.note:
            fam.setdefault(r.list, set()).update(got)
    want = {"cpg4", "cpg8", C.TAIL, C.MIXED[0], C.MIXED[1], C.SHORT, C.KEYS, C.LEVELS}
    for name in ("igemm", "glds", "halo"):
        assert fam[name] == want, (name, want - fam[name])


def required_stat_rows(lib):
    """The rows STAT_ROWS must hold, written out here: (kind, list, variant, dtype, norm, what the row is there for, note
    class) -> count.  Kept apart from the table on purpose: a row deleted there is a row missing here."""
    MIXED, TAIL, KEYS, LEVELS, SHORT = C.MIXED, C.TAIL, C.KEYS, C.LEVELS, C.SHORT
    LE, GT = "N <= 64", "N > 64"
    need = collections.Counter()
    igemm = {  # tile: (the group-statistics rows, the N classes of its fwd_block / fwd_xf rows)
        (256, 16, 4, 1): ([(TAIL, SHORT)], [LE]), (64, 16, 4, 1): ([MIXED], [LE]), (256, 32, 4, 1): ([(TAIL, SHORT)], [LE]),
        (64, 32, 4, 1): ([(LEVELS, KEYS, TAIL)], [LE]), (128, 64, 2, 2): ([(KEYS, LE), (TAIL, GT)], [LE, GT]),
        (64, 64, 2, 2): ([MIXED + (KEYS,), (TAIL,)], [GT]), (128, 128, 2, 2): ([(KEYS, TAIL)], [GT])}
    assert {t + (0, 0) for t in igemm} == set(P.variants(lib, "igemm"))
    for dtype in ("bf16", "f32"):
        for t, (whys, classes) in igemm.items():
            for why in whys:
                need[("fwd_gstats", "igemm", t + (0, 0), dtype, "", why, "")] += 1
            for kind in ("fwd_block", "fwd_xf"):
                for cls in classes:
                    need[(kind, "igemm", t + (0, 0), dtype, "", (cls,), "")] += 1
        for norm in ("group", "batch"):
            need[("fwd_norm", "igemm", (64, 64, 2, 2, 0, 0), dtype, norm, (), "")] += 1
    need[("fwd_gstats", "igemm", (64, 32, 4, 1, 0, 0), "bf16", "", MIXED, "fallback")] += 1
    need[("fwd_gstats", "igemm", (64, 16, 4, 1, 0, 0), "bf16", "", MIXED, "refused")] += 1
    for v in P.variants(lib, "glds"):
        for why in (MIXED, (LEVELS, TAIL)):
            need[("fwd_gstats", "glds", v, "bf16", "", why, "")] += 1
    halo = {(256, 128, 4, 2, 65, 1): MIXED, (128, 128, 2, 2, 65, 1): (TAIL,), (128, 128, 4, 2, 65, 1): MIXED, (128, 64, 4, 2, 65, 1): (TAIL,),
            (128, 32, 4, 1, 65, 1): MIXED, (192, 128, 4, 2, 65, 1): (TAIL,), (64, 64, 4, 2, 65, 1): MIXED,
            (256, 128, 4, 2, 81, 1): MIXED, (128, 128, 4, 2, 81, 1): MIXED, (128, 64, 4, 2, 81, 1): (TAIL,), (128, 32, 4, 1, 81, 1): MIXED,
            (64, 64, 4, 2, 81, 1): MIXED,
            (128, 128, 2, 2, 33, 0): MIXED, (128, 128, 4, 2, 33, 0): (TAIL,), (128, 64, 4, 2, 33, 0): MIXED, (64, 64, 4, 2, 33, 0): (TAIL,),
            (128, 32, 4, 1, 33, 0): MIXED}
    assert set(halo) == set(P.variants(lib, "halo"))
    for v, why in halo.items():
        need[("fwd_gstats", "halo", v, "bf16", "", why, "")] += 1
    # the fused halo tiles: each HMAX at the map widths it is there for, a GroupNorm and a BatchNorm launch of each
    halo_norm = {(33, 0): ["up to 32 wide"], (65, 1): ["33 ... 63 wide", "64 wide", "up to 32 wide, no twins"],
                 (81, 1): ["65 ... 79 wide", "80 wide"]}
    assert {(128, 128, 4, 2) + hp for hp in halo_norm} == set(P.variants(lib, "halo_norm"))
    for hp, whys in halo_norm.items():
        for why in whys:
            for norm in ("group", "batch"):
                need[("fwd_norm", "halo_norm", (128, 128, 4, 2) + hp, "bf16", norm, (why,), "")] += 1
    return need


def stat_row_key(r):
    return (r.kind, r.list, r.variant, r.dtype, r.extra.get("norm", ""), r.why, r.note.split(":")[0])


def test_statistics_table_is_exactly_the_required_rows(lib):
    """Deleting any row of STAT_ROWS, or swapping it for one with another purpose, fails here and names it; what a row
    declares (Row.why) is computed on the row itself, here and in the edges test above."""
    need, have = required_stat_rows(lib), collections.Counter(stat_row_key(r) for r in C.STAT_ROWS)
    assert sorted(need - have) == [], "rows missing from STAT_ROWS"
    assert sorted(have - need) == [], "rows of STAT_ROWS that required_stat_rows does not list"
    assert sum(need.values()) == len(C.STAT_ROWS) == 93
    width = {"up to 32 wide": (1, 32, 1), "up to 32 wide, no twins": (1, 32, 0), "33 ... 63 wide": (33, 63, 1), "64 wide": (64, 64, 1),
             "65 ... 79 wide": (65, 79, 1), "80 wide": (80, 80, 1)}
    for r in C.STAT_ROWS:
        if r.list == "halo_norm":
            lo, hi, pairing = width[r.why[0]]
            assert lo <= max(w for _, w in r.case[5]) <= hi and r.options.get("conv.halo_pairing", 1) == pairing, r.id
        for cls in set(r.why) & {"N <= 64", "N > 64"}:
            assert (r.case[2] <= 64) == (cls == "N <= 64"), r.id
    # live: each single deletion is noticed, and named
    for i, r in enumerate(C.STAT_ROWS):
        rest = collections.Counter(stat_row_key(q) for q in C.STAT_ROWS[:i] + C.STAT_ROWS[i + 1:])
        assert list((need - rest).elements()) == [stat_row_key(r)], r.id


def test_narrow_integer_passes_are_exact():
    """|y| <= 255 on the actual fp64 reference of every row that runs a statistics pass: then the sum of squares over the
    256 rows of the tallest tile stays below 256 * 255^2 < 2^24 and every fp32 partial is exact in any order."""
    seen = set()
    for r in C.ROWS + C.STAT_ROWS:
        if not r.kind.startswith("fwd") or r.list == "splitk":
            continue
        for q in ((r, r._replace(case=(r.case[0], 8, r.case[1], 1, 1, r.case[5]))) if r.kind == "fwd_xf" else (r,)):
            if C._key(q.case) in seen:
                continue
            seen.add(C._key(q.case))
            inp, ref = C.narrow_inputs(q), C.narrow_reference(q)
            for t in inp["xs"] + [inp["w"]]:
                assert torch.equal(t, t.round()) and t.abs().max() <= 1
            assert torch.equal(inp["shift"], inp["shift"].round()) and inp["shift"].abs().max() <= 2
            for y in ref:
                assert y.dtype == torch.float64 and torch.equal(y, y.round()) and y.abs().max() <= 255, q.id
                assert torch.equal(y.float().to(torch.bfloat16).double(), y)                 # exact in the bf16 store as well
                # the BatchNorm launches, the replica rows and block A sum the convolution without the shift
                assert (y - inp["shift"].double().view(1, -1, 1, 1)).abs().max() <= 255, q.id
            assert (C.packed_rows(ref) != 0).any(0).all(), q.id                              # no channel is zero throughout
    assert 256 * 255 ** 2 < 2 ** 24


def test_group_key_layout_is_stated_once(lib):
    """C.row_key: level-major, image-major -- what conv_plan.h stats_row_key (the host form of the kernels' stats_key) gives
    and what test_conv_fwd_fused_statistics spells with a reshape per level."""
    for r in C.STAT_ROWS:
        if r.kind != "fwd_gstats" or C.gemm(r._replace(kind="fwd"))[0] > 1000:
            continue
        layer, keys = P.Layer(*r.case), C.row_keys(r)
        M = C.gemm(r._replace(kind="fwd"))[0]
        assert len(keys) == M
        for m in range(M):
            assert int(keys[m]) == C.row_key(r, m) == P.stats_row_key(lib, layer, m), (r.id, m)
        ref, G, B = C.narrow_reference(r), r.extra["groups"], r.case[0]
        parts = []
        for t in ref:
            tg = t.reshape(B, G, -1)
            parts += torch.stack([tg.sum(-1), (tg ** 2).sum(-1)], dim=-1).reshape(-1).tolist()
        assert C.group_sums(C.packed_rows(ref), r, G) == parts


def _rejected(words, want):
    with pytest.raises(AssertionError):
        C.check_stat_words(words, want, "mutation")


def test_word_comparison_rejects_what_the_old_tolerance_accepted():
    """The exact comparison (hi * 2^47 + lo == S * 2^32) rejects the sums a broken epilogue would leave: one 16-row fragment
    left out, the rows behind M counted, the group behind the last one counted (it lands on the next key's first group),
    every key shifted by one image.  On the largest row (363 x 361, 131 043 pixels) the tolerance the statistics were
    checked with before, rtol 1e-4 and atol 1e-4 * max, ACCEPTS the sums without one fragment -- 16 of 131 043 rows move a
    sum of squares by 1.2e-4 of its value -- which is why the sums are now compared to the word."""
    big = C.BY_ID["igemm-256x16x4x1x0x0-fwd-bf16-halo=0,smallc=0,tile=0-b1c16n12k1s1_363x361"]
    rows = C.packed_rows(C.narrow_reference(big))
    good = C.channel_sums(rows)
    C.check_stat_words(C.words_of(good), good)
    holed = rows.clone()
    holed[16 * 5:16 * 6] = 0
    bad = C.channel_sums(holed)
    assert bad != good
    as_before = lambda v: torch.tensor(v, dtype=torch.float64)
    torch.testing.assert_close(as_before(bad), as_before(good), rtol=1e-4, atol=1e-4 * max(float(as_before(good).abs().max()), 1.0))
    _rejected(C.words_of(bad), good)
    _rejected(C.words_of(C.channel_sums(torch.cat([rows, rows[-3:]]))), good)              # M-tail rows counted
    # group statistics, on the row with summed and skipped levels
    r = next(q for q in C.STAT_ROWS if q.list == "igemm" and q.variant[:2] == (64, 64) and q.kind == "fwd_gstats")
    rows, G, keys = C.packed_rows(C.narrow_reference(r)), r.extra["groups"], C.row_keys(r)
    good = C.group_sums(rows, r, G)
    C.check_stat_words(C.words_of(good), good)
    holed = rows.clone()
    holed[256:272] = 0                                                                     # the first 4 x 4 image
    _rejected(C.words_of(C.group_sums(holed, r, G)), good)
    # rows behind M counted: they carry the last row's key
    _rejected(C.words_of(C.group_sums(torch.cat([rows, rows[-3:]]), r, G, keys=torch.cat([keys, keys[-3:]]))), good)
    # the group behind the last one: its accumulator is the next key's first group
    cpg, nkeys = r.case[2] // G, r.case[0] * len(r.case[5])
    t = rows[:, :cpg].to(torch.int64)
    s1 = torch.zeros(nkeys, dtype=torch.int64).index_add_(0, keys, t.sum(1)).tolist()
    s2 = torch.zeros(nkeys, dtype=torch.int64).index_add_(0, keys, (t * t).sum(1)).tolist()
    spilled = list(good)
    for k in range(nkeys - 1):
        spilled[(k + 1) * G * 2] += s1[k]
        spilled[(k + 1) * G * 2 + 1] += s2[k]
    _rejected(C.words_of(spilled), good)
    _rejected(C.words_of(C.group_sums(rows, r, G, keys=(keys + 1) % nkeys)), good)         # a key shifted by one image
    # a sum that differs by one unit of the low word; a unit of the high word without its 2^47 taken from the low one; the
    # same carry done right is the same sum (atomics may leave a low word beyond 47 bits)
    w = C.words_of(good)
    w[3][0] += 1
    _rejected(w, good)
    w = C.words_of(good)
    w[3][1] += 1
    _rejected(w, good)
    w[3][0] -= 1 << 47
    C.check_stat_words(w, good)
    # negative sums and sums beyond 2^15 (the high word) round-trip
    C.check_stat_words(C.words_of([-5, 3 << 20, -(7 << 33), 0]), [-5, 3 << 20, -(7 << 33), 0])
