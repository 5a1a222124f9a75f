"""CPU: the table of tests/conv_variant_cases.py (the rows of tests/test_conv_variants_gpu.py) against the host build of
csrc/conv_plan.h -- every compiled variant of every KD6D_CONV_*_TILES list has a row per direction, every row plans the
variant it declares whatever the device size, the integer pass is exact for every row, the table stays small, and the two
comparisons reject the results a broken tile kernel would give."""
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
    for name in P.LISTS:
        if name in C.OUT_OF_SCOPE:
            continue
        for v in P.variants(lib, name):
            for kind in C.DIRECTIONS[name]:
                for dtype in C.DTYPES[name]:
                    if (name, v, kind, dtype) not in have:
                        missing.append("%s %s %s %s" % (name, "x".join(str(x) for x in v), kind, dtype))
    return missing


def test_every_compiled_variant_has_a_row_per_direction(lib):
    assert set(C.DIRECTIONS) == set(C.DTYPES) == set(P.LISTS) - set(C.OUT_OF_SCOPE)
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
