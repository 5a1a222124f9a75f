"""The list plan of the weight gradient (csrc/conv_plan.h: plan_wgrad_list, wgrad_list_decode) on the CPU: the header is
built for the host (tests/wgrad_list_plan_host.cpp, g++) and asked for lists of 1-4 entries, lists with calls the list
kernel does not take and call sequences longer than one list, on devices of 64, 256 and 304 CUs."""
import ctypes
import itertools
import os
import subprocess

import pytest

import conv_plan_lib as P
import conv_variant_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
LL = ctypes.c_longlong
NCUS = (64, 256, 304)
SHAPE_INTS = 29

# (layer, dtype, with_bias, cu_budget): the small ragged shapes of the variant table and layers of the students' sizes
TR_ROWS = [r for r in C.ROWS if r.list == "wgrad_tr"]
SMALL_ROW = next(r for r in C.ROWS if r.list == "wgrad_small")
F32_ROW = next(r for r in C.ROWS if r.list == "wgrad")
BIG = [(16, 128, 256, 3, 1, [(16, 16)]), (16, 256, 128, 1, 1, [(16, 16)]), (16, 64, 128, 3, 1, [(32, 32)]),
       (16, 32, 64, 3, 1, [(64, 64)]), (16, 256, 256, 3, 1, [(32, 32), (16, 16), (8, 8)]), (16, 16, 32, 3, 1, [(128, 128)])]


def _call(case, dtype=P.BF16, bias=0, budget=0):
    return (P.Layer(*case), dtype, bias, budget)


LISTABLE = [_call(r.case) for r in TR_ROWS] + [_call(c, bias=i % 2, budget=(0, 64, 128)[i % 3]) for i, c in enumerate(BIG)]
# (call, option wgrad.small): a narrow-family row (forced, as the table runs it) and fp32 rows
NOT_LISTABLE = [(_call(SMALL_ROW.case), 1), (_call(F32_ROW.case, dtype=P.F32), -1), (_call(F32_ROW.case, dtype=P.F32, bias=1), -1)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("wgrad_list_plan")), "libwgradlist.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "wgrad_list_plan_host.cpp")])
    return ctypes.CDLL(so)


def plan(lib, calls, ncu, begin=0, wgrad_small=-1):
    n = len(calls)
    shapes = (ctypes.c_int * (SHAPE_INTS * n))()
    for i, (layer, _, _, _) in enumerate(calls):
        v = list(layer.shape("wgrad"))
        shapes[SHAPE_INTS * i:SHAPE_INTS * i + len(v)] = v
    ints = lambda k: (ctypes.c_int * n)(*[c[k] for c in calls])      # noqa: E731
    nmax = lib.wl_list_max()
    out, per = (LL * (4 + 5 * nmax))(), (LL * (5 * n))()
    lib.wl_plan(shapes, ints(1), ints(2), ints(3), n, wgrad_small, ncu, begin, out, per)
    slots = [dict(zip(("call", "variant", "grid_x", "grid_y", "first_block"), out[4 + 5 * e:9 + 5 * e])) for e in range(out[0])]
    own = [dict(zip(("listable", "family", "grid_x", "grid_y", "lds"), per[5 * i:5 * i + 5])) for i in range(n)]
    return dict(n=out[0], end=out[1], grid=out[2], lds=out[3], slots=slots), own


def check_list(lib, L, own, begin):
    """One list against the calls' own plans."""
    first = 0
    for e, s in enumerate(L["slots"]):
        o = own[s["call"]]
        assert o["listable"] and o["family"] == P.WG_TR
        assert (s["grid_x"], s["grid_y"]) == (o["grid_x"], o["grid_y"]), "an entry keeps its own launch's grid"
        assert s["variant"] in (16, 32, 64, 128)
        assert s["first_block"] == first, "first blocks are the prefix sum of the entries' grids"
        if e:
            assert s["first_block"] > L["slots"][e - 1]["first_block"], "strictly increasing"
        first += s["grid_x"] * s["grid_y"]
    assert L["grid"] == first == sum(s["grid_x"] * s["grid_y"] for s in L["slots"])
    assert L["lds"] == max([own[s["call"]]["lds"] for s in L["slots"]], default=0)
    calls_in = [s["call"] for s in L["slots"]]
    assert calls_in == sorted(calls_in) and all(begin <= c < L["end"] for c in calls_in)
    # every listable call of [begin, end) has a slot; every other call has none
    assert calls_in == [i for i in range(begin, L["end"]) if own[i]["listable"]]
    # every workgroup is exactly one (entry, block_x, block_y) inside that entry's grid
    gx = (ctypes.c_int * 4)(*[s["grid_x"] for s in L["slots"]] + [0] * (4 - L["n"]))
    gy = (ctypes.c_int * 4)(*[s["grid_y"] for s in L["slots"]] + [0] * (4 - L["n"]))
    seen, out = set(), (ctypes.c_int * 3)()
    for block in range(L["grid"]):
        lib.wl_decode(gx, gy, L["n"], block, out)
        e, bx, by = out[0], out[1], out[2]
        assert 0 <= e < L["n"] and 0 <= bx < L["slots"][e]["grid_x"] and 0 <= by < L["slots"][e]["grid_y"], (block, e, bx, by)
        seen.add((e, bx, by))
    assert len(seen) == L["grid"], "two workgroups decode to the same tile"


def test_argument_struct_under_the_kernel_argument_limit(lib):
    assert lib.wl_list_max() == 4
    assert 0 < lib.wl_arg_bytes() < lib.wl_arg_limit() == 4096


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("n", (1, 2, 3, 4))
def test_lists_of_listable_calls(lib, ncu, n):
    combos = list(itertools.combinations(range(len(LISTABLE)), n))
    for pick in combos[::max(1, len(combos) // 40)]:
        for order in (pick, pick[::-1]):
            calls = [LISTABLE[i] for i in order]
            L, own = plan(lib, calls, ncu)
            assert L["n"] == n and L["end"] == n and all(o["listable"] for o in own)
            check_list(lib, L, own, 0)


@pytest.mark.parametrize("ncu", NCUS)
def test_every_variant_is_listable(lib, ncu, tmp_path):
    seen = set()
    for c in LISTABLE:
        L, own = plan(lib, [c], ncu)
        assert L["n"] == 1
        seen.add(L["slots"][0]["variant"])
    assert seen == {v[0] for v in P.variants(P.build_lib(tmp_path), "wgrad_tr")}      # all of KD6D_CONV_WGRAD_TR_TILES


@pytest.mark.parametrize("ncu", NCUS)
def test_calls_the_list_kernel_does_not_take(lib, ncu):
    for bad, small in NOT_LISTABLE:
        for pos in range(4):
            calls = [LISTABLE[0], LISTABLE[5], LISTABLE[9]]
            calls.insert(pos, bad)
            L, own = plan(lib, calls, ncu, wgrad_small=small)
            assert not own[pos]["listable"] and own[pos]["family"] != P.WG_TR
            assert L["n"] == 3 and L["end"] == 4 and pos not in [s["call"] for s in L["slots"]]
            check_list(lib, L, own, 0)
    # nothing listable at all: an empty list that still consumes the calls
    L, own = plan(lib, [NOT_LISTABLE[1][0], NOT_LISTABLE[2][0]], ncu)
    assert L["n"] == 0 and L["grid"] == 0 and L["end"] == 2


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("n", (5, 6, 9, 13))
def test_more_calls_than_one_list(lib, ncu, n):
    pool = LISTABLE + [c for c, _ in NOT_LISTABLE[1:]]
    calls = [pool[(3 * i) % len(pool)] for i in range(n)]
    begin, covered = 0, []
    while begin < n:
        L, own = plan(lib, calls, ncu, begin=begin)
        assert L["end"] > begin and L["n"] <= 4
        check_list(lib, L, own, begin)
        covered += [s["call"] for s in L["slots"]]
        # a list that is not the last one is full
        if L["end"] < n:
            assert L["n"] == 4
        begin = L["end"]
    assert begin == n
    listable = [i for i in range(n) if own[i]["listable"]]
    assert covered == listable, "consecutive lists keep the call order and take every listable call once"
