"""CPU: stem_bwd_rule of csrc/conv_plan.h -- which blocks take the fused pooled-BatchNorm backward + weight gradient
(kd6d_bn_pool_bwd_wgrad, csrc/stem_bwd.hip), on what grid, with how much LDS and how large a slab -- built with g++ from
the same header the library plans with (tests/stem_plan_host.cpp)."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BF16, F32 = 0, 1
NCU = 256
FIELDS = "NOUT R tiles_per_img ntiles Qpad prow grid parts lds slab_floats tiles_per_wg tr_m_chunk tr_parts".split()
# (B, H, W, Cout): the stems of darknet_tiny_h / darknet_tiny at the benchmark batch, and the shapes of
# tests/test_stem_fused_gpu.py
STEMS = [(16, 256, 256, 8), (16, 256, 256, 16)]
TEST_SHAPES = [(1, 4, 4, 8), (2, 8, 8, 8), (3, 20, 12, 16), (1, 6, 128, 8), (2, 64, 64, 8), (4, 128, 128, 8)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("stemplan")), "libstemplan.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "stem_plan_host.cpp")])
    return ctypes.CDLL(so)


def plan(lib, B, H, W, cout, cin=8, ks=3, stride=1, pad=None, dtype=BF16, bias=0, need_dx=0, fused=1, budget=0, row0=(0, 0)):
    pad = ks // 2 if pad is None else pad
    geom = (ctypes.c_int * 10)(B, cin, cout, ks, stride, pad, H, W, row0[0], row0[1])
    out = (ctypes.c_longlong * len(FIELDS))()
    if not lib.sp_plan(geom, dtype, bias, need_dx, fused, NCU, budget, out):
        return None
    return dict(zip(FIELDS, out))


@pytest.mark.parametrize("shape", STEMS + TEST_SHAPES)
def test_rule_accepts_the_stem_shapes(lib, shape):
    B, H, W, cout = shape
    p = plan(lib, B, H, W, cout)
    assert p is not None and p["NOUT"] == cout
    # whole pool windows per tile, at most 512 pixels: the kernel keeps one or two work items per thread
    assert p["R"] % 2 == 0 and 2 <= p["R"] <= H and p["R"] * W <= 512
    assert p["tiles_per_img"] == -(-H // p["R"]) and p["ntiles"] == B * p["tiles_per_img"]
    Wp = W + 2
    assert p["Qpad"] % 32 == 0 and p["R"] * W <= p["Qpad"] < p["R"] * W + 32       # whole 32-pixel steps
    # the furthest patch row a fragment read touches: the last tap of the last (tail) pixel; then eight zero rows; whole
    # 1-KB LDS-DMA bursts
    last = p["Qpad"] - 1
    furthest = (last // W) * Wp + last % W + 1 + 2 * Wp + 2
    assert p["prow"] % 64 == 0 and p["prow"] - 8 > furthest
    assert p["prow"] - 8 >= (p["R"] + 2) * Wp + 1
    assert 128 + p["Qpad"] * 2 * cout + p["prow"] * 16 <= p["lds"] <= 64 << 10
    assert p["lds"] >= 16 * 80 * 4


@pytest.mark.parametrize("shape", STEMS + TEST_SHAPES)
@pytest.mark.parametrize("budget", [0, 4, 64])
def test_grid_is_fixed_and_the_slab_holds_it(lib, shape, budget):
    """parts = the launch's fixed grid, known from the geometry and the budget alone (before any graph capture); the slab is
    parts x cout*9*8 floats, what ParamStore.slab(entry, parts) allocates for the (cout, 3, 3, 8) weight entry."""
    B, H, W, cout = shape
    p = plan(lib, B, H, W, cout, budget=budget)
    # consecutive tiles per workgroup: as many as fit the pixel split of the transposing kernel for the same shape / budget
    assert p["tiles_per_wg"] == max(1, p["tr_m_chunk"] // (p["R"] * W))
    assert p["grid"] == p["parts"] == -(-p["ntiles"] // p["tiles_per_wg"]) and 1 <= p["parts"] <= p["ntiles"]
    assert p["slab_floats"] == p["parts"] * cout * 72
    assert p["slab_floats"] * 4 <= 8 << 20
    assert plan(lib, B, H, W, cout, budget=budget) == p


def test_benchmark_stem_plan(lib):
    """The students' stems: a workgroup's tiles are exactly one pixel split of the transposing kernel, in whole 32-pixel
    steps -- the condition under which the slab holds that kernel's partial images bit for bit."""
    for cout in (8, 16):
        for budget in (0, 128, 64):
            p = plan(lib, 16, 256, 256, cout, budget=budget)
            assert (p["R"], p["ntiles"], p["tiles_per_wg"], p["grid"]) == (2, 2048, 4, 512)
            assert p["tiles_per_wg"] * p["R"] * 256 == p["tr_m_chunk"] and p["parts"] == p["tr_parts"]
            assert (p["R"] * 256) % 32 == 0 and 256 % p["R"] == 0
            assert p["lds"] <= 40 << 10


def test_rule_rejects_everything_else(lib):
    B, H, W = 16, 256, 256
    assert plan(lib, B, H, W, 8) is not None
    assert plan(lib, B, H, W, 8, stride=2) is None
    assert plan(lib, B, H, W, 8, ks=1) is None
    assert plan(lib, B, H, W, 8, pad=0) is None
    for cin in (16, 32):
        assert plan(lib, B, H, W, 8, cin=cin) is None
    for cout in (24, 32, 64):
        assert plan(lib, B, H, W, cout) is None
    assert plan(lib, B, H, W, 8, need_dx=1) is None                  # a block whose input wants its gradient
    assert plan(lib, B, H, W, 8, dtype=F32) is None
    assert plan(lib, B, H, W, 8, bias=1) is None
    assert plan(lib, B, H, W, 8, fused=0) is None                    # option stem.fused = 0
    assert plan(lib, B, H, W, 8, row0=(64, 0)) is None and plan(lib, B, H, W, 8, row0=(0, 64)) is None
    assert plan(lib, 2, 6, 7, 8) is None and plan(lib, 2, 7, 6, 8) is None      # odd sizes: no whole pool windows
    assert plan(lib, 2, 64, 258, 8) is None                          # wider than a tile of two rows holds
