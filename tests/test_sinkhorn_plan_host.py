"""CPU: the host decisions of csrc/sinkhorn_dense.hip -- epsilon schedule, workspace layout, which softmin kernel a pass
takes, rows per workgroup and grids -- built for the host with g++ from the SAME header the launcher includes
(csrc/sinkhorn_plan.h through tests/sinkhorn_plan_host.cpp)."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from oracle.sinkhorn_ref import epsilon_schedule

HERE = os.path.dirname(os.path.abspath(__file__))
LL, I, D_ = ctypes.c_longlong, ctypes.c_int, ctypes.c_double
F = lambda v: float(np.float32(v))                      # noqa: E731  the value a float argument carries
DIFF, MATRIX, SCREEN = 0, 1, 2
REGIONS = ("la", "lb", "pot0", "pot1", "grad_xx", "grad_xy", "center", "n2", "xs", "ys", "xt", "yt", "partials")
CONSTANTS = ("threads", "rows", "grad_rows", "mrows", "mrows_wide", "wide_from", "split_bytes", "yt_bytes", "yt_pad",
             "center_wgs", "max_steps", "center_floats", "slack_floats")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sinkhorn_plan") / "libsinkhornplan.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(HERE, "sinkhorn_plan_host.cpp")])
    L = ctypes.CDLL(so)
    L.sp_mfma_eps_rel.restype = D_
    L.sp_schedule.argtypes = [D_, D_, D_, D_, ctypes.POINTER(D_), I, ctypes.POINTER(D_)]
    L.sp_lam.argtypes, L.sp_lam.restype = [D_] * 5, ctypes.c_float
    L.sp_workspace.argtypes, L.sp_workspace.restype = [I, I, I, I, ctypes.POINTER(LL)], LL
    L.sp_path.argtypes = [I, D_, D_, LL, LL, I]
    L.sp_screen_threshold.argtypes, L.sp_screen_threshold.restype = [D_, D_], ctypes.c_float
    L.sp_matrix_rows.argtypes = [I, LL]
    L.sp_softmin_launch.argtypes = [I] * 6 + [ctypes.POINTER(I)]
    c = (I * len(CONSTANTS))()
    L.sp_constants(c)
    L.k = dict(zip(CONSTANTS, c))
    return L


def _schedule(L, d, blur, scaling, reach=0.5, cap=5000):
    vals, facts = (D_ * cap)(), (D_ * 2)()
    n = L.sp_schedule(d, blur, scaling, reach, vals, cap, facts)
    return n, list(vals[:min(n, cap)]), facts[0], facts[1]


def test_constants(plan):
    assert plan.k == {"threads": 512, "rows": 256, "grad_rows": 128, "mrows": 64, "mrows_wide": 128, "wide_from": 8192,
                      "split_bytes": 96, "yt_bytes": 64, "yt_pad": 128, "center_wgs": 64, "max_steps": 4096,
                      "center_floats": 64, "slack_floats": 16}
    assert plan.sp_mfma_eps_rel() == 1.5e-4


# ---- schedule ---------------------------------------------------------------------------------------------------------
def test_schedule_matches_the_oracle(plan):
    """Counts equal; values within 4 n 2^-52 max(1, |2 ln d|, |2 ln blur|) relative: numpy's arange accumulates
    start + i ((start + step) - start), the header e_start + (i - 1) e_step, so the exponents differ by a few ulp of the
    largest exponent per step."""
    worst = 0.0
    for d in (9e-4, 1e-3, 0.7, 1.3, F(math.sqrt(2.0)), 22.6, 905.1):
        for blur in (F(0.001), F(0.05), F(0.5)):
            for scaling in (F(0.5), F(0.8), F(0.9), F(0.99)):
                want = epsilon_schedule(2, d, blur, scaling)
                n, got, dd, rho = _schedule(plan, d, blur, scaling)
                assert n == len(want) == len(got), (d, blur, scaling, n, len(want))
                assert dd == d and rho == 0.25
                assert got[0] == d * d and got[-1] == blur * blur
                bound = 4.0 * n * 2.0 ** -52 * max(1.0, abs(2 * math.log(d)), abs(2 * math.log(blur)))
                rel = max(abs(g - w) / w for g, w in zip(got, want))
                assert rel <= bound, (d, blur, scaling, rel, bound)
                worst = max(worst, rel / bound)
    print("worst share of the bound: %.3f" % worst)


def test_schedule_degenerate_ends(plan):
    for d, blur in ((0.05, F(0.05)), (0.01, F(0.05)), (F(0.05), F(0.05))):
        n, got, _, _ = _schedule(plan, d, blur, 0.5)
        assert n == 2 and got == [d * d, blur * blur]
    n, got, d, _ = _schedule(plan, 0.0, F(0.001), 0.5)
    assert n == 2 and d == 1e-12 and got[0] == 1e-24
    assert _schedule(plan, 1e-13, F(0.001), 0.5)[2] == 1e-12 and _schedule(plan, 2e-12, F(0.001), 0.5)[2] == 2e-12
    # the 4096-step cap of the geometric part
    n, got, _, _ = _schedule(plan, 1e6, 1e-6, 0.9999)
    assert n == 4098 and len(got) == 4098 and got[0] == 1e12 and got[-1] == 1e-6 * 1e-6
    assert got[1] == math.exp(2 * math.log(1e6)) and got[4096] == math.exp(2 * math.log(1e6) + 4095 * (2 * math.log(0.9999)))
    # scaling >= 1 (the entry point refuses it): no geometric part
    assert _schedule(plan, 1.0, F(0.001), 1.0)[0] == 2


def test_lam(plan):
    for reach in (0.0, -1.0):
        assert _schedule(plan, 1.0, 0.05, 0.5, reach)[3] == -1.0
        for eps in (1e-6, 1.0, 100.0):
            assert plan.sp_lam(1.0, 0.05, 0.5, reach, eps) == 1.0
    reach = F(0.3)
    assert _schedule(plan, 1.0, 0.05, 0.5, reach)[3] == reach * reach
    for eps in (1e-6, 0.09, 1.0, 100.0):
        assert plan.sp_lam(1.0, 0.05, 0.5, reach, eps) == np.float32(1.0 / (1.0 + eps / (reach * reach)))


# ---- workspace --------------------------------------------------------------------------------------------------------
def _old_total(N, M, D):
    """kd6d_sinkhorn_dense_workspace_floats before the layout moved into the header, literally"""
    n128, m128 = (N + 127) & ~127, (M + 127) & ~127
    return N + M + 4 * (N + M) + 2 * N * D + 64 + (25 * (N + M) + 16 + 16 * (n128 + m128) if D == 16 else 0)


SIZES = (1, 63, 64, 127, 128, 129, 300, 8191, 8192, 16384)


def test_workspace_layout(plan):
    from kd6d import _lib
    out = (LL * 26)()
    for D, N, M in itertools.product((2, 4, 8, 16), SIZES, SIZES):
        assert _lib.lib.kd6d_sinkhorn_dense_workspace_floats(N, M, D) == _old_total(N, M, D)
        for mis in (0, 4, 8, 12):
            total = plan.sp_workspace(N, M, D, mis, out)
            assert total == _old_total(N, M, D), (N, M, D, mis)
            r = {name: (out[2 * i], out[2 * i + 1]) for i, name in enumerate(REGIONS)}
            # sizes
            f = 4
            assert r["la"] == (0, N * f) and r["lb"][1] == M * f
            assert r["pot0"][1] == r["pot1"][1] == 2 * (N + M) * f
            assert r["grad_xx"][1] == r["grad_xy"][1] == N * D * f and r["center"][1] == 64 * f
            if D == 16:
                assert r["n2"][1] == (N + M) * f and r["xs"][1] == N * 96 and r["ys"][1] == M * 96
                assert r["xt"][1] == ((N + 127) & ~127) * 64 and r["yt"][1] == ((M + 127) & ~127) * 64
                assert r["partials"] == (r["xt"][0], 2 * 64 * 16 * f)
                assert r["partials"][1] <= r["xt"][1]                    # the one allowed overlap: partials inside xt
            else:
                # nothing beyond the centre is counted
                assert all(r[name][1] == 0 for name in REGIONS[7:])
                assert total * f == r["center"][0] + r["center"][1]
            # pairwise disjoint, in this order, inside the total
            end = 0
            for name in REGIONS[:-1]:
                off, size = r[name]
                assert off >= end and size >= 0, (name, N, M, D, mis)
                end = off + size
            assert end <= total * f
            if D == 16:
                for name in ("xs", "ys", "xt", "yt"):
                    assert (r[name][0] + mis) % 16 == 0, (name, N, M, D, mis)
                assert r["xs"][0] - (r["n2"][0] + r["n2"][1]) < 16    # no more than the alignment between them
    # the borrowed partials fill xt of the smallest problem exactly
    plan.sp_workspace(1, 1, 16, 0, out)
    assert out[2 * 12 + 1] == out[2 * 10 + 1] == 8192


# ---- path table -------------------------------------------------------------------------------------------------------
# D = 16: (dense_mfma, dense_screen, gradient-carrying?) -> path at eps one ulp below, at and one ulp above the rule
# kMfmaEpsRel * diameter^2
PATHS_D16 = {
    (0, 0, 0): (DIFF, DIFF, DIFF),       (0, 0, 1): (DIFF, DIFF, DIFF),
    (0, 1, 0): (DIFF, DIFF, DIFF),       (0, 1, 1): (DIFF, DIFF, DIFF),
    (1, 0, 0): (DIFF, MATRIX, MATRIX),   (1, 0, 1): (DIFF, MATRIX, MATRIX),
    (1, 1, 0): (SCREEN, MATRIX, MATRIX), (1, 1, 1): (SCREEN, MATRIX, MATRIX),
    (2, 0, 0): (MATRIX, MATRIX, MATRIX), (2, 0, 1): (MATRIX, MATRIX, MATRIX),
    (2, 1, 0): (MATRIX, MATRIX, MATRIX), (2, 1, 1): (MATRIX, MATRIX, MATRIX),
    # mode 3: the gradient-carrying launch keeps the difference form where the rule holds; its companion does not
    (3, 0, 0): (DIFF, MATRIX, MATRIX),   (3, 0, 1): (DIFF, DIFF, DIFF),
    (3, 1, 0): (SCREEN, MATRIX, MATRIX), (3, 1, 1): (SCREEN, DIFF, DIFF),
}


def test_path_table(plan):
    rel = plan.sp_mfma_eps_rel()
    for d in (0.01, 1.3, 22.6):
        at = rel * d * d
        eps3 = (float(np.nextafter(at, 0.0)), at, float(np.nextafter(at, np.inf)))
        for (mfma, screen, grad), want in PATHS_D16.items():
            assert tuple(plan.sp_path(16, e, d, mfma, screen, grad) for e in eps3) == want, (d, mfma, screen, grad)
            for D in (2, 4, 8):
                assert [plan.sp_path(D, e, d, mfma, screen, grad) for e in eps3] == [DIFF] * 3
        # mode 2 at any eps
        for e in (1e-30, 1e-12, at * 1e-3):
            assert plan.sp_path(16, e, d, 2, 0, 0) == MATRIX and plan.sp_path(16, e, d, 2, 1, 0) == MATRIX
    assert len(PATHS_D16) == 4 * 2 * 2


def test_screen_threshold(plan):
    for eps, d in ((1e-6, 1.0), (2.5e-5, 1.3), (1e-2, 22.6)):
        want = 40.0 + (0.5 / eps) * 1.4426950408889634 * d * d * 2.0 ** -20
        assert plan.sp_screen_threshold(eps, d) == np.float32(want)


# ---- rows and grids ---------------------------------------------------------------------------------------------------
def test_matrix_rows(plan):
    want = {(-1, 1): 64, (-1, 8191): 64, (-1, 8192): 128, (7, 1): 64, (7, 8191): 64, (7, 8192): 128,
            (64, 1): 64, (64, 8191): 64, (64, 8192): 64, (128, 1): 128, (128, 8191): 128, (128, 8192): 128}
    for (opt, nmax), rows in want.items():
        assert plan.sp_matrix_rows(nmax, opt) == rows, (opt, nmax)


def test_softmin_launches(plan):
    out = (I * 4)()
    threads = plan.k["threads"]
    # (path, gradient-carrying?) -> rows per workgroup (None: the matrix_rows() value), block (None: 4 x rows, a wave per
    # 32 rows and column half), rows covered: max(N, M) or N
    forms = {(DIFF, 0): (256, threads, "nmax"), (DIFF, 1): (128, threads, "nmax"),
             (MATRIX, 0): (None, None, "nmax"), (MATRIX, 1): (64, 256, "N"),
             (SCREEN, 0): (None, None, "nmax"), (SCREEN, 1): (None, None, "N")}
    sizes = (1, 64, 65, 128, 129, 8192)
    for (path, grad), (rows, block, over) in forms.items():
        for N, M, mrows in itertools.product(sizes, sizes, (64, 128)):
            for softmins in ((2,) if grad else (4, 2)):
                plan.sp_softmin_launch(path, grad, softmins, N, M, mrows, out)
                r, gx, gy, b = out
                assert r == (rows or mrows) and b == (block or {64: 256, 128: 512}[mrows]), (path, grad, N, M, mrows)
                extent = max(N, M) if over == "nmax" else N
                assert gx * r >= extent > (gx - 1) * r, (path, grad, N, M, mrows)
                assert gy == softmins
