"""CPU: the per-layer convolution kernel choice of csrc/conv_plan.h -- family, variant, grid, block, dynamic LDS and
launch arguments of every forward / data-gradient / weight-gradient call -- built for the host with g++ from the SAME
header the launchers include (through tests/conv_plan_host.cpp).  libkd6d.so is not loaded here.

(a) the answers the library gave through its public ABI BEFORE the choice moved into the header
    (tests/golden/conv_plan_parent.json, tests/golden/make_golden_conv_plan.py);
(b) the kernels the library launched on an MI355X before the move, one rocprofv3 kernel trace per layer list
    (tests/golden/conv_dispatch_b16.json, tests/golden/make_golden_conv_dispatch.py);
(c) invariants of every plan over a generated sweep of shapes and option values."""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import step_layers  # noqa: E402

from conv_plan_lib import (BF16, F32, GLDS, HALO, IGEMM, LISTS, NCU, OPT_DEFAULT, SMALLC, SPLITK, WG_GENERIC, WG_SMALL,  # noqa: E402
                           WG_TR, WS_BYTES, Layer, build_lib, fusable, plan_conv, plan_wgrad)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_lib(tmp_path_factory.mktemp("conv_plan"))


def _ceil(a, b):
    return -(-a // b)


# ---- (a) the library's answers before the move --------------------------------------------------------------------
def test_header_reproduces_the_recorded_answers_of_the_public_abi(lib):
    with open(os.path.join(HERE, "golden", "conv_plan_parent.json")) as f:
        doc = json.load(f)
    assert doc["ncu"] == NCU and len(doc["layers"]) == 83
    n_parts = n_fus = n_true = 0
    for l in doc["layers"]:
        parts, fus = iter(l["parts"]), iter(l["fusable"])
        for b in doc["batches"]:
            layer = Layer(b, l["cin"], l["cout"], l["k"], l["stride"], l["levels"])
            for dt in range(len(doc["dtypes"])):
                for bias in doc["bias"]:
                    for budget in doc["budgets"]:
                        for small in doc["wgrad_small"]:
                            got = plan_wgrad(lib, layer, dt, bias, budget, wgrad_small=small).parts
                            assert got == next(parts), (l["name"], b, dt, bias, budget, small)
                            n_parts += 1
                for _, kind, groups in doc["norms"]:
                    for pairing in doc["halo_pairing"]:
                        want = next(fus)
                        assert fusable(lib, layer, dt, kind, groups, halo_pairing=pairing) == want, (l["name"], b, dt, kind, groups)
                        n_fus += 1
                        n_true += want
        assert next(parts, None) is None and next(fus, None) is None
    assert n_parts == 83 * 128 and n_fus == 83 * 48 and 0 < n_true < n_fus          # the sweep discriminates


# ---- (b) the kernels the library launched before the move ---------------------------------------------------------
def _tf(v):
    return "true" if v else "false"


def _conv_dispatches(p, mode):
    """(kernel<template arguments>, grid x / y in threads, block, LDS bytes) as a kernel trace reports a planned launch: the
    trace gives grid sizes in threads (workgroups x block) and the dynamic LDS as launched."""
    if p.family == SMALLC:
        name = "conv3x3_smallc_kernel<%d,%d,%d>" % (p.CG, p.NB, mode)
    elif p.family == HALO:
        name = "conv3x3_halo_kernel<%d,%d,%d,%d,%d,%d,%s,%s>" % (p.BP, p.BC, p.WP, p.WC, mode, p.HMAX, _tf(p.PDB), _tf(p.NORM))
    elif p.family in (SPLITK, GLDS):
        name = "conv_igemm_glds_kernel<%d,%d,%d,%d,%d,%d,%s>" % (p.BP, p.BC, p.WP, p.WC, mode, p.NSTAGE, _tf(p.family == SPLITK))
    else:
        name = "conv_igemm_kernel<bf16,%d,%d,%d,%d,%d,%s,%s>" % (p.BP, p.BC, p.WP, p.WC, mode, _tf(p.XF), _tf(p.NORM))
    out = [[name, p.grid_x * p.threads, p.grid_y, p.threads, p.lds]]
    if p.family == SPLITK:
        out.append(["splitk_finalize_kernel", p.finalize_grid * 256, 1, 256, 0])
    return out


def _wgrad_dispatches(p):
    if p.family == WG_SMALL:
        name = "conv_wgrad_small_kernel<%d,%d,%d>" % (p.CG, p.NB, p.KS)
    elif p.family == WG_TR:
        name = "conv_wgrad_tr_kernel<%d,%d,%d>" % (p.BN, p.WN, p.WJ)
    else:
        name = "conv_wgrad_kernel<float,%d,%d,%d,%d>" % (p.BN, p.BJ, p.WN, p.WJ)
    return [[name, p.grid_x * 256, p.grid_y, 256, p.lds]]


def test_plans_name_the_kernels_the_library_launched_on_the_gpu(lib):
    with open(os.path.join(HERE, "golden", "conv_dispatch_b16.json")) as f:
        doc = json.load(f)
    sets = {"all": step_layers.TEACHER + step_layers.STUDENT, "teacher640": step_layers.TEACHER_640,
            "student640": step_layers.STUDENT_640}
    assert sorted(doc["runs"]) == sorted("%s_%s" % (k, s) for k in ("fwd", "dgrad", "wgrad") for s in sets)
    n = 0
    for run, recorded in doc["runs"].items():
        kind, which = run.split("_")
        want = []
        for name, cin, cout, k, stride, levels in sets[which]:
            if name.startswith(("t.", "t640.")) and kind != "fwd":       # tools/bench_conv.py: the teacher is frozen
                continue
            layer = Layer(step_layers.B, cin, cout, k, stride, levels)
            if kind == "wgrad":
                want += _wgrad_dispatches(plan_wgrad(lib, layer))
            else:
                want += _conv_dispatches(plan_conv(lib, layer, kind, ws=int(kind == "fwd")), int(kind == "dgrad"))
        assert want == recorded, run
        n += len(recorded)
    assert n == 158 and any(r[0] == "splitk_finalize_kernel" for r in doc["runs"]["fwd_all"])


# ---- (c) invariants over a generated sweep ------------------------------------------------------------------------
CS = (8, 16, 32, 64, 128, 192, 256, 512, 1024)
NS = (8, 16, 24, 32, 48, 64, 128, 240, 256, 1024)
PYRAMIDS = ([(2, 2)], [(32, 32)], [(64, 64)], [(60, 80)], [(256, 256)], [(240, 320)], [(480, 640)],
            [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], [(60, 80), (30, 40), (15, 20), (8, 10), (4, 5)])
BATCHES = (1, 16, 48)
# every option at its documented values (csrc/kd6d_common.h), one at a time
OPTION_RUNS = ([{}] + [{"halo": v} for v in (0, 1, 2, 3, 4, 5, 6, 9, 11, 12, 13, 14, 15)] + [{"halo_pairing": 0}, {"halo_wide": 0}]
               + [{"smallc": v} for v in (0, 1)] + [{"smallc_wmax": 256}] + [{"splitk": v} for v in (0, 104, 216)]
               + [{"tile": v} for v in (0, 1, 2, 3, 4)] + [{"wgrad_small": v} for v in (0, 1)])
FLAG_RUNS = ({}, {"stats": 1}, {"stats": 1, "groups": 8}, {"stats": 1, "replicas": 8}, {"stats": 1, "groups": 8, "norm": 1},
             {"stats": 1, "norm": 1})
OFF = {"halo": HALO, "smallc": SMALLC, "splitk": SPLITK, "tile": GLDS}


def _check_conv(p, layer, kind, flags, opts, pair, seen):
    o = dict(OPT_DEFAULT, **opts)
    M, N, C, K = layer.shape(kind)[0:4]
    what = (kind, layer.batch, layer.cin, layer.cout, layer.k, layer.stride, layer.levels, flags, opts, pair, dict(p))
    assert 0 < p.lds <= 163840, what
    assert p.grid_x == p.n_ptiles * p.n_ctiles > 0 and p.grid_y >= 1 and p.threads in (256, 512), what
    assert p.n_ptiles * p.BP >= M > (p.n_ptiles - 1) * p.BP and p.n_ctiles * p.BC >= N > (p.n_ctiles - 1) * p.BC, what
    for name, fam in OFF.items():
        assert not (o[name] == 0 and p.family == fam), what
    same = layer.k == 3 and layer.stride == 1
    if p.family == SPLITK:
        nk = _ceil(K, 64)
        assert kind == "fwd" and p.nsplit * p.nk_split >= nk > (p.nsplit - 1) * p.nk_split and p.grid_y == p.nsplit, what
        assert p.nsplit * M * N * 4 <= WS_BYTES and not flags.get("stats") and flags.get("ws"), what
        assert p.lds == (p.BP + p.BC) * 128 * p.NSTAGE and 0 < p.finalize_grid <= 2048, what
        seen["splitk"].add((p.BP, p.BC, p.WP, p.WC, p.NSTAGE, 0))
    elif p.family == HALO:
        assert same and C % 64 == 0 and p.halo == layer.wmax + 1 <= p.HMAX and p.total_rows == layer.rows_in, what
        assert layer.wmax <= (80 if o["halo_wide"] else 64), what
        assert p.PDB or p.halo <= 33, what                                  # the twins: maps <= 32 wide only
        if flags.get("norm"):
            assert kind == "fwd" and (p.BP, p.BC, p.NORM, p.fused_epilogue) == (128, 128, 1, 1), what
        seen["halo_norm" if p.NORM else "halo"].add((p.BP, p.BC, p.WP, p.WC, p.HMAX, p.PDB))
    elif p.family == SMALLC:
        assert same and C in (8, 16, 32) and p.halo == layer.wmax + 1 and p.total_rows == layer.rows_in, what
        if layer.wmax > 256:
            assert layer.wmax <= o["smallc_wmax"] and (256 + 2 * (layer.wmax + 1) + 1) * 2 * C <= 32768, what
        assert not flags.get("groups") and not flags.get("norm") and flags.get("replicas", 0) <= 1, what
        assert p.lds >= p.patch_bytes + p.wbytes + 1024 and p.patch_bytes >= (256 + 2 * p.halo + 1) * 2 * C, what
        seen["smallc"].add((p.CG, p.NB, 0, 0, 0, 0))
    elif p.family == GLDS:
        assert N > 32 and not flags.get("norm") and flags.get("replicas", 0) <= 1, what
        assert p.lds == (p.BP + p.BC) * 128 * p.NSTAGE, what
        seen["glds"].add((p.BP, p.BC, p.WP, p.WC, p.NSTAGE, 0))
    else:
        assert p.family == IGEMM and p.lds == (p.BP + p.BC) * 256 + (8 * C if p.XF else 0), what
        assert p.NORM == int(kind == "fwd" and not p.XF and bool(flags.get("norm") or flags.get("replicas", 0) > 1)), what
        seen["igemm"].add((p.BP, p.BC, p.WP, p.WC, 0, 0))
    if flags.get("norm") and kind == "dgrad":
        assert p.family in (GLDS, IGEMM) and not p.fused_epilogue, what


def _check_wgrad(p, layer, dtype, bias, opts, seen):
    o = dict(OPT_DEFAULT, **opts)
    M = layer.rows_out
    what = (layer.batch, layer.cin, layer.cout, layer.k, layer.stride, layer.levels, dtype, bias, opts, dict(p))
    assert p.parts >= 1 and 0 < p.lds <= 163840 and p.grid_x > 0 and p.grid_y > 0, what
    if p.family == WG_SMALL:
        assert dtype == BF16 and not bias and o["wgrad_small"] != 0 and p.R >= 1 and p.lds <= 144 * 1024, what
        assert p.parts == p.grid_x <= p.ntiles == layer.batch * p.tiles_per_img and p.tiles_per_img * p.R >= layer.levels[0][0], what
        seen["wgrad_small"].add((p.CG, p.NB, p.KS, 0, 0, 0))
    else:
        assert p.family == (WG_TR if dtype == BF16 else WG_GENERIC), what
        assert p.parts * p.m_chunk >= M > (p.parts - 1) * p.m_chunk and p.grid_y == p.parts, what
        assert p.grid_x == p.n_jtiles * _ceil(layer.cout, p.BN) and p.n_jtiles * p.BJ >= layer.k ** 2 * layer.cin, what
        seen["wgrad_tr" if dtype == BF16 else "wgrad"].add((p.BN, p.WN, p.WJ, 0, 0, 0) if dtype == BF16 else (p.BN, p.BJ, p.WN, p.WJ, 0, 0))


def test_invariants_of_every_plan_over_a_sweep(lib):
    seen = {n: set() for n in LISTS}
    for k in (1, 3):
        for stride in (1, 2):
            for levels in PYRAMIDS:
                for B in BATCHES:
                    for cin in CS:
                        for cout in NS:
                            layer = Layer(B, cin, cout, k, stride, levels)
                            for opts in OPTION_RUNS:
                                # (a forced patch-kernel variant can only matter where the patch kernels' shape rule holds)
                                if (opts.get("halo", 0) > 0 or opts.get("smallc", 0) > 0) and (k != 3 or stride != 1):
                                    continue
                                if "wgrad_small" in opts or not opts:
                                    for bias in (0, 1):
                                        _check_wgrad(plan_wgrad(lib, layer, BF16, bias, **opts), layer, BF16, bias, opts, seen)
                                if "wgrad_small" in opts:
                                    continue
                                for pair in ((0, 1) if ("halo" in opts or not opts) else (0,)):
                                    for kind in ("fwd", "dgrad"):
                                        if kind == "dgrad" and cout % 8:
                                            continue
                                        flags = {"ws": int(kind == "fwd")}
                                        _check_conv(plan_conv(lib, layer, kind, pair=pair, **flags, **opts), layer, kind, flags, opts,
                                                    pair, seen)
                            # default options: the flags that steer dispatch, fp32, BatchNorm on load
                            for flags in FLAG_RUNS:
                                if flags.get("groups") and cout % 8:
                                    continue
                                for kind in ("fwd", "dgrad") if flags.get("norm") else ("fwd",):
                                    _check_conv(plan_conv(lib, layer, kind, **flags), layer, kind, flags, {}, 0, seen)
                            _check_conv(plan_conv(lib, layer, "fwd", dtype=F32, ws=1), layer, "fwd", {"ws": 1}, {}, 0, seen)
                            assert plan_conv(lib, layer, "fwd", dtype=F32, ws=1).family == IGEMM
                            if stride == 1:
                                p = plan_conv(lib, layer, "fwd", xf=1, stats=1, replicas=8)
                                assert p.family == IGEMM and p.XF and not p.NORM
                                _check_conv(p, layer, "fwd", {"stats": 1}, {}, 0, seen)
                            _check_wgrad(plan_wgrad(lib, layer, F32, 0), layer, F32, 0, {}, seen)
    # every variant of every family's list is reached, and nothing outside the lists is ever planned
    buf = (ctypes.c_int * (6 * 64))()
    for i, name in enumerate(LISTS):
        listed = {tuple(buf[6 * r:6 * r + 6]) for r in range(lib.cp_variants(i, buf))}
        assert seen[name] == listed, (name, sorted(listed - seen[name]), sorted(seen[name] - listed))


def test_levels_packed_differently_stay_off_the_patch_kernels(lib):
    for cin, fam in ((8, SMALLC), (256, HALO)):
        assert plan_conv(lib, Layer(16, cin, 64, 3, 1, [(256, 256)] if cin == 8 else [(32, 32)]), smallc=1).family == fam
        assert plan_conv(lib, Layer(16, cin, 64, 3, 1, [(256, 256)] if cin == 8 else [(32, 32)], out_shift=16), smallc=1).family \
            not in (SMALLC, HALO)


def test_quirks_kept_as_they_were(lib):
    tower = Layer(16, 256, 256, 3, 1, [(60, 80), (30, 40), (15, 20), (8, 10), (4, 5)])
    # a forced twin (conv.halo 10-15) is ignored on maps wider than 32
    assert plan_conv(lib, tower, halo=12) == plan_conv(lib, tower)
    # split-K checks the workspace against the split count asked for, then recomputes the count from whole k-steps
    top = Layer(16, 512, 256, 3, 1, [(8, 8)])                # 72 k-steps, 1 MB per split, 64 MB of workspace
    p = plan_conv(lib, top, ws=1, halo=0, splitk=240)
    assert p.family == SPLITK and (p.nk_split, p.nsplit) == (2, 36)
    assert plan_conv(lib, top, ws=1, halo=0, splitk=270).family != SPLITK      # 70 asked for, though 36 would be launched
    # dgrad with a fused normalisation falls through the halo rule after a non-zero pick
    assert plan_conv(lib, Layer(16, 128, 128, 3, 1, [(32, 32)]), "dgrad", stats=1, norm=1).family in (GLDS, IGEMM)
    # conv.fuse_norm = 0: nothing is fusable
    lay = Layer(16, 128, 128, 3, 1, [(32, 32)])
    assert fusable(lib, lay, BF16, 1, 32) == 1 and fusable(lib, lay, BF16, 1, 32, fuse_norm=2) == 0
