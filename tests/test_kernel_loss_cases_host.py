"""CPU: the kernel distances' reference, builders and tolerances (tests/kernel_loss_cases.py), the opt-in surface
(--kd_kernel_losses, cfg['KD']['KERNEL_LOSSES'], SamplesLoss(kernel_losses=True)) and the argument checks of
kd6d_kernel_div_fwd_bwd / kd6d_kernel_dense_fwd_bwd, which fail on the host before any device is touched."""
import ctypes
import os
import re

import pytest
import torch

import kernel_loss_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "ape.yaml")
BASE = ["--config_file", YAML, "--config_file_t", YAML]
KD_DEFAULT_KEYS = {"LOSS_WEIGHT_KD", "LEVEL", "GLEVEL", "GTYPE", "GP", "GBLUR", "GnD", "WEIGHTED_OT", "DETACH", "SCALING",
                   "REACH"}


# ---- the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.KINDS)
def test_closed_form_agrees_with_autograd(kind):
    """fp64: value, dL/dalpha and dL/dx in closed form vs autograd of the three-term expression, at 1e-12 of the
    largest magnitude -- on sets with duplicate student points, a student point on a teacher point and a zero weight."""
    cases = [C.point_sets(3, N, M, D, 0) for N, M, D in ((1, 1, 2), (3, 5, 2), (16, 17, 2), (65, 17, 2), (40, 33, 16), (9, 70, 4))]
    cases += [tuple(t.permute(1, 0, 2) if t.dim() == 3 else t.t() for t in (L["a"][0], L["x"][0], L["b"][0], L["y"][0]))
              for L in (C.small_case(64, 65),)]
    for a, x, b, y in cases:
        dup = (x[:, :, None, :] == x[:, None, :, :]).all(-1).sum() > x.shape[0] * x.shape[1] or x.shape[1] < 3
        on_teacher = (x[:, :, None, :] == y[:, None, :, :]).all(-1).any() or x.shape[1] < 2
        assert bool(dup) and bool(on_teacher), "the builder's plants are missing"
        for blur in C.BLURS:
            ref = C.reference(a, x, b, y, kind, blur)
            got = C.closed_form(a, x, b, y, kind, blur, C.F64)
            for o in C.OUTPUTS:
                m = float(ref[o].abs().max())
                assert float((got[o] - ref[o]).abs().max()) <= 1e-12 * max(m, 1e-300), (kind, blur, o, tuple(x.shape))


def test_clamp_rule_coincident_points_have_the_clamped_value_and_no_gradient():
    """Two coincident points: k = -1e-4 (energy), exp(-1e-4) (laplacian), 1 (gaussian) on every pair, no gradient."""
    x = torch.full((1, 1, 2), 0.4)
    a, b = torch.full((1, 1), 0.5), torch.full((1, 1), 0.25)
    for kind, k0 in (("energy", -1e-4), ("laplacian", float(torch.exp(torch.tensor(-1e-4, dtype=C.F64)))), ("gaussian", 1.0)):
        r = C.reference(a, x, b, x.clone(), kind, 0.05)
        assert float(r["loss"]) == pytest.approx(k0 * (0.5 * 0.25 + 0.5 * 0.0625 - 0.125), rel=1e-12)
        assert float(r["grad_x"].abs().max()) == 0.0
        assert float(r["grad_alpha"]) == pytest.approx(k0 * (0.5 - 0.25), rel=1e-12)


def test_builders_keep_both_precisions_on_one_side_of_the_clamp():
    """Every launch / case the GPU tests use: no pair's clamped variable strictly inside (0, 1e-7), for either blur;
    the plants are there; a violating set is detected."""
    for N, M in C.SMALL_SIZES:
        L = C.small_case(N, M)
        assert L["xs"].dtype == torch.float32 and int(L["s_cnt"].min()) == N and int(L["t_cnt"].max()) == M
        for p in range(C.N_PROBLEMS):
            assert C.clamped_variables_ok(L["x"][p].permute(1, 0, 2), L["y"][p].permute(1, 0, 2))
        assert bool((L["xs"][~L["s_seg"]] == C.CANARY).all()) and int((~L["s_seg"]).sum()) >= C.N_PROBLEMS + 1
        starts = L["s_start"].tolist()
        assert starts != sorted(starts) and L["t_start"].tolist() != sorted(L["t_start"].tolist()), "segments in problem order"
        if N >= 4:
            assert bool((L["a"][0][2] == 0).all())
    for D in C.DENSE_DIMS:
        for N, M in C.DENSE_SIZES + (C.CROSS_SIZE,):
            a, x, b, y = C.dense_case(N, M, D)
            assert C.clamped_variables_ok(x[None], y[None]) and x.dtype == torch.float32
            assert float(x.min()) >= 0.3 - 1e-6 and float(x.max()) <= 0.6 + 2 * C.NEAR and float(a.max()) <= 0.95
    for shape in C.SAMPLES_SHAPES:
        a, x, b, y = C.samples_case(*shape)
        assert C.clamped_variables_ok(x, y)
    x = torch.tensor([[[0.4, 0.4], [0.4 + 1e-4, 0.4]]])
    assert not C.clamped_variables_ok(x, x[:, :1])                     # r2 = 1e-8 * (1 + ...) inside (0, 1e-7)
    assert not C.clamped_variables_ok(torch.tensor([[[0.4, 0.4], [0.4 + 2e-7, 0.4]]]), x[:, :1], blurs=(0.001,))


def test_recorded_deviations_cover_a_fresh_measurement():
    dev = C.measure_deviations()
    assert sorted(dev) == sorted(C.RECORDED_DEV) == sorted("%s.%s" % (k, o) for k in C.KINDS for o in C.OUTPUTS)
    for k, v in dev.items():
        print("  %s: measured %.3e recorded %.3e" % (k, v, C.RECORDED_DEV[k]))
        assert v <= C.RECORDED_DEV[k] * 1.001 + 1e-12, (k, v, C.RECORDED_DEV[k])
    for kind in C.KINDS:
        for o in C.OUTPUTS:
            assert C.bound(kind, o) == max(C.FACTOR * C.RECORDED_DEV["%s.%s" % (kind, o)], C.FLOOR)
            assert C.bound(kind, o) <= 5e-3
    text = open(os.path.join(ROOT, "profiles", "kernel_loss_tolerances.md")).read()
    for k, v in C.RECORDED_DEV.items():
        assert k in text and "%.3e" % v in text, (k, v)


# ---- the opt-in surface ---------------------------------------------------------------------------------------------
def test_refusals_without_the_flag_are_unchanged_and_name_it():
    from kd6d.kd_losses import KDLoss
    from kd6d.losses import SamplesLoss
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    for kind in C.KINDS:
        with pytest.raises(NotImplementedError, match="--kd_kernel_losses"):
            KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE=kind))
        with pytest.raises(NotImplementedError, match="--kd_kernel_losses"):
            KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE=kind, KERNEL_LOSSES=False))
        with pytest.raises(NotImplementedError, match="kernel_losses=True"):
            SamplesLoss(kind)
        with pytest.raises(NotImplementedError, match="kernel_losses=True"):
            SamplesLoss(kind, p=2, blur=0.05, scaling=0.5, reach=0.5)
    with pytest.raises(NotImplementedError):
        KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE="sinkhorn", WEIGHTED_OT=False))
    with pytest.raises(NotImplementedError):
        KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE="energy", KERNEL_LOSSES=True, WEIGHTED_OT=False))


def test_accepted_with_the_flag_and_what_stays_refused():
    from kd6d import _lib
    from kd6d.kd_losses import KDLoss
    from kd6d.losses import SamplesLoss
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    for kind in C.KINDS:
        ev = KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE=kind, KERNEL_LOSSES=True, GBLUR=0.05))
        assert ev.kernel == _lib.KERNEL_KINDS[kind] == C.KINDS.index(kind)
        # p, scaling and reach are accepted and ignored, as geomloss does
        L = SamplesLoss(kind, p=1, blur=0.05, scaling=0.9, reach=0.3, kernel_losses=True)
        assert L.kernel == ev.kernel and L.blur == 0.05
    assert KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE="sinkhorn", KERNEL_LOSSES=True)).kernel is None
    assert SamplesLoss("sinkhorn", kernel_losses=True).kernel is None
    for bad in ("l1", "l2"):
        with pytest.raises(NotImplementedError, match="geomloss has no such loss"):
            KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE=bad, KERNEL_LOSSES=True))
        with pytest.raises(NotImplementedError, match="geomloss has no such loss"):
            SamplesLoss(bad, kernel_losses=True)
    with pytest.raises(NotImplementedError):
        SamplesLoss("hausdorff", kernel_losses=True)
    for kind in ("gaussian", "laplacian"):
        for blur in (0.0, -0.05):
            with pytest.raises(ValueError, match="blur"):
                KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=dict(GTYPE=kind, KERNEL_LOSSES=True, GBLUR=blur))
            with pytest.raises(ValueError, match="blur"):
                SamplesLoss(kind, blur=blur, kernel_losses=True)
    SamplesLoss("energy", blur=0.0, kernel_losses=True)              # the energy distance has no blur
    with pytest.raises(RuntimeError, match="GPU only"):
        SamplesLoss("energy", kernel_losses=True)(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2))
    with pytest.raises(NotImplementedError, match="second measure"):
        SamplesLoss("energy", kernel_losses=True)(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2).requires_grad_(True))


def test_command_line_flag():
    from kd6d.arguments.argument_kd import get_argparser, get_args
    cfg, cfg_t = get_args(BASE + ["--gtype", "energy"])
    assert set(cfg["KD"]) == KD_DEFAULT_KEYS and len(KD_DEFAULT_KEYS) == 11 and cfg["KD"]["GTYPE"] == "energy"
    assert "KERNEL_LOSSES" not in cfg_t["KD"]
    cfg, cfg_t = get_args(BASE + ["--gtype", "energy", "--kd_kernel_losses"])
    assert cfg["KD"]["KERNEL_LOSSES"] is True and cfg["KD"]["GTYPE"] == "energy"
    assert set(cfg["KD"]) == KD_DEFAULT_KEYS | {"KERNEL_LOSSES"}
    assert get_argparser().parse_args([]).kd_kernel_losses is False
    cfg, _ = get_args(BASE + ["--kd_kernel_losses", "--kd_per_object"])
    assert cfg["KD"]["KERNEL_LOSSES"] is True and cfg["KD"]["PER_OBJECT"] is True and cfg["KD"]["GTYPE"] == "sinkhorn"
    help_text = " ".join(get_argparser().format_help().split())
    assert "nearly diagonal" in help_text and "--kd_kernel_losses" in help_text
    # the model's loss is built from cfg["KD"]: with the flag it takes the kernel, l1 stays refused
    from kd6d.kd_losses import KDLoss
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS
    assert KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=cfg["KD"]).kernel is None
    cfg, _ = get_args(BASE + ["--gtype", "laplacian", "--blur", "0.05", "--kd_kernel_losses"])
    assert KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=cfg["KD"]).kernel == 1
    cfg, _ = get_args(BASE + ["--gtype", "l1", "--kd_kernel_losses"])
    with pytest.raises(NotImplementedError, match="geomloss has no such loss"):
        KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg=cfg["KD"])


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_host_checks_fail_loudly_without_gpu():
    from kd6d import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(64)         # never dereferenced: every call below fails its argument checks on the host

    def small(kind=0, n_images=4, blur=0.05, ptr=p):
        return lib.kd6d_kernel_div_fwd_bwd(kind, ptr, p, p, p, p, p, p, p, n_images, blur, p, p, None, p, p, None)

    def dense(kind=0, N=10, M=10, D=2, blur=0.05, ws=p, nws=64, x=p):
        return lib.kd6d_kernel_dense_fwd_bwd(kind, x, p, p, p, N, M, D, blur, ws, nws, p, p, p, None)

    def failed(rc, *words):
        msg = lib.kd6d_last_error()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)

    failed(small(ptr=None), b"kd6d_kernel_div_fwd_bwd", b"null pointer")
    failed(lib.kd6d_kernel_div_fwd_bwd(0, *([None] * 8), 4, 0.05, *([None] * 6)), b"null pointer")
    for kind in (-1, 3):
        failed(small(kind=kind), b"kd6d_kernel_div_fwd_bwd", b"kind=%d" % kind)
        failed(dense(kind=kind), b"kd6d_kernel_dense_fwd_bwd", b"kind=%d" % kind)
    for kind in (0, 1):
        for blur in (0.0, -1.0, float("nan")):
            failed(small(kind=kind, blur=blur), b"kd6d_kernel_div_fwd_bwd", b"blur")
            failed(dense(kind=kind, blur=blur), b"kd6d_kernel_dense_fwd_bwd", b"blur")
    failed(small(n_images=-1), b"n_images=-1")
    failed(small(kind=2, blur=0.0, n_images=-2), b"n_images=-2")          # energy: blur is not looked at
    assert small(n_images=0) == 0, "n_images = 0 is a no-op"
    failed(dense(x=None), b"kd6d_kernel_dense_fwd_bwd", b"null pointer")
    failed(dense(ws=None), b"null pointer")
    for D in (0, 1, 3, 6, 32):
        failed(dense(D=D), b"kd6d_kernel_dense_fwd_bwd", b"D=%d" % D)
    failed(dense(N=0), b"N=0")
    failed(dense(M=-3), b"M=-3")
    need = int(lib.kd6d_kernel_dense_workspace_floats(1000, 70, 16))
    assert need == -(-1000 // C.ROWS) + -(-70 // C.ROWS)
    failed(dense(N=1000, M=70, D=16, nws=need - 1), b"workspace_floats=%d" % (need - 1))
    try:
        _lib.check(dense(N=1000, M=70, D=16, nws=0), "kd6d_kernel_dense_fwd_bwd")
        raise AssertionError("check() must raise")
    except _lib.Kd6dError as e:
        assert "workspace_floats=0" in str(e)
    assert lib.kd6d_kernel_div_max_points() == 128 == lib.kd6d_sinkhorn_max_points()


def test_header_stays_at_abi_11_and_matches_the_bindings():
    from kd6d import _lib
    src = open(os.path.join(ROOT, "include", "kd6d.h")).read()
    assert re.search(r"#define\s+KD6D_ABI_VERSION\s+11\b", src) and _lib.ABI_VERSION == 11 == _lib.lib.kd6d_abi_version()
    for name, code in (("GAUSSIAN", 0), ("LAPLACIAN", 1), ("ENERGY", 2)):
        assert re.search(r"#define\s+KD6D_KERNEL_%s\s+%d\b" % (name, code), src)
        assert _lib.KERNEL_KINDS[name.lower()] == code
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kd6d_[a-z0-9_]+)\s*\(", code))
    new = {"kd6d_kernel_div_fwd_bwd", "kd6d_kernel_div_max_points", "kd6d_kernel_dense_workspace_floats",
           "kd6d_kernel_dense_fwd_bwd"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    assert declared == set(_lib.SIGNATURES) | {"kd6d_last_error"}
    for n in new:
        assert hasattr(_lib.lib, n)
    assert _lib.lib.kd6d_kernel_dense_workspace_floats.restype is ctypes.c_int64
    # argument counts of the bindings = those of the declarations
    for n in new:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, code)
        args = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[n]), (n, len(args), len(_lib.SIGNATURES[n]))
    build = open(os.path.join(ROOT, "kd-6d-pose-adlp_amd", "build.py")).read()
    assert '"kernel_loss.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]' in build
