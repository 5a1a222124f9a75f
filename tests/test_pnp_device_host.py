"""CPU: the device PnP-RANSAC entry points of the C ABI (ABI 11) -- declared, bound, and refusing bad arguments on the
host before any HIP call -- and the --pnp_solver flag."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_11_in_header_and_binding():
    from kd6d import _lib
    src = open(os.path.join(ROOT, "include", "kd6d.h")).read()
    assert re.search(r"#define KD6D_ABI_VERSION 11\b", src)
    assert _lib.ABI_VERSION == 11 and _lib.lib.kd6d_abi_version() == 11
    for name in ("kd6d_pnp_ransac", "kd6d_teacher_pnp_gate", "kd6d_pnp_workspace_floats"):
        assert name in src and name in _lib.SIGNATURES
    assert _lib.lib.kd6d_pnp_workspace_floats(4, 300) == 4 * 300 * 16


def _ransac(lib, P=2, cap=4, ptrs=True, iters=300, ws_floats=None):
    p = ctypes.c_void_p(16) if ptrs else None          # never dereferenced: every call below fails its checks first
    ws = lib.kd6d_pnp_workspace_floats(P, max(iters, 1)) if ws_floats is None else ws_floats
    return lib.kd6d_pnp_ransac(P, cap, p, p, p, p, 5.0, iters, 0, p, p, p, p, p, ws, None)


def _gate(lib, B=2, cap=4, n_cls=15, rows=15, iters=300, ptrs=True):
    p = ctypes.c_void_p(16) if ptrs else None
    ws = lib.kd6d_pnp_workspace_floats(B, max(iters, 1))
    return lib.kd6d_teacher_pnp_gate(p, n_cls, 0.1, p, p, p, cap, B, p, rows, p, 5.0, iters, 0, p, ws, None)


def test_pnp_argument_checks_fail_loudly_without_gpu():
    from kd6d import _lib
    lib = _lib.lib
    cases = [(lambda: _ransac(lib, ptrs=False), b"null pointer"), (lambda: _ransac(lib, cap=33), b"cap=33"),
             (lambda: _ransac(lib, cap=0), b"cap=0"), (lambda: _ransac(lib, iters=0), b"iters=0"),
             (lambda: _ransac(lib, ws_floats=10), b"workspace"),
             (lambda: _gate(lib, ptrs=False), b"null pointer"), (lambda: _gate(lib, cap=64), b"cap=64"),
             (lambda: _gate(lib, iters=-1), b"iters=-1"), (lambda: _gate(lib, n_cls=17, rows=20), b"n_cls=17"),
             (lambda: _gate(lib, n_cls=15, rows=8), b"n_cls=15")]
    for call, msg in cases:
        assert call() == -1
        err = lib.kd6d_last_error()
        assert msg in err, (msg, err)
    try:
        _lib.check(_ransac(lib, cap=33), "kd6d_pnp_ransac")
        raise AssertionError("check() must raise")
    except _lib.Kd6dError as e:
        assert "cap=33" in str(e)


def test_pnp_solver_flag_defaults_to_host_and_maps_to_runtime():
    from kd6d.arguments.argument_kd import _runtime, get_argparser, get_args
    args = get_argparser().parse_args([])
    assert args.pnp_solver == "host" and args.teacher_pnp_gate is False
    assert _runtime(args, "c.yaml", "")["PNP_SOLVER"] == "host"
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    cfg, cfg_t = get_args(["--config_file", ape, "--config_file_t", ape])
    assert cfg["RUNTIME"]["PNP_SOLVER"] == "host" and cfg_t["RUNTIME"]["PNP_SOLVER"] == "host"
    cfg, cfg_t = get_args(["--config_file", ape, "--config_file_t", ape, "--pnp_solver", "device", "--teacher_pnp_gate"])
    assert cfg["RUNTIME"]["PNP_SOLVER"] == "device" and cfg_t["RUNTIME"]["PNP_SOLVER"] == "device"
    assert cfg_t["RUNTIME"]["TEACHER_PNP_GATE"] is True
    import pytest
    with pytest.raises(SystemExit):
        get_argparser().parse_args(["--pnp_solver", "cv2"])
