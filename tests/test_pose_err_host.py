"""CPU: the device pose scorer's host side -- kd6d_pose_errors declared, exported, bound and refusing bad arguments
before any HIP call; the orchestration of evaluate_pose_predictions_device (walk order, subsample draws, missing
predictions) against the reference's own capture through a numpy stand-in for the launch; the scorer switch of
valid(); the command line of test.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, G)


def test_pose_errors_declared_exported_bound_under_abi_11():
    from kd6d import _lib
    src = open(os.path.join(ROOT, "include", "kd6d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint kd6d_pose_errors\s*\(", code)
    assert re.search(r"#define KD6D_ABI_VERSION 11\b", src) and _lib.lib.kd6d_abi_version() == 11
    assert hasattr(_lib.lib, "kd6d_pose_errors") and len(_lib.SIGNATURES["kd6d_pose_errors"]) == 15
    assert _lib.POSE_ERR_MAX_V == 1000 and re.search(r"#define KD6D_POSE_ERR_MAX_V 1000\b", src)
    from kd6d import ops
    assert callable(ops.pose_errors)
    build = open(os.path.join(ROOT, "kd-6d-pose-adlp_amd", "build.py")).read()
    assert '"pose_err.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]' in build


def _call(lib, P=2, max_v=1000, missing=None, vidx=False, nn=False):
    """Every pointer is a never-dereferenced dummy: each call here ends in the argument checks or launches nothing."""
    p = ctypes.c_void_p(16)
    req = {n: p for n in ("verts", "voff", "vcnt", "K", "Rg", "Tg", "Rp", "Tp", "sym", "err")}
    if missing:
        req[missing] = None
    return lib.kd6d_pose_errors(P, max_v, req["verts"], req["voff"], req["vcnt"], p if vidx else None, req["K"],
                                req["Rg"], req["Tg"], req["Rp"], req["Tp"], req["sym"], req["err"], p if nn else None,
                                None)


def test_pose_errors_argument_checks_fail_loudly_without_gpu():
    from kd6d import _lib
    lib = _lib.lib
    for name in ("verts", "voff", "vcnt", "K", "Rg", "Tg", "Rp", "Tp", "sym", "err"):
        assert _call(lib, missing=name) == -1, name
        assert b"kd6d_pose_errors: null pointer" in lib.kd6d_last_error(), name
    for kw, msg in ((dict(P=-1), b"n_problems=-1"), (dict(max_v=0), b"max_v=0"), (dict(max_v=1001), b"max_v=1001"),
                    (dict(max_v=-5), b"max_v=-5")):
        assert _call(lib, **kw) == -1
        assert msg in lib.kd6d_last_error(), (msg, lib.kd6d_last_error())
    with pytest.raises(_lib.Kd6dError, match="max_v=1001"):
        _lib.check(_call(lib, max_v=1001), "kd6d_pose_errors")
    # nothing to score: success, no launch; the optional pointers may be given or not
    assert _call(lib, P=0) == 0 and _call(lib, P=0, vidx=True, nn=True) == 0 and _call(lib, P=0, max_v=1) == 0


def numpy_errors(max_v, verts, voff, vcnt, vidx, K, Rg, Tg, Rp, Tp, sym, want_nn=False):
    """float64 stand-in for the launch, same arrays in, err out: kd6d_pose_errors' contract (voff / vcnt / vidx / sym)
    with compute_pose_diff's arithmetic."""
    P = len(voff)
    err = np.zeros((P, 2))
    nn = np.full((P, max_v), -1, np.int64)
    for p in range(P):
        n = int(vcnt[p])
        assert 1 <= n <= max_v <= 1000
        idx = np.arange(n) if vidx is None else np.asarray(vidx[p, :n], np.int64)
        m = np.asarray(verts, np.float64)[int(voff[p]) + idx]
        Kp = np.asarray(K[p], np.float64)
        a = m @ np.asarray(Rg[p], np.float64).T + np.asarray(Tg[p], np.float64)
        b = m @ np.asarray(Rp[p], np.float64).T + np.asarray(Tp[p], np.float64)
        j = np.arange(n)
        if sym[p]:
            j = np.argmin(np.linalg.norm(a[:, None, :] - b[None, :, :], axis=2), axis=1)
        b = b[j]
        nn[p, :n] = j

        def pin(x):
            q = x @ Kp.T
            return q[:, :2] / (q[:, 2:3] + 1e-8)
        err[p] = np.linalg.norm(a - b, axis=1).mean(), np.linalg.norm(pin(a) - pin(b), axis=1).mean()
    return (err, nn) if want_nn else err


def close(a, b, tol=1e-9):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (a.keys(), b.keys())
        for k in a:
            close(a[k], b[k], tol)
    elif isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            close(x, y, tol)
    else:
        assert abs(a - b) <= tol * max(1.0, abs(b)), (a, b)


def test_device_orchestration_reproduces_the_reference_capture():
    """eval_inputs(21) under np.random.seed(7): class 1 has 1500 vertices (a draw per scored object), class 2 is
    symmetric, several objects have no prediction.  With a float64 stand-in for the launch the tables must be the
    reference's own capture to 1e-9: that pins the walk order, the draws and the handling of missing predictions."""
    from kd6d.libs import evaluate as E
    from make_golden_eval import _Mesh, eval_inputs
    z = np.load(os.path.join(G, "eval_metrics.npz"))
    meshes, diam, Kk, preds = eval_inputs(int(z["seed"]))
    ref = json.loads(str(z["evaluate_json"]))
    seen = []

    def spy(max_v, verts, voff, vcnt, vidx, *rest):
        seen.append((max_v, len(voff), None if vidx is None else vidx.shape, verts.shape, voff.dtype, vidx.dtype))
        return numpy_errors(max_v, verts, voff, vcnt, vidx, *rest)

    np.random.seed(7)
    res = E.evaluate_pose_predictions_device(preds, 4, [_Mesh(m) for m in meshes], diam, {"cls_2": ["Z", 0]}, None,
                                             errors_fn=spy)
    mine = json.loads(json.dumps([res[0], res[1], res[2], res[3], res[4], [float(x) for x in res[5]]], sort_keys=True))
    close(mine, ref, 1e-9)
    n_missing = sum(1 for it in preds.values() for c in it["meta"]["class_ids"]
                    if not any(p[1] == c for p in it["pred"]))
    n_objects = sum(len(it["meta"]["class_ids"]) for it in preds.values())
    assert n_missing > 0 and len(seen) == 1
    max_v, P, vshape, pool_shape, off_dtype, idx_dtype = seen[0]
    assert P == n_objects - n_missing                                   # objects without a prediction are never sent
    assert max_v == 1000 and vshape == (P, 1000) and pool_shape == (300 + 1500 + 800, 3)
    assert off_dtype == np.int32 and idx_dtype == np.int32


def test_device_scorer_without_draws_passes_no_index_table_and_keeps_host_constants():
    from kd6d.libs import evaluate as E
    rng = np.random.default_rng(0)
    mesh = [type("M", (), {"vertices": rng.normal(0, 30, (40, 3))})(), type("M", (), {"vertices": rng.normal(0, 30, (8, 3))})()]
    K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])
    preds = {"a": {"meta": {"K": K, "class_ids": [0, 1], "rotations": [np.eye(3)] * 2,
                            "translations": [np.array([[0.0], [0.0], [800.0]])] * 2},
                   "pred": [[0.9, 0, np.eye(3), np.array([[1.0], [0.0], [800.0]])]]},
             "b": {"meta": {"K": K, "class_ids": [1], "rotations": [np.eye(3)], "translations": [np.array([[0.0], [0.0], [900.0]])]},
                   "pred": []}}
    calls = []

    def fn(max_v, verts, voff, vcnt, vidx, *rest):
        calls.append((max_v, vidx, list(voff), list(vcnt)))
        return numpy_errors(max_v, verts, voff, vcnt, vidx, *rest)
    state = np.random.get_state()[1].copy()
    dev = E.evaluate_pose_predictions_device(preds, 3, mesh, [100.0, 100.0], {}, None, errors_fn=fn)
    assert (np.random.get_state()[1] == state).all()                # no mesh above 1000 vertices: no draw
    host = E.evaluate_pose_predictions(preds, 3, mesh, [100.0, 100.0], {})
    close(json.loads(json.dumps(dev[:5])), json.loads(json.dumps(host[:5])), 1e-6)
    assert calls == [(40, None, [0], [40])]
    assert dev[0][1] == {"ADI.05d": 0.0, "ADI.10d": 0.0, "ADI.20d": 0.0, "ADI.50d": 0.0}    # class 1: nothing predicted
    # no prediction at all: nothing is launched
    calls.clear()
    E.evaluate_pose_predictions_device({"b": preds["b"]}, 3, mesh, [100.0, 100.0], {}, None, errors_fn=fn)
    assert calls == []


def test_valid_refuses_an_unknown_scorer():
    from kd6d.libs.eval_libs import valid
    with pytest.raises(ValueError, match="nonsense"):
        valid({}, 0, [], None, "cpu", [], scorer="nonsense")


def test_eval_parser_yields_the_reference_runtime_keys():
    from kd6d.arguments.argument import get_argparser, get_args
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    cfg = get_args(["--config_file", ape, "--weight_file", "w.pth", "--test_file", "list.txt", "--backbone", "darknet_tiny_h",
                    "--working_dir", "out/", "--num_workers", "3", "--running_device", "cuda"])
    rt = cfg["RUNTIME"]
    assert {"LOCAL_RANK", "CONFIG_FILE", "NUM_WORKERS", "WEIGHT_FILE", "WORKING_DIR", "RUNNING_DEVICE"} <= set(rt)
    assert (rt["CONFIG_FILE"], rt["WEIGHT_FILE"], rt["WORKING_DIR"], rt["NUM_WORKERS"], rt["RUNNING_DEVICE"],
            rt["LOCAL_RANK"]) == (ape, "w.pth", "out/", 3, "cuda", 0)
    assert cfg["DATASETS"]["TEST"] == "list.txt" and cfg["MODEL"]["BACKBONE"] == "darknet_tiny_h"
    assert cfg["MODEL"]["OUT_CHANNEL"] == 128                                      # custom_cfg ran
    assert (rt["PNP_SOLVER"], rt["EVAL_SCORER"], rt["SYNTHETIC"], rt["PRECISION"]) == ("host", "host", False, "bf16")
    d = get_argparser().parse_args([])
    assert d.backbone == "darknet53" and d.config_file == "./configs/ape.yaml" and d.working_dir == "./outputs/"
    cfg = get_args(["--config_file", ape, "--synthetic", "--pnp_solver", "device", "--eval_scorer", "device",
                    "--precision", "fp32"])
    assert (cfg["RUNTIME"]["PNP_SOLVER"], cfg["RUNTIME"]["EVAL_SCORER"], cfg["RUNTIME"]["SYNTHETIC"],
            cfg["RUNTIME"]["PRECISION"]) == ("device", "device", True, "fp32")
    with pytest.raises(SystemExit):
        get_argparser().parse_args(["--eval_scorer", "cuda"])


def test_train_entry_flag_eval_scorer_lands_in_runtime_only():
    from kd6d.arguments.argument_kd import get_args
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    cfg, cfg_t = get_args(["--config_file", ape, "--config_file_t", ape])
    assert cfg["RUNTIME"]["EVAL_SCORER"] == "host" and cfg_t["RUNTIME"]["EVAL_SCORER"] == "host"
    cfg, cfg_t = get_args(["--config_file", ape, "--config_file_t", ape, "--eval_scorer", "device"])
    assert cfg["RUNTIME"]["EVAL_SCORER"] == "device" and "EVAL_SCORER" not in cfg["KD"]


def test_eval_entry_refuses_the_cpu_as_a_child_process():
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "--config_file", ape, "--backbone", "darknet_tiny_h",
                        "--synthetic", "--running_device", "cpu"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert "the kd6d step runs on MI355X only (--running_device cuda)" in r.stderr
    train = open(os.path.join(ROOT, "train_kd.py")).read()
    assert "the kd6d step runs on MI355X only (--running_device cuda); the CPU restatement " in train
