"""CPU: the host side of the BOP metrics (kd6d/libs/bop_metrics.py) -- symmetry sets, the float64 scorer against
closed-form answers and against the case module's restatement, threshold and AR arithmetic, the orchestration of
evaluate_bop_predictions through errors_fn, the results file, the flags, and kd6d_bop_errors declared, exported, bound
and refusing bad arguments before any HIP call."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import bop_metric_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APE = os.path.join(ROOT, "configs", "ape.yaml")


# ---- symmetry sets ----------------------------------------------------------------------------------------------------
def _check_rigid(S):
    for s in S:
        R = s[:, :3]
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        assert abs(np.linalg.det(R) - 1.0) < 1e-12
    np.testing.assert_array_equal(S[0], np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1))


def test_symmetry_sets_from_the_yaml():
    from kd6d.libs.bop_metrics import CONTINUOUS_N, symmetry_set
    assert CONTINUOUS_N == 315 == math.ceil(math.pi / 0.01)
    types = {"cls_0": ["Z", 180], "cls_1": ["Z", 0], "cls_2": ["Z", 180, "X", 180], "cls_4": ["X", 180, "Y", 180, "Z", 180]}
    sizes = {0: 2, 1: 315, 2: 4, 3: 1, 4: 8}
    for c, n in sizes.items():
        S = symmetry_set(c, types)
        assert S.shape == (n, 3, 4) and S.dtype == np.float64
        _check_rigid(S)
        assert np.abs(S[:, :, 3]).max() == 0.0                     # yaml axes pass through the origin
    np.testing.assert_allclose(symmetry_set(0, types)[1, :, :3], np.diag([-1.0, -1.0, 1.0]), atol=1e-15)
    S = symmetry_set(1, types)                                      # rotations by 2 pi j / 315 about Z, in order
    for j in (1, 7, 314):
        a = 2 * math.pi * j / 315
        np.testing.assert_allclose(S[j, :, :3], [[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]],
                                   atol=1e-15)
    four = symmetry_set(2, types)[:, :, :3]                         # Z-180 x X-180: I, Rx, Rz, Rz Rx
    want = [np.eye(3), np.diag([1.0, -1, -1]), np.diag([-1.0, -1, 1]), np.diag([-1.0, 1, -1])]
    for R in want:
        assert any(np.allclose(R, G, atol=1e-15) for G in four)
    assert symmetry_set(7, None).shape == (1, 3, 4) and symmetry_set(7, {}).shape == (1, 3, 4)
    with pytest.raises(ValueError, match="symmetry axis"):
        symmetry_set(0, {"cls_0": ["W", 180]})


def test_symmetry_sets_from_models_info_win_over_the_yaml(tmp_path):
    from kd6d.libs import bop_metrics as B
    models = C.write_bop_tree(str(tmp_path))
    info = B.load_models_info(models)
    assert sorted(info) == ["1", "5", "9"] and B.load_models_info(str(tmp_path)) is None and B.load_models_info(None) is None
    assert B.class_object_ids(models) == [1, 5, 9]
    S = B.symmetry_set(2, {"cls_2": ["Y", 90]}, info["9"])           # the yaml entry is ignored
    assert S.shape == (630, 3, 4)
    _check_rigid(S)
    o = np.array([0.0, 0.0, 5.0])
    for s in S:                                                     # every transform keeps the offset point: S o = o
        np.testing.assert_allclose(s[:, :3] @ o + s[:, 3], o, atol=1e-12)
    # product set R = R_c R_d, t = R_c t_d + t_c: continuous-major, the discrete pair (identity, listed) inside
    d = np.asarray(C.MODEL_INFO_630["symmetries_discrete"][0]).reshape(4, 4)[:3]
    a = 2 * math.pi * 3 / 315
    Rc = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    tc = o - Rc @ o
    np.testing.assert_allclose(S[6], np.concatenate([Rc, tc[:, None]], axis=1), atol=1e-12)
    np.testing.assert_allclose(S[7], np.concatenate([Rc @ d[:, :3], (Rc @ d[:, 3] + tc)[:, None]], axis=1), atol=1e-12)
    # the DATASETS section: models_info.json is the source for every class, an object without an entry is asymmetric
    ds = {"MESH_DIR": models, "SYMMETRY_TYPES": {"cls_0": ["Z", 0], "cls_1": ["Z", 90]}}
    sets = B.dataset_symmetry_sets(ds, 3)
    assert [len(s) for s in sets] == [1, 2, 630]
    np.testing.assert_allclose(sets[1][1, :, :3], np.diag([-1.0, -1.0, 1.0]), atol=1e-15)
    ds_yaml = {"MESH_DIR": str(tmp_path / "nowhere"), "SYMMETRY_TYPES": ds["SYMMETRY_TYPES"]}
    assert [len(s) for s in B.dataset_symmetry_sets(ds_yaml, 3)] == [315, 4, 1]


def test_docstring_names_the_unpinned_boundary_and_the_missing_vsd_term():
    from kd6d.libs import bop_metrics as B
    assert "bop_toolkit is not available" in B.__doc__ and "RESTATEMENT" in B.__doc__ and "VSD" in B.__doc__
    assert "VSD" in B.AR_NOTE and "VSD" in B.format_ar_line({"AR_MSSD": 0.5, "AR_MSPD": 0.25, "AR": 0.375, "n_objects": 3})
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "bop_toolkit" in design and "VSD" in design and "csrc/bop_err.hip" in design
    assert "--bop_metrics" in open(os.path.join(ROOT, "README.md")).read()


# ---- the scorer: closed forms and the restatement ----------------------------------------------------------------------
def test_host_scorer_known_answers():
    from kd6d.libs.bop_metrics import bop_errors_host
    case, exact, names = C.closed_form_case()
    for fn in (lambda c: bop_errors_host(**c), lambda c: C.restate(c, np.float64)):
        err = fn(case)
        for k, name in enumerate(names):
            for col in (0, 1):
                if not np.isnan(exact[k, col]):
                    assert abs(err[k, col] - exact[k, col]) <= 1e-9 * max(1.0, exact[k, col]), (name, col, err[k], exact[k])
    assert names[0].startswith("one vertex") and exact[0, 0] == 75.0 and exact[1, 0] == 0.0     # 2 r, then 0 with Z-180
    assert exact[2, 0] == 13.0 and exact[3, 1] == pytest.approx(600.0 * 6.0 / 800.0, rel=1e-10)   # |d|, f d / z (the 1e-8 beside z is 1.25e-11 of it)


def test_host_scorer_equals_the_restatement_and_honours_the_edges():
    from kd6d.libs.bop_metrics import bop_errors_host
    case = C.mixed_case()
    np.testing.assert_allclose(bop_errors_host(**case), C.restate(case, np.float64), rtol=1e-10, atol=1e-10)
    few = C.subset(case, np.array([0, 8, 20]))                      # S = 1, 2, 630
    base = bop_errors_host(**few)
    ident = dict(few, scnt=np.array([0, few["scnt"][1], few["scnt"][2]], np.int32))
    np.testing.assert_array_equal(bop_errors_host(**ident)[0], base[0])        # scnt 0 = the identity alone
    empty = dict(few, vcnt=np.array([few["vcnt"][0], 0, few["vcnt"][2]], np.int32))
    got = bop_errors_host(**empty)
    assert (got[1] == 0).all() and (got[0] == base[0]).all() and (got[2] == base[2]).all()
    assert bop_errors_host(**C.subset(case, np.array([], np.int64))).shape == (0, 2)
    syms3x4 = dict(few, syms=C.unpack_syms(few["syms"]))
    np.testing.assert_array_equal(bop_errors_host(**syms3x4), base)


def test_symmetry_pool_rows_are_rotation_row_major_then_translation():
    """kd6d_bop_errors reads 12 floats per symmetry: R row-major, then t -- not the rows of [R | t]."""
    from kd6d.libs import bop_metrics as B
    S = B.symmetry_set(0, None, C.MODEL_INFO_630)
    for pool in (B.pack_symmetries(S), C.pack_syms(S)):
        assert pool.shape == (630, 12)
        for k in (0, 1, 7, 629):
            np.testing.assert_array_equal(pool[k, :9], S[k, :, :3].reshape(9))
            np.testing.assert_array_equal(pool[k, 9:], S[k, :, 3])
    assert np.abs(S[1:, :, 3]).max() > 1.0                          # translations that a wrong layout would misplace
    np.testing.assert_array_equal(B.unpack_symmetries(B.pack_symmetries(S)), S)
    np.testing.assert_array_equal(C.unpack_syms(C.pack_syms(S)), S)
    np.testing.assert_array_equal(B.unpack_symmetries(S), S)
    # the orchestration hands the pool over in that layout
    preds, meshes, diam, sets = C.recall_collection()
    seen = []
    B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, None, errors_fn=C.restate_errors_fn(np.float64, seen))
    np.testing.assert_array_equal(seen[0][0]["syms"], B.pack_symmetries(np.concatenate(sets)))
    # and the scorer reads it so: a transform with a translation, scored by hand
    v = np.array([[1.0, 2.0, 3.0]])
    s = np.concatenate([C.rot([0, 0, 1], 0.5), np.array([[4.0], [5.0], [6.0]])], axis=1)[None]
    Rg, Tg = C.random_rot(np.random.default_rng(0)), np.array([1.0, 2.0, 700.0])
    want = np.linalg.norm((v[0] + [0.5, 0, 0] + Tg) - (Rg @ (s[0, :, :3] @ v[0] + s[0, :, 3]) + Tg))
    got = B.bop_errors_host(v, np.array([0]), np.array([1]), B.pack_symmetries(s), np.array([0]), np.array([1]),
                            C.K0[None], Rg[None], Tg[None], np.eye(3)[None], (Tg + [0.5, 0, 0])[None])
    assert got[0, 0] == pytest.approx(want, rel=1e-12)


def test_tolerances_are_the_recorded_ones_and_come_from_the_restatement():
    tol = C.tolerances()
    for name in ("mssd", "mspd"):
        for k in ("rel", "abs"):
            assert tol[name][k] == C.MARGIN * tol[name]["dev_" + k]
            assert abs(tol[name][k] / C.RECORDED[name][k] - 1.0) < 0.02, (name, k, tol[name][k], C.RECORDED[name][k])
    # fp32 at these magnitudes: nothing near the cap a wrong reduction would need
    assert max(tol[n]["rel"] for n in tol) < 5e-4 and max(tol[n]["abs"] for n in tol) < 1e-3
    profile = open(os.path.join(ROOT, "profiles", "bop_err_device.md")).read()
    for name in ("mssd", "mspd"):
        for k in ("rel", "abs"):
            assert ("%.3e" % C.RECORDED[name][k]) in profile, (name, k)
    for r64, r32 in C.references().values():                        # the restatement itself meets the bound
        for col in (0, 1):
            assert C.within(r32[:, col], r64[:, col], col).all()


def test_mixed_case_covers_the_sizes_the_issue_names():
    case = C.mixed_case()
    assert len(case["voff"]) == 49
    assert sorted(set(case["vcnt"].tolist())) == [1, 2, 63, 64, 65, 257, 1500]
    assert sorted(set(case["scnt"].tolist())) == [1, 2, 3, 16, 17, 315, 630]
    assert len(set(case["voff"][case["vcnt"] == 257].tolist())) == 7          # distinct meshes
    assert len(set(case["voff"][case["vcnt"] == 65].tolist())) == 1           # a shared mesh
    assert len({tuple(k.reshape(-1)) for k in case["K"]}) == 49
    err = C.restate(case, np.float64)
    assert err[0].max() == 0.0 and err[:, 0].max() > 10.0


# ---- thresholds and average recalls -------------------------------------------------------------------------------------
def test_threshold_and_ar_arithmetic_on_hand_made_errors():
    from kd6d.libs.bop_metrics import AR_NOTE, MSPD_THRESHOLDS, MSSD_THRESHOLDS, bop_tables
    assert MSSD_THRESHOLDS == [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]
    assert MSPD_THRESHOLDS == [5, 10, 15, 20, 25, 30, 35, 40, 45, 50]
    diam = [100.0, 200.0, 50.0]
    # class 0: four objects on a 640-wide image; one error exactly ON a threshold (strict <: missed there), one missing
    objects = [(0, 1.0)] * 4 + [(1, 2.0)] * 2
    errors = [(4.0, 4.0), (10.0, 10.0), (30.0, 49.0), None,
              (19.0, 19.0), (101.0, 60.0)]          # class 1: diameter 200, a 1280-wide image (r = 2)
    t = bop_tables(3, objects, errors, diam)
    c0, c1 = t["per_class"][0], t["per_class"][1]
    assert t["per_class"][2] == {} and c0["n"] == 4 and c1["n"] == 2 and t["n_objects"] == 6
    #            theta: .05   .10   .15   .20   .25   .30   .35   .40   .45   .50     (limits 5 ... 50 mm)
    assert list(c0["mssd_recall"].values()) == [.25, .25, .5, .5, .5, .5, .75, .75, .75, .75]     # 10 mm is not < 10 mm
    assert list(c0["mspd_recall"].values()) == [.25, .25, .5, .5, .5, .5, .5, .5, .5, .75]        # 10 px is not < 10 px
    assert list(c0["mssd_recall"]) == ["0.05", "0.10", "0.15", "0.20", "0.25", "0.30", "0.35", "0.40", "0.45", "0.50"]
    assert list(c0["mspd_recall"]) == ["5", "10", "15", "20", "25", "30", "35", "40", "45", "50"]
    # class 1: limits 10 ... 100 mm and 10 ... 100 px (theta * r): 19 px passes from theta = 10 on, 60 px from 35 on
    assert list(c1["mssd_recall"].values()) == [0, .5, .5, .5, .5, .5, .5, .5, .5, .5]
    assert list(c1["mspd_recall"].values()) == [0, .5, .5, .5, .5, .5, 1, 1, 1, 1]
    assert c0["AR_MSSD"] == pytest.approx(0.55) and c0["AR_MSPD"] == pytest.approx(0.475)
    assert c1["AR_MSSD"] == pytest.approx(0.45) and c1["AR_MSPD"] == pytest.approx(0.65)
    assert t["AR_MSSD"] == pytest.approx(0.5) and t["AR_MSPD"] == pytest.approx(0.5625)      # mean over the classes SEEN
    assert t["AR"] == pytest.approx(0.53125) and t["note"] == AR_NOTE
    nothing = bop_tables(2, [], [], diam)
    assert nothing["AR"] == 0.0 and nothing["per_class"] == [{}, {}]
    json.dumps(t)


# ---- orchestration through errors_fn ------------------------------------------------------------------------------------
def test_evaluate_bop_predictions_orchestration_through_errors_fn():
    from kd6d.libs import bop_metrics as B
    preds, meshes, diam, sets = C.recall_collection()
    seen = []
    t = B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, None, errors_fn=C.restate_errors_fn(np.float64, seen))
    (case, err), = seen                                             # ONE call for the whole collection
    # walk order: class-major, images in dict order; objects without a prediction are never sent
    want = [(c, name) for c in range(3) for name, it in preds.items()
            if c in it["meta"]["class_ids"] and any(q[1] == c for q in it["pred"])]
    n_objects = sum(len(it["meta"]["class_ids"]) for it in preds.values())
    P = len(want)
    assert 0 < P < n_objects == t["n_objects"]
    sizes, s_sizes = [40, 700, 1300], [1, 2, 315]
    offs, s_offs = [0, 40, 740], [0, 1, 3]
    assert case["verts"].shape == (2040, 3) and case["verts"].dtype == np.float64
    assert case["syms"].shape == (318, 12) and case["syms"].dtype == np.float64
    for k in ("voff", "vcnt", "soff", "scnt"):
        assert case[k].dtype == np.int32 and case[k].shape == (P,)
    for k, shape in (("K", (P, 3, 3)), ("Rg", (P, 3, 3)), ("Rp", (P, 3, 3)), ("Tg", (P, 3)), ("Tp", (P, 3))):
        assert case[k].shape == shape and case[k].dtype == np.float64
    for p, (c, name) in enumerate(want):
        it = preds[name]
        gi = it["meta"]["class_ids"].index(c)
        best = [q for q in it["pred"] if q[1] == c][0]
        assert (case["voff"][p], case["vcnt"][p], case["soff"][p], case["scnt"][p]) == (offs[c], sizes[c], s_offs[c], s_sizes[c])
        np.testing.assert_array_equal(case["K"][p], it["meta"]["K"])
        np.testing.assert_array_equal(case["Rg"][p], it["meta"]["rotations"][gi])
        np.testing.assert_array_equal(case["Tg"][p], it["meta"]["translations"][gi].reshape(3))
        np.testing.assert_array_equal(case["Rp"][p], best[2])
        np.testing.assert_array_equal(case["Tp"][p], best[3].reshape(3))
    # the tables are bop_tables of those errors, a missing prediction missed everywhere, r from the image width
    objects, errors, k = [], [], 0
    for c in range(3):
        for name, it in preds.items():
            if c in it["meta"]["class_ids"]:
                objects.append((c, it["meta"]["width"] / 640.0))
                hit = any(q[1] == c for q in it["pred"])
                errors.append(tuple(err[k]) if hit else None)
                k += hit
    assert {r for _, r in objects} == {1.0, 2.0}
    assert json.dumps(t) == json.dumps(B.bop_tables(3, objects, errors, diam))
    assert 0.2 < t["AR_MSSD"] < 0.9 and 0.2 < t["AR_MSPD"] < 0.95             # the thresholds are exercised, not saturated
    # the seed's promise: no float64 error within 1e-3 relative of a threshold; the fp32 restatement gives the same tables
    scored, err64 = C.recall_collection_objects()
    assert C.near_threshold(err64, scored, diam) == []
    t32 = B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, None, errors_fn=C.restate_errors_fn(np.float32))
    assert json.dumps(t32) == json.dumps(t)
    # the same scorer as the module's own
    t_host = B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, None, errors_fn=B.bop_errors_host)
    assert json.dumps(t_host) == json.dumps(t)
    # a meta without a width (the synthetic loaders) scores at r = 1; nothing predicted: nothing is called
    calls = []
    bare = {n: {"meta": {k: v for k, v in it["meta"].items() if k != "width"}, "pred": []} for n, it in preds.items()}
    t0 = B.evaluate_bop_predictions(bare, 4, meshes, diam, sets, None, errors_fn=lambda *a: calls.append(a))
    assert calls == [] and t0["AR"] == 0.0 and t0["n_objects"] == n_objects
    # two objects of one class in one image: the walk's assumption is asserted
    name = next(iter(preds))
    twice = {name: {"meta": dict(preds[name]["meta"], class_ids=[0, 0], rotations=[np.eye(3)] * 2,
                                 translations=[np.array([[0.0], [0.0], [700.0]])] * 2), "pred": []}}
    with pytest.raises(AssertionError, match="one object per class and image"):
        B.evaluate_bop_predictions(twice, 4, meshes, diam, sets, None, errors_fn=B.bop_errors_host)


# ---- the results file -------------------------------------------------------------------------------------------------
def test_bop_csv_round_trip_and_the_synthetic_refusal(tmp_path):
    from kd6d.libs import bop_metrics as B
    preds, _, _, _ = C.recall_collection()
    path = str(tmp_path / "results.csv")
    n = B.write_bop_csv(path, preds, [1, 5, 9])
    lines = open(path).read().splitlines()
    assert lines[0] == "scene_id,im_id,obj_id,score,R,t,time" and len(lines) == n + 1
    assert n == sum(len(it["pred"]) for it in preds.values()) > 24
    want = [(int(name.split("/")[-1][:-4]), q) for name, it in preds.items() for q in it["pred"]]
    for line, (im, q) in zip(lines[1:], want):
        f = line.split(",")
        assert len(f) == 7 and (int(f[0]), int(f[1]), int(f[2]), f[6]) == (2, im, [1, 5, 9][q[1]], "-1")
        assert float(f[3]) == pytest.approx(q[0], rel=1e-8)
        R, t = [float(x) for x in f[4].split(" ")], [float(x) for x in f[5].split(" ")]
        assert len(R) == 9 and len(t) == 3
        np.testing.assert_allclose(R, np.asarray(q[2]).reshape(9), rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(t, np.asarray(q[3]).reshape(3), rtol=1e-8)
    assert B.bop_scene_im_id("/data/lm/test/000015/rgb/000123.png") == (15, 123)
    for bad in ("val0_3", "a/b/c.png", "x/rgb/000001.png"):
        with pytest.raises(ValueError, match="BOP layout"):
            B.bop_scene_im_id(bad)
    from kd6d.arguments.argument import get_args
    with pytest.raises(SystemExit) as e:
        get_args(["--config_file", APE, "--synthetic", "--bop_csv", path])
    assert str(e.value) == B.BOP_CSV_SYNTHETIC_ERROR and "--synthetic" in str(e.value)


def test_both_parsers_know_the_flags():
    from kd6d.arguments import argument, argument_kd
    cfg = argument.get_args(["--config_file", APE])
    assert cfg["RUNTIME"]["BOP_METRICS"] is False and cfg["RUNTIME"]["BOP_CSV"] == ""
    cfg = argument.get_args(["--config_file", APE, "--bop_metrics", "--bop_csv", "out.csv"])
    assert cfg["RUNTIME"]["BOP_METRICS"] is True and cfg["RUNTIME"]["BOP_CSV"] == "out.csv"
    cfg = argument.get_args(["--config_file", APE, "--synthetic", "--bop_metrics"])
    assert cfg["RUNTIME"]["BOP_METRICS"] is True and cfg["RUNTIME"]["SYNTHETIC"] is True
    cfg, cfg_t = argument_kd.get_args(["--config_file", APE, "--config_file_t", APE])
    assert cfg["RUNTIME"]["BOP_METRICS"] is False
    cfg, cfg_t = argument_kd.get_args(["--config_file", APE, "--config_file_t", APE, "--bop_metrics"])
    assert cfg["RUNTIME"]["BOP_METRICS"] is True and "BOP_METRICS" not in cfg["KD"]
    with pytest.raises(SystemExit):
        argument_kd.get_argparser().parse_args(["--bop_csv", "x.csv"])          # the results file is test.py's


def test_valid_signature_keeps_its_defaults():
    import inspect
    from kd6d.libs.eval_libs import valid
    sig = inspect.signature(valid.__wrapped__ if hasattr(valid, "__wrapped__") else valid)
    assert list(sig.parameters)[-1] == "bop" and sig.parameters["bop"].default is None


# ---- the C ABI on the host ----------------------------------------------------------------------------------------------
def test_bop_errors_declared_exported_bound_and_built_like_pose_err():
    from kd6d import _lib, ops
    src = open(os.path.join(ROOT, "include", "kd6d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint kd6d_bop_errors\s*\(", code) and re.search(r"\bint64_t kd6d_bop_errors_workspace_floats\s*\(", code)
    assert re.search(r"#define KD6D_ABI_VERSION 11\b", src) and _lib.lib.kd6d_abi_version() == 11      # new symbols only
    assert len(_lib.SIGNATURES["kd6d_bop_errors"]) == 16 and len(_lib.SIGNATURES["kd6d_bop_errors_workspace_floats"]) == 2
    assert hasattr(_lib.lib, "kd6d_bop_errors") and callable(ops.bop_errors)
    assert "Bitwise property" in src and "pure function of problem p's own inputs" in src
    build = open(os.path.join(ROOT, "kd-6d-pose-adlp_amd", "build.py")).read()
    assert '"bop_err.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]' in build
    ws = _lib.lib.kd6d_bop_errors_workspace_floats
    assert (ws(0, 5), ws(3, 0), ws(3, 1), ws(7, 630), ws(100000, 20000)) == (0, 6, 6, 8820, 4000000000)


def _call(lib, P=2, missing=None, ws_floats=4):
    """Every pointer is a never-dereferenced dummy: each call here ends in the argument checks or launches nothing."""
    p = ctypes.c_void_p(16)
    a = {n: p for n in ("verts", "voff", "vcnt", "syms", "soff", "scnt", "K", "Rg", "Tg", "Rp", "Tp", "ws", "err")}
    if missing:
        a[missing] = None
    return lib.kd6d_bop_errors(P, a["verts"], a["voff"], a["vcnt"], a["syms"], a["soff"], a["scnt"], a["K"], a["Rg"],
                               a["Tg"], a["Rp"], a["Tp"], a["ws"], ws_floats, a["err"], None)


def test_bop_errors_argument_checks_fail_loudly_without_gpu():
    from kd6d import _lib
    lib = _lib.lib
    for name in ("verts", "voff", "vcnt", "syms", "soff", "scnt", "K", "Rg", "Tg", "Rp", "Tp", "ws", "err"):
        assert _call(lib, missing=name) == -1, name
        assert b"kd6d_bop_errors: null pointer" in lib.kd6d_last_error(), name
    assert _call(lib, P=-1) == -1 and b"n_problems=-1" in lib.kd6d_last_error()
    assert _call(lib, P=2, ws_floats=3) == -1 and b"workspace of 3 floats" in lib.kd6d_last_error()
    assert _call(lib, P=1, ws_floats=2 * 65536 * 16) == -1 and b"at most" in lib.kd6d_last_error()
    with pytest.raises(_lib.Kd6dError, match="workspace of 3 floats"):
        _lib.check(_call(lib, P=2, ws_floats=3), "kd6d_bop_errors")
    # nothing to score: success without a launch, and no pointer is looked at
    assert _call(lib, P=0) == 0 and _call(lib, P=0, missing="verts", ws_floats=0) == 0
