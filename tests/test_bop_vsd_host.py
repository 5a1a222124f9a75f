"""CPU: the float64 definitions of BOP's VSD (kd6d/libs/bop_metrics.py: render_depth_host, vsd_errors_host) against the
closed-form table and against the independent restatement of tests/bop_vsd_cases.py; the rasteriser contract; the
conditions the device tests rely on (ambiguous pixels <= 1 % of a render, b[p] <= 2 % of n_u, the recorded tolerances);
PLY faces and depth reading; the walk of evaluate_bop_vsd with errors_fn = vsd_errors_host; the tables, keys and flags."""
import json
import os

import numpy as np
import pytest

import bop_metric_cases as MC
import bop_vsd_cases as C
from kd6d.libs import bop_metrics as B
from kd6d.libs import dataset as D


def _host(case, idx=None):
    case = case if idx is None else C.subset(case, np.asarray(idx))
    return B.vsd_errors_host(*[case[k] for k in C.ARG_ORDER], C.DELTA, C.TAUS)


# ---- the closed forms ---------------------------------------------------------------------------------------------------
def test_closed_forms_of_vsd_errors_host():
    case, rows = C.closed_form_call()
    counts, err = _host(case)
    assert len(rows) == 9
    for p, r in enumerate(rows):
        assert (counts[p, 0], counts[p, 1]) == (r["n_u"], r["n_inter"]), r["name"]
        assert err[p].tolist() == [a / d for a, d in r["err"]], r["name"]
    # the restatement gives the same integers
    ref_counts, _, b = C.reference_counts(case)
    assert np.array_equal(ref_counts, counts) and (b == 0).all()


# ---- the rasteriser -----------------------------------------------------------------------------------------------------
def test_plate_coverage_and_depth_are_exact():
    H, W = C.PLATE_HW
    d = B.render_depth_host(C.plate().vertices, C.plate().faces, C.K_PLATE, np.eye(3), [0, 0, 1000.0], H, W)
    want = np.zeros((H, W))
    want[9:29, 11:41] = 1000.0
    assert np.array_equal(d, want) and (d > 0).sum() == 600
    assert np.array_equal(C.restate_render(C.plate(), C.K_PLATE, np.eye(3), [0, 0, 1000.0], H, W), want)


def test_a_pixel_centre_on_a_shared_edge_is_covered_once_with_that_depth():
    H, W = C.PLATE_HW
    sq = C.plate(u=(10.0, 40.0), v=(8.0, 28.0))                       # integer corners: the diagonal passes pixel centres
    R = C.rot([0, 1, 0], 0.0)
    d = B.render_depth_host(sq.vertices, sq.faces, C.K_PLATE, R, [0, 0, 1000.0], H, W)
    assert (d > 0).sum() == 31 * 21                                   # inclusive edges: the border pixels are covered
    on_diagonal = [(8 + 2 * k, 10 + 3 * k) for k in range(11)]        # (row, column): 2 (u - 10) = 3 (v - 8)
    assert all(d[r, c] == 1000.0 for r, c in on_diagonal)
    one = B.render_depth_host(sq.vertices, sq.faces[:1], C.K_PLATE, R, [0, 0, 1000.0], H, W)
    two = B.render_depth_host(sq.vertices, sq.faces[1:], C.K_PLATE, R, [0, 0, 1000.0], H, W)
    assert all(one[r, c] == 1000.0 and two[r, c] == 1000.0 for r, c in on_diagonal)      # both triangles own the edge
    assert ((one > 0) & (two > 0)).sum() == 11 and np.array_equal(np.maximum(one, two), d)


def test_face_order_duplicates_and_both_windings():
    rng = np.random.default_rng(2)
    m = C.meshes()[2]
    K, R, T = C.render_cases()[4][2:5]
    d = B.render_depth_host(m.vertices, m.faces, K, R, T, 97, 130)
    f = m.faces[rng.permutation(len(m.faces))]
    f = np.concatenate([f, f[:40]])
    assert np.array_equal(B.render_depth_host(m.vertices, f, K, R, T, 97, 130), d)
    flipped = B.render_depth_host(m.vertices, m.faces[:, ::-1], K, R, T, 97, 130)                   # no culling
    assert np.array_equal(flipped > 0, d > 0) and np.abs(flipped - d).max() < 1e-9
    assert np.array_equal(C.restate_render(m, K, R, T, 97, 130) > 0, d > 0)
    assert np.abs(C.restate_render(m, K, R, T, 97, 130) - d).max() < 1e-8


def test_a_triangle_with_a_vertex_behind_the_camera_is_dropped():
    H, W = C.PLATE_HW
    v = np.array([[-20.0, -10, 1000], [25.0, -5, 1000], [0.0, 30, 1000], [0.0, 30, -5.0], [0.0, 30, 0.0]])
    ok = B.render_depth_host(v, [[0, 1, 2]], C.K_PLATE, np.eye(3), [0, 0, 0.0], H, W)
    assert (ok > 0).sum() > 50
    for bad in (3, 4):                                                # z < 0 and z == 0
        assert not B.render_depth_host(v, [[0, 1, bad]], C.K_PLATE, np.eye(3), [0, 0, 0.0], H, W).any()
        both = B.render_depth_host(v, [[0, 1, bad], [0, 1, 2]], C.K_PLATE, np.eye(3), [0, 0, 0.0], H, W)
        assert np.array_equal(both, ok)
    # a degenerate (zero-area) triangle is skipped
    assert not B.render_depth_host(v, [[0, 1, 1]], C.K_PLATE, np.eye(3), [0, 0, 0.0], H, W).any()


def test_host_definition_equals_the_restatement_on_the_render_cases():
    ms = C.meshes()
    for name, mi, K, R, T, H, W in C.render_cases():
        if mi == 3 and (H, W) != (48, 64):
            continue                                                  # one 1281-face render through the slow definition is enough
        d = B.render_depth_host(ms[mi].vertices, ms[mi].faces, K, R, T, H, W)
        r = C.restate_render(ms[mi], K, R, T, H, W)
        assert np.array_equal(d > 0, r > 0), name
        assert np.abs(d - r).max() < 1e-7, name


# ---- what the device tests rely on --------------------------------------------------------------------------------------
def test_tolerances_are_the_recorded_ones_and_the_references_stay_within_their_caps():
    tol = C.tolerances()
    print("eps_px %.4e eps_d %.4e" % (tol["eps_px"], tol["eps_d"]))
    assert tol["eps_px"] == pytest.approx(C.RECORDED["eps_px"], rel=1e-3)
    assert tol["eps_d"] == pytest.approx(C.RECORDED["eps_d"], rel=1e-3)
    assert 1e-5 < tol["eps_px"] < 1e-2 and 1e-5 < tol["eps_d"] < 1e-1       # fp32 at 100 ... 1000: nothing else is plausible
    sizes = set()
    for (name, mi, K, R, T, H, W), (ref, amb) in zip(C.render_cases(), C.render_references()):
        sizes.add((H, W))
        assert amb.sum() <= 0.01 * max((ref > 0).sum(), 1), name
    assert sizes == {(48, 64), (50, 70), (97, 130), (150, 200)}
    names = " ".join(c[0] for c in C.render_cases())
    assert "cut by the border" in names and "several tiles" in names and "outside the image" in names
    counts, err, b = C.mixed_reference()
    assert len(b) == 30 and (b <= 0.02 * np.maximum(counts[:, 0], 1)).all()
    assert (counts[:, 0] > 0).all() and err.min() == 0.0 and err.max() == 1.0


def test_mixed_call_through_the_host_definition():
    case = C.mixed_call()
    idx = [0, 1, 2, 9, 26]
    counts, err = _host(case, idx)
    ref_counts, ref_err, b = C.mixed_reference()
    assert (np.abs(counts - ref_counts[idx]) <= b[idx][:, None]).all()
    assert len(set(case["frame"].tolist())) == 26 and len(case["frame"]) == 30       # frames shared by several problems


# ---- PLY faces and depth reading ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
@pytest.mark.parametrize("types", [("uchar", "int"), ("uchar", "uint"), ("ushort", "short")])
def test_load_ply_faces(tmp_path, fmt, types):
    verts = np.arange(18, dtype=np.float64).reshape(6, 3) * 1.5
    polys = [[0, 1, 2], [0, 2, 3, 4], [5, 4, 3, 2, 1]]
    for extra, name in ((False, "vertex_indices"), (True, "vertex_index")):
        path = str(tmp_path / ("m_%s_%d.ply" % (fmt, extra)))
        C.write_ply(path, verts, polys, fmt, types[0], types[1], extra, name)
        f = D.load_ply_faces(path)
        assert f.dtype == np.int32
        assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [5, 4, 3], [5, 3, 2], [5, 2, 1]]
        assert np.allclose(D.load_ply_vertices(path), verts)          # the vertex reader is untouched by the face element


def test_load_bop_meshes_fills_faces_and_vertex_only_files_have_none(tmp_path):
    models = tmp_path / "models"
    models.mkdir()
    C.write_ply(str(models / "obj_000002.ply"), C.cube().vertices, C.CUBE_FACES, "binary_little_endian", extra=True)
    with open(str(models / "obj_000007.ply"), "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                "0 0 0\n1 1 1\n")
    meshes, table = D.load_bop_meshes(str(models))
    assert table == {"2": 0, "7": 1}
    assert meshes[0].faces.tolist() == C.CUBE_FACES and np.allclose(meshes[0].vertices, C.cube().vertices)
    assert meshes[1].faces.shape == (0, 3) and D.Mesh(np.zeros((1, 3))).faces is None
    with pytest.raises(ValueError, match="no faces"):
        B.evaluate_bop_vsd({}, 3, meshes, [1.0, 1.0], lambda m: None, None, errors_fn=B.vsd_errors_host)


def test_load_depth_mm(tmp_path):
    rgb, raw = C.write_depth_tree(str(tmp_path))
    cache = {}
    d = D.load_depth_mm(rgb, cache)
    assert d.dtype == np.float32 and d.shape == raw.shape and d[0, 0] == 0
    assert np.array_equal(d, raw.astype(np.float32) * np.float32(0.1)) and raw.max() > 50000    # 16 bits are kept
    assert any(k.endswith("scene_camera.json") for k in cache)
    missing = rgb.replace("000007", "000008")
    with pytest.raises(FileNotFoundError, match="depth/000008.png"):
        D.load_depth_mm(missing, cache)


def test_a_bop_tree_with_faces_and_depth_scores_one_through_the_readers(tmp_path):
    """load_bop_meshes (faces) + get_single_bop_annotation + load_depth_mm feed evaluate_bop_vsd: predictions = ground
    truth on the frames of tests/frame_cache_cases.py score AR_VSD = 1, and a frame without its depth image is an error."""
    import frame_cache_cases as F
    tree = F.write_cache_tree(str(tmp_path / "tree"))
    C.add_faces_and_depth(tree, F.EVAL_IDS)
    meshes, table = D.load_bop_meshes(tree["models"])
    assert table == {"1": 0, "5": 1} and [len(m.faces) for m in meshes] == [12, 320]
    metas = []
    for im in F.EVAL_IDS:
        path = os.path.join(tree["scene"], "rgb", "%06d.png" % im)
        K, _, cls, Rs, Ts = D.get_single_bop_annotation(path, table)
        metas.append({"path": path, "K": K, "class_ids": cls, "rotations": Rs, "translations": Ts})
    cache = {}
    out = B.evaluate_bop_vsd(C.gt_predictions(metas), 3, meshes, [40.0, 35.0], lambda m: D.load_depth_mm(m["path"], cache),
                             None, errors_fn=B.vsd_errors_host)
    assert [e["n"] for e in out["per_class"]] == [3, 2] and out["AR_VSD"] == 1.0
    os.remove(os.path.join(tree["scene"], "depth", "%06d.png" % F.EVAL_IDS[-1]))
    with pytest.raises(FileNotFoundError, match="depth/%06d.png" % F.EVAL_IDS[-1]):
        B.evaluate_bop_vsd(C.gt_predictions(metas), 3, meshes, [40.0, 35.0], lambda m: D.load_depth_mm(m["path"], cache),
                           None, errors_fn=B.vsd_errors_host)


# ---- the walk -----------------------------------------------------------------------------------------------------------
def _moved(preds, shift):
    out = {}
    for name, it in preds.items():
        out[name] = {"meta": it["meta"], "pred": [[s, c, R, T + np.asarray(shift).reshape(3, 1)] for s, c, R, T in it["pred"]]}
    return out


def test_evaluate_bop_vsd_walk():
    preds, ms, diam, depths = C.eval_collection()
    calls = []

    def fn(*a):
        calls.append(len(a[2]))
        return B.vsd_errors_host(*a)
    depth_fn = lambda meta: depths[meta["path"]]  # noqa: E731
    same = B.evaluate_bop_vsd(preds, 4, ms, diam, depth_fn, None, errors_fn=fn)
    assert same["AR_VSD"] == 1.0 and [e["n"] for e in same["per_class"]] == [4, 2, 3] and calls == [9]
    assert same["vsd_thresholds"] == {"delta": 15.0, "tau": B.VSD_TAUS, "theta": B.VSD_THETAS}
    del calls[:]
    by_one = B.evaluate_bop_vsd(preds, 4, ms, diam, depth_fn, None, errors_fn=fn, max_images_per_call=1)
    assert json.dumps(by_one) == json.dumps(same) and len(calls) == 6 and sum(calls) == 9        # chunking by one frame
    far = B.evaluate_bop_vsd(_moved(preds, [10 * max(diam), 0, 0]), 4, ms, diam, depth_fn, None, errors_fn=fn)
    assert far["AR_VSD"] == 0.0                                       # ten diameters sideways
    # a class without predictions counts as missed, and never reaches the scorer
    del calls[:]
    no1 = {n: {"meta": it["meta"], "pred": [q for q in it["pred"] if q[1] != 1]} for n, it in preds.items()}
    out = B.evaluate_bop_vsd(no1, 4, ms, diam, depth_fn, None, errors_fn=fn)
    assert [e["AR_VSD"] for e in out["per_class"]] == [1.0, 0.0, 1.0] and out["AR_VSD"] == pytest.approx(2.0 / 3.0)
    assert sum(calls) == 7


def test_tables_keys_and_the_three_term_line():
    t = B.bop_vsd_tables(3, [0, 0, 2], [np.zeros(10), None, np.full(10, 0.26)])
    assert t["per_class"][1] == {} and t["per_class"][0] == {"n": 2, "AR_VSD": 0.5}
    assert t["per_class"][2]["AR_VSD"] == pytest.approx(0.5)          # 0.26 < theta for theta = 0.30 ... 0.50: 5 of 10
    assert t["AR_VSD"] == pytest.approx(0.5)
    preds, ms, diam, sets = MC.recall_collection()
    two = B.evaluate_bop_predictions(preds, 4, ms, diam, sets, None, errors_fn=B.bop_errors_host)
    before = json.dumps(two)
    keys = set(two)
    vt = B.bop_vsd_tables(3, [c for c in range(3) for it in preds.values() if c in it["meta"]["class_ids"]],
                          [np.zeros(10)] * two["n_objects"])
    three = B.add_vsd_tables(json.loads(before), vt)
    assert set(three) == keys | {"vsd_thresholds", "AR_VSD", "AR_BOP", "AR_BOP_note"}
    assert three["AR"] == two["AR"] and three["note"] == B.AR_NOTE and three["AR_VSD"] == 1.0
    assert three["AR_BOP"] == pytest.approx((1.0 + two["AR_MSSD"] + two["AR_MSPD"]) / 3.0)
    assert json.dumps(two) == before                                   # without vsd the dict is today's
    line = B.format_ar_bop_line(three)
    assert line.startswith("BOP AR_VSD 1.0000  AR_MSSD ") and "AR_BOP" in line and "three terms" in line
    assert B.format_ar_line(two).startswith("BOP AR_MSSD ") and "VSD term is not built" in B.format_ar_line(two)


def test_flags(capsys):
    from kd6d.arguments import argument, argument_kd
    ape = os.path.join(C.ROOT, "configs", "ape.yaml")
    cfg = argument.get_args(["--config_file", ape, "--synthetic", "--bop_metrics", "--bop_vsd"])
    assert cfg["RUNTIME"]["BOP_VSD"] is True and cfg["RUNTIME"]["BOP_METRICS"] is True
    assert argument.get_args(["--config_file", ape, "--synthetic", "--bop_metrics"])["RUNTIME"]["BOP_VSD"] is False
    with pytest.raises(SystemExit):
        argument.get_args(["--config_file", ape, "--synthetic", "--bop_vsd"])
    assert "--bop_vsd requires --bop_metrics" in capsys.readouterr().err
    p = argument_kd.get_argparser()
    args = p.parse_args(["--bop_vsd"])
    with pytest.raises(SystemExit):
        argument_kd.check_bop_flags(p, args)
    assert "--bop_vsd requires --bop_metrics" in capsys.readouterr().err
    args = p.parse_args(["--bop_vsd", "--bop_metrics"])
    argument_kd.check_bop_flags(p, args)
    assert args.bop_vsd and args.bop_metrics


def test_synthetic_cube_faces_close_the_cube():
    from kd6d.synthetic import CUBE_FACES, cube_keypoints
    v = cube_keypoints([100.0])[0].astype(np.float64)
    assert CUBE_FACES.shape == (12, 3) and CUBE_FACES.tolist() == C.CUBE_FACES
    edges = {}
    for a, b, c in CUBE_FACES:
        for e in ((a, b), (b, c), (c, a)):
            edges[tuple(sorted(e))] = edges.get(tuple(sorted(e)), 0) + 1
    assert len(edges) == 18 and set(edges.values()) == {2}            # a closed surface: every edge in two triangles
    n = np.cross(v[CUBE_FACES[:, 1]] - v[CUBE_FACES[:, 0]], v[CUBE_FACES[:, 2]] - v[CUBE_FACES[:, 0]])
    assert (np.abs(n) > 0).sum(axis=1).tolist() == [1] * 12           # every triangle lies in a face of the cube


# ---- the C ABI on the host ----------------------------------------------------------------------------------------------
def _abi(lib, which, n=2, missing=None, ws_ints=8, n_tau=10, H=48, W=64):
    """Every pointer is a never-dereferenced dummy: each call here ends in the argument checks or launches nothing."""
    import ctypes
    p = ctypes.c_void_p(16)
    names = ("verts", "faces", "voff", "vcnt", "foff", "fcnt", "K", "Rg", "Tg", "Rp", "Tp", "diam", "frame", "depth", "ws",
             "counts", "err", "out")
    a = {k: (None if k == missing else p) for k in names}
    if which == "render":
        return lib.kd6d_render_depth(n, a["verts"], 8, a["faces"], 12, a["voff"], a["vcnt"], a["foff"], a["fcnt"], a["K"],
                                     a["Rg"], a["Tg"], H, W, a["ws"], ws_ints, a["out"], None)
    tau = None if missing == "tau" else (ctypes.c_float * 16)(*([0.1] * 16))
    return lib.kd6d_bop_vsd(n, a["verts"], 8, a["faces"], 12, a["voff"], a["vcnt"], a["foff"], a["fcnt"], a["K"], a["Rg"],
                            a["Tg"], a["Rp"], a["Tp"], a["diam"], a["frame"], a["depth"], 3, H, W, 15.0, tau, n_tau, a["ws"],
                            ws_ints, a["counts"], a["err"], None)


def test_entry_points_are_declared_bound_and_check_their_arguments_without_gpu():
    import re
    from kd6d import _lib, ops
    lib = _lib.lib
    src = open(os.path.join(C.ROOT, "include", "kd6d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint kd6d_render_depth\s*\(", code) and re.search(r"\bint kd6d_bop_vsd\s*\(", code)
    assert re.search(r"\bint64_t kd6d_bop_vsd_workspace_ints\s*\(", code)
    assert re.search(r"#define KD6D_ABI_VERSION 11\b", src) and lib.kd6d_abi_version() == 11          # new symbols only
    assert callable(ops.render_depth) and callable(ops.bop_vsd) and ops.VSD_MAX_TAU == 16
    build = open(os.path.join(C.ROOT, "kd-6d-pose-adlp_amd", "build.py")).read()
    assert '"bop_vsd.hip": ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]' in build
    ws = lib.kd6d_bop_vsd_workspace_ints
    assert (ws(0), ws(-3), ws(1), ws(13000)) == (0, 0, 4, 52000)
    for name in ("verts", "faces", "voff", "vcnt", "foff", "fcnt", "K", "Rg", "Tg", "ws", "out"):
        assert _abi(lib, "render", missing=name) == -1 and b"kd6d_render_depth: null pointer" in lib.kd6d_last_error(), name
    for name in ("verts", "faces", "voff", "vcnt", "foff", "fcnt", "K", "Rg", "Tg", "Rp", "Tp", "diam", "frame", "depth", "tau",
                 "ws", "counts", "err"):
        assert _abi(lib, "vsd", missing=name) == -1 and b"kd6d_bop_vsd: null pointer" in lib.kd6d_last_error(), name
    assert _abi(lib, "vsd", n=-1) == -1 and b"n=-1" in lib.kd6d_last_error()
    assert _abi(lib, "vsd", n_tau=17) == -1 and b"n_tau=17" in lib.kd6d_last_error()
    assert _abi(lib, "vsd", n_tau=0) == -1 and b"n_tau=0" in lib.kd6d_last_error()
    assert _abi(lib, "vsd", ws_ints=7) == -1 and b"workspace of 7 ints" in lib.kd6d_last_error()
    assert _abi(lib, "render", ws_ints=7) == -1 and b"workspace of 7 ints" in lib.kd6d_last_error()
    assert _abi(lib, "render", H=0) == -1 and b"image of 64 x 0 pixels" in lib.kd6d_last_error()
    assert _abi(lib, "vsd", W=64 * 70000) == -1 and b"image of" in lib.kd6d_last_error()
    # nothing to do: success without a launch, and no pointer is looked at
    assert _abi(lib, "vsd", n=0, missing="verts", ws_ints=0) == 0 and _abi(lib, "render", n=0, missing="out", ws_ints=0) == 0
