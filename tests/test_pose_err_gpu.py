"""GPU: kd6d_pose_errors (csrc/pose_err.hip) against the reference's own compute_pose_diff capture
(tests/golden/eval_metrics.npz), its matches against float64 argmin, the accuracy tables of
evaluate_pose_predictions_device against the reference's evaluate_pose_predictions capture, bitwise determinism and
batch independence, valid(scorer="device") and the evaluation entry test.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_pose_err_host import close, numpy_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, G)

# Worst relative deviation of err from the reference rows, measured on the MI355X (profiles/pose_err_device.md); the
# test asserts 4 x that (the draw-dependent spread over 24 rows), never more than CAP: fp32 at these magnitudes cannot
# justify more, and a kernel that needs it is wrong.
MEASURED_REL = {"e3": 1.293e-7, "e2": 3.826e-7}
CAP = 1e-4
TAU = 0.01            # mm: ten times the fp32 error of a distance formed at ~1500 mm coordinates
CHILD_TIMEOUT = 600


def _golden_rows():
    from make_golden_eval import eval_inputs
    z = np.load(os.path.join(G, "eval_metrics.npz"))
    meshes, diam, K, preds = eval_inputs(int(z["seed"]))
    probs = []
    for row in z["pose_diff"]:
        i, mi, sym = int(row[0]), int(row[1]), int(row[2])
        it = preds["img%02d" % i]
        n = len(meshes[mi])
        np.random.seed(100 + i)
        idx = np.random.choice(n, 1000, replace=True) if n > 1000 else np.arange(n)
        probs.append(dict(mesh=mi, idx=idx, sym=sym, K=K, Rg=it["meta"]["rotations"][0],
                          Tg=it["meta"]["translations"][0].reshape(3), Rp=row[7:16].reshape(3, 3), Tp=row[16:19],
                          want=row[3:5]))
    return meshes, probs


def _arrays(meshes, probs, with_vidx=True):
    """Host arrays of a batch in kd6d_pose_errors' layout (float64 where the device takes fp32)."""
    offs = np.concatenate([[0], np.cumsum([len(m) for m in meshes])])
    max_v = max(len(p["idx"]) for p in probs)
    vidx = np.zeros((len(probs), max_v), np.int32)
    for k, p in enumerate(probs):
        vidx[k, :len(p["idx"])] = p["idx"]
    return dict(max_v=max_v, verts=np.concatenate(meshes), voff=np.asarray([offs[p["mesh"]] for p in probs], np.int32),
                vcnt=np.asarray([len(p["idx"]) for p in probs], np.int32), vidx=vidx if with_vidx else None,
                K=np.stack([p["K"] for p in probs]), Rg=np.stack([p["Rg"] for p in probs]),
                Tg=np.stack([p["Tg"] for p in probs]), Rp=np.stack([p["Rp"] for p in probs]),
                Tp=np.stack([p["Tp"] for p in probs]), sym=np.asarray([p["sym"] for p in probs], np.int32))


def _launch(a, dev, want_nn=False):
    from kd6d import ops

    def t(x):
        return None if x is None else torch.from_numpy(
            np.ascontiguousarray(x, np.float32 if x.dtype == np.float64 else x.dtype)).to(dev)
    return ops.pose_errors(t(a["verts"]), t(a["voff"]), t(a["vcnt"]), t(a["vidx"]), t(a["K"]), t(a["Rg"]), t(a["Tg"]),
                           t(a["Rp"]), t(a["Tp"]), t(a["sym"]), max_v=a["max_v"], want_nn=want_nn)


def test_golden_rows_match_the_reference_capture(gpu_device):
    """The 24 pose_diff rows (meshes of 300, 1500 and 800 vertices, symmetric and not), e3 / e2 captured from the
    reference's compute_pose_diff, index draws under np.random.seed(100 + i) as the capture made them."""
    meshes, probs = _golden_rows()
    assert len(probs) == 24 and {len(p["idx"]) for p in probs} == {300, 1000, 800}
    err = _launch(_arrays(meshes, probs), gpu_device).cpu().numpy().astype(np.float64)
    want = np.stack([p["want"] for p in probs])
    rel = np.abs(err - want) / np.abs(want)
    for k, p in enumerate(probs):
        print("row %2d mesh %d sym %d: e3 %.9g (ref %.9g, rel %.2e)  e2 %.9g (ref %.9g, rel %.2e)"
              % (k, p["mesh"], p["sym"], err[k, 0], want[k, 0], rel[k, 0], err[k, 1], want[k, 1], rel[k, 1]))
    print("worst relative deviation: e3 %.3e  e2 %.3e" % (rel[:, 0].max(), rel[:, 1].max()))
    for col, name in enumerate(("e3", "e2")):
        bound = min(4.0 * MEASURED_REL[name], CAP)
        assert 4.0 * MEASURED_REL[name] <= CAP, "the measured deviation of %s needs more than the cap" % name
        assert rel[:, col].max() <= bound, (name, rel[:, col].max(), bound)


def test_symmetric_matches_equal_float64_argmin_away_from_ties(gpu_device):
    meshes, probs = _golden_rows()
    probs = [p for p in probs if p["sym"]]
    assert len(probs) == 12
    a = _arrays(meshes, probs)
    err, nn = _launch(a, gpu_device, want_nn=True)
    nn = nn.cpu().numpy()
    for k, p in enumerate(probs):
        n = len(p["idx"])
        m = meshes[p["mesh"]][p["idx"]]
        ga = m @ p["Rg"].T + p["Tg"]
        gb = m @ p["Rp"].T + p["Tp"]
        d = np.linalg.norm(ga[:, None, :] - gb[None, :, :], axis=2)
        want = np.argmin(d, axis=1)
        two = np.partition(d, 1, axis=1)[:, :2]
        near_tie = (two[:, 1] - two[:, 0]) < TAU
        share = near_tie.mean()
        differ = nn[k, :n] != want
        print("sym row %2d: %d vertices, %.3f %% within tau of a tie, %d matches differ" % (k, n, 100 * share, differ.sum()))
        assert share <= 0.01, "row %d: %.2f %% of the vertices lie within tau of a tie" % (k, 100 * share)
        assert not (differ & ~near_tie).any(), (k, np.nonzero(differ & ~near_tie)[0][:8])
        assert (nn[k, n:] == -1).all() and nn[k, :n].min() >= 0 and nn[k, :n].max() < n
        # a duplicate drawn twice ties exactly: the lowest position wins, as np.argmin
        assert (nn[k, :n][differ] >= 0).all()


def _capture_inputs():
    from make_golden_eval import _Mesh, eval_inputs
    z = np.load(os.path.join(G, "eval_metrics.npz"))
    meshes, diam, K, preds = eval_inputs(int(z["seed"]))
    return [_Mesh(m) for m in meshes], diam, preds, json.loads(str(z["evaluate_json"]))


def _compare_tables(got, ref, n_per_class, near_classes, note=""):
    """Accuracies are threshold counts: equal (a class with an error within 1e-4 relative of a threshold gets the
    slack of one object).  AUC is 1000 bins of 0.1 mm: one bin-edge flip of one object moves it by
    100 / (1000 n_objects), one flip per object is allowed -> 0.1."""
    adi, auc, rep, adi_d, rep_d, rng = got
    r_adi, r_auc, r_rep, r_adi_d, r_rep_d, r_rng = ref
    close(json.loads(json.dumps([float(x) for x in rng])), r_rng, 1e-12)
    for c in range(len(r_adi)):
        slack = (100.0 / n_per_class[c] if c in near_classes else 0.0) + 1e-9
        assert adi[c].keys() == r_adi[c].keys() and rep[c].keys() == r_rep[c].keys() and auc[c].keys() == r_auc[c].keys()
        for k in r_adi[c]:
            assert abs(adi[c][k] - r_adi[c][k]) <= slack, ("class %d %s%s" % (c, k, note), adi[c][k], r_adi[c][k])
        for k in r_rep[c]:
            assert abs(rep[c][k] - r_rep[c][k]) <= slack, ("class %d %s%s" % (c, k, note), rep[c][k], r_rep[c][k])
        for k in r_auc[c]:
            assert abs(auc[c][k] - r_auc[c][k]) <= 0.1 + 1e-9, ("class %d AUC" % c, auc[c][k], r_auc[c][k])
    for mine, theirs in ((adi_d, r_adi_d), (rep_d, r_rep_d)):
        for b in range(len(theirs)):
            assert mine[b].keys() == theirs[b].keys()
            for k in theirs[b]:
                slack = 100.0 if near_classes else 1e-9        # a depth bin mixes classes: only checked without slack
                assert abs(mine[b][k] - theirs[b][k]) <= slack, ("depth bin %d %s%s" % (b, k, note), mine[b][k], theirs[b][k])


def _near_threshold_classes(per_object, diam):
    """per_object: (class, e3, e2) in float64.  Classes with an error within 1e-4 relative of a threshold."""
    from kd6d.libs.evaluate import ADI_THRESHOLDS, REP_THRESHOLDS
    near = set()
    for c, e3, e2 in per_object:
        if any(abs(e3 / diam[c] - th) <= 1e-4 * th for th in ADI_THRESHOLDS) or \
                any(abs(e2 - th) <= 1e-4 * th for th in REP_THRESHOLDS):
            near.add(c)
    return near


def test_tables_match_the_reference_capture(gpu_device):
    from kd6d.libs import evaluate as E
    meshes, diam, preds, ref = _capture_inputs()
    sym = {"cls_2": ["Z", 0]}
    # float64 errors of the capture's objects, to see whether any sits on a threshold
    per_object = []

    def spy(max_v, verts, voff, vcnt, vidx, *rest):
        err = numpy_errors(max_v, verts, voff, vcnt, vidx, *rest)
        offs = [0, 300, 1800]
        per_object.extend((offs.index(int(o)), e[0], e[1]) for o, e in zip(voff, err))
        return err
    np.random.seed(7)
    res64 = E.evaluate_pose_predictions_device(preds, 4, meshes, diam, sym, None, errors_fn=spy)
    close(json.loads(json.dumps([res64[0], res64[1], res64[2], res64[3], res64[4]], sort_keys=True)), ref[:5], 1e-9)
    near = _near_threshold_classes(per_object, diam)
    note = " (class within 1e-4 of a threshold: slack of one object)" if near else ""
    n_per_class = [sum(1 for it in preds.values() if c in it["meta"]["class_ids"]) for c in range(3)]
    np.random.seed(7)
    got = E.evaluate_pose_predictions_device(preds, 4, meshes, diam, sym, gpu_device)
    print("device tables:", json.dumps(got[:3]))
    _compare_tables(got, ref, n_per_class, near, note)
    # the vertex pool of this mesh list was uploaded once and is found again
    assert sum(1 for held, *_ in E._POOLS if len(held) == 3 and all(a is m.vertices for a, m in zip(held, meshes))) == 1
    np.random.seed(7)
    again = E.evaluate_pose_predictions_device(preds, 4, meshes, diam, sym, gpu_device)
    assert json.dumps(again) == json.dumps(got)
    assert sum(1 for held, *_ in E._POOLS if len(held) == 3 and all(a is m.vertices for a, m in zip(held, meshes))) == 1


def test_two_launches_agree_bit_for_bit(gpu_device):
    meshes, probs = _golden_rows()
    a = _arrays(meshes, probs)
    e1, n1 = _launch(a, gpu_device, want_nn=True)
    e2, n2 = _launch(a, gpu_device, want_nn=True)
    assert torch.equal(e1, e2) and torch.equal(n1, n2)
    assert torch.isfinite(e1).all()


def test_mixed_batch_equals_every_problem_alone(gpu_device):
    """vcnt of 8, 300 and 1000, sym 0 and 1, with an index table and without: each problem's result is a function of
    its own inputs only, whatever the batch and max_v around it."""
    rng = np.random.default_rng(11)
    meshes = [rng.normal(0, 40, (n, 3)) for n in (8, 300, 1000)]
    K = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1.0]])

    def pose(z):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.linalg.det(q)
        return q, np.array([rng.normal(0, 60), rng.normal(0, 40), z])
    probs = []
    for mi in (0, 1, 2, 1, 0, 2):
        for sym in (0, 1):
            Rg, Tg = pose(900.0)
            Rp, Tp = pose(905.0)
            if mi != 1:
                Rp = Rg @ np.linalg.qr(np.eye(3) + rng.normal(0, 0.02, (3, 3)))[0]
            probs.append(dict(mesh=mi, idx=np.arange(len(meshes[mi])), sym=sym, K=K, Rg=Rg, Tg=Tg, Rp=Rp, Tp=Tp))
    shuffled = [dict(p, idx=rng.permutation(len(meshes[p["mesh"]]))) for p in probs]
    for batch, with_vidx in ((probs, False), (probs, True), (shuffled, True)):
        err, nn = _launch(_arrays(meshes, batch, with_vidx), gpu_device, want_nn=True)
        for k, p in enumerate(batch):
            e1, n1 = _launch(_arrays(meshes, [p], with_vidx), gpu_device, want_nn=True)
            n = len(p["idx"])
            assert torch.equal(e1[0], err[k]), (k, with_vidx, e1, err[k])
            assert torch.equal(n1[0, :n], nn[k, :n]) and bool((nn[k, n:] == -1).all())
    # the identity table and no table are the same launch
    assert torch.equal(_launch(_arrays(meshes, probs, True), gpu_device), _launch(_arrays(meshes, probs, False), gpu_device))
    # and the values are right: float64 restatement, loose fp32 bound
    want = numpy_errors(**_arrays(meshes, probs, False))
    got = _launch(_arrays(meshes, probs, False), gpu_device).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-4)


def test_pose_errors_wrapper_refuses_indices_outside_the_pool(gpu_device):
    meshes, probs = _golden_rows()
    a = _arrays(meshes, probs[:2])
    a["voff"] = a["voff"].copy(); a["voff"][1] = 2600 - 100
    with pytest.raises(ValueError, match="outside the vertex pool"):
        _launch(a, gpu_device)
    b = _arrays(meshes, probs[:2])
    b["vcnt"] = b["vcnt"].copy(); b["vcnt"][0] = 0
    with pytest.raises(ValueError, match="vcnt"):
        _launch(b, gpu_device)


def test_valid_device_scorer_matches_host_scorer(gpu_device):
    """The loader of test_eval_gpu.py::test_valid_loop_plumbing (8-vertex meshes: no draw is involved)."""
    from test_eval_gpu import _setup
    from kd6d.libs.eval_libs import valid
    from kd6d.synthetic import make_batch
    z, model, images, targets = _setup(gpu_device)
    cfg = model.cfg
    loader = []
    for i in range(2):
        im, tg = make_batch(2, 50 + i, crop=int(z["crop"]))
        im.tensors = im.tensors.to(gpu_device)
        metas = [{"path": "b%d_%d" % (i, j), "K": t.K.numpy(), "class_ids": [int(c) for c in t.class_ids],
                  "rotations": [r.numpy() for r in t.rotations], "translations": [x.numpy().reshape(3, 1) for x in t.translations]}
                 for j, t in enumerate(tg)]
        loader.append((im, tg, metas))
    n_cls = cfg["DATASETS"]["N_CLASS"] - 1
    meshes = [targets[0].keypoints_3d[c].numpy() for c in range(n_cls)]
    host_preds, dev_preds = {}, {}
    host = valid(cfg, 0, loader, model, gpu_device, meshes, scorer="host", preds_out=host_preds)
    dev = valid(cfg, 0, loader, model, gpu_device, meshes, scorer="device", preds_out=dev_preds)
    assert sorted(host_preds) == sorted(dev_preds) == ["b0_0", "b0_1", "b1_0", "b1_1"]
    n_per_class = [sum(1 for it in host_preds.values() if c in it["meta"]["class_ids"]) for c in range(n_cls)]
    print("valid host:", json.dumps(host[:3]), " device:", json.dumps(dev[:3]))
    ref = json.loads(json.dumps([host[0], host[1], host[2], host[3], host[4], [float(x) for x in host[5]]]))
    _compare_tables(dev, ref, n_per_class, set())
    with pytest.raises(ValueError):
        valid(cfg, 0, loader, model, gpu_device, meshes, scorer="nonsense")


def _run_entry(args):
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(ROOT, "test.py")] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30, cwd=ROOT)


def test_eval_entry_writes_predictions_and_metrics(gpu_device, tmp_path):
    from oracle import kd_step_ref as O
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    wd = str(tmp_path / "run1")
    base = ["--config_file", ape, "--backbone", "darknet_tiny_h", "--synthetic", "--pnp_solver", "device",
            "--eval_scorer", "device"]
    r = _run_entry(base + ["--working_dir", wd])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Random initialized weights." in r.stdout
    preds = json.load(open(os.path.join(wd, "preds.json")))
    assert sorted(preds) == sorted("val%d_%d" % (i, j) for i in range(2) for j in range(16))   # 2 batches of IMS_PER_BATCH
    for it in preds.values():
        assert {"K", "class_ids", "rotations", "translations"} <= set(it["meta"]) and len(it["pred"]) <= 1
        for score, cid, R, T in it["pred"]:
            assert np.asarray(R).shape == (3, 3) and np.asarray(T).shape == (3, 1)
    metrics = json.load(open(os.path.join(wd, "metrics.json")))
    assert set(metrics) == {"adi_per_class", "auc_per_class", "rep_per_class", "adi_per_depth", "rep_per_depth", "depth_range"}
    present = sorted({c for it in preds.values() for c in it["meta"]["class_ids"]})
    for c in present:
        assert set(metrics["adi_per_class"][c]) == {"ADI.05d", "ADI.10d", "ADI.20d", "ADI.50d"}
    assert "cls_%02d" % present[0] in r.stdout and "ADI.05d" in r.stdout
    # a saved, seeded state dict is loaded by name and the same images are scored
    wfile = str(tmp_path / "seeded.pth")
    torch.save(O.seeded_state_dict(O.PoseNetRef("darknet_tiny_h"), 1), wfile)
    wd2 = str(tmp_path / "run2")
    r2 = _run_entry(base + ["--working_dir", wd2, "--weight_file", wfile])
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert "Weights are loaded from " + wfile in r2.stdout and "Random initialized" not in r2.stdout
    assert sorted(json.load(open(os.path.join(wd2, "preds.json")))) == sorted(preds)
