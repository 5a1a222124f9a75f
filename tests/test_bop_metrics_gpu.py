"""GPU: kd6d_bop_errors (csrc/bop_err.hip) against the float64 restatement of tests/bop_metric_cases.py at every lane,
wave and symmetry-tile tail, against closed-form answers, its bitwise properties (batch, vertex order, symmetry order,
duplicates), its edges, and end to end through valid(..., bop={}) and test.py --bop_metrics.  Tolerances: 4 x the float32
restatement's own deviation (bop_metric_cases.tolerances(), profiles/bop_err_device.md)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bop_metric_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600


def _dev(case, dev):
    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x, np.float32 if x.dtype == np.float64 else x.dtype)).to(dev)
    return {k: t(v) for k, v in case.items()}


def _launch(case, dev, **kw):
    from kd6d import ops
    d = _dev(case, dev)
    return ops.bop_errors(d["verts"], d["voff"], d["vcnt"], d["syms"].reshape(-1, 12), d["soff"], d["scnt"], d["K"],
                          d["Rg"], d["Tg"], d["Rp"], d["Tp"], **kw)


def _report(name, got, ref):
    tol = C.tolerances()
    for col, m in enumerate(("mssd", "mspd")):
        d = np.abs(got[:, col] - ref[:, col])
        big = ref[:, col] >= C.SMALL
        print("%s %s: worst |got - ref64| %.3e below %g, worst relative %.3e from it on (bounds abs %.3e, rel %.3e)"
              % (name, m, d[~big].max() if (~big).any() else 0.0, C.SMALL,
                 (d[big] / ref[big, col]).max() if big.any() else 0.0, tol[m]["abs"], tol[m]["rel"]))


def test_mixed_launch_against_float64(gpu_device):
    """One launch of 49 problems: V in {1, 2, 63, 64, 65, 257, 1500} x S in {1, 2, 3, 16, 17, 315, 630}, shared and
    distinct meshes, a K per problem, pose errors 0 ... 20 degrees / 10 mm."""
    case = C.mixed_case()
    ref = C.references()["mixed"][0]
    got = _launch(case, gpu_device).cpu().numpy().astype(np.float64)
    for k in range(len(ref)):
        print("problem %2d V %4d S %3d: mssd %.7g (ref %.7g)  mspd %.7g (ref %.7g)"
              % (k, case["vcnt"][k], case["scnt"][k], got[k, 0], ref[k, 0], got[k, 1], ref[k, 1]))
    _report("mixed", got, ref)
    assert np.isfinite(got).all()
    for col in (0, 1):
        ok = C.within(got[:, col], ref[:, col], col)
        assert ok.all(), (col, np.nonzero(~ok)[0], got[~ok, col], ref[~ok, col])


def test_closed_forms_on_the_device(gpu_device):
    """2r for the half turn and 0 with it in the set, |d| for a translation, f d / z for an image-plane shift of a planar
    mesh, and pred = gt o S_k for k in the set: both errors within the absolute bound of 0."""
    case, exact, names = C.closed_form_case()
    ref = C.references()["closed"][0]
    tol = C.tolerances()
    got = _launch(case, gpu_device).cpu().numpy().astype(np.float64)
    _report("closed", got, ref)
    n_zero = 0
    for k, name in enumerate(names):
        for col, m in enumerate(("mssd", "mspd")):
            assert C.within(got[k:k + 1, col], ref[k:k + 1, col], col).all(), (name, m, got[k], ref[k])
            if not np.isnan(exact[k, col]):
                assert abs(got[k, col] - exact[k, col]) <= tol[m]["rel"] * exact[k, col] + tol[m]["abs"], (name, m, got[k], exact[k])
                n_zero += exact[k, col] == 0.0
    assert n_zero == 2 * 13                    # the Z-180 case and the twelve pred = gt o S_k cases, both metrics


def test_bitwise_properties(gpu_device):
    case = C.mixed_case()
    P = len(case["voff"])
    base = _launch(case, gpu_device)
    assert torch.equal(base, _launch(case, gpu_device))                         # two launches agree
    # a problem alone equals the same problem inside the batch (every symmetry-count class, the largest meshes)
    for k in (0, 8, 16, 24, 32, 40, 41, 45, 47, 48):
        alone = _launch(C.subset(case, np.array([k])), gpu_device)
        assert torch.equal(alone[0], base[k]), (k, alone, base[k])
    rev = _launch(C.subset(case, np.arange(P)[::-1].copy()), gpu_device)
    assert torch.equal(rev.flip(0), base)
    # permuting a problem's vertices: every mesh of the pool shuffled in place
    rng = np.random.default_rng(1)
    verts = case["verts"].copy()
    for off, n in {(int(o), int(n)) for o, n in zip(case["voff"], case["vcnt"])}:
        verts[off:off + n] = verts[off:off + n][rng.permutation(n)]
    assert not np.array_equal(verts, case["verts"])
    assert torch.equal(_launch(dict(case, verts=verts), gpu_device), base)
    # permuting a problem's symmetries: every set of the pool shuffled in place (the identity no longer first)
    syms = case["syms"].copy()
    for off, n in {(int(o), int(n)) for o, n in zip(case["soff"], case["scnt"])}:
        syms[off:off + n] = syms[off:off + n][rng.permutation(n)]
    assert not np.array_equal(syms, case["syms"])
    assert torch.equal(_launch(dict(case, syms=syms), gpu_device), base)


def test_duplicate_and_extra_symmetries(gpu_device):
    """Appending a duplicate of one of its symmetries leaves a problem's err bit-identical (also where it opens a new
    tile or another register-tile size); appending any other transform never raises it, and appending the transform that
    carries the ground truth onto the prediction lowers it."""
    case = C.mixed_case()
    P = len(case["voff"])
    base = _launch(case, gpu_device)
    rng = np.random.default_rng(2)
    sets = {}
    for off, n in zip(case["soff"], case["scnt"]):
        sets[(int(off), int(n))] = case["syms"][int(off):int(off) + int(n)]
    for extra in ("duplicate", "other"):
        pool, soff, scnt, at = [], [], [], 0
        for p in range(P):
            S = sets[(int(case["soff"][p]), int(case["scnt"][p]))]
            if extra == "duplicate":
                add = S[int(rng.integers(0, len(S)))][None]
            elif p % 2 == 0:     # the transform that carries the ground truth onto the prediction: pred = gt o E
                Rg, Tg, Rp, Tp = case["Rg"][p], case["Tg"][p], case["Rp"][p], case["Tp"][p]
                add = C.pack_syms(np.concatenate([Rg.T @ Rp, (Rg.T @ (Tp - Tg))[:, None]], axis=1))
            else:                # any rigid transform
                add = C.pack_syms(np.concatenate([C.random_rot(rng), rng.normal(0, 3, (3, 1))], axis=1))
            pool.append(np.concatenate([S, add]))
            soff.append(at); scnt.append(len(S) + 1)
            at += len(S) + 1
        more = dict(case, syms=np.concatenate(pool), soff=np.asarray(soff, np.int32), scnt=np.asarray(scnt, np.int32))
        got = _launch(more, gpu_device)
        if extra == "duplicate":
            assert torch.equal(got, base)
        else:
            assert bool((got <= base).all())
            assert bool((got[2::2] < base[2::2]).all())          # with E in the set the error drops to rounding (problem 0 is at 0 already)
            # (no comparison with float64 here: these sets are not among the cases the tolerances were derived from --
            # with E the error is the rounding of a ~1200 mm translation, and the float32 restatement itself leaves the
            # bound on one of them; accuracy is the business of the mixed launch and the closed forms)


def test_edges_and_wrapper_refusals(gpu_device):
    from kd6d import ops
    case = C.mixed_case()
    few = C.subset(case, np.array([0, 8, 20, 27]))                   # S = 1, 2, 630, 630
    base = _launch(few, gpu_device)
    # n_problems = 0
    none = _launch(C.subset(case, np.array([], np.int64)), gpu_device)
    assert tuple(none.shape) == (0, 2)
    # scnt = 0 is the identity alone, whatever soff says; problem 0's set is the identity
    ident = dict(few, scnt=np.array([0, 0, few["scnt"][2], few["scnt"][3]], np.int32),
                 soff=np.array([10 ** 6, few["soff"][1], few["soff"][2], few["soff"][3]], np.int32))
    got = _launch(ident, gpu_device)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2:], base[2:])
    only = _launch(dict(C.subset(few, np.array([1])), soff=np.array([0], np.int32), scnt=np.array([1], np.int32)), gpu_device)
    assert torch.equal(got[1], only[0])                             # ... and equals the explicit identity of the pool
    assert bool((got[1] >= base[1]).all())
    # an empty symmetry pool with identity-only problems
    bare = dict(C.subset(few, np.array([0, 1])), syms=np.zeros((0, 12)), soff=np.zeros(2, np.int32), scnt=np.zeros(2, np.int32))
    assert torch.equal(_launch(bare, gpu_device), got[:2])
    # vcnt = 0 gives {0, 0} and leaves the neighbours alone
    empty = dict(few, vcnt=np.array([few["vcnt"][0], 0, few["vcnt"][2], 0], np.int32),
                 voff=np.array([few["voff"][0], 10 ** 7, few["voff"][2], few["voff"][3]], np.int32))
    got = _launch(empty, gpu_device)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]) and bool((got[1] == 0).all()) and bool((got[3] == 0).all())
    # validate=False with the workspace sized by the caller is the same launch
    assert torch.equal(_launch(few, gpu_device, validate=False, max_scnt=630), base)
    assert torch.equal(_launch(few, gpu_device, validate=False), base)
    # out-of-pool indices are refused before anything is launched
    Nv, Ns = len(case["verts"]), len(case["syms"])
    for key, val, msg in (("voff", Nv - 5, "vertex pool"), ("voff", -1, "vertex pool"), ("vcnt", Nv + 1, "vertex pool"),
                          ("soff", Ns - 3, "symmetry pool"), ("soff", -2, "symmetry pool"), ("scnt", Ns + 1, "symmetry pool")):
        bad = dict(few, **{key: few[key].copy()})
        bad[key][3] = val
        with pytest.raises(ValueError, match=msg):
            _launch(bad, gpu_device)
    with pytest.raises(AssertionError, match="max_scnt"):
        _launch(few, gpu_device, max_scnt=16)
    d = _dev(few, gpu_device)
    with pytest.raises(AssertionError):
        ops.bop_errors(d["verts"], d["voff"], d["vcnt"], d["syms"], d["soff"], d["scnt"][:3], d["K"], d["Rg"], d["Tg"],
                       d["Rp"], d["Tp"])


def test_recalls_of_a_collection_equal_float64(gpu_device):
    """evaluate_bop_predictions on the device against the float64 restatement through errors_fn: 24 images, 3 classes
    (asymmetric, half turn, continuous), missing predictions, two image widths.  No float64 error of the collection lies
    within 1e-3 relative of a threshold (checked on the CPU too), so the tables must be equal."""
    from kd6d.libs import bop_metrics as B
    preds, meshes, diam, sets = C.recall_collection()
    objects, err64 = C.recall_collection_objects()
    assert C.near_threshold(err64, objects, diam) == []
    ref = B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, None, errors_fn=C.restate_errors_fn(np.float64))
    got = B.evaluate_bop_predictions(preds, 4, meshes, diam, sets, gpu_device)
    print("device:", json.dumps({k: got[k] for k in ("AR_MSSD", "AR_MSPD", "AR")}))
    assert json.dumps(got) == json.dumps(ref)


class _EncodedPoses(torch.nn.Module):
    """Stands in for the network in valid(): logits whose confident cells vote the projected box corners of the targets'
    poses with pixel noise (test_train_entry_gpu._encoded_pose_logits), handed to the REAL evaluation tail of the module
    -- pose candidates on the GPU, PnP-RANSAC on the device.  A random-weight network solves no pose at all."""

    def __init__(self, post_processor, batches):
        super().__init__()
        self.post_processor, self.batches, self.calls = post_processor, batches, 0

    def forward(self, images, targets=None):
        cls, reg, levels, B = self.batches[self.calls % len(self.batches)]
        self.calls += 1
        return self.post_processor(cls, reg, levels, B, targets), {}


def _synthetic_setup(dev):
    """The synthetic valid loader of train_kd.py / test.py, RUNTIME.PNP_SOLVER = device, and the stand-in model."""
    from kd6d import engine
    from kd6d.arguments.argument import get_args
    from kd6d.libs.train_libs import build_model_teacher
    from kd6d.models.model_kd import PoseModuleKD
    from kd6d.synthetic import make_batch
    from test_train_entry_gpu import _encoded_pose_logits
    from train_kd import synthetic_valid_loader
    cfg = get_args(["--config_file", os.path.join(ROOT, "configs", "ape.yaml"), "--backbone", "darknet_tiny_h",
                    "--synthetic", "--pnp_solver", "device", "--bop_metrics"])
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False)
    torch.manual_seed(0)
    real = build_model_teacher(cfg, PoseModuleKD, "cuda")
    assert real.pnp_solver == "device" and real.post_processor.solver == "device"
    loader, meshes = synthetic_valid_loader(cfg, "cuda")
    rng = np.random.default_rng(4)
    size, batches = cfg["RUNTIME"]["IMAGE_SIZE"], []
    levels = [(size // s, size // s) for s in engine.ANCHOR_STRIDES]
    for i, (images, _, metas) in enumerate(loader):
        B = len(metas)
        _, targets = make_batch(B, 900000 + i, crop=size)         # the loader's own seeds: the same targets
        assert all(np.array_equal(t.rotations[0].numpy(), m["rotations"][0]) for t, m in zip(targets, metas))
        cls, reg = _encoded_pose_logits(targets, levels, B, noise=rng.uniform(0.2, 3.0, B), rng=rng)
        batches.append((cls.to(dev), reg.to(dev), levels, B))
    return cfg, _EncodedPoses(real.post_processor, batches).to(dev), loader, meshes


def test_valid_with_bop_equals_the_host_scorer_and_changes_nothing_else(gpu_device):
    from kd6d.libs import bop_metrics as B
    from kd6d.libs.eval_libs import _Mesh, valid
    cfg, model, loader, meshes = _synthetic_setup(gpu_device)
    plain_preds, bop_preds, bop = {}, {}, {}
    plain = valid(cfg, 0, loader, model, gpu_device, meshes, scorer="device", preds_out=plain_preds)
    with_bop = valid(cfg, 0, loader, model, gpu_device, meshes, scorer="device", preds_out=bop_preds, bop=bop)

    def canon(x):
        if isinstance(x, dict):
            return {str(k): canon(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [canon(v) for v in x]
        return np.asarray(x).tolist() if isinstance(x, (np.ndarray, np.generic)) else x
    assert len(with_bop) == 6 and json.dumps(canon(with_bop)) == json.dumps(canon(plain))        # the 6-tuple
    assert json.dumps(canon(bop_preds)) == json.dumps(canon(plain_preds))                        # what preds.json holds
    every = bop.pop("predictions")
    assert sorted(every) == sorted(plain_preds) and len(every) == 32
    n_pred = sum(len(it["pred"]) for it in every.values())
    print("valid(bop): %d images, %d predictions kept, AR_MSSD %.4f AR_MSPD %.4f AR %.4f"
          % (len(every), n_pred, bop["AR_MSSD"], bop["AR_MSPD"], bop["AR"]))
    assert n_pred >= 16                                              # the encoded poses are solved (noise 0.2 ... 3 px)
    for name, it in every.items():
        assert it["meta"] is plain_preds[name]["meta"]
        assert all(len(q) == 4 for q in it["pred"])
        if plain_preds[name]["pred"]:
            assert float(it["pred"][0][0]) == float(plain_preds[name]["pred"][0][0])             # the best one is the first
    n_cls = cfg["DATASETS"]["N_CLASS"] - 1
    ms = [_Mesh(m) for m in meshes]
    sets = B.dataset_symmetry_sets(cfg["DATASETS"], n_cls)
    assert [len(s) for s in sets][9:11] == [8, 2]                    # configs/ape.yaml: cls_9 and cls_10
    seen = []

    def host(*arrays):
        err = B.bop_errors_host(*arrays)
        seen.append((arrays, err))
        return err
    ref = B.evaluate_bop_predictions(every, cfg["DATASETS"]["N_CLASS"], ms, cfg["DATASETS"]["MESH_DIAMETERS"], sets, None,
                                     errors_fn=host)
    if seen:
        (arrays, err), = seen
        cls_of = {int(o): c for c, o in enumerate(np.cumsum([0] + [len(m.vertices) for m in ms])[:-1])}
        objects = [(cls_of[int(o)], 1.0) for o in arrays[1]]
        near = C.near_threshold(err, objects, cfg["DATASETS"]["MESH_DIAMETERS"])
        print("float64 errors of the scored objects:", np.round(err, 3).tolist())
        assert near == [], "an object within 1e-3 relative of a threshold: %s" % near
    assert json.dumps(bop) == json.dumps(ref)
    assert bop["n_objects"] == 32 and "VSD" in bop["note"]


def test_eval_entry_writes_the_bop_block(gpu_device, tmp_path):
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    base = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(ROOT, "test.py"), "--config_file", ape,
            "--backbone", "darknet_tiny_h", "--synthetic", "--pnp_solver", "device", "--eval_scorer", "device"]
    out = {}
    for tag, extra in (("plain", []), ("bop", ["--bop_metrics"])):
        wd = str(tmp_path / tag)
        r = subprocess.run(base + ["--working_dir", wd] + extra, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30,
                           cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[tag] = (json.load(open(os.path.join(wd, "metrics.json"))), open(os.path.join(wd, "preds.json")).read(), r.stdout)
    metrics, preds, stdout = out["bop"]
    plain_metrics, plain_preds, plain_stdout = out["plain"]
    assert "bop" not in plain_metrics and "BOP AR_MSSD" not in plain_stdout
    assert preds == plain_preds                                     # preds.json is the same file
    assert {k: v for k, v in metrics.items() if k != "bop"} == plain_metrics
    bop = metrics["bop"]
    assert {"AR_MSSD", "AR_MSPD", "AR", "per_class", "mssd_thresholds", "mspd_thresholds", "n_objects", "note"} == set(bop)
    assert "predictions" not in bop and bop["n_objects"] == 32 and len(bop["per_class"]) == 15
    seen = [e for e in bop["per_class"] if e]
    assert seen and all(len(e["mssd_recall"]) == 10 and len(e["mspd_recall"]) == 10 for e in seen)
    assert bop["AR"] == pytest.approx(0.5 * (bop["AR_MSSD"] + bop["AR_MSPD"]))
    assert "BOP AR_MSSD" in stdout and "VSD term is not built" in stdout and "bop cls_" in stdout


def test_eval_entry_on_a_bop_tree_scores_and_writes_the_results_file(gpu_device, tmp_path):
    """test.py --bop_metrics --bop_csv on a small BOP tree (tests/frame_cache_cases.py: scene 000002, objects 1 and 5
    with meshes, 9 without) to which this test adds a models_info.json: the symmetry sets come from that file, every
    ground-truth object of the list is counted, the results file has the BOP header."""
    import frame_cache_cases as F
    from test_frame_cache_gpu import _yaml_for
    tree = F.write_cache_tree(str(tmp_path / "tree"))
    with open(os.path.join(tree["models"], "models_info.json"), "w") as f:
        json.dump({"1": {"diameter": 120.0}, "5": {"diameter": 80.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}, f)
    cfgp = _yaml_for(tree, str(tmp_path / "bop.yaml"))
    wd, csv = str(tmp_path / "eval"), str(tmp_path / "results.csv")
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(ROOT, "test.py"), "--config_file", cfgp,
           "--backbone", "darknet_tiny_h", "--pnp_solver", "device", "--num_workers", "0", "--working_dir", wd,
           "--bop_metrics", "--bop_csv", csv]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    bop = json.load(open(os.path.join(wd, "metrics.json")))["bop"]
    assert bop["n_objects"] == 5 and [e.get("n") for e in bop["per_class"][:3]] == [3, 2, None]   # images 2, 3, 4, 6
    lines = open(csv).read().splitlines()
    assert lines[0] == "scene_id,im_id,obj_id,score,R,t,time"
    for line in lines[1:]:
        f = line.split(",")
        assert len(f) == 7 and int(f[0]) == 2 and int(f[1]) in F.EVAL_IDS and int(f[2]) in (1, 5) and f[6] == "-1"
        assert len(f[4].split(" ")) == 9 and len(f[5].split(" ")) == 3
    assert "%d estimates written to %s" % (len(lines) - 1, csv) in r.stdout and "VSD term is not built" in r.stdout
