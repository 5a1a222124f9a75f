"""GPU: kd6d_render_depth and kd6d_bop_vsd (csrc/bop_vsd.hip) against the float64 restatement of tests/bop_vsd_cases.py
-- coverage exactly and depth within eps_d outside the reference's own ambiguous pixels, counts within the reference's own
b[p] -- against the closed-form table (exactly), their bitwise properties (two launches, batch, order, face order,
duplicated faces), their edges, and end to end through valid(..., bop={}, vsd=...) and test.py --bop_metrics --bop_vsd.
Tolerances: 4 x the float32 restatement's own deviation (bop_vsd_cases.tolerances(), profiles/bop_vsd_device.md)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bop_vsd_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600


def _t(x, dev):
    x = np.asarray(x)
    return torch.from_numpy(np.ascontiguousarray(x, np.float32 if x.dtype == np.float64 else x.dtype)).to(dev)


def _vsd(case, dev, **kw):
    from kd6d import ops
    d = {k: _t(case[k], dev) for k in C.ARG_ORDER}
    counts, err = ops.bop_vsd(*[d[k] for k in C.ARG_ORDER], C.DELTA, C.TAUS, **kw)
    return counts.cpu().numpy(), err.cpu().numpy()


def _render(mesh_list, items, H, W, dev, **kw):
    """items: (mesh index, K, R, T) -> (n, H, W) numpy."""
    from kd6d import ops
    voffs = np.concatenate([[0], np.cumsum([len(m.vertices) for m in mesh_list])])
    foffs = np.concatenate([[0], np.cumsum([len(m.faces) for m in mesh_list])])
    i32 = lambda v: _t(np.asarray(v, np.int32), dev)  # noqa: E731
    stack = lambda xs, shape: np.stack(xs) if xs else np.zeros((0,) + shape)  # noqa: E731
    out = ops.render_depth(_t(np.concatenate([m.vertices for m in mesh_list]), dev),
                           _t(np.concatenate([m.faces for m in mesh_list]), dev),
                           i32([voffs[i] for i, *_ in items]), i32([len(mesh_list[i].vertices) for i, *_ in items]),
                           i32([foffs[i] for i, *_ in items]), i32([len(mesh_list[i].faces) for i, *_ in items]),
                           _t(stack([K for _, K, _, _ in items], (3, 3)), dev),
                           _t(stack([R for _, _, R, _ in items], (3, 3)), dev),
                           _t(stack([np.asarray(T, np.float64) for _, _, _, T in items], (3,)), dev), H, W, **kw)
    return out.cpu().numpy()


def test_render_depth_against_float64(gpu_device):
    tol = C.tolerances()
    ms = C.meshes()
    for (name, mi, K, R, T, H, W), (ref, amb) in zip(C.render_cases(), C.render_references()):
        got = _render(ms, [(mi, K, R, T)], H, W, gpu_device)[0].astype(np.float64)
        sure = ~amb
        n_cov = int((ref > 0).sum())
        wrong = int(((got > 0) != (ref > 0))[sure].sum())
        both = sure & (ref > 0) & (got > 0)
        worst = float(np.abs(got - ref)[both].max()) if both.any() else 0.0
        print("%-42s covered %5d ambiguous %3d coverage mismatches %d worst depth deviation %.3e mm (eps_d %.3e)"
              % (name, n_cov, int(amb.sum()), wrong, worst, tol["eps_d"]))
        assert amb.sum() <= 0.01 * max(n_cov, 1)
        assert wrong == 0, name
        assert worst <= tol["eps_d"], name
        assert (got[ref == 0][sure[ref == 0]] == 0).all()


def test_render_depth_batch_is_bitwise_the_single_renders(gpu_device):
    ms = C.meshes()
    same = [(mi, K, R, T) for _, mi, K, R, T, H, W in C.render_cases() if (H, W) == (97, 130)]
    assert len(same) >= 3
    batch = _render(ms, same, 97, 130, gpu_device)
    again = _render(ms, same[::-1], 97, 130, gpu_device)[::-1]
    assert np.array_equal(batch, again)
    for i, item in enumerate(same):
        assert np.array_equal(batch[i], _render(ms, [item], 97, 130, gpu_device)[0])


def test_mixed_launch_counts_against_float64(gpu_device):
    case = C.mixed_call()
    ref_counts, ref_err, b = C.mixed_reference()
    counts, err = _vsd(case, gpu_device)
    assert counts.shape == ref_counts.shape and counts.dtype == np.int32 and err.shape == ref_err.shape
    diff = np.abs(counts.astype(np.int64) - ref_counts)
    for p in range(len(b)):
        print("problem %2d: n_u %5d n_inter %5d  worst count difference %d (b %d, %.2f %% of n_u)"
              % (p, ref_counts[p, 0], ref_counts[p, 1], diff[p].max(), b[p], 100.0 * b[p] / max(ref_counts[p, 0], 1)))
    assert (b <= 0.02 * np.maximum(ref_counts[:, 0], 1)).all()
    assert (diff <= b[:, None]).all()
    # err is one division of the kernel's own integers
    want = np.where(counts[:, :1] > 0, counts[:, 2:].astype(np.float32) / np.maximum(counts[:, :1], 1).astype(np.float32),
                    np.float32(1))
    assert np.array_equal(err, want.astype(np.float32))


def test_closed_forms_are_exact_on_the_device(gpu_device):
    case, rows = C.closed_form_call()
    counts, err = _vsd(case, gpu_device)
    for p, r in enumerate(rows):
        exact = np.asarray([np.float32(a) / np.float32(c) for a, c in r["err"]], np.float32)
        print("%-60s n_u %3d n_inter %3d err %s" % (r["name"], counts[p, 0], counts[p, 1], err[p].tolist()))
        assert (counts[p, 0], counts[p, 1]) == (r["n_u"], r["n_inter"]), r["name"]
        if r["n_u"]:
            assert [int(c) * d for c, (a, d) in zip(counts[p, 2:], r["err"])] == [a * r["n_u"] for a, d in r["err"]], r["name"]
        assert np.array_equal(err[p], exact), r["name"]


def test_bitwise_properties(gpu_device):
    case = C.mixed_call()
    P = len(case["voff"])
    counts, err = _vsd(case, gpu_device)
    c2, e2 = _vsd(case, gpu_device)
    assert np.array_equal(counts, c2) and np.array_equal(err, e2)                       # two launches
    rev = np.arange(P)[::-1].copy()
    cr, er = _vsd(C.subset(case, rev), gpu_device)
    assert np.array_equal(cr[::-1], counts) and np.array_equal(er[::-1], err)           # a reversed batch
    for p in (0, 3, 13, 27):
        c1, e1 = _vsd(C.subset(case, np.asarray([p])), gpu_device)
        assert np.array_equal(c1[0], counts[p]) and np.array_equal(e1[0], err[p])       # alone
    # shuffled and duplicated faces: a second face pool holding every mesh's faces permuted, with 37 of them repeated
    rng = np.random.default_rng(5)
    ms = C.meshes()
    foffs = np.concatenate([[0], np.cumsum([len(m.faces) for m in ms])])
    pools, offs, cnts = [], [], []
    for m in ms:
        f = m.faces[rng.permutation(len(m.faces))]
        f = np.concatenate([f, f[rng.integers(0, len(f), 37)]])
        f = f[rng.permutation(len(f))]
        offs.append(sum(len(q) for q in pools)); cnts.append(len(f)); pools.append(f)
    mesh_of = {int(o): i for i, o in enumerate(foffs[:-1])}
    shuf = dict(case)
    shuf["faces"] = np.concatenate(pools)
    shuf["foff"] = np.asarray([offs[mesh_of[int(o)]] for o in case["foff"]], np.int32)
    shuf["fcnt"] = np.asarray([cnts[mesh_of[int(o)]] for o in case["foff"]], np.int32)
    cs, es = _vsd(shuf, gpu_device)
    assert np.array_equal(cs, counts) and np.array_equal(es, err)


def test_edges_and_wrapper_refusals(gpu_device):
    from kd6d import ops
    case = C.mixed_call()
    # n_problems == 0
    c0, e0 = _vsd(C.subset(case, np.zeros(0, np.int64)), gpu_device)
    assert c0.shape == (0, 12) and e0.shape == (0, 10)
    assert _render(C.meshes(), [], 48, 64, gpu_device).shape == (0, 48, 64)
    # a mesh with one triangle, and an estimate entirely outside the image
    tri = C.Mesh([[-20.0, -10, 0], [25.0, -5, 0], [0.0, 30, 0]], [[0, 1, 2]])
    H, W = C.PLATE_HW
    Tg = np.array([0.0, 0, 1000.0])
    gt = C.restate_render(tri, C.K_PLATE, np.eye(3), Tg, H, W)
    n = int((gt > 0).sum())
    assert n > 50
    probs = [dict(mesh=0, K=C.K_PLATE, Rg=np.eye(3), Tg=Tg, Rp=np.eye(3), Tp=Tg, diameter=50.0, frame=0),
             dict(mesh=0, K=C.K_PLATE, Rg=np.eye(3), Tg=Tg, Rp=np.eye(3), Tp=Tg + [900.0, 0, 0], diameter=50.0, frame=0)]
    small = C.pack([tri], probs, gt[None])
    counts, err = _vsd(small, gpu_device)
    assert counts[0].tolist() == [n, n] + [0] * 10 and (err[0] == 0).all()
    assert counts[1].tolist() == [n, 0] + [n] * 10 and (err[1] == 1).all()
    got = _render([tri], [(0, C.K_PLATE, np.eye(3), Tg)], H, W, gpu_device)[0]
    assert np.array_equal(got > 0, gt > 0) and np.abs(got[gt > 0] - 1000.0).max() <= C.tolerances()["eps_d"]
    # validate=True: a face index outside the vertex pool, a frame index outside the depth pool -- nothing is launched
    bad_face = dict(small)
    bad_face["faces"] = np.asarray([[0, 1, 3]], np.int32)
    with pytest.raises(ValueError, match="face index"):
        _vsd(bad_face, gpu_device)
    bad_frame = dict(small)
    bad_frame["frame"] = np.asarray([0, 1], np.int32)
    with pytest.raises(ValueError, match="depth pool"):
        _vsd(bad_frame, gpu_device)
    bad_off = dict(small)
    bad_off["voff"] = np.asarray([0, 2], np.int32)
    with pytest.raises(ValueError, match="outside the pools"):
        _vsd(bad_off, gpu_device)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        ops.bop_vsd(*[_t(small[k], gpu_device) for k in C.ARG_ORDER], C.DELTA, [0.1] * 17)


def test_evaluate_bop_vsd_on_the_device_equals_the_host_walk(gpu_device):
    from kd6d.libs import bop_metrics as B
    preds, ms, diam, depths = C.eval_collection()
    fn = lambda meta: depths[meta["path"]]  # noqa: E731
    dev = B.evaluate_bop_vsd(preds, 4, ms, diam, fn, gpu_device, max_images_per_call=4)
    host = B.evaluate_bop_vsd(preds, 4, ms, diam, fn, None, errors_fn=B.vsd_errors_host)
    print("AR_VSD device %.4f host %.4f" % (dev["AR_VSD"], host["AR_VSD"]))
    assert dev["AR_VSD"] == host["AR_VSD"] == 1.0 and json.dumps(dev) == json.dumps(host)


def test_a_bop_tree_through_the_loader_scores_one_on_the_device(gpu_device, tmp_path):
    """The real-data path of --bop_vsd below valid(): build_test_dataset's metas, vsd_setup's meshes (PLY faces) and depth
    provider (load_depth_mm), evaluate_bop_vsd on the device -- predictions = ground truth score AR_VSD = 1."""
    import frame_cache_cases as F
    from kd6d.arguments.argument import get_args
    from kd6d.libs import bop_metrics as B
    from kd6d.libs.train_libs import build_test_dataset, dataset_meshes, vsd_setup
    from test_frame_cache_gpu import _yaml_for
    tree = F.write_cache_tree(str(tmp_path / "tree"))
    C.add_faces_and_depth(tree, F.EVAL_IDS)
    cfg = get_args(["--config_file", _yaml_for(tree, str(tmp_path / "vsd.yaml")), "--backbone", "darknet_tiny_h",
                    "--num_workers", "0", "--bop_metrics", "--bop_vsd"])
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False)
    loader = build_test_dataset(cfg, "cuda")
    ms, depth_fn = vsd_setup(cfg, loader, dataset_meshes(loader), gpu_device)
    assert [len(m.faces) for m in ms] == [12, 320]
    metas = [m for _, _, batch in loader for m in batch]
    assert len(metas) == len(F.EVAL_IDS)
    dev = B.evaluate_bop_vsd(C.gt_predictions(metas), 3, ms, [40.0, 35.0], depth_fn, gpu_device)
    host = B.evaluate_bop_vsd(C.gt_predictions(metas), 3, ms, [40.0, 35.0], depth_fn, None, errors_fn=B.vsd_errors_host)
    assert [e["n"] for e in dev["per_class"]] == [3, 2] and dev["AR_VSD"] == 1.0 and json.dumps(dev) == json.dumps(host)


def test_valid_with_vsd_adds_the_three_term_keys(gpu_device):
    from kd6d.libs.eval_libs import valid
    from kd6d.libs.train_libs import vsd_setup
    from test_bop_metrics_gpu import _synthetic_setup
    cfg, model, loader, meshes = _synthetic_setup(gpu_device)
    plain, bop = {}, {}
    valid(cfg, 0, loader, model, gpu_device, meshes, scorer="device", bop=plain)
    ms, depth_fn = vsd_setup(cfg, loader, meshes, gpu_device)
    valid(cfg, 0, loader, model, gpu_device, ms, scorer="device", bop=bop, vsd=depth_fn)
    plain.pop("predictions"); bop.pop("predictions")
    new = {"vsd_thresholds", "AR_VSD", "AR_BOP", "AR_BOP_note"}
    assert set(bop) == set(plain) | new and not (set(plain) & new)
    for k in plain:
        if k != "per_class":
            assert json.dumps(bop[k]) == json.dumps(plain[k]), k
    for a, b in zip(plain["per_class"], bop["per_class"]):
        assert {k: v for k, v in b.items() if k != "AR_VSD"} == a and (not a or 0.0 <= b["AR_VSD"] <= 1.0)
    print("valid(vsd): AR_VSD %.4f AR_MSSD %.4f AR_MSPD %.4f AR_BOP %.4f" % (bop["AR_VSD"], bop["AR_MSSD"], bop["AR_MSPD"],
                                                                               bop["AR_BOP"]))
    assert 0.0 <= bop["AR_VSD"] <= 1.0
    assert bop["AR_BOP"] == pytest.approx((bop["AR_VSD"] + bop["AR_MSSD"] + bop["AR_MSPD"]) / 3.0)
    assert "three terms" in bop["AR_BOP_note"] and "restatement" in bop["AR_BOP_note"] and "two terms" in bop["note"]
    with pytest.raises(ValueError, match="vsd needs bop"):
        valid(cfg, 0, loader, model, gpu_device, ms, scorer="device", vsd=depth_fn)


def test_eval_entry_prints_the_three_term_line(gpu_device, tmp_path):
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    wd = str(tmp_path / "vsd")
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(ROOT, "test.py"), "--config_file", ape,
           "--backbone", "darknet_tiny_h", "--synthetic", "--pnp_solver", "device", "--eval_scorer", "device",
           "--bop_metrics", "--bop_vsd", "--working_dir", wd]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    bop = json.load(open(os.path.join(wd, "metrics.json")))["bop"]
    assert 0.0 <= bop["AR_VSD"] <= 1.0 and bop["AR_BOP"] == pytest.approx((bop["AR_VSD"] + bop["AR_MSSD"] + bop["AR_MSPD"]) / 3)
    assert bop["AR"] == pytest.approx(0.5 * (bop["AR_MSSD"] + bop["AR_MSPD"])) and "predictions" not in bop
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOP AR_VSD")]
    assert len(line) == 1 and "AR_MSSD" in line[0] and "AR_MSPD" in line[0] and "AR_BOP" in line[0]
    assert "BOP AR_MSSD" not in r.stdout                            # the three-term line replaces the two-term one
