"""Cost of scoring poses on the GPU (csrc/pose_err.hip) against the host scorer (kd6d/libs/evaluate.py).  Run on the
GPU box.

    python tools/bench_pose_err.py [--reps 10] [--frames 1000] [--out profiles/pose_err_device]

Device figures are hip-event times of a captured graph holding `reps` back-to-back launches, replayed 5 times (per
launch, launch overhead amortised):
  * asym:  kd6d_pose_errors on 2048 problems of 1000 vertices, vertex i against vertex i;
  * sym:   the same problems, every ground-truth vertex against its nearest predicted vertex;
  * mix:   a LINEMOD-13-shaped validation: `frames` frames x 13 classes (13 000 problems at the default), meshes of
           5000 vertices subsampled to 1000, 2 of the 13 classes symmetric.
On the mix's inputs, wall time of evaluate_pose_predictions_device (host orchestration + upload + launch + copy back)
and of the host evaluate_pose_predictions (float64 numpy, one object at a time, one process on the CPUs the box
gives).  Last, one whole valid() over the synthetic loader (darknet_tiny_h, --pnp_solver device) with
scorer = host and = device.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from kd6d import ops  # noqa: E402
from kd6d.libs import evaluate as E  # noqa: E402

K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])
N_CLS, SYM_CLS, MESH_V = 13, (9, 10), 5000


def rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.linalg.det(q)


def near(rng, R):
    w = rng.normal(0, 0.02, 3)
    u, _, vt = np.linalg.svd((np.eye(3) + np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])) @ R)
    return u @ vt


def graph_time(fn, reps):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / (5 * reps)


def device_problems(P, n_meshes, sym, rng, dev, draws):
    """P problems of 1000 vertices over n_meshes meshes of MESH_V vertices (draws) or 1000 vertices (no index table)."""
    nv = MESH_V if draws else 1000
    verts = torch.from_numpy(rng.normal(0, 40, (n_meshes * nv, 3)).astype(np.float32)).to(dev)
    cls = np.arange(P) % n_meshes
    Rg = np.stack([rot(rng) for _ in range(P)])
    Rp = np.stack([near(rng, R) for R in Rg])
    Tg = np.stack([[rng.normal(0, 60), rng.normal(0, 40), 700 + rng.uniform(0, 600)] for _ in range(P)])
    Tp = Tg + rng.normal(0, 4, (P, 3))
    t = lambda x, d: torch.from_numpy(np.ascontiguousarray(x, d)).to(dev)  # noqa: E731
    vidx = t(rng.integers(0, nv, (P, 1000)), np.int32) if draws else None
    symv = np.isin(cls, sym).astype(np.int32) if isinstance(sym, tuple) else np.full(P, sym, np.int32)
    return dict(verts=verts, voff=t(cls * nv, np.int32), vcnt=t(np.full(P, 1000), np.int32), vidx=vidx,
                K=t(np.stack([K] * P), np.float32), Rg=t(Rg, np.float32), Tg=t(Tg, np.float32), Rp=t(Rp, np.float32),
                Tp=t(Tp, np.float32), sym=t(symv, np.int32))


def time_kernel(a, reps):
    fn = lambda: ops.pose_errors(a["verts"], a["voff"], a["vcnt"], a["vidx"], a["K"], a["Rg"], a["Tg"], a["Rp"],  # noqa: E731
                                 a["Tp"], a["sym"], max_v=1000, validate=False)
    fn()                                          # indices were built inside the pool above
    return graph_time(fn, reps)


class Mesh:
    def __init__(self, v):
        self.vertices = v


def mix_predictions(frames, rng):
    meshes = [Mesh(rng.normal(0, 40, (MESH_V, 3))) for _ in range(N_CLS)]
    diam = [float(np.linalg.norm(m.vertices.max(0) - m.vertices.min(0))) for m in meshes]
    preds = {}
    for i in range(frames):
        Rs = [rot(rng) for _ in range(N_CLS)]
        Ts = [np.array([[rng.normal(0, 60)], [rng.normal(0, 40)], [700 + rng.uniform(0, 600)]]) for _ in range(N_CLS)]
        preds["f%05d" % i] = {"meta": {"K": K, "class_ids": list(range(N_CLS)), "rotations": Rs, "translations": Ts},
                              "pred": [[0.9, c, near(rng, Rs[c]), Ts[c] + rng.normal(0, 4, (3, 1))] for c in range(N_CLS)]}
    return meshes, diam, preds, {"cls_%d" % c: ["Z", 180] for c in SYM_CLS}


def time_valid(dev):
    from kd6d.arguments.argument import get_args
    from kd6d.libs.eval_libs import valid
    from kd6d.libs.train_libs import build_model_teacher
    from kd6d.models.model_kd import PoseModuleKD
    from train_kd import synthetic_valid_loader
    cfg = get_args(["--config_file", os.path.join(HERE, "configs", "ape.yaml"), "--backbone", "darknet_tiny_h",
                    "--synthetic", "--pnp_solver", "device"])
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False)
    torch.manual_seed(0)
    model = build_model_teacher(cfg, PoseModuleKD, "cuda")
    loader, meshes = synthetic_valid_loader(cfg, "cuda")
    out = {"images": sum(len(m) for _, _, m in loader)}
    for scorer in ("host", "device"):
        valid(cfg, 0, loader, model, dev, meshes, scorer=scorer)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        valid(cfg, 0, loader, model, dev, meshes, scorer=scorer)
        torch.cuda.synchronize()
        out["ms_" + scorer] = round((time.perf_counter() - t0) * 1000.0, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = {"vertices": 1000}
    P = 2048
    for name, sym in (("asym", 0), ("sym", 1)):
        us = time_kernel(device_problems(P, 1, sym, rng, dev, draws=False), a.reps)
        res[name] = {"problems": P, "us_per_launch": round(us, 1), "us_per_problem": round(us / P, 3)}
        print("%-5s %d problems x 1000 vertices: %.1f us per launch (%.3f us per problem)" % (name, P, us, us / P))
    Pm = a.frames * N_CLS
    us = time_kernel(device_problems(Pm, N_CLS, SYM_CLS, rng, dev, draws=True), a.reps)
    res["mix"] = {"problems": Pm, "symmetric_classes": len(SYM_CLS), "classes": N_CLS, "us_per_launch": round(us, 1),
                  "us_per_problem": round(us / Pm, 3)}
    print("mix   %d problems (%d of %d classes symmetric): %.1f us per launch (%.3f us per problem)"
          % (Pm, len(SYM_CLS), N_CLS, us, us / Pm))
    meshes, diam, preds, symt = mix_predictions(a.frames, rng)
    np.random.seed(3)
    E.evaluate_pose_predictions_device(preds, N_CLS + 1, meshes, diam, symt, dev)      # warm: pool upload, allocator
    np.random.seed(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = E.evaluate_pose_predictions_device(preds, N_CLS + 1, meshes, diam, symt, dev)
    t_dev = time.perf_counter() - t0
    np.random.seed(3)
    t0 = time.perf_counter()
    h = E.evaluate_pose_predictions(preds, N_CLS + 1, meshes, diam, symt)
    t_host = time.perf_counter() - t0
    worst = max(abs(d[1][c]["AUC    "] - h[1][c]["AUC    "]) for c in range(N_CLS))
    res["evaluate"] = {"problems": Pm, "device_ms": round(t_dev * 1000.0, 1),
                       "host_ms": round(t_host * 1000.0, 1), "host_over_device": round(t_host / t_dev, 1),
                       "host_over_kernel": round(t_host * 1e6 / us, 1), "worst_auc_difference": worst}
    print("evaluate_pose_predictions on %d objects: device %.1f ms (kernel %.2f ms of it), host %.1f ms -> %.1fx "
          "(%.0fx against the kernel alone); worst AUC difference %.3g"
          % (Pm, t_dev * 1000.0, us / 1000.0, t_host * 1000.0, t_host / t_dev, t_host * 1e6 / us, worst))
    res["valid"] = time_valid(dev)
    print("valid() over the synthetic loader (%d images, darknet_tiny_h, pnp_solver device): scorer host %.2f ms, "
          "scorer device %.2f ms" % (res["valid"]["images"], res["valid"]["ms_host"], res["valid"]["ms_device"]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
