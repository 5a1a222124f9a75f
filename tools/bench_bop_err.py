"""Cost of BOP's MSSD / MSPD on the GPU (csrc/bop_err.hip) against the float64 host scorer
(kd6d/libs/bop_metrics.py::bop_errors_host).  Run on the GPU box.

    python tools/bench_bop_err.py [--reps 10] [--frames 1000] [--host_frames 20] [--out profiles/bop_err_device]

Device figures are hip-event times of a captured graph holding `reps` back-to-back kd6d_bop_errors calls (two launches
each), replayed 5 times (per call, launch overhead amortised), meshes of 5000 vertices, ALL of them scored:
  * asym:  2048 problems, the identity alone;
  * cont:  2048 problems, one continuous symmetry (315 transforms each);
  * mix:   a LINEMOD-13-shaped validation: `frames` frames x 13 classes (13 000 problems at the default), 2 of the 13
           classes symmetric (one half turn, one continuous symmetry).
The host column is the wall time of bop_errors_host on the mix's inputs; it is measured on the problems of the first
`host_frames` frames and scaled to all of them (the scorer is a loop over objects, its time is linear in them).  The
deviation of the device errors from the host's on those problems is reported too.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))
sys.path.insert(0, os.path.join(HERE, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_pose_err import K, MESH_V, N_CLS, graph_time, near, rot  # noqa: E402
from kd6d import ops  # noqa: E402
from kd6d.libs.bop_metrics import bop_errors_host, pack_symmetries, symmetry_set  # noqa: E402

SYM_TYPES = {"cls_9": ["Z", 180], "cls_10": ["Z", 0]}


def problems(P, n_meshes, sets, rng):
    """P problems in class order over n_meshes meshes of MESH_V vertices; sets: per mesh an (S, 3, 4) array.  numpy."""
    cls = np.arange(P) % n_meshes
    s_offs = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    Rg = np.stack([rot(rng) for _ in range(P)])
    Tg = np.stack([[rng.normal(0, 60), rng.normal(0, 40), 700 + rng.uniform(0, 600)] for _ in range(P)])
    return dict(verts=rng.normal(0, 40, (n_meshes * MESH_V, 3)), voff=(cls * MESH_V).astype(np.int32),
                vcnt=np.full(P, MESH_V, np.int32), syms=pack_symmetries(np.concatenate(sets)),
                soff=s_offs[cls].astype(np.int32), scnt=np.asarray([len(sets[c]) for c in cls], np.int32),
                K=np.stack([K] * P), Rg=Rg, Tg=Tg, Rp=np.stack([near(rng, R) for R in Rg]), Tp=Tg + rng.normal(0, 4, (P, 3)))


ORDER = ("verts", "voff", "vcnt", "syms", "soff", "scnt", "K", "Rg", "Tg", "Rp", "Tp")


def upload(a, dev):
    return [torch.from_numpy(np.ascontiguousarray(a[k], np.float32 if a[k].dtype == np.float64 else a[k].dtype)).to(dev)
            for k in ORDER]


def time_kernel(a, dev, reps):
    d = upload(a, dev)
    m = int(a["scnt"].max())
    fn = lambda: ops.bop_errors(*d, validate=False, max_scnt=m)  # noqa: E731  (indices were built inside the pools above)
    ops.bop_errors(*d)                                           # once with the check
    return graph_time(fn, reps), fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--host_frames", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = {"vertices": MESH_V}
    P = 2048
    for name, spec in (("asym", []), ("cont", ["Z", 0])):
        S = symmetry_set(0, {"cls_0": spec})
        us, _ = time_kernel(problems(P, 1, [S], rng), dev, a.reps)
        pairs = P * MESH_V * len(S)
        res[name] = {"problems": P, "symmetries": len(S), "us_per_call": round(us, 1), "us_per_problem": round(us / P, 3),
                     "vertex_symmetry_pairs_per_s": pairs / (us * 1e-6)}
        print("%-5s %d problems x %d vertices x %d symmetries: %.1f us per call (%.3f us per problem, %.3g pairs/s)"
              % (name, P, MESH_V, len(S), us, us / P, pairs / (us * 1e-6)))
    sets = [symmetry_set(c, SYM_TYPES) for c in range(N_CLS)]
    Pm = a.frames * N_CLS
    mix = problems(Pm, N_CLS, sets, rng)
    us, fn = time_kernel(mix, dev, a.reps)
    res["mix"] = {"problems": Pm, "classes": N_CLS, "symmetric_classes": 2, "us_per_call": round(us, 1),
                  "us_per_problem": round(us / Pm, 3)}
    print("mix   %d problems (cls_9 half turn, cls_10 continuous): %.1f us per call (%.3f us per problem)" % (Pm, us, us / Pm))
    n = min(a.host_frames, a.frames) * N_CLS
    sub = dict(mix, **{k: mix[k][:n] for k in ORDER if k not in ("verts", "syms")})
    t0 = time.perf_counter()
    host = bop_errors_host(**sub)
    t_host = (time.perf_counter() - t0) * Pm / n
    got = fn()[:n].cpu().numpy().astype(np.float64)
    dev_abs = np.abs(got - host).max(axis=0)
    res["host"] = {"measured_problems": n, "host_ms_scaled_to_mix": round(t_host * 1000.0, 1),
                   "host_over_kernel": round(t_host * 1e6 / us, 1),
                   "worst_abs_difference": {"mssd": float(dev_abs[0]), "mspd": float(dev_abs[1])}}
    print("bop_errors_host on the mix: %.1f ms (measured on %d problems, scaled to %d) -> %.0fx the device call; worst "
          "|device - host| mssd %.3g mm, mspd %.3g px" % (t_host * 1000.0, n, Pm, t_host * 1e6 / us, dev_abs[0], dev_abs[1]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
