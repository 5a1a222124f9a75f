"""Cost of BOP's VSD on the GPU (csrc/bop_vsd.hip) against the float64 host scorer
(kd6d/libs/bop_metrics.py::vsd_errors_host).  Run on the GPU box.

    python tools/bench_bop_vsd.py [--reps 10] [--frames 256] [--host_problems 4] [--out profiles/bop_vsd_device]

Device figures are hip-event times of a captured graph holding `reps` back-to-back calls, replayed 5 times (per call,
launch overhead amortised), on LINEMOD-shaped problems: 640 x 480 images, K of LINEMOD, meshes of 5120 faces (a bumpy
ball of ~45 mm radius: a subdivided icosahedron), z = 700 ... 1300 mm, pose errors of a few degrees and millimetres:
  * render:  256 depth maps in one kd6d_render_depth call;
  * vsd:     1024 problems against 79 frames (13 objects per frame) in one kd6d_bop_vsd call;
  * mix:     a LINEMOD-13-shaped chunk of a validation: `frames` frames x 13 classes in one call (evaluate_bop_vsd scores
             a run in such chunks, max_images_per_call frames each, so that the depth pool stays bounded).
A frame's depth image is the nearest ground-truth surface of its 13 objects (ops.render_depth), as --synthetic builds it.
The host column is the wall time of vsd_errors_host on the first `host_problems` problems of the mix, scaled to all of
them (the scorer is a loop over problems, its time is linear in them); the counts of device and host on those problems
are compared too.
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
sys.path.insert(0, os.path.join(HERE, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_pose_err import K, N_CLS, graph_time, near, rot  # noqa: E402
from bop_vsd_cases import icosphere  # noqa: E402
from kd6d import ops  # noqa: E402
from kd6d.libs.bop_metrics import VSD_DELTA, VSD_TAUS, vsd_errors_host  # noqa: E402

H, W = 480, 640
ORDER = ("verts", "faces", "voff", "vcnt", "foff", "fcnt", "K", "Rg", "Tg", "Rp", "Tp", "diameter", "frame", "depth")


def meshes(n, rng):
    v, f = icosphere(4)
    out = []
    for _ in range(n):
        a, b = rng.uniform(2, 4, 2)
        out.append(v * (45.0 + 5.0 * np.sin(a * v[:, :1]) * np.cos(b * v[:, 1:2])) * rng.uniform(0.7, 1.2, (1, 3)))
    return out, f


def t(x, dev):
    x = np.asarray(x)
    return torch.from_numpy(np.ascontiguousarray(x, np.float32 if x.dtype == np.float64 else x.dtype)).to(dev)


def problems(frames, rng, dev):
    """frames x N_CLS problems, frame-major, and the frames' depth images (device)."""
    ms, f = meshes(N_CLS, rng)
    nv, nf = len(ms[0]), len(f)
    P = frames * N_CLS
    cls = np.arange(P) % N_CLS
    Rg = np.stack([rot(rng) for _ in range(P)])
    Tg = np.stack([[rng.normal(0, 120), rng.normal(0, 90), 700 + rng.uniform(0, 600)] for _ in range(P)])
    a = dict(verts=np.concatenate(ms), faces=np.concatenate([f] * N_CLS).astype(np.int32),
             voff=(cls * nv).astype(np.int32), vcnt=np.full(P, nv, np.int32), foff=(cls * nf).astype(np.int32),
             fcnt=np.full(P, nf, np.int32), K=np.stack([K] * P), Rg=Rg, Tg=Tg, Rp=np.stack([near(rng, R) for R in Rg]),
             Tp=Tg + rng.normal(0, 4, (P, 3)),
             diameter=np.asarray([2 * np.linalg.norm(ms[c], axis=1).max() for c in cls]),
             frame=(np.arange(P) // N_CLS).astype(np.int32))
    d = {k: t(a[k], dev) for k in ORDER if k != "depth"}
    depth = torch.empty(frames, H, W, dtype=torch.float32, device=dev)
    for i in range(frames):                                             # the nearest gt surface of the frame's objects
        s = slice(i * N_CLS, (i + 1) * N_CLS)
        maps = ops.render_depth(d["verts"], d["faces"], d["voff"][s], d["vcnt"][s], d["foff"][s], d["fcnt"][s], d["K"][s],
                                d["Rg"][s], d["Tg"][s], H, W, validate=(i == 0))
        far = torch.where(maps > 0, maps, torch.full_like(maps, float("inf"))).amin(dim=0)
        depth[i] = torch.where(torch.isinf(far), torch.zeros_like(far), far)
    d["depth"] = depth
    a["depth"] = depth
    return a, d, nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--host_problems", type=int, default=4)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    mix, d, nf = problems(a.frames, rng, dev)
    Pm = a.frames * N_CLS
    res = {"image": [W, H], "faces": nf}

    n = 256
    fn = lambda: ops.render_depth(d["verts"], d["faces"], d["voff"][:n], d["vcnt"][:n], d["foff"][:n], d["fcnt"][:n],  # noqa: E731
                                  d["K"][:n], d["Rg"][:n], d["Tg"][:n], H, W, validate=False)
    covered = float((fn() > 0).sum()) / n
    us = graph_time(fn, a.reps)
    res["render"] = {"maps": n, "us_per_call": round(us, 1), "us_per_map": round(us / n, 3), "covered_pixels_per_map": covered}
    print("render %d maps of %d faces, %.0f covered pixels each: %.1f us per call (%.3f us per map)" % (n, nf, covered, us, us / n))

    def vsd(P):
        args = [d[k][:P] if k not in ("verts", "faces", "depth") else d[k] for k in ORDER]
        return lambda: ops.bop_vsd(*args, VSD_DELTA, VSD_TAUS, validate=False)
    ops.bop_vsd(*[d[k] for k in ORDER], VSD_DELTA, VSD_TAUS)            # once with the check
    for name, P in (("vsd", min(1024, Pm)), ("mix", Pm)):
        us = graph_time(vsd(P), a.reps)
        res[name] = {"problems": P, "us_per_call": round(us, 1), "us_per_problem": round(us / P, 3)}
        print("%-6s %d problems: %.1f us per call (%.3f us per problem)" % (name, P, us, us / P))

    n = min(a.host_problems, Pm)
    sub = {k: (mix[k][:n] if k not in ("verts", "faces", "depth") else mix[k]) for k in ORDER}
    sub["depth"] = mix["depth"][:(n + N_CLS - 1) // N_CLS].cpu().numpy()
    t0 = time.perf_counter()
    hc, he = vsd_errors_host(*[sub[k] for k in ORDER], VSD_DELTA, VSD_TAUS)
    t_host = (time.perf_counter() - t0) * Pm / n
    counts, err = vsd(n)()
    diff = np.abs(counts.cpu().numpy().astype(np.int64) - hc)
    us = res["mix"]["us_per_call"]
    res["host"] = {"measured_problems": n, "host_s_scaled_to_mix": round(t_host, 1), "host_over_kernel": round(t_host * 1e6 / us, 1),
                   "n_u": hc[:, 0].tolist(), "worst_count_difference": int(diff.max()),
                   "worst_err_difference": float(np.abs(err.cpu().numpy() - he).max())}
    print("vsd_errors_host on the mix: %.1f s (measured on %d problems, scaled to %d) -> %.0fx the device call; n_u %s, worst "
          "count difference %d, worst |err difference| %.3g" % (t_host, n, Pm, t_host * 1e6 / us, hc[:, 0].tolist(),
                                                                 int(diff.max()), res["host"]["worst_err_difference"]))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
