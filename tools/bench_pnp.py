"""Cost of PnP-RANSAC on the GPU (csrc/pnp.hip) against the host solver (kd6d/libs/pnp.py).  Run on the GPU box.

    python tools/bench_pnp.py [--reps 20] [--host_problems 8] [--out profiles/pnp_device]

Device figures are hip-event times of a captured graph holding `reps` back-to-back launches, replayed 5 times (the
figure is per launch, launch overhead amortised as in a replayed training step):
  * eval:  kd6d_pnp_ransac on 16 x MAX_GT = 64 problems of 32 cells each (1-px votes, 20 % 60-px outliers), iters 300;
  * gate:  kd6d_teacher_pnp_gate at B = 16 and B = 48 (the grouped teacher of --teacher_group 3), 10 cells per image
           (POSITIVE_NUM) and 32 cells per image, iters 300.
  * remap: kd6d_pose_remap (the two chained pose remaps of --augment, one lane per instance) at 16 and 64 instances,
           Resize from another camera, then shift-scale-rotate at the ape.yaml limits.
Host: wall time per problem of solve_pnp_ransac on the first `host_problems` eval problems (same inputs).
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
from kd6d._lib import MAX_GT  # noqa: E402
from kd6d.libs import pnp  # noqa: E402

CAP, ITERS = 32, 300
K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1.0]])


def box():
    h = 100.0 / np.sqrt(3) / 2 * np.array([1.0, 1.2, 0.8])
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def problems(P, cells, rng):
    kp = np.zeros((P, CAP, 8, 2), np.float32)
    for p in range(P):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.linalg.det(q)
        t = np.array([rng.normal(0, 60), rng.normal(0, 40), 900 + rng.normal(0, 80)])
        uv, _ = pnp.project(K, q, t, np.tile(box(), (cells, 1)))
        uv += rng.normal(0, 1.0, uv.shape)
        o = rng.random(len(uv)) < 0.2
        uv[o] += rng.normal(0, 60, (int(o.sum()), 2))
        kp[p, :cells] = uv.reshape(cells, 8, 2)
    return kp


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host_problems", type=int, default=8)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = {"iters": ITERS, "cap": CAP}
    # eval: 16 images x MAX_GT slots, full problems
    P = 16 * MAX_GT
    kp_h = problems(P, CAP, rng)
    kp = torch.from_numpy(kp_h.reshape(P * CAP, 8, 2)).to(dev)
    cnt = torch.full((P,), CAP, dtype=torch.int32, device=dev)
    boxes = torch.from_numpy(np.stack([box()] * P).astype(np.float32)).to(dev)
    Ks = torch.from_numpy(np.stack([K] * P).astype(np.float32)).to(dev)
    ws = ops.pnp_workspace(P, ITERS, dev)
    us = graph_time(lambda: ops.pnp_ransac(kp, cnt, boxes, Ks, 5.0, ITERS, 0, workspace=ws), a.reps)
    ok = ops.pnp_ransac(kp, cnt, boxes, Ks, 5.0, ITERS, 0, workspace=ws)[0]
    res["eval"] = {"problems": P, "cells": CAP, "us_per_launch": round(us, 1), "us_per_problem": round(us / P, 2),
                   "solved": int(ok.sum())}
    print("eval  %d problems x %d cells: %.1f us per launch (%.2f us per problem), %d solved"
          % (P, CAP, us, us / P, int(ok.sum())))
    # gate
    res["gate"] = []
    n_cls = 15
    for B in (16, 48):
        for cells in (10, 32):
            kp_g = torch.from_numpy(problems(B, cells, rng).reshape(B * CAP, 8, 2)).to(dev)
            t_cnt0 = torch.full((B,), cells, dtype=torch.int32, device=dev)
            t_cnt = t_cnt0.clone()
            t_row = torch.zeros(B * CAP, dtype=torch.int32, device=dev)
            cls = torch.full((1, 16), -8.0, device=dev)
            cls[0, 0] = 4.0
            kp3d = torch.from_numpy(np.stack([np.stack([box()] * n_cls)] * B).astype(np.float32)).to(dev)
            Kb = torch.from_numpy(np.stack([K] * B).astype(np.float32)).to(dev)
            wsg = ops.pnp_workspace(B, ITERS, dev)

            def gate():
                t_cnt.copy_(t_cnt0)
                ops.teacher_pnp_gate(cls, n_cls, 0.1, t_row, t_cnt, kp_g, CAP, kp3d, Kb, 5.0, ITERS, 0, workspace=wsg)
            us = graph_time(gate, a.reps)
            kept = int((t_cnt > 0).sum())
            res["gate"].append({"B": B, "cells": cells, "us_per_launch": round(us, 1),
                                "us_per_16_images": round(us * 16 / B, 1), "kept": kept})
            print("gate  B=%d, %d cells: %.1f us per launch (%.1f us per 16 images), %d/%d kept"
                  % (B, cells, us, us * 16 / B, kept, B))
    # pose remap of the augmentation chain: n_inst instances, one per image
    res["remap"] = []
    for n in (16, 64):
        src_K = K.copy(); src_K[0, 0] *= 0.9; src_K[1, 1] *= 0.9; src_K[0, 2] += 7.0; src_K[1, 2] -= 5.0
        Rs, Ts, Mr, Ms = [], [], [], []
        for _ in range(n):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            Rs.append(q * np.linalg.det(q))
            Ts.append([rng.normal(0, 60), rng.normal(0, 40), 900 + rng.normal(0, 80)])
            Mr.append((K @ np.linalg.inv(src_K))[:2])
            a_, sc = np.deg2rad(rng.uniform(-10, 10)), 1 + rng.uniform(-0.05, 0.05)
            al, be = np.cos(a_) * sc, np.sin(a_) * sc
            Ms.append([[al, be, (1 - al) * 320 - be * 240 + rng.uniform(-32, 32)],
                       [-be, al, be * 320 + (1 - al) * 240 + rng.uniform(-24, 24)]])
        f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)  # noqa: E731
        img = torch.arange(n, dtype=torch.int32, device=dev)
        cls0 = torch.zeros(n, dtype=torch.int32, device=dev)
        bx = torch.from_numpy(box()[None].astype(np.float32)).to(dev)
        args_ = (img, cls0, f64(np.stack([src_K] * n)), f64(Rs), f64(Ts), bx, K, f64(Mr), f64(Ms))
        pose_o = torch.empty(n, 2, 12, device=dev)
        ok_o = torch.empty(n, 2, dtype=torch.int32, device=dev)
        us = graph_time(lambda: ops.pose_remap(*args_, pose_out=pose_o, ok_out=ok_o), a.reps)
        torch.cuda.synchronize()
        res["remap"].append({"n_inst": n, "us_per_launch": round(us, 1), "solved": int(ok_o.sum())})
        print("remap %d instances: %.1f us per launch, %d/%d stages solved" % (n, us, int(ok_o.sum()), 2 * n))
    # host solver on the same eval problems
    n = min(a.host_problems, P)
    t0 = time.perf_counter()
    hok = 0
    for p in range(n):
        hok += int(pnp.solve_pnp_ransac(np.tile(box(), (CAP, 1)), kp_h[p].reshape(-1, 2).astype(np.float64), K)[0])
    dt = (time.perf_counter() - t0) / n
    res["host"] = {"problems": n, "ms_per_problem": round(dt * 1000.0, 1), "solved": hok}
    print("host  solve_pnp_ransac: %.1f ms per problem (%d problems, %d solved)" % (dt * 1000.0, n, hok))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
