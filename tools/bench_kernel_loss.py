"""Kernel distances (csrc/kernel_loss.hip) per launch, 1 MI355X.

1. The KD step's launch: kd6d_kernel_div_fwd_bwd (gaussian / laplacian / energy) against kd6d_sinkhorn_div_fwd_bwd on the
   same B = 16 step inputs -- 16 images, about ten student positives and ten teacher cells each, eight keypoints, in the
   step's slot layout -- at the reference's settings (p 2, blur 0.001, scaling 0.5, reach 0.5).
2. The dense launch: kd6d_kernel_dense_fwd_bwd at 16384 x 16384 points, D = 16 (BASELINE config 5's size) and at
   2048 x 2048, priced against the fp32 vector peak: per (row, column) pair D subtracts + D FMAs for r2, D FMAs for the
   gradient (x rows only) and about 12 operations for the kernel itself.

Each figure is the time of one launch inside a captured graph of `reps` launches (no host launch gaps), replayed
`rounds` times after a warm-up; the candidates alternate within a round; median and range over the rounds.
Prints one JSON line and the markdown table of profiles/kernel_losses.md."""
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from kd6d import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
lib, check, P = _lib.lib, _lib.check, ops._ptr
KINDS = ("gaussian", "laplacian", "energy")


def graph_of(fn, reps):
    """fn() launched `reps` times on a side stream, captured -> the graph."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    return g


def time_graphs(graphs, reps, rounds):
    """{name: per-launch ms of every round}, the graphs alternating within a round."""
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps)
    return out


def stats(ms):
    return dict(median_us=1e3 * float(np.median(ms)), min_us=1e3 * float(np.min(ms)), max_us=1e3 * float(np.max(ms)))


def step_inputs(B=16, cap_s=48, cap_t=32, seed=0):
    r = np.random.default_rng(seed)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    s_cnt, t_cnt = r.integers(8, 13, B), r.integers(8, 13, B)
    centre = 0.3 + 0.4 * r.random((B, 1, 8, 2))
    xs = np.zeros((B, cap_s, 8, 2)); yt = np.zeros((B, cap_t, 8, 2))
    xs[:] = centre + 0.02 * r.standard_normal((B, cap_s, 8, 2))           # votes scattered ~ 13 px around a keypoint
    yt[:] = centre + 0.005 * r.standard_normal((B, cap_t, 8, 2))
    alpha = np.repeat(0.05 + 0.9 * r.random((B, cap_s, 1)), 8, 2)
    beta = 0.05 + 0.9 * r.random((B, cap_t, 8))
    return dict(xs=f(xs.reshape(-1, 8, 2)), alpha=f(alpha.reshape(-1, 8)), s_start=i(np.arange(B) * cap_s), s_cnt=i(s_cnt),
                yt=f(yt.reshape(-1, 8, 2)), beta=f(beta.reshape(-1, 8)), t_start=i(np.arange(B) * cap_t), t_cnt=i(t_cnt), B=B)


def bench_step(reps=200, rounds=9):
    d = step_inputs()
    B = d["B"]
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    gx, ga = torch.zeros_like(d["xs"]), torch.zeros_like(d["alpha"])
    args = (P(d["xs"]), P(d["alpha"]), P(d["s_start"]), P(d["s_cnt"]), P(d["yt"]), P(d["beta"]), P(d["t_start"]), P(d["t_cnt"]), B)
    outs = (P(loss), P(valid), None, P(gx), P(ga))

    def sinkhorn():
        check(lib.kd6d_sinkhorn_div_fwd_bwd(*args, 2.0, 0.001, 0.5, 0.5, *outs, ops._stream()), "kd6d_sinkhorn_div_fwd_bwd")

    def kernel(code, blur):
        return lambda: check(lib.kd6d_kernel_div_fwd_bwd(code, *args, blur, *outs, ops._stream()), "kd6d_kernel_div_fwd_bwd")

    graphs = {"sinkhorn blur 0.001": graph_of(sinkhorn, reps)}
    for k in KINDS:
        for blur in ((0.001, 0.05) if k != "energy" else (0.001,)):
            graphs["%s blur %g" % (k, blur)] = graph_of(kernel(_lib.KERNEL_KINDS[k], blur), reps)
    t = time_graphs(graphs, reps, rounds)
    assert int(valid.min()) == 1
    return {k: stats(v) for k, v in t.items()}


def bench_dense(N, M, D, reps, rounds):
    r = np.random.default_rng(1)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    x, y = f(0.3 + 0.3 * r.random((N, D))), f(0.3 + 0.3 * r.random((M, D)))
    a, b = f(0.05 + 0.9 * r.random(N)), f(0.05 + 0.9 * r.random(M))
    nws = int(lib.kd6d_kernel_dense_workspace_floats(N, M, D))
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    loss, gx, ga = torch.empty(1, dtype=torch.float32, device=dev), torch.empty_like(x), torch.empty_like(a)

    def kernel(code):
        return lambda: check(lib.kd6d_kernel_dense_fwd_bwd(code, P(x), P(a), P(y), P(b), N, M, D, 0.05, P(ws), nws, P(loss), P(gx),
                                                           P(ga), ops._stream()), "kd6d_kernel_dense_fwd_bwd")

    t = time_graphs({k: graph_of(kernel(_lib.KERNEL_KINDS[k]), reps) for k in KINDS}, reps, rounds)
    pairs_x, pairs_y = float(N) * (N + M), float(M) * M
    laneops = pairs_x * (3 * D + 12) + pairs_y * (2 * D + 12)          # fp32 lane-operations (an FMA counted once)
    peak = 256 * 4 * 32 * 2.4e9                                        # lanes per clock x clock (157 TFLOP/s / 2)
    out = {}
    for k, v in t.items():
        s = stats(v)
        sec = s["median_us"] * 1e-6
        s.update(pairs_per_s=(pairs_x + pairs_y) / sec, frac_of_fp32_vector_peak=laneops / sec / peak)
        out[k] = s
    return out


if __name__ == "__main__":
    res = {"step_B16": bench_step(), "dense_16384x16384_D16": bench_dense(16384, 16384, 16, 3, 5),
           "dense_2048x2048_D16": bench_dense(2048, 2048, 16, 20, 7)}
    print(json.dumps({"workload": "kernel distances per launch (tools/bench_kernel_loss.py)", "results": res}))
    print("| launch | median us | min us | max us | pairs/s | share of fp32 vector peak |")
    print("|---|---|---|---|---|---|")
    for grp, rows in res.items():
        for k, s in rows.items():
            print("| %s: %s | %.1f | %.1f | %.1f | %s | %s |" % (
                grp, k, s["median_us"], s["min_us"], s["max_us"],
                "%.3e" % s["pairs_per_s"] if "pairs_per_s" in s else "", "%.1f %%" % (100 * s["frac_of_fp32_vector_peak"])
                if "frac_of_fp32_vector_peak" in s else ""))
