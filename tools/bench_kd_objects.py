"""Cost of the per-object KD term (--kd_per_object) launch by launch, against the per-image launches on the same batch.
Run on the GPU box.

    python tools/bench_kd_objects.py [--reps 20] [--out profiles/kd_per_object_launches]

Figures are hip-event times of a captured graph holding `reps` back-to-back launches, replayed 5 times (us per launch,
launch overhead amortised), for B = 16 and B = 128 images of 256 x 256 with 3 objects each (synthetic batches, random
head outputs with every ground-truth class emitting on the teacher side, positives from kd6d_ssc_assign):
  * teacher_select (per image)          against  teacher_select_objects (B x 4 workgroups)
  * sinkhorn over B problems            against  sinkhorn over 4 B problems (the object segments)
  * kd_mean over B                      against  kd_mean over 4 B
  * kd_group_objects, kd_scatter_objects: the two launches the per-object term adds.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))
import torch  # noqa: E402

from kd6d import kd_losses as KL, ops  # noqa: E402
from kd6d._lib import check, lib  # noqa: E402
from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS, make_batch, teacher_cls_bias  # noqa: E402


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


def bench_batch(B, reps, dev, crop=256, instances=3):
    _, targets = make_batch(B, 1, crop=crop, instances=instances, mixed_classes=True)
    tgt = KL.PackedTargets(targets, dev)
    levels = [(max(crop // 8 // 2 ** i, 1),) * 2 for i in range(5)]
    rows = B * sum(h * w for h, w in levels)
    g = torch.Generator().manual_seed(0)
    bias = torch.tensor(teacher_cls_bias(instances, True) + [0.0])
    tcls = (torch.randn(rows, 16, generator=g) * 0.5 + bias).to(dev)          # every LINEMOD class emits
    treg = (torch.randn(rows, 240, generator=g) * 0.3).to(dev)
    scls = (torch.randn(rows, 16, generator=g) * 2.0 - 1.0).clamp(-6, 6).to(dev)
    sreg = (torch.randn(rows, 240, generator=g) * 0.3).to(dev)
    P, st = ops._ptr, ops._stream
    out = {"batch": B, "objects": B * instances}
    tk = {}
    for mode in (False, True):
        flats = KL.teacher_flats(B, dev, per_object=mode)
        sel = lambda: KL.teacher_select(tcls, treg, levels, B, tgt.bbox_trans, flats=flats, zeroed=True, per_object=mode,  # noqa: E731
                                        class_ids=tgt.class_ids, n_gt=tgt.n_gt)
        tk[mode] = sel()
        out["teacher_select_objects" if mode else "teacher_select"] = graph_time(sel, reps)
    ev = KL.KDLoss(INTERNAL_K, MESH_DIAMETERS, kd_cfg={"PER_OBJECT": True})
    pre = ev.assign(levels, B, tgt, torch.rand(rows, generator=g).to(dev))
    ev.forward(scls, sreg, levels, B, tgt, tk[True], pre=pre)
    torch.cuda.synchronize()
    c, o = ev.ctx, ev.obj
    out["positives_per_image"] = float(c["pos_cnt"].float().mean())
    out["valid_objects"] = int(c["n_valid"])
    cap, nobj = ev.cap, B * KL.MAX_GT
    n = B * cap
    f32 = dict(dtype=torch.float32, device=dev)
    s_start = torch.arange(B, dtype=torch.int32, device=dev) * cap
    li, vi = torch.zeros(B, **f32), torch.zeros(B, dtype=torch.int32, device=dev)
    gx, ga = torch.zeros(n, 8, 2, **f32), torch.zeros(n, 8, **f32)
    lk, nv = torch.zeros(1, **f32), torch.zeros(1, dtype=torch.int32, device=dev)
    ti = tk[False]

    def sink_img():
        check(lib.kd6d_sinkhorn_div_fwd_bwd(P(c["xs"]), P(c["alpha"]), P(s_start), P(c["pos_cnt"]), P(ti.t_kp_norm), P(ti.t_beta),
                                            P(ti.t_start), P(ti.t_cnt), B, ev.p, ev.blur, ev.scaling, ev.reach, P(li), P(vi),
                                            None, P(gx), P(ga), st()), "sinkhorn")

    to = tk[True]

    def sink_obj():
        check(lib.kd6d_sinkhorn_div_fwd_bwd(P(o["xs"]), P(o["alpha"]), P(o["start"]), P(o["cnt"]), P(to.t_kp_norm), P(to.t_beta),
                                            P(to.t_start), P(to.t_cnt), nobj, ev.p, ev.blur, ev.scaling, ev.reach, P(o["loss"]),
                                            P(o["valid"]), None, P(o["g_xs"]), P(o["g_alpha"]), st()), "sinkhorn")

    def group():
        check(lib.kd6d_kd_group_objects(P(c["pos_cnt"]), P(c["pos_gt"]), P(c["xs"]), P(c["alpha"]), B, cap, P(o["start"]),
                                        P(o["cnt"]), P(o["dest"]), P(o["xs"]), P(o["alpha"]), st()), "group")

    def scatter():
        check(lib.kd6d_kd_scatter_objects(P(c["pos_cnt"]), P(c["pos_gt"]), P(o["dest"]), P(o["valid"]), P(o["g_xs"]),
                                          P(o["g_alpha"]), B, cap, P(c["g_xs"]), P(c["g_alpha"]), P(c["valid"]), st()), "scatter")

    out["sinkhorn_images"] = graph_time(sink_img, reps)
    out["sinkhorn_objects"] = graph_time(sink_obj, reps)
    out["kd_mean_images"] = graph_time(lambda: check(lib.kd6d_kd_mean(P(li), P(vi), B, P(lk), P(nv), st())), reps)
    out["kd_mean_objects"] = graph_time(lambda: check(lib.kd6d_kd_mean(P(o["loss"]), P(o["valid"]), nobj, P(lk), P(nv), st())), reps)
    out["kd_group_objects"] = graph_time(group, reps)
    out["kd_scatter_objects"] = graph_time(scatter, reps)
    return {k: (round(v, 2) if isinstance(v, float) else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = [bench_batch(B, a.reps, dev) for B in (16, 128)]
    keys = ["teacher_select", "teacher_select_objects", "sinkhorn_images", "sinkhorn_objects", "kd_mean_images",
            "kd_mean_objects", "kd_group_objects", "kd_scatter_objects"]
    print("| launch (us) | " + " | ".join("B = %d" % r["batch"] for r in res) + " |")
    print("|---|" + "---|" * len(res))
    for k in keys:
        print("| %s | " % k + " | ".join("%.2f" % r[k] for r in res) + " |")
    for r in res:
        per_img = r["teacher_select"] + r["sinkhorn_images"] + r["kd_mean_images"]
        per_obj = (r["teacher_select_objects"] + r["sinkhorn_objects"] + r["kd_mean_objects"] + r["kd_group_objects"]
                   + r["kd_scatter_objects"])
        r["sum_per_image_us"], r["sum_per_object_us"] = round(per_img, 2), round(per_obj, 2)
        print("B = %d: %d valid objects, %.1f positives per image; KD launches per image %.1f us, per object %.1f us"
              % (r["batch"], r["valid_objects"], r["positives_per_image"], per_img, per_obj))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
