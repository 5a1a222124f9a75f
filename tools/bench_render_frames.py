"""Cost of rendering training frames on the GPU (csrc/render_frames.hip).  Run on the GPU box.

    python tools/bench_render_frames.py [--reps 10] [--frames 64] [--out profiles/render_frames]

Figures are hip-event times of a captured graph holding `reps` back-to-back kd6d_render_frames calls, replayed 5 times
(per call, launch overhead amortised): `frames` frames of 640 x 480 under LINEMOD's K, each with 1 and with 4 objects --
surrogate meshes (synthetic.surrogate_mesh, 5120 faces), poses and lights as the rendered frame source draws them
(kd6d/libs/render_source.py: z = 600 ... 1400 mm, the projected box inside the frame), noise backgrounds -- with and
without the depth output.  The scene draw on the host and the build of a whole store (draw + upload + render + the
visible-pixel count) are timed by wall clock beside it.  For context the JSON repeats the loaders' rates recorded in
profiles/frame_cache.md (host loader, device cache, the training step).
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

from bench_pose_err import graph_time  # noqa: E402
from kd6d import ops  # noqa: E402
from kd6d.libs import render_source as RS  # noqa: E402
from kd6d.synthetic import INTERNAL_K, LINEMOD_CLASSES  # noqa: E402

H, W = 480, 640
CONTEXT = {"source": "profiles/frame_cache.md", "host_loader_images_per_s": 333, "device_cache_images_per_s": 52000,
           "host_loader_augment_images_per_s": 269, "device_cache_augment_images_per_s": 753, "train_step_images_per_s": 6200}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K = np.asarray(INTERNAL_K, np.float64).reshape(3, 3)
    meshes, kp3d = RS.surrogate_meshes(15)
    res = {"image": [W, H], "faces": int(len(meshes[0].faces)), "frames_per_call": a.frames, "context": CONTEXT, "runs": []}
    for inst in (1, 4):
        t0 = time.perf_counter()
        st = RS.RenderedFrames(meshes, kp3d, a.frames, K, H, W, dev, seed=1, instances=inst, classes=LINEMOD_CLASSES,
                               keep_depth=True, log=None)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        # every frame with exactly `inst` objects: the store draws 1 ... inst, the bench wants the full count
        rng = np.random.Generator(np.random.PCG64(7))
        t0 = time.perf_counter()
        st.instances = inst
        scenes = st._draw(rng)
        draw_s = time.perf_counter() - t0
        kp = kp3d.numpy().astype(np.float64)
        for s in scenes:
            while len(s["cls"]) < inst:
                c = int(rng.choice([c for c in LINEMOD_CLASSES if c not in s["cls"]]))
                R = RS._random_rotation(rng)
                s["cls"].append(c); s["R"].append(R); s["T"].append(RS.place(rng, K, kp[c], R, H, W, st.z_range))
        arrays = st._arrays(scenes)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in {**st.pool, **arrays}.items()}
        args = [d[k] for k in RS.ARRAY_ORDER]
        ops.render_frames(*args, H, W, out=(st.frames, st.masks, st.depth))                  # once with the check
        covered = float((st.masks > 0).sum()) / a.frames
        for depth in (False, True):
            out = (st.frames, st.masks, st.depth if depth else None)
            us = graph_time(lambda: ops.render_frames(*args, H, W, out=out, validate=False), a.reps)
            run = {"objects_per_frame": inst, "depth_output": depth, "us_per_call": round(us, 1),
                   "us_per_frame": round(us / a.frames, 2), "frames_per_s": round(a.frames * 1e6 / us, 0),
                   "covered_pixels_per_frame": round(covered, 0)}
            res["runs"].append(run)
            print("%d object(s) per frame, depth %s: %.1f us per call of %d frames = %.2f us per frame = %.0f frames/s "
                  "(%.0f covered pixels per frame)" % (inst, depth, us, a.frames, us / a.frames, a.frames * 1e6 / us, covered))
        res["runs"].append({"objects_per_frame": "1..%d" % inst, "store_build_s": round(build_s, 3),
                            "store_build_frames_per_s": round(a.frames / build_s, 0), "host_draw_s": round(draw_s, 4)})
        print("store of %d frames with 1..%d objects: built in %.3f s (%.0f frames/s, first call included); host scene draw "
              "%.4f s" % (a.frames, inst, build_s, a.frames / build_s, draw_s))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
