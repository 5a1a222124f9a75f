"""Cost of the two stages `--aug_chain full` adds to the augmentation front-end (csrc/augment.hip: kd6d_aug_background,
kd6d_aug_sharpen).  Run on the GPU box.

    python tools/bench_aug_full.py [--reps 10] [--frames 64] [--front_iters 30] [--skip_front] [--out profiles/aug_full_chain]

Device figures are hip-event times of a captured graph holding `reps` back-to-back calls of the C entry point (its
per-image parameters already on the device), replayed 5 times: per call, launch overhead amortised.  `frames` frames of
640 x 480 noise with two instance rectangles:
  * background: every frame draws one, from a pool of 64 VOC-sized (375 x 500) images and from a pool of 64 images of
                the frame's size (the resize degenerates to a copy); the mask leaves ~86 % of the pixels to replace;
  * sharpen:    every frame, ks = 5 and ks = 11, ratio mode (init + three launches per call);
  * filter:     kd6d_aug_filter's box blur alone at the same ks -- one blur by global loads, where a sharpen call forms
                two on LDS tiles plus the edge / blend arithmetic -- as the context for what the tiling buys.
Buffers are the same in every call: 59 MB of frames sit in the 256 MiB Infinity Cache, so these are CACHE figures.
The host columns are the numpy restatement (tests/augment_full_ref.py) on one frame.  `front`: wall time per batch of
AugmentFront.run (B = 16, every base stage on, host pose remap), synchronised per batch, with the base and the full chain
on the same draws otherwise.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))
sys.path.insert(0, os.path.join(HERE, "tools"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import augment_full_ref as FR  # noqa: E402
from bench_pose_err import graph_time  # noqa: E402
from kd6d import ops  # noqa: E402
from kd6d.libs import augment as A  # noqa: E402
from kd6d.ops import check, lib  # noqa: E402

H, W = 480, 640
LINEMOD_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])


def frames_masks(n, rng, dev):
    f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    m = np.zeros((n, H, W), np.float32)
    m[:, 150:300, 200:400] = 1
    m[:, 320:400, 420:560] = 2
    return f, m, torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev)


def pool_of(n, hw, rng, dev):
    imgs = {"bg%03d" % i: rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8) for i in range(n)}
    return A.BackgroundPool("", list(imgs), dev, 2 ** 32, probe=lambda p: imgs[p].shape[:2], decode=lambda p: imgs[p]), imgs


def host_time(fn, reps=3):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def kernels(a, dev, res):
    rng = np.random.default_rng(0)
    n = a.frames
    f, m, fd, md = frames_masks(n, rng, dev)
    rows = []
    for name, hw in (("background, pool of 375 x 500", (375, 500)), ("background, pool of 480 x 640 (copy)", (H, W))):
        pool, imgs = pool_of(64, hw, rng, dev)
        idx = torch.from_numpy((np.arange(n) % 64).astype(np.int32)).to(dev)
        x = fd.clone()
        fn = lambda: check(lib.kd6d_aug_background(ops._ptr(x), ops._ptr(md), n, H, W, ops._ptr(pool.pool), pool.nbytes,  # noqa: E731
                                                   ops._ptr(pool.off), ops._ptr(pool.hw), pool.n, ops._ptr(idx),
                                                   ops._stream()), "kd6d_aug_background")
        us = graph_time(fn, a.reps)
        back = imgs["bg000"]
        ms = host_time(lambda: FR.merge_background(f[0], m[0], back))
        rows.append({"call": name, "us_per_call": round(us, 1), "us_per_frame": round(us / n, 2), "host_ms_per_frame": round(ms, 1)})
    out = torch.empty_like(fd)
    ws = torch.empty(int(lib.kd6d_aug_sharpen_ws_bytes(n)) // 8 + 1, dtype=torch.int64, device=dev)
    mode = torch.ones(n, dtype=torch.int32, device=dev)
    alpha = torch.full((n,), 0.7, dtype=torch.float64, device=dev)
    for ks in (5, 11):
        k = torch.full((n,), ks, dtype=torch.int32, device=dev)
        fn = lambda: check(lib.kd6d_aug_sharpen(ops._ptr(fd), ops._ptr(out), n, H, W, ops._ptr(k), ops._ptr(mode),  # noqa: E731
                                                ops._ptr(alpha), ops._ptr(ws), ws.numel() * 8, ops._stream()),
                           "kd6d_aug_sharpen")
        us = graph_time(fn, a.reps)
        ms = host_time(lambda: FR.pencil_sharpen(f[0], ks, True, 0.7), reps=1)
        rows.append({"call": "sharpen, ks = %d" % ks, "us_per_call": round(us, 1), "us_per_frame": round(us / n, 2),
                     "host_ms_per_frame": round(ms, 1)})
        fn = lambda: check(lib.kd6d_aug_filter(ops._ptr(fd), ops._ptr(out), n, H, W, ops._ptr(k), None, 0, 0,  # noqa: E731
                                               ops._stream()), "kd6d_aug_filter")
        us = graph_time(fn, a.reps)
        rows.append({"call": "filter (blur alone), ks = %d" % ks, "us_per_call": round(us, 1),
                     "us_per_frame": round(us / n, 2), "host_ms_per_frame": None})
    print("| call (%d frames of %d x %d) | us per call | us per frame | numpy restatement, ms per frame |" % (n, W, H))
    print("|---|---|---|---|")
    for r in rows:
        print("| %s | %.1f | %.2f | %s |" % (r["call"], r["us_per_call"], r["us_per_frame"],
                                             "-" if r["host_ms_per_frame"] is None else "%.1f" % r["host_ms_per_frame"]))
    res["kernels"] = {"frames": n, "image": [W, H], "rows": rows}


def front(a, dev, res):
    import random
    from PIL import Image
    B = 16
    rng = np.random.default_rng(1)
    _, _, fd, md = frames_masks(B, rng, dev)
    box = np.array([[[x, y, z] for x in (-40, 40) for y in (-40, 40) for z in (-40, 40)]], np.float64)
    K2 = LINEMOD_K.copy(); K2[0, 0] *= 0.97; K2[0, 2] += 4.0
    targets = [types.SimpleNamespace(class_ids=torch.zeros(2, dtype=torch.long), keypoints_3d=torch.from_numpy(box).float())
               for _ in range(B)]
    Rs, Ts = [np.eye(3)] * 2, [np.array([[-30.0], [-20.0], [800.0]]), np.array([[200.0], [150.0], [900.0]])]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(16):
            Image.fromarray(rng.integers(0, 256, (375, 500, 3), dtype=np.uint8), "RGB").save(os.path.join(d, "%02d.png" % i))
        for chain in ("base", "full"):
            solver = dict(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_SHIFT=0.05, AUGMENTATION_SCALE=0.05, AUGMENTATION_ROTATION=10,
                          AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2, AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=5,
                          AUGMENTATION_Noise=0.03, AUGMENTATION_Grayscalize=False)
            if chain == "full":
                solver.update(AUGMENTATION_BACKGROUND_DIR=d, AUGMENTATION_Sharpen=0.5)
            cfg = dict(SOLVER=solver, INPUT=dict(INTERNAL_K=LINEMOD_K.reshape(-1).tolist(), INTERNAL_WIDTH=W, INTERNAL_HEIGHT=H),
                       DATASETS={}, RUNTIME=dict(AUG_CHAIN=chain))
            ac = A.AugConfig(cfg)
            fr = A.AugmentFront(ac, dev)
            random.seed(0); np.random.seed(0)
            batches = [A.collate_params([A.draw_params(ac, K2, [0, 0], Rs, Ts, box) for _ in range(B)]) for _ in range(4)]
            for p in batches[:2]:
                fr.run(fd, md, targets, p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.front_iters):
                fr.run(fd, md, targets, batches[i % len(batches)])
            torch.cuda.synchronize()
            out[chain] = round((time.perf_counter() - t0) / a.front_iters * 1e3, 3)
            if chain == "full":
                out["drew_background"] = float(np.mean([(p["bg"] >= 0).mean() for p in batches]))
                out["drew_sharpen"] = float(np.mean([(p["sharpen_ks"] > 0).mean() for p in batches]))
    print("AugmentFront.run, B = %d of %d x %d, ms per batch: %s" % (B, W, H, out))
    res["front_ms_per_batch"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--front_iters", type=int, default=30)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--skip_front", action="store_true", help="kernels only (for a run under a kernel tracer)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    kernels(a, dev, res)
    if not a.skip_front:
        front(a, dev, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
