"""Loader throughput on real-data batches: the host loader against the device-resident frame cache
(train_kd.py --frame_cache device; kd6d/libs/frame_cache.py, csrc/frame_cache.hip).  Run on the GPU box.

    python tools/bench_loader.py [--config_file cfg.yaml] [--batch 16] [--num_workers 8] [--batches 40] [--repeat 32]
                                 [--aug_pose_remap both --rounds 3]

Both sides are `kd6d.libs.train_libs.build_dataset(cfg, frame_cache="off" / "device")` over the SAME image list, without
and with `--augment`; the training loader is iterated (epochs chained), the model is not run, and the GPU is synchronised
once per batch.  The host side is the loader every run without the flag uses, workers and all; its DataLoader starts
its workers anew every epoch, as in training.  Reported per side: batches/s and images/s over a window of at least
`--batches` batches and `--min_seconds` seconds after 2 warm-up batches, and for the cached side the build time and the
bytes cached.  --aug_pose_remap {host,device,both}: where the augmented loaders solve their pose remaps (train_kd.py
--aug_pose_remap); `both` times the two modes alternating, `--rounds` times each, inside this one run.

--config_file names a yaml whose DATASETS point at a data set on this machine (frames at the internal resolution).
Without it a tree is written at run time by tests/frame_cache_cases.write_cache_tree at 480 x 640: 7 NOISE frames (PNG
does not compress them, so decoding them costs more than decoding a photograph of that size), each listed `--repeat`
times -- the host loader decodes a listed frame at every visit whether or not the file repeats, the cache stores every
list entry in its own slot.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))
sys.path.insert(0, os.path.join(HERE, "tests"))
import torch  # noqa: E402


def noise_cfg(root, repeat):
    import yaml
    import frame_cache_cases as C
    from kd6d.arguments.argument import custom_cfg
    tree = C.write_cache_tree(root, size=(480, 640))
    lst = os.path.join(root, "train", "bench_list.txt")
    with open(tree["list"]) as f:
        names = [ln for ln in f.read().split("\n") if ln]
    with open(lst, "w") as f:
        f.write("".join(n + "\n" for _ in range(repeat) for n in names))
    with open(os.path.join(HERE, "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["MODEL"]["BACKBONE"] = "darknet_tiny_h"
    cfg = custom_cfg(cfg)
    cfg["DATASETS"].update(TRAIN=lst, VALID=tree["eval_list"], TEST=tree["eval_list"], MESH_DIR=tree["models"],
                           BBOX_FILE=tree["bbox"], SYMMETRY_TYPES={})
    cfg["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2,
                         AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05)
    return cfg


def file_cfg(path):
    from kd6d.arguments.argument import custom_cfg
    from kd6d.arguments.argument_kd import load_yaml
    cfg = load_yaml(path)
    cfg["MODEL"].setdefault("BACKBONE", "darknet_tiny_h")
    return custom_cfg(cfg)


def measure(cfg, dev, augment, mode, budget_gb, batches, min_seconds, warmup=2, pose_remap="host"):
    from kd6d.libs.train_libs import build_dataset
    cfg["RUNTIME"]["AUG_POSE_REMAP"] = pose_remap if augment else "host"
    t0 = time.time()
    train, _ = build_dataset(cfg, dev, augment=augment, frame_cache=mode, frame_cache_gb=budget_gb)
    torch.cuda.synchronize()
    setup = time.time() - t0
    seen, t_start, images, done = 0, None, 0, False
    while not done:
        for im, tgt, metas in train:
            torch.cuda.synchronize()
            seen += 1
            if seen == warmup:
                t_start = time.time()
            elif seen > warmup:
                images += im.tensors.shape[0]
                done = seen >= warmup + batches and time.time() - t_start >= min_seconds
            if done:
                break
    dt = time.time() - t_start
    timed = seen - warmup
    out = {"loader": "cached" if mode == "device" else "host", "augment": bool(augment), "batches": timed,
           "seconds": round(dt, 2), "batches_per_s": round(timed / dt, 2), "images_per_s": round(images / dt, 1),
           "frames_in_list": len(train.loader.dataset), "setup_s": round(setup, 2)}
    if augment:
        out["aug_pose_remap"] = pose_remap
    if mode == "device":
        c = train.cache
        out.update(cache_build_s=round(c.build_seconds, 2), cache_bytes=c.nbytes, cached_frames=c.n, invalid_frames=c.n_invalid)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config_file", type=str, default="")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--batches", type=int, default=40, help="timed batches, at least")
    p.add_argument("--min_seconds", type=float, default=2.0, help="... and the timed window lasts at least this long")
    p.add_argument("--repeat", type=int, default=32, help="noise tree: times each of the 7 frames is listed")
    p.add_argument("--frame_cache_gb", type=float, default=64.)
    p.add_argument("--aug_pose_remap", type=str, default="host", choices=["host", "device", "both"],
                   help="pose remaps of the augmented loaders: host, device, or both alternating (--rounds each)")
    p.add_argument("--rounds", type=int, default=1, help="times every augmented measurement is repeated")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    tmp = None
    if args.config_file:
        cfg, source = file_cfg(args.config_file), args.config_file
    else:
        tmp = tempfile.TemporaryDirectory()
        cfg, source = noise_cfg(tmp.name, args.repeat), "noise frames 480x640, 7 files x %d" % args.repeat
    cfg["RUNTIME"] = {"PRECISION": "bf16", "N_GPU": 1, "DISTRIBUTED": False, "NUM_WORKERS": args.num_workers}
    cfg["SOLVER"]["IMS_PER_BATCH"] = args.batch
    print(json.dumps({"source": source, "batch": args.batch, "num_workers": args.num_workers,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    remaps = ("host", "device") if args.aug_pose_remap == "both" else (args.aug_pose_remap,)
    for mode in ("off", "device"):
        print(json.dumps(measure(cfg, dev, False, mode, args.frame_cache_gb, args.batches, args.min_seconds)), flush=True)
    for mode in ("off", "device"):
        for _ in range(max(1, args.rounds)):
            for remap in remaps:
                print(json.dumps(measure(cfg, dev, True, mode, args.frame_cache_gb, args.batches, args.min_seconds,
                                         pose_remap=remap)), flush=True)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
