"""Derived configuration keys (the hard-coded layer of arguments/argument.py:51-104) and the command line of the
evaluation entry test.py (arguments/argument.py:6-48: get_argparser / get_args)."""
import argparse

_BACKBONES = {
    # name: (FEAT_CHANNELS, OUT_CHANNEL, VAL_FREQ)
    "darknet_tiny": ([0, 0, 128, 128], 256, 500),
    "darknet_tiny_h": ([0, 0, 64, 64], 128, 500),       # half the channels of darknet_tiny
    "darknet53": ([0, 0, 256, 512, 1024], 256, 2000),
}

_SOLVER_DEFAULTS = {
    "GRAD_CLIP": 1.0, "VAL_FREQ": 5000, "AUGMENTATION_OCCLUSION": 0, "AUGMENTATION_Grayscalize": False,
    "AUGMENTATION_Smooth": 0, "AUGMENTATION_Sharpen": 0, "AUGMENTATION_BACKGROUND_DIR": None,
}


def custom_cfg(cfg):
    name = cfg["MODEL"]["BACKBONE"]
    if name not in _BACKBONES:
        raise AssertionError("Unsupported backbone %r (the HIP path implements %s)" % (name, sorted(_BACKBONES)))
    feat, out_c, val_freq = _BACKBONES[name]
    cfg["MODEL"]["OUT_CHANNEL"] = out_c
    cfg["MODEL"]["FEAT_CHANNELS"] = list(feat)
    cfg["SOLVER"]["VAL_FREQ"] = val_freq
    cfg["MODEL"]["N_CONV"] = 4
    cfg["MODEL"]["PRIOR"] = 0.01
    cfg["MODEL"].setdefault("USE_HIGHER_LEVELS", True)
    cfg["SOLVER"].update(FOCAL_GAMMA=2.0, FOCAL_ALPHA=0.25, TOP_K=9, POSITIVE_NUM=10)
    cfg["INPUT"].update(PIXEL_MEAN=[0.485, 0.456, 0.406], PIXEL_STD=[0.229, 0.224, 0.225], SIZE_DIVISIBLE=32)
    for k, v in _SOLVER_DEFAULTS.items():
        cfg["SOLVER"].setdefault(k, v)
    cfg["DATASETS"].setdefault("SYMMETRY_TYPES", {})
    return cfg


def get_argparser():
    """The reference's options of arguments/argument.py:6-22 that evaluation reads, under their names and defaults, plus
    the additive ones of this build (--synthetic, --precision, --pnp_solver, --eval_scorer, --image_size, --frame_cache,
    --frame_cache_gb, --bop_metrics, --bop_vsd, --bop_csv, --frame_source and the --render_* flags)."""
    from .argument_kd import add_bop_flags, add_frame_cache_flags, add_render_flags
    p = argparse.ArgumentParser()
    p.add_argument("--local_rank", type=int, default=0)
    p.add_argument("--config_file", type=str, default="./configs/ape.yaml")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--working_dir", type=str, default="./outputs/")
    p.add_argument("--test_file", type=str, default="")
    p.add_argument("--weight_file", type=str, default="")
    p.add_argument("--running_device", type=str, default="cuda")
    p.add_argument("--backbone", type=str, default="darknet53")
    # additive (this build)
    p.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--synthetic", action="store_true", help="seeded LINEMOD-shaped synthetic batches (no dataset)")
    p.add_argument("--image_size", type=int, default=256, help="synthetic crop size")
    p.add_argument("--pnp_solver", type=str, default="host", choices=["host", "device"],
                   help="PnP-RANSAC of evaluation: host = numpy (kd6d/libs/pnp.py), device = HIP (csrc/pnp.hip)")
    p.add_argument("--eval_scorer", type=str, default="host", choices=["host", "device"],
                   help="pose errors of evaluation: host = float64 numpy, one object at a time "
                        "(kd6d/libs/evaluate.py); device = HIP (csrc/pose_err.hip), every object in one launch")
    add_frame_cache_flags(p)
    add_bop_flags(p)
    add_render_flags(p, training=False)
    p.add_argument("--bop_csv", type=str, default="",
                   help="write every kept prediction in the BOP results format (scene_id,im_id,obj_id,score,R,t,time) to "
                        "this file; with or without --bop_metrics.  Not with --synthetic")
    return p


def get_args(argv=None):
    """-> cfg: the yaml (a `_BASE_` file honoured) with cfg['RUNTIME'] filled as arguments/argument.py:32-38 does
    (LOCAL_RANK, CONFIG_FILE, NUM_WORKERS, WEIGHT_FILE, WORKING_DIR, RUNNING_DEVICE) plus this build's keys."""
    from .argument_kd import check_bop_flags, frame_cache_runtime, load_yaml, render_runtime
    parser = get_argparser()
    args = parser.parse_args(argv)
    check_bop_flags(parser, args)
    if args.bop_csv and args.synthetic:
        from ..libs.bop_metrics import BOP_CSV_SYNTHETIC_ERROR
        raise SystemExit(BOP_CSV_SYNTHETIC_ERROR)
    fc = frame_cache_runtime(args)
    fc.update(render_runtime(args))
    cfg = load_yaml(args.config_file)
    cfg["RUNTIME"] = dict(LOCAL_RANK=args.local_rank, CONFIG_FILE=args.config_file, NUM_WORKERS=args.num_workers,
                          WEIGHT_FILE=args.weight_file, WORKING_DIR=args.working_dir,
                          RUNNING_DEVICE=args.running_device, PRECISION=args.precision, SYNTHETIC=bool(args.synthetic),
                          IMAGE_SIZE=int(args.image_size), PNP_SOLVER=args.pnp_solver, EVAL_SCORER=args.eval_scorer,
                          BOP_METRICS=bool(args.bop_metrics), BOP_VSD=bool(args.bop_vsd), BOP_CSV=args.bop_csv,
                          **fc)
    if len(args.test_file) > 0:
        cfg["DATASETS"]["TEST"] = args.test_file
    cfg["DATASETS"].setdefault("MIXED_CLASSES", False)
    cfg["MODEL"]["BACKBONE"] = args.backbone
    return custom_cfg(cfg)
