"""Command line + yaml -> (cfg, cfg_t): the flag surface of arguments/argument_kd.py:15-106.

Every reference flag keeps its name, type and default.  Additive flags of this build:
--precision {bf16,fp32}, --synthetic, --augment, --skip_teacher_eval, --batch_size (per-step GLOBAL batch,
overrides SOLVER.IMS_PER_BATCH), --image_size, --mixed_classes, --teacher_pnp_gate, --pnp_solver, --eval_scorer, --kd_per_object, --kd_kernel_losses,
--synthetic_instances, --frame_cache, --frame_cache_gb, --aug_pose_remap, --aug_chain, --aug_background_gb, --bop_metrics, --bop_vsd, --frame_source and
the --render_* flags; yaml files may name a `_BASE_` file.
"""
import argparse
import os

import yaml

from .argument import custom_cfg


def str2bool(v):
    if isinstance(v, bool):
        return v
    s = v.lower()
    if s in ("yes", "true", "t", "y", "1"):
        return True
    if s in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def get_argparser():
    p = argparse.ArgumentParser()
    p.add_argument("--local_rank", type=int, default=0)
    p.add_argument("--config_file", type=str, default="./configs/ape.yaml")
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--working_dir", type=str, default="./outputs/")
    p.add_argument("--test_file", type=str, default="")
    p.add_argument("--weight_file", type=str, default="")
    p.add_argument("--running_device", type=str, default="cuda")
    p.add_argument("--backbone", type=str, default="darknet_tiny_h")
    p.add_argument("--max_iters", type=int, default=20000, help="max iteration")
    p.add_argument("--base_lr", type=float, default=0.001, help="base learning rate")
    # teacher
    p.add_argument("--config_file_t", type=str, default="./configs/occ_linemod.yaml")
    p.add_argument("--backbone_t", type=str, default="darknet53")
    p.add_argument("--weight_file_t", type=str, default="")
    # distillation
    p.add_argument("--kd_weight", type=float, default=5, help="weight of loss_kd_loss")
    p.add_argument("--kd_level", type=str, default="pred", help="level to be distilled")
    p.add_argument("--gtype", type=str, default="sinkhorn", help="function of kd loss",
                   choices=["l1", "l2", "sinkhorn", "gaussian", "laplacian", "energy"])
    p.add_argument("--glevel", type=str, default="point", help="level of kd loss", choices=["point"])
    p.add_argument("--p", type=float, default=2.0, help="p of loss_kd_loss")
    p.add_argument("--blur", type=float, default=0.001,
                   help="blur of loss_kd_loss.  For --gtype gaussian / laplacian it is the kernel's width: the reference's "
                        "default of 0.001 on frame-normalised coordinates makes such a kernel nearly diagonal (points "
                        "further apart than a few thousandths of the frame do not see each other)")
    p.add_argument("--gnD", type=int, default=2, help="dimensions of loss_kd_loss")
    p.add_argument("--weightedOT", type=str2bool, nargs="?", const=True, default=True, help="weighted OT of loss_kd_loss")
    p.add_argument("--wot_detach", type=str2bool, nargs="?", const=True, default=False, help="weighted ot with detached cls")
    p.add_argument("--scaling", type=float, default=0.5, help="param for sinkhorn loss")
    p.add_argument("--reach", type=float, default=0.5, help="param for sinkhorn loss")
    # additive (this build)
    p.add_argument("--precision", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--synthetic", action="store_true", help="seeded LINEMOD-shaped synthetic batches (no dataset)")
    p.add_argument("--augment", action="store_true",
                   help="real data: run the reference's train transform chain (Resize, occlusion, shift-scale-rotate, HSV, "
                        "blur, noise, grey, remove_invalids, symmetry handling) on the GPU front-end (kd6d/libs/augment.py)")
    p.add_argument("--aug_pose_remap", type=str, default="host", choices=["host", "device"],
                   help="--augment: where the two pose remaps of an item (Resize, shift-scale-rotate) are solved: host = "
                        "numpy, two solves per instance when the item is drawn (kd6d/libs/pnp.py); device = HIP "
                        "(csrc/pnp.hip), every instance of a batch in one launch of the augmentation front-end, read back "
                        "with its area table")
    p.add_argument("--aug_chain", type=str, default="base", choices=["base", "full"],
                   help="--augment: base = the chain without RandomBackground and RandomPencilSharpen (a yaml that sets "
                        "SOLVER.AUGMENTATION_BACKGROUND_DIR or AUGMENTATION_Sharpen is refused); full = both stages run on "
                        "the GPU front-end when the yaml enables them (csrc/augment.hip: kd6d_aug_background, "
                        "kd6d_aug_sharpen)")
    p.add_argument("--aug_background_gb", type=float, default=8.,
                   help="--aug_chain full: most GiB of device memory the decoded backgrounds of "
                        "SOLVER.AUGMENTATION_BACKGROUND_DIR may take per process (kept at their native sizes); a "
                        "directory that does not fit is refused")
    p.add_argument("--skip_teacher_eval", action="store_true")
    p.add_argument("--launch", type=str, default="graph", choices=["graph", "pipeline", "eager"],
                   help="graph: replay the captured step (hipGraph); pipeline: also overlap the teacher forward of "
                        "the next batch with the student step of the current one; eager: launch kernel by kernel")
    p.add_argument("--teacher_group", type=int, default=1,
                   help="--launch pipeline only: run the frozen teacher over the batches of this many consecutive steps in "
                        "one pass, cut into as many graph segments (kd6d.graph.GroupedTeacherKDStep; 2 * group batches "
                        "of look-ahead).  1 = one teacher forward per step")
    p.add_argument("--batch_size", type=int, default=0, help="global batch; 0 = SOLVER.IMS_PER_BATCH")
    p.add_argument("--image_size", type=int, default=256, help="synthetic crop size")
    p.add_argument("--val_freq", type=int, default=0, help="validate every N steps; 0 = the backbone's default")
    p.add_argument("--teacher_pnp_gate", action="store_true",
                   help="keep a teacher's cells only if RANSAC-PnP solves a pose from them (postprocess_kd.py:187-202); "
                        "with --pnp_solver host it needs --launch eager (one host synchronisation per step), with "
                        "--pnp_solver device it runs in every launch mode and with any --teacher_group")
    p.add_argument("--pnp_solver", type=str, default="host", choices=["host", "device"],
                   help="PnP-RANSAC of the teacher gate and of evaluation: host = numpy (kd6d/libs/pnp.py), one call "
                        "per object; device = HIP (csrc/pnp.hip), a batch per launch, no host synchronisation")
    p.add_argument("--eval_scorer", type=str, default="host", choices=["host", "device"],
                   help="pose errors of validation: host = float64 numpy, one object at a time "
                        "(kd6d/libs/evaluate.py); device = HIP (csrc/pose_err.hip), every object of a validation in one launch")
    p.add_argument("--two_launch_norm_bwd", action="store_true",
                   help="BatchNorm / GroupNorm backward as reduce + apply launches instead of one launch with an "
                        "in-kernel barrier (the remedy train_kd.py names when a barrier wait timed out)")
    p.add_argument("--exchange", type=str, default="between", choices=["between", "overlap"],
                   help="data-parallel gradient exchange: one all-reduce between the step's two graphs, or two slices inside "
                        "the step (FPN + head beside the backbone sweep; kd6d/libs/distributed.py EXCHANGE_MODE)")
    p.add_argument("--rccl_single_rank", action="store_true",
                   help="one process, one GPU, but the whole data-parallel path: a one-rank process group, the kd6d "
                        "communicator, the parameter broadcast and every step's all-reduce (rehearsal on a one-GPU box)")
    p.add_argument("--mixed_classes", type=str2bool, nargs="?", const=True, default=None,
                   help="synthetic batches mix the 13 LINEMOD classes (default: DATASETS.MIXED_CLASSES of the yaml)")
    p.add_argument("--kd_per_object", action="store_true",
                   help="distil per object: one OT problem per (image, ground-truth instance) -- the instance's positives "
                        "against the teacher's cells of its class -- instead of one per image (the reference's rule, "
                        "correct for one object per image only).  Not with --teacher_pnp_gate")
    p.add_argument("--kd_kernel_losses", action="store_true",
                   help="accept --gtype gaussian / laplacian / energy: geomloss' kernel distances (MMD) between the "
                        "student's and the teacher's weighted keypoint votes, in one pass over the pairs "
                        "(csrc/kernel_loss.hip) in the Sinkhorn launch's place; --p, --scaling and --reach do not enter "
                        "them.  Without this flag only --gtype sinkhorn is accepted")
    p.add_argument("--synthetic_instances", type=int, default=1, choices=[1, 2, 3, 4],
                   help="--synthetic: objects of distinct classes per image (masks in vertical strips)")
    add_frame_cache_flags(p)
    add_bop_flags(p)
    add_render_flags(p, training=True)
    return p


RENDER_SYNTHETIC_ERROR = ("--frame_source render cannot be combined with --synthetic: both replace the image lists, "
                          "choose one")
RENDER_FRAME_CACHE_ERROR = ("--frame_source render cannot be combined with --frame_cache device: rendered frames already "
                            "live in device memory (--frame_cache_gb bounds them) and there is no image list to cache")


def add_render_flags(p, training):
    """The flags of the rendered frame source (kd6d/libs/render_source.py, csrc/render_frames.hip); both entry points take all of
    them; test.py renders the valid list alone and does not use the two of the training list."""
    p.add_argument("--frame_source", type=str, default="list", choices=["list", "render"],
                   help="list = the image lists of the yaml (or --synthetic); render = frames drawn on the GPU by "
                        "kd6d_render_frames: shaded objects at random poses over a background, with their visible "
                        "masks, kept in device memory and fed through the frame cache's loader (DZI crop, --augment and "
                        "--aug_pose_remap apply unchanged).  Not with --synthetic or --frame_cache device")
    p.add_argument("--render_meshes", type=str, default="surrogate", choices=["dataset", "surrogate"],
                   help="dataset = the PLYs of DATASETS.MESH_DIR (faces, per-vertex red/green/blue; grey without) with "
                        "DATASETS.BBOX_FILE; surrogate = one coloured ellipsoid per class inside the class's cube box, "
                        "nothing read from disk")
    p.add_argument("--render_valid_frames", type=int, default=256,
                   help="frames of the rendered valid / test list (a fixed seed, never refreshed)")
    p.add_argument("--render_instances", type=int, default=1, choices=[1, 2, 3, 4],
                   help="a rendered frame shows 1 ... N objects of distinct classes; they may occlude one another")
    p.add_argument("--render_backgrounds", type=str, default="noise",
                   help="noise = procedural low-frequency colour fields; or a directory of .png / .jpg files at the "
                        "frame size (a file of another size is refused)")
    p.add_argument("--render_seed", type=int, default=0, help="seed of the rendered scenes (mixed with the rank)")
    only = "" if training else " (test.py renders the valid list alone: accepted, not used)"
    p.add_argument("--render_frames", type=int, default=2048, help="frames of the rendered training list per rank" + only)
    p.add_argument("--render_refresh", type=str, default="epoch", choices=["epoch", "never"],
                   help="epoch = redraw and re-render the training list after every pass, in place" + only)


def render_runtime(args):
    """-> the RUNTIME keys of the rendered frame source; refuses --frame_source render with --synthetic or with
    --frame_cache device."""
    source = getattr(args, "frame_source", "list")
    if source == "render" and bool(getattr(args, "synthetic", False)):
        raise SystemExit(RENDER_SYNTHETIC_ERROR)
    if source == "render" and getattr(args, "frame_cache", "off") != "off":
        raise SystemExit(RENDER_FRAME_CACHE_ERROR)
    return dict(FRAME_SOURCE=source, RENDER_MESHES=getattr(args, "render_meshes", "surrogate"),
                RENDER_FRAMES=int(getattr(args, "render_frames", 2048)),
                RENDER_VALID_FRAMES=int(getattr(args, "render_valid_frames", 256)),
                RENDER_INSTANCES=int(getattr(args, "render_instances", 1)),
                RENDER_REFRESH=getattr(args, "render_refresh", "epoch"),
                RENDER_BACKGROUNDS=getattr(args, "render_backgrounds", "noise"), RENDER_SEED=int(getattr(args, "render_seed", 0)))


FRAME_CACHE_SYNTHETIC_ERROR = ("--frame_cache device cannot be combined with --synthetic: synthetic batches are made on the "
                               "device already and there is no image list to cache")


def add_frame_cache_flags(p):
    """The two flags train_kd.py and test.py share (kd6d/libs/frame_cache.py)."""
    p.add_argument("--frame_cache", type=str, default="off", choices=["off", "device"],
                   help="real data: device = decode every frame of the train / valid / test lists once, keep frames, "
                        "instance masks and annotations in device memory and assemble the batches there "
                        "(csrc/frame_cache.hip); same sampler, jitter, augmentation and crop, so the batches are the host "
                        "loader's.  Data-parallel runs: EVERY rank caches the whole list (the distributed sampler draws "
                        "from all of it each epoch), so the memory is needed per GPU.  Not with --synthetic")
    p.add_argument("--frame_cache_gb", type=float, default=64.,
                   help="--frame_cache device: most GiB of frames + masks one cached list may take per process; a list "
                        "that does not fit is refused before anything is allocated (no fall-back to the host loader)")


def add_bop_flags(p):
    """The flags train_kd.py and test.py share (kd6d/libs/bop_metrics.py)."""
    p.add_argument("--bop_metrics", action="store_true",
                   help="validation additionally scores EVERY object with BOP's MSSD and MSPD (all vertices, exact symmetry "
                        "sets, csrc/bop_err.hip) and reports AR_MSSD, AR_MSPD and their mean; BOP's VSD term is not in that mean "
                        "(--bop_vsd adds it)")
    p.add_argument("--bop_vsd", action="store_true",
                   help="with --bop_metrics: additionally score BOP's VSD term on the device (csrc/bop_vsd.hip: a depth "
                        "rasteriser and the bop19 visibility comparison against the scene's depth/ images; --synthetic "
                        "renders the frame's depth from its ground truth) and report AR_VSD and the three-term AR_BOP")


def check_bop_flags(parser, args):
    """--bop_vsd needs --bop_metrics: AR_BOP is the mean of AR_VSD and the two terms that flag scores."""
    if getattr(args, "bop_vsd", False) and not getattr(args, "bop_metrics", False):
        parser.error("--bop_vsd requires --bop_metrics")


def frame_cache_runtime(args):
    """-> the RUNTIME keys of the two flags; refuses --frame_cache device --synthetic."""
    mode = getattr(args, "frame_cache", "off")
    if mode != "off" and bool(getattr(args, "synthetic", False)):
        raise SystemExit(FRAME_CACHE_SYNTHETIC_ERROR)
    return dict(FRAME_CACHE=mode, FRAME_CACHE_GB=float(getattr(args, "frame_cache_gb", 64.)))


AUG_POSE_REMAP_ERROR = "--aug_pose_remap device needs --augment: without it no pose is remapped"


def aug_pose_remap_runtime(args):
    """-> RUNTIME.AUG_POSE_REMAP; refuses --aug_pose_remap device without --augment."""
    mode = getattr(args, "aug_pose_remap", "host")
    if mode == "device" and not bool(getattr(args, "augment", False)):
        raise ValueError(AUG_POSE_REMAP_ERROR)
    return mode


AUG_CHAIN_ERROR = "--aug_chain full needs --augment: without it no transform chain runs"


def aug_chain_runtime(args):
    """-> the RUNTIME keys of --aug_chain / --aug_background_gb; refuses --aug_chain full without --augment."""
    chain = getattr(args, "aug_chain", "base")
    if chain == "full" and not bool(getattr(args, "augment", False)):
        raise ValueError(AUG_CHAIN_ERROR)
    return dict(AUG_CHAIN=chain, AUG_BACKGROUND_GB=float(getattr(args, "aug_background_gb", 8.)))


def load_yaml(path):
    """yaml -> dict.  A top-level `_BASE_: other.yaml` (path relative to the file; additive key of this build) is
    loaded first and the file's own sections are merged over it key by key."""
    with open(path, "r") as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader) or {}
    base = cfg.pop("_BASE_", None)
    if base is None:
        return cfg
    out = load_yaml(os.path.join(os.path.dirname(os.path.abspath(path)), base))

    def merge(dst, src):
        for k, v in src.items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = v
    merge(out, cfg)
    return out


def _runtime(args, config_file, weight_file):
    return dict(LOCAL_RANK=args.local_rank, CONFIG_FILE=config_file, NUM_WORKERS=args.num_workers,
                WEIGHT_FILE=weight_file, RUNNING_DEVICE=args.running_device, PRECISION=args.precision,
                TEACHER_PNP_GATE=bool(args.teacher_pnp_gate), PNP_SOLVER=getattr(args, "pnp_solver", "host"),
                EVAL_SCORER=getattr(args, "eval_scorer", "host"),
                TWO_LAUNCH_NORM_BWD=bool(args.two_launch_norm_bwd), EXCHANGE=args.exchange,
                RCCL_SINGLE_RANK=bool(getattr(args, "rccl_single_rank", False)),
                BOP_METRICS=bool(getattr(args, "bop_metrics", False)), BOP_VSD=bool(getattr(args, "bop_vsd", False)))


def build_cfgs(args):
    if getattr(args, "kd_per_object", False) and args.teacher_pnp_gate:
        from ..kd_losses import PER_OBJECT_GATE_ERROR
        raise SystemExit(PER_OBJECT_GATE_ERROR)
    cfg = load_yaml(args.config_file)
    cfg["RUNTIME"] = _runtime(args, args.config_file, args.weight_file)
    cfg["RUNTIME"]["WORKING_DIR"] = args.working_dir
    cfg["RUNTIME"]["SYNTHETIC"] = bool(args.synthetic)
    cfg["RUNTIME"]["AUGMENT"] = bool(getattr(args, "augment", False))
    cfg["RUNTIME"]["AUG_POSE_REMAP"] = aug_pose_remap_runtime(args)
    cfg["RUNTIME"].update(aug_chain_runtime(args))
    cfg["RUNTIME"].update(frame_cache_runtime(args))
    cfg["RUNTIME"].update(render_runtime(args))
    cfg["RUNTIME"]["SKIP_TEACHER_EVAL"] = bool(args.skip_teacher_eval)
    cfg["RUNTIME"]["LAUNCH"] = args.launch
    cfg["RUNTIME"]["TEACHER_GROUP"] = max(1, int(args.teacher_group))
    cfg["RUNTIME"]["IMAGE_SIZE"] = int(args.image_size)
    cfg["RUNTIME"]["SYNTHETIC_INSTANCES"] = int(getattr(args, "synthetic_instances", 1))
    if args.mixed_classes is not None:
        cfg["DATASETS"]["MIXED_CLASSES"] = bool(args.mixed_classes)
    cfg["DATASETS"].setdefault("MIXED_CLASSES", False)
    if len(args.test_file) > 0:
        cfg["DATASETS"]["TEST"] = args.test_file
    cfg["MODEL"]["BACKBONE"] = args.backbone
    cfg = custom_cfg(cfg)
    cfg["SOLVER"]["MAX_ITER"] = args.max_iters
    cfg["SOLVER"]["BASE_LR"] = args.base_lr
    if args.batch_size > 0:
        cfg["SOLVER"]["IMS_PER_BATCH"] = args.batch_size
    if args.val_freq > 0:
        cfg["SOLVER"]["VAL_FREQ"] = args.val_freq
    cfg.setdefault("KD", {})
    cfg["KD"]["LOSS_WEIGHT_KD"] = args.kd_weight
    cfg["KD"]["LEVEL"] = args.kd_level
    if cfg["KD"]["LEVEL"] == "pred":
        cfg["KD"].update(GLEVEL=args.glevel, GTYPE=args.gtype, GP=args.p, GBLUR=args.blur, GnD=args.gnD,
                         WEIGHTED_OT=args.weightedOT, DETACH=args.wot_detach, SCALING=args.scaling, REACH=args.reach)
    cfg_t = load_yaml(args.config_file_t)
    cfg_t["RUNTIME"] = _runtime(args, args.config_file_t, args.weight_file_t)
    cfg_t["MODEL"]["BACKBONE"] = args.backbone_t
    cfg_t = custom_cfg(cfg_t)
    cfg_t.setdefault("KD", {})
    if getattr(args, "kd_per_object", False):      # both modules read it: the teacher selects, the student solves per object
        cfg["KD"]["PER_OBJECT"] = True
        cfg_t["KD"]["PER_OBJECT"] = True
    if getattr(args, "kd_kernel_losses", False):   # the student's loss alone reads it
        cfg["KD"]["KERNEL_LOSSES"] = True
    return cfg, cfg_t


def get_args(argv=None):
    parser = get_argparser()
    args = parser.parse_args(argv)
    check_bop_flags(parser, args)
    return build_cfgs(args)
