"""Evaluation entry point -- the reference's test.py:32-137 on the MI355X-native kd6d path: score a saved
checkpoint without starting a training run.

    python test.py --config_file ./configs/ape.yaml --backbone darknet_tiny_h --weight_file outputs/ape/kd/final.pth \
        --working_dir outputs/ape/test/ --pnp_solver device --eval_scorer device [--test_file list.txt | --synthetic]
        [--frame_cache device | --frame_source render] [--bop_metrics [--bop_vsd]] [--bop_csv results.csv]

Builds the network named by --backbone, loads --weight_file (a bare state dict or one under a 'model' key, loosely by
name as the reference does; says whether weights were loaded or are random), builds the valid-style loader over
DATASETS.TEST (--test_file overrides it; --synthetic: the seeded held-out batches train_kd.py validates on) and runs
kd6d.libs.eval_libs.valid().  Writes, under --working_dir,
    preds.json    per image: meta plus the best prediction [score, class, R, T], numpy converted to lists (what the
                  reference's valid() writes, eval_libs.py:96-100)
    metrics.json  the six values valid() returns: per-class ADI / AUC / REP accuracies, ADI / REP per depth bin and
                  the depth range
and prints the per-class ADI / AUC / REP table (utils.py:620-653).

--bop_metrics additionally scores EVERY object (not only the most confident one of an image) with BOP's MSSD and MSPD on
the device (csrc/bop_err.hip: all vertices, the exact symmetry sets of models_info.json or DATASETS.SYMMETRY_TYPES), adds
the recalls and average recalls as "bop" to metrics.json and prints one line per class.  The AR it prints is the mean of
AR_MSSD and AR_MSPD: BOP's third term, VSD, needs depth images and a renderer and is not in it.  --bop_vsd (with
--bop_metrics) scores that term too, on the device (csrc/bop_vsd.hip: a depth rasteriser and the bop19 visibility comparison
against <scene>/depth/<im>.png; --synthetic renders a frame's depth from its ground truth), adds AR_VSD and the three-term
AR_BOP = (AR_VSD + AR_MSSD + AR_MSPD) / 3 to the "bop" block and prints a three-term line instead of the two-term one.
--bop_csv FILE (with or without --bop_metrics, not with --synthetic) writes every kept prediction in the BOP results format
scene_id,im_id,obj_id,score,R,t,time for the official toolkit.

One process: rank 0 evaluates, as valid() does; the reference's multi-process gather of predictions
(libs/train_libs.py accumulate_dicts) is not rebuilt.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "kd-6d-pose-adlp_amd"))

import numpy as np  # noqa: E402


def print_accuracy_per_class(adi_per_class, auc_per_class, rep_per_class):
    """utils.py:620-653: one title line, then one line per class that was seen."""
    assert len(adi_per_class) == len(rep_per_class)
    first = True
    for c, (adi, auc, rep) in enumerate(zip(adi_per_class, auc_per_class, rep_per_class)):
        if len(adi) == 0:
            continue
        if first:
            print("\t" + "".join(k + " " for k in list(adi) + list(auc) + list(rep)))
            first = False
        print("cls_%02d" % c + "".join("\t%.2f" % v for v in list(adi.values()) + list(auc.values()) + list(rep.values())))


def _jsonable(x):
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if hasattr(x, "detach"):
        return x.detach().cpu().tolist()
    return x


def main(argv=None):
    from kd6d.arguments.argument import get_args
    cfg = get_args(argv)
    device = cfg["RUNTIME"]["RUNNING_DEVICE"]
    if device != "cuda":
        raise SystemExit("the kd6d step runs on MI355X only (--running_device cuda); the CPU restatement "
                         "lives in oracle/ and is test infrastructure")
    import torch
    from kd6d.libs.eval_libs import valid
    from kd6d.libs.train_libs import build_model_teacher, build_test_dataset, dataset_meshes
    from kd6d.models.model_kd import PoseModuleKD as PoseModule
    torch.manual_seed(0)
    np.random.seed(0)
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False)
    torch.cuda.set_device(int(cfg["RUNTIME"]["LOCAL_RANK"]))
    wd = cfg["RUNTIME"]["WORKING_DIR"]
    print("working directory: " + wd)
    os.makedirs(wd, exist_ok=True)

    model = build_model_teacher(cfg, PoseModule, device)      # builds the backbone, loads WEIGHT_FILE loosely, says which
    if cfg["RUNTIME"]["SYNTHETIC"]:
        from train_kd import synthetic_valid_loader
        loader, meshes = synthetic_valid_loader(cfg, device)
    elif cfg["RUNTIME"].get("FRAME_SOURCE", "list") == "render":  # the rendered valid list train_kd.py validates on
        if cfg["RUNTIME"].get("BOP_CSV", ""):
            raise SystemExit("--bop_csv cannot be combined with --frame_source render: rendered frames have no BOP scene / image ids")
        from kd6d.libs.train_libs import build_rendered_dataset
        loader = build_rendered_dataset(cfg, device, training=False)[1]
        meshes = dataset_meshes(loader)
    else:
        loader = build_test_dataset(cfg, device, frame_cache=cfg["RUNTIME"].get("FRAME_CACHE", "off"),
                                    frame_cache_gb=cfg["RUNTIME"].get("FRAME_CACHE_GB", 64.))
        meshes = dataset_meshes(loader)

    preds = {}
    want_bop, bop_csv = cfg["RUNTIME"].get("BOP_METRICS", False), cfg["RUNTIME"].get("BOP_CSV", "")
    bop = {} if (want_bop or bop_csv) else None
    vsd = None
    if cfg["RUNTIME"].get("BOP_VSD", False):
        from kd6d.libs.train_libs import vsd_setup
        meshes, vsd = vsd_setup(cfg, loader, meshes, device)
    out = valid(cfg, 0, loader, model, device, meshes, scorer=cfg["RUNTIME"]["EVAL_SCORER"], preds_out=preds, bop=bop,
                **({"vsd": vsd} if vsd is not None else {}))
    every = bop.pop("predictions") if bop is not None else None
    with open(os.path.join(wd, "preds.json"), "w") as f:
        json.dump(_jsonable(preds), f)
    names = ("adi_per_class", "auc_per_class", "rep_per_class", "adi_per_depth", "rep_per_depth", "depth_range")
    metrics = dict(zip(names, out))
    if want_bop:
        metrics["bop"] = bop
    with open(os.path.join(wd, "metrics.json"), "w") as f:
        json.dump(_jsonable(metrics), f, indent=1)
    print("%d images scored (%s scorer, %s PnP)" % (len(preds), cfg["RUNTIME"]["EVAL_SCORER"], cfg["RUNTIME"]["PNP_SOLVER"]))
    print_accuracy_per_class(out[0], out[1], out[2])
    if want_bop:
        from kd6d.libs.bop_metrics import format_ar_bop_line, format_ar_line
        for c, e in enumerate(bop["per_class"]):
            if e and vsd is not None:
                print("bop cls_%02d\tn %d\tAR_VSD %.4f\tAR_MSSD %.4f\tAR_MSPD %.4f"
                      % (c, e["n"], e["AR_VSD"], e["AR_MSSD"], e["AR_MSPD"]))
            elif e:
                print("bop cls_%02d\tn %d\tAR_MSSD %.4f\tAR_MSPD %.4f" % (c, e["n"], e["AR_MSSD"], e["AR_MSPD"]))
        print(format_ar_bop_line(bop) if vsd is not None else format_ar_line(bop))
    if bop_csv:
        from kd6d.libs.bop_metrics import class_object_ids, write_bop_csv
        n = write_bop_csv(bop_csv, every, class_object_ids(cfg["DATASETS"]["MESH_DIR"]))
        print("%d estimates written to %s (BOP results format)" % (n, bop_csv))


if __name__ == "__main__":
    main()
