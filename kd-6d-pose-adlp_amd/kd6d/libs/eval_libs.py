"""Validation loop of the evaluation path: libs/eval_libs.py:44-110 of the reference without its dataset side.

`valid()` runs the model in eval mode over a loader of (images, targets, meta_infos), keeps the most confident
pose per image (`new_p[0][:-1]`: score, class, R, T -- the 2D points are dropped as in the reference) and scores
the collection with `evaluate_pose_predictions`.  As in eval_libs.py:69-76 every prediction is first re-solved for the
frame's own camera (`remap_predictions`: identity when the frame carries the internal camera, which is what the
synthetic loaders and frames stored at the internal resolution do).  Meshes are passed in by the caller
(kd6d.libs.train_libs.dataset_meshes / the synthetic loaders).
"""
import numpy as np
import torch

from .distributed import get_rank
from .evaluate import evaluate_pose_predictions, evaluate_pose_predictions_device, remap_predictions

SCORERS = ("host", "device")


class _Mesh:
    def __init__(self, vertices):
        self.vertices = np.asarray(vertices)


@torch.no_grad()
def valid(cfg, steps, loader, model, device, meshes, logger=None, scorer="host", preds_out=None, vsd=None, bop=None):
    """meshes: per class id an (n,3) vertex array (or an object with `.vertices`).  -> the 6-tuple of
    evaluate_pose_predictions on rank 0, None elsewhere.
    scorer: "host" scores object by object in float64 numpy (evaluate_pose_predictions); "device" scores every object of
    the run in one kd6d_pose_errors launch (evaluate_pose_predictions_device).  preds_out: a dict that receives the
    collected {path: {'meta', 'pred'}} entries (what the reference's valid() writes to preds.json).
    bop: a dict (train_kd.py / test.py --bop_metrics), or None.  With a dict valid() ADDITIONALLY keeps every remapped
    prediction [score, class, R, T] of every image -- scoring needs each object's pose, not only the most confident one
    of the image -- in a side collection, scores it on rank 0 with kd6d_bop_errors (csrc/bop_err.hip; always the device,
    whatever `scorer` says) and fills the dict with bop_metrics.bop_tables' MSSD / MSPD recalls and average recalls, plus
    the side collection itself under "predictions".  It logs BOP/AR_MSSD, BOP/AR_MSPD and BOP/AR.  The AR has two terms:
    BOP's VSD term is not in it.  The return value and preds_out are the same with and without it.
    vsd: a depth provider (train_kd.py / test.py --bop_vsd), or None; needs `bop`.  depth_fn(meta) -> the frame's (H, W)
    depth image in mm, 0 = missing (dataset.load_depth_mm of meta["path"], or bop_metrics.rendered_depth_provider for
    the synthetic loaders); the meshes then carry `.faces`.  valid() scores BOP's VSD of every object on the device
    (csrc/bop_vsd.hip, bop_metrics.evaluate_bop_vsd) and ADDS to the dict: vsd_thresholds, AR_VSD per class and over
    the run, AR_BOP = (AR_VSD + AR_MSSD + AR_MSPD) / 3 and AR_BOP_note; it logs BOP/AR_VSD and BOP/AR_BOP.  The existing
    keys are untouched: "AR" stays the two-term mean with its note.  (Both are passed by keyword; `bop` stays the last
    parameter of the signature.)"""
    if vsd is not None and bop is None:
        raise ValueError("valid(): vsd needs bop={} (AR_BOP is the mean of AR_VSD, AR_MSSD and AR_MSPD)")
    if scorer not in SCORERS:
        raise ValueError("valid(): scorer=%r (one of %s)" % (scorer, ", ".join(SCORERS)))
    was_training = model.training
    model.eval()
    preds, every = {}, {}
    for images, targets, meta_infos in loader:
        if hasattr(images, "to"):
            images = images.to(device)
        pred, _ = model(images, targets=targets)
        for m, p in zip(meta_infos, pred):
            if len(p) and "K" in m and cfg.get("INPUT", {}).get("INTERNAL_K") is not None and \
                    not np.allclose(np.asarray(m["K"], np.float64).reshape(3, 3),
                                    np.asarray(cfg["INPUT"]["INTERNAL_K"], np.float64).reshape(3, 3)):
                kp3d = targets.kp3d[0].cpu().numpy() if hasattr(targets, "kp3d") else None     # (n_class, 8, 3) box corners
                if kp3d is not None:            # eval_libs.py:71-76: poses solved for the internal camera -> the frame's own
                    p = remap_predictions(cfg["INPUT"]["INTERNAL_K"], cfg["INPUT"].get("INTERNAL_WIDTH"),
                                          cfg["INPUT"].get("INTERNAL_HEIGHT"), kp3d, m, p)
            best = [list(p[0][:-1])] if len(p) else []
            preds[m["path"]] = {"meta": m, "pred": best}
            if bop is not None:
                every[m["path"]] = {"meta": m, "pred": [list(q[:4]) for q in p]}
    model.train(was_training)
    if preds_out is not None:
        preds_out.update(preds)
    if bop is not None:
        bop["predictions"] = every
    if get_rank() != 0:
        return None
    ms = [m if hasattr(m, "vertices") else _Mesh(m) for m in meshes]
    if bop is not None:
        from . import bop_metrics as B
        n_cls = cfg["DATASETS"]["N_CLASS"] - 1
        bop.update(B.evaluate_bop_predictions(every, cfg["DATASETS"]["N_CLASS"], ms, cfg["DATASETS"]["MESH_DIAMETERS"],
                                              B.dataset_symmetry_sets(cfg["DATASETS"], n_cls), device))
        if logger is not None:
            for k in ("AR_MSSD", "AR_MSPD", "AR"):
                logger.add_scalar("BOP/" + k, bop[k], steps)
        if vsd is not None:
            B.add_vsd_tables(bop, B.evaluate_bop_vsd(every, cfg["DATASETS"]["N_CLASS"], ms,
                                                     cfg["DATASETS"]["MESH_DIAMETERS"], vsd, device))
            if logger is not None:
                for k in ("AR_VSD", "AR_BOP"):
                    logger.add_scalar("BOP/" + k, bop[k], steps)
    if scorer == "device":
        out = evaluate_pose_predictions_device(preds, cfg["DATASETS"]["N_CLASS"], ms, cfg["DATASETS"]["MESH_DIAMETERS"],
                                               cfg["DATASETS"].get("SYMMETRY_TYPES", {}), device)
    else:
        out = evaluate_pose_predictions(preds, cfg["DATASETS"]["N_CLASS"], ms, cfg["DATASETS"]["MESH_DIAMETERS"],
                                        cfg["DATASETS"].get("SYMMETRY_TYPES", {}))
    if logger is not None:            # eval_libs.py:112-146 of the reference: per class, then the mean over classes seen
        all_adi, all_rep, n_valid = {}, {}, 0
        for i, (adi, rep) in enumerate(zip(out[0], out[2])):
            if adi:
                logger.add_scalars("ADI/class_%02d" % i, adi, steps)
                logger.add_scalars("REP/class_%02d" % i, rep, steps)
                for k, v in adi.items():
                    all_adi[k] = all_adi.get(k, 0.0) + v
                for k, v in rep.items():
                    all_rep[k] = all_rep.get(k, 0.0) + v
                n_valid += 1
        if n_valid:
            logger.add_scalars("ADI/all_class", {k: v / n_valid for k, v in all_adi.items()}, steps)
            logger.add_scalars("REP/all_class", {k: v / n_valid for k, v in all_rep.items()}, steps)
    return out
