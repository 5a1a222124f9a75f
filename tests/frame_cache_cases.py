"""Helper of tests/test_frame_cache_host.py and tests/test_frame_cache_gpu.py (not collected): a BOP tree for the
device-resident frame cache.  The meshes, the 3D-box json and a scene of 20 x 24 frames come from
tests/golden/bop_fixture.write_tree; a second scene is added beside it:

  7 frames of 37 x 52 (5772 bytes each, no multiple of 16), 1 to 3 kept instances per frame, among them one 16-bit grey
  frame, one RGBA frame, and one frame whose only object id is unknown (no slot in training, no instance otherwise).

Lists: `list` the 7 frames; `eval_list` the frames whose known objects are of distinct classes (what the entry-point tests
validate on: the evaluator scores one object per class and image);
`small_list` one 20 x 24 frame of the fixture's own scene (the mixed-size refusal)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from bop_fixture import write_tree  # noqa: E402

H, W = 37, 52
# image id -> (kind, object ids).  Ids 1 and 5 have a mesh (classes 0 and 1), 9 has none.
FRAMES = ((1, "rgb", [1, 5, 1]), (2, "rgb", [5]), (3, "grey16", [1, 9]), (4, "rgba", [5, 1]), (5, "rgb", [9]),
          (6, "rgb", [1]), (7, "rgb", [5, 1, 5]))
UNKNOWN_ONLY = 5            # image id of the frame that is unusable in training
EVAL_IDS = [2, 3, 4, 6]     # at least one known object, no class twice
INTERNAL_K = [572.4, 0, 26.0, 0, 573.6, 18.0, 0, 0, 1]


def write_cache_tree(root, size=(H, W)):
    """-> dict: list / eval_list / small_list files, models, bbox, the scene directory, the frames as written."""
    from PIL import Image
    base = write_tree(root)
    h, w = size
    rng = np.random.default_rng(11)
    scene = os.path.join(root, "train", "000002")
    os.makedirs(os.path.join(scene, "rgb")); os.makedirs(os.path.join(scene, "mask_visib"))
    cam, gt, written = {}, {}, {}
    for im_id, kind, objs in FRAMES:
        name = os.path.join(scene, "rgb", "%06d.png" % im_id)
        if kind == "rgb":
            arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            Image.fromarray(arr, "RGB").save(name)
        elif kind == "grey16":
            arr = rng.integers(0, 65536, (h, w), dtype=np.uint16)
            Image.fromarray(arr).save(name)
        else:
            arr = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            arr[:, :, 3] = np.where(rng.random((h, w)) < 0.3, 0, 255)
            Image.fromarray(arr, "RGBA").save(name)
        written[im_id] = arr
        cam[str(im_id)] = {"cam_K": [572.4, 0, 0.5 * w + 0.25 * im_id, 0, 573.6, 0.5 * h - 0.5 * im_id, 0, 0, 1],
                           "depth_scale": 1.0}
        gt[str(im_id)] = []
        for k, oid in enumerate(objs):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            gt[str(im_id)].append({"cam_R_m2c": q.reshape(-1).tolist(),
                                   "cam_t_m2c": [float(rng.normal(0, 8)), float(rng.normal(0, 6)), 900.0 + 40.0 * k],
                                   "obj_id": oid})
            m = np.zeros((h, w), np.uint8)
            y0, x0 = (3 + 9 * k) * h // H, (2 + 13 * k) * w // W
            m[y0:y0 + 14 * h // H, x0:x0 + 20 * w // W] = 255
            Image.fromarray(m, "L").save(os.path.join(scene, "mask_visib", "%06d_%06d.png" % (im_id, k)))
    json.dump(cam, open(os.path.join(scene, "scene_camera.json"), "w"))
    json.dump(gt, open(os.path.join(scene, "scene_gt.json"), "w"))
    train = os.path.join(root, "train")
    lists = {}
    for key, ids in (("list", [f[0] for f in FRAMES]), ("eval_list", EVAL_IDS)):
        lists[key] = os.path.join(train, "cache_%s.txt" % key)
        with open(lists[key], "w") as f:
            f.write("".join("000002/rgb/%06d.png\n" % i for i in ids))
    lists["small_list"] = os.path.join(train, "cache_small_list.txt")
    with open(lists["small_list"], "w") as f:
        f.write("000001/rgb/000003.png\n")
    return dict(lists, models=base["models"], bbox=base["bbox"], scene=scene, frames=written, gt=gt, cam=cam, H=h, W=w,
                small_path=os.path.join(base["scene"], "rgb", "000003.png"))


def make_cfg(tree, batch=3, augment=False):
    """configs/ape.yaml on the helper tree: frames already at the internal resolution; with `augment` the keys
    train_kd.py --augment accepts (no background directory, no sharpening), an INTERNAL_K close to the cameras but not
    equal (Resize is a real warp)."""
    import yaml
    from kd6d.arguments.argument import custom_cfg
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["RUNTIME"] = {"PRECISION": "fp32", "N_GPU": 1, "DISTRIBUTED": False, "NUM_WORKERS": 0}
    cfg["MODEL"]["BACKBONE"] = "darknet_tiny_h"
    cfg = custom_cfg(cfg)
    cfg["DATASETS"].update(TRAIN=tree["list"], VALID=tree["list"], TEST=tree["eval_list"], MESH_DIR=tree["models"],
                           BBOX_FILE=tree["bbox"], N_CLASS=3, SYMMETRY_TYPES={})
    cfg["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=list(INTERNAL_K))
    cfg["SOLVER"]["IMS_PER_BATCH"] = batch
    if augment:
        cfg["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2,
                             AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05,
                             AUGMENTATION_Grayscalize=False, AUGMENTATION_Sharpen=0, AUGMENTATION_BACKGROUND_DIR=None)
    return cfg


def datasets(tree, training=True, key="list"):
    from kd6d.libs.dataset import BOP_Dataset
    return BOP_Dataset(tree[key], tree["models"], tree["bbox"], training=training)
