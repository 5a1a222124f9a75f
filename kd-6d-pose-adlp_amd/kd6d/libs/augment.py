"""Train-time augmentation of full frames (`train_kd.py --augment`): the reference's train transform chain
(libs/train_libs.py:212-238) and its post-transform block (dataset.py:166-176), in the reference's order:

  1 Resize                  M = INTERNAL_K K^-1; skipped when M is the identity (then a cv2 warp is an exact copy)
  2 RandomOcclusion         AUGMENTATION_OCCLUSION
  2b RandomBackground       AUGMENTATION_BACKGROUND_DIR (--aug_chain full only)
  3 RandomShiftScaleRotate  AUGMENTATION_SHIFT / _SCALE / _ROTATION
  4 RandomHSV               AUGMENTATION_ColorH / _ColorS / _ColorV
  4b RandomPencilSharpen    AUGMENTATION_Sharpen (--aug_chain full only)
  5 RandomSmooth            AUGMENTATION_Smooth (largest box size)
  6 RandomNoise             AUGMENTATION_Noise
  7 Grayscalize             AUGMENTATION_Grayscalize
  8 remove_invalids(10)     instances under 10 visible pixels are dropped, mask ids renumbered 1..k
  9 symmetry_handling       DATASETS.SYMMETRY_TYPES

Split of the work:
  * dataset item (`draw_params`, worker process): every scalar parameter, drawn with `random` as the reference
    draws them, plus a 64-bit key for the per-pixel randomness; the two pose remaps (Resize, then SSR) with
    kd6d.libs.pnp.remap_pose.  Occlusion takes a fixed block of five random.random() per instance slot; the device
    maps them with random.uniform's own formula a + (b - a) u.
  * `AugmentFront.run` (DziLoader, GPU): the pixel work in csrc/augment.hip, one readback of the (B, n) area table
    (waited on with an event of the front-end's stream), the drop / relabel decision, symmetry handling.
  * RUNTIME.AUG_POSE_REMAP = "device" (train_kd.py --aug_pose_remap device): `draw_params` solves nothing -- it records
    the source poses in double (`pose_src`) and draws exactly what it draws otherwise -- and `AugmentFront.run` starts
    with ONE kd6d_pose_remap launch (csrc/pnp.hip: one lane per instance, both remaps chained) whose result comes back
    with the area table, behind the same single wait.  The poses agree with the host solver's to well under 1e-3
    projected px (profiles/aug_pose_remap.md); frames and masks do not depend on them.

Deviations from the reference:
  * the remap of an instance uses the 8 box corners of its CLASS (keypoints_3d[class_ids[i]]); PoseAnnot.transform
    passes keypoints_3d[i], indexed by instance, which is only the class's box for class 0;
  * an image that keeps no instance after the chain falls back to its frame after Resize only, with its
    Resize-remapped pose (the reference draws another image instead);
  * per-pixel random bytes / noise come from a counter-based hash on the device, not numpy's stream.
RandomBackground and RandomPencilSharpen are opt-in: RUNTIME.AUG_CHAIN = "full" (train_kd.py --aug_chain full).  On the
default "base" chain enabling them still raises NotImplementedError, and nothing is drawn for them.  On the full chain:
  * `draw_params` draws, per item, RandomBackground's coin from numpy's global stream and its file index from `random`
    (after the occlusion block), and RandomPencilSharpen's test, box size, mode and alpha from `random` (after HSV);
  * `AugmentFront` decodes the background directory ONCE into a BackgroundPool (device memory, native sizes, budget
    RUNTIME.AUG_BACKGROUND_GB) and kd6d_aug_background resizes while it samples; kd6d_aug_sharpen is the LDS-tiled
    box filter with the two whole-image min-max normalisations;
  * deviations: the directory is listed sorted and joined with os.path.join (the reference concatenates dir + name in
    os.listdir order); a missing or empty directory is an error (the reference silently disables the stage); a file
    that cannot be decoded is an error naming it (the reference draws another file); frames are 3-channel here (the
    dataset's clean-up drops alpha), so the alpha-channel merge is not built; the resize stays bilinear at an exact 2x
    downscale, where cv2 switches INTER_LINEAR to its area path; AUGMENTATION_Sharpen = 0 draws nothing (the reference
    draws one random.random() and discards it).
Both are restatements like warp / HSV / blur: parity unpinned at the cv2 boundary (tests/augment_full_ref.py).
"""
import os
import random

import numpy as np
import torch

from .._lib import AUG_MAX_ID, MAX_GT
from .pnp import remap_pose

MIN_AREA = 10
POSE_REMAP_MODES = ("host", "device")
AUG_CHAINS = ("base", "full")
BACKGROUND_EXTS = (".png", ".jpg")
SHARPEN_KS = (5, 7, 9, 11)            # RandomPencilSharpen's ks_candidates


def list_backgrounds(directory):
    """The .png / .jpg file names of a background directory, sorted (names only).  Missing or empty: ValueError."""
    if not os.path.isdir(directory):
        raise ValueError("SOLVER.AUGMENTATION_BACKGROUND_DIR: %s is not a directory" % (directory,))
    names = sorted(f for f in os.listdir(directory) if f.endswith(BACKGROUND_EXTS))
    if not names:
        raise ValueError("SOLVER.AUGMENTATION_BACKGROUND_DIR: %s holds no .png / .jpg file" % (directory,))
    return names


class AugConfig:
    """The augmentation keys of a yaml, with the reference's own enable guards.  RUNTIME.AUG_CHAIN (train_kd.py
    --aug_chain): "base" (default, also when RUNTIME or the key is absent) refuses AUGMENTATION_BACKGROUND_DIR and
    AUGMENTATION_Sharpen; "full" honours them (None / 0 = that stage off).  The object holds names and numbers only,
    so it pickles into loader workers; the pixels of the backgrounds live in AugmentFront's BackgroundPool."""

    def __init__(self, cfg):
        s, inp = cfg["SOLVER"], cfg["INPUT"]
        rt = cfg.get("RUNTIME") or {}
        self.chain = rt.get("AUG_CHAIN", "base") or "base"
        if self.chain not in AUG_CHAINS:
            raise ValueError("RUNTIME.AUG_CHAIN must be one of %s (got %r)" % (AUG_CHAINS, self.chain))
        bg_dir, sharpen = s.get("AUGMENTATION_BACKGROUND_DIR"), s.get("AUGMENTATION_Sharpen", 0)
        if self.chain == "base":
            if bg_dir is not None:
                raise NotImplementedError("SOLVER.AUGMENTATION_BACKGROUND_DIR: RandomBackground is not rebuilt "
                                          "for --augment on the base chain; pass --aug_chain full")
            if sharpen:
                raise NotImplementedError("SOLVER.AUGMENTATION_Sharpen: RandomPencilSharpen is not rebuilt for --augment "
                                          "on the base chain; pass --aug_chain full")
        self.background_dir, self.background_files = None, []
        if bg_dir is not None:
            self.background_dir = str(bg_dir)
            self.background_files = list_backgrounds(self.background_dir)
        self.background_gb = float(rt.get("AUG_BACKGROUND_GB", 8.))
        self.sharpen = float(sharpen or 0)
        self.K = np.array(inp["INTERNAL_K"], np.float64).reshape(3, 3)
        self.width, self.height = int(inp["INTERNAL_WIDTH"]), int(inp["INTERNAL_HEIGHT"])
        self.occlusion = float(s.get("AUGMENTATION_OCCLUSION", 0) or 0)
        self.shift = float(s.get("AUGMENTATION_SHIFT", 0) or 0)
        self.scale = float(s.get("AUGMENTATION_SCALE", 0) or 0)
        self.rotation = float(s.get("AUGMENTATION_ROTATION", 0) or 0)
        self.hsv = tuple(float(s.get(k, 0) or 0) for k in ("AUGMENTATION_ColorH", "AUGMENTATION_ColorS",
                                                            "AUGMENTATION_ColorV"))
        self.smooth = int(s.get("AUGMENTATION_Smooth", 0) or 0)
        self.noise = float(s.get("AUGMENTATION_Noise", 0) or 0)
        self.gray = bool(s.get("AUGMENTATION_Grayscalize", False))
        self.symmetry_types = cfg["DATASETS"].get("SYMMETRY_TYPES") or {}
        self.pose_remap = (cfg.get("RUNTIME") or {}).get("AUG_POSE_REMAP", "host")
        if self.pose_remap not in POSE_REMAP_MODES:
            raise ValueError("RUNTIME.AUG_POSE_REMAP must be one of %s (got %r)" % (POSE_REMAP_MODES, self.pose_remap))

    # the guards of transform.py
    @property
    def occlusion_on(self):
        return self.occlusion > 0

    @property
    def background_on(self):
        return len(self.background_files) > 0

    @property
    def sharpen_on(self):
        return self.sharpen > 0

    @property
    def ssr_on(self):
        return (self.shift + self.scale + self.rotation) > 0.01

    @property
    def hsv_on(self):
        return sum(self.hsv) > 0.01

    @property
    def smooth_on(self):
        return self.smooth > 1

    @property
    def noise_on(self):
        return self.noise > 0.01


def resize_matrix(dst_K, src_K):
    """transform.Resize: M = dst_K inv(src_K) (3x3, float64)."""
    return np.matmul(np.asarray(dst_K, np.float64).reshape(3, 3), np.linalg.inv(np.asarray(src_K, np.float64).reshape(3, 3)))


def is_identity_warp(M, width, height, tol=1e-6):
    """True when M moves no pixel of a width x height frame by more than tol px (far below cv2's 1/1024 px step):
    the cv2 8-bit warp is then an exact copy."""
    M = np.asarray(M, np.float64)
    pts = np.array([[0, 0, 1], [width, 0, 1], [0, height, 1], [width, height, 1]], np.float64).T
    return bool(np.abs(M[:2] @ pts - pts[:2]).max() < tol)


def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D from its documented formula (degrees, counter-clockwise)."""
    a = np.deg2rad(angle)
    alpha, beta = np.cos(a) * scale, np.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy], [-beta, alpha, beta * cx + (1 - alpha) * cy]])


def shift_scale_rotate_matrix(shift_limit, scale_limit, rotate_limit, width, height, rng=random):
    """utils.py:161-179 generate_shiftscalerotate_matrix: draws randint, randint, uniform, uniform in that order;
    3x3, cast to float32 like the reference."""
    dw, dh = int(width * shift_limit), int(height * shift_limit)
    pleft = rng.randint(-dw, dw)
    ptop = rng.randint(-dh, dh)
    shiftM = np.array([[1.0, 0.0, -pleft], [0.0, 1.0, -ptop], [0.0, 0.0, 1.0]])
    cx, cy = width / 2, height / 2
    ang = rng.uniform(-rotate_limit, rotate_limit)
    sfactor = rng.uniform(-scale_limit, +scale_limit) + 1
    rsM = np.concatenate((rotation_matrix_2d((cx, cy), ang, sfactor), [[0, 0, 1]]), axis=0)
    return np.matmul(rsM, shiftM).astype(np.float32)


def remap_poses(K, class_ids, rotations, translations, bbox_3d, dst_K, M):
    """PoseAnnot.transform's pose part with the CLASS's box corners as the remap points."""
    Rs, Ts = [], []
    for i, c in enumerate(class_ids):
        R, T, _ = remap_pose(K, rotations[i], translations[i], np.asarray(bbox_3d[int(c)], np.float64), dst_K,
                             np.asarray(M, np.float64))
        Rs.append(np.asarray(R, np.float32).reshape(3, 3))
        Ts.append(np.asarray(T, np.float32).reshape(3, 1))
    return np.asarray(Rs, np.float32).reshape(-1, 3, 3), np.asarray(Ts, np.float32).reshape(-1, 3, 1)


def draw_params(ac, K, class_ids, rotations, translations, bbox_3d, rng=random, np_rng=np.random):
    """Everything random of one item, in the chain's order, and the two pose remaps.  -> dict.
    ac.pose_remap == "device": no remap is solved here; the item carries its source poses in double (`pose_src`) for
    kd6d_pose_remap instead of R_resize / T_resize / R / T.  The draws are the same, in the same order.
    np_rng: RandomBackground's coin comes from numpy's global stream in the reference (np.random.rand), its file
    index from `random`.  With both stages of the full chain off nothing is drawn for them."""
    n = len(class_ids)
    if n > AUG_MAX_ID:
        raise ValueError("--augment handles at most %d instances per frame (got %d)" % (AUG_MAX_ID, n))
    on_device = ac.pose_remap == "device"
    p = {}
    Mr = resize_matrix(ac.K, K)
    p["M_resize"] = Mr[:2].copy()
    if on_device:
        p["pose_src"] = {"K": np.asarray(K, np.float64).reshape(3, 3).copy(),
                         "class_ids": np.asarray(class_ids, np.int64).reshape(n),
                         "rotations": np.asarray(rotations, np.float64).reshape(n, 3, 3).copy(),
                         "translations": np.asarray(translations, np.float64).reshape(n, 3).copy()}
    else:
        p["R_resize"], p["T_resize"] = remap_poses(K, class_ids, rotations, translations, bbox_3d, ac.K, Mr)
    if ac.occlusion_on:
        p["occl_u"] = np.array([[rng.random() for _ in range(5)] for _ in range(MAX_GT)], np.float64)
    if ac.background_on:
        coin = np_rng.rand()
        p["bg"] = rng.randint(0, len(ac.background_files) - 1) if coin < 0.5 else -1
    if ac.ssr_on:
        Ms = shift_scale_rotate_matrix(ac.shift, ac.scale, ac.rotation, ac.width, ac.height, rng)
        p["M_ssr"] = Ms[:2].astype(np.float64)
        if not on_device:
            p["R"], p["T"] = remap_poses(ac.K, class_ids, p["R_resize"], p["T_resize"], bbox_3d, ac.K, Ms)
    elif not on_device:
        p["R"], p["T"] = p["R_resize"], p["T_resize"]
    if ac.hsv_on:
        p["hsv"] = np.array([rng.uniform(-1, 1) * r + 1 for r in ac.hsv], np.float32)
    if ac.sharpen_on:
        p["sharpen_ks"], p["sharpen_mode"], p["sharpen_alpha"] = 0, 0, 0.0
        if rng.random() < ac.sharpen:
            p["sharpen_ks"] = rng.choice(list(SHARPEN_KS))
            p["sharpen_mode"] = int(rng.random() < 0.5)          # 1: edge = img / blur, 0: img - blur
            p["sharpen_alpha"] = rng.uniform(0.5, 0.95)
    if ac.smooth_on:
        p["ksize"] = rng.choice(list(range(1, ac.smooth + 1, 2)))
    if ac.noise_on:
        p["sigma"] = rng.uniform(0, ac.noise)
    p["key"] = rng.getrandbits(64)
    p["n"] = n
    return p


def collate_params(ps):
    """list of draw_params dicts -> one dict of stacked arrays (per-instance poses stay lists).  Items drawn for the
    device remap: `pose_src` = the instances of the batch, image after image, in kd6d_pose_remap's arrays -- inst_img,
    inst_cls (n_inst,) int32, src_K (B, 9), src_R (n_inst, 9), src_T (n_inst, 3) float64 -- and start (B + 1,): image
    b owns instances start[b] ... start[b + 1] - 1."""
    out = {"M_resize": np.stack([p["M_resize"] for p in ps]), "n": np.array([p["n"] for p in ps], np.int32),
           "key": np.array([p["key"] for p in ps], np.uint64)}
    if "pose_src" in ps[0]:
        src = [p["pose_src"] for p in ps]
        cnt = [len(q["class_ids"]) for q in src]
        out["pose_src"] = {
            "inst_img": np.repeat(np.arange(len(ps), dtype=np.int32), cnt),
            "inst_cls": np.concatenate([q["class_ids"] for q in src]).astype(np.int32),
            "src_K": np.stack([q["K"].reshape(9) for q in src]).astype(np.float64),
            "src_R": np.concatenate([q["rotations"].reshape(-1, 9) for q in src]).astype(np.float64),
            "src_T": np.concatenate([q["translations"].reshape(-1, 3) for q in src]).astype(np.float64),
            "start": np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)}
    else:
        for k in ("R_resize", "T_resize", "R", "T"):
            out[k] = [p[k] for p in ps]
    if "occl_u" in ps[0]:
        out["occl_u"] = np.stack([p["occl_u"] for p in ps])
    if "M_ssr" in ps[0]:
        out["M_ssr"] = np.stack([p["M_ssr"] for p in ps])
    if "hsv" in ps[0]:
        out["hsv"] = np.stack([p["hsv"] for p in ps]).astype(np.float32)
    if "ksize" in ps[0]:
        out["ksize"] = np.array([p["ksize"] for p in ps], np.int32)
    if "sigma" in ps[0]:
        out["sigma"] = np.array([p["sigma"] for p in ps], np.float32)
    if "bg" in ps[0]:
        out["bg"] = np.array([p["bg"] for p in ps], np.int32)
    if "sharpen_ks" in ps[0]:
        out["sharpen_ks"] = np.array([p["sharpen_ks"] for p in ps], np.int32)
        out["sharpen_mode"] = np.array([p["sharpen_mode"] for p in ps], np.int32)
        out["sharpen_alpha"] = np.array([p["sharpen_alpha"] for p in ps], np.float64)
    return out


def batch_key(keys):
    """One 64-bit launch key from the items' keys (the device hash also mixes in the image index)."""
    k = 0
    for v in np.asarray(keys, np.uint64).tolist():
        k = (k * 0x100000001B3 ^ int(v)) & 0xFFFFFFFFFFFFFFFF
    return k


# ---- thin launch wrappers (device tensors in, asynchronous on the current stream) --------------------------------
def _dev(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dtype, non_blocking=False).contiguous()


def warp(frames, masks, mats, out_hw):
    """frames (B,H,W,3) uint8, masks (B,H,W) float32 or None, mats (B,2,3) forward matrices (host) -> warped."""
    from .. import ops
    from ..ops import check, lib
    B, H, W, _ = frames.shape
    Ho, Wo = out_hw
    dev = frames.device
    m = _dev(np.asarray(mats, np.float64).reshape(B, 6), torch.float64, dev)
    out = torch.empty(B, Ho, Wo, 3, dtype=torch.uint8, device=dev)
    mout = torch.empty(B, Ho, Wo, dtype=torch.float32, device=dev) if masks is not None else None
    check(lib.kd6d_aug_warp_u8(ops._ptr(frames), ops._ptr(masks), B, H, W, ops._ptr(m), Ho, Wo, ops._ptr(out),
                               ops._ptr(mout), ops._stream()), "kd6d_aug_warp_u8")
    return out, mout


def mask_stats(masks, max_id):
    """-> (B, max_id, 5) int32 device tensor {area, xmin, ymin, xmax, ymax}."""
    from .. import ops
    from ..ops import check, lib
    B, H, W = masks.shape
    st = torch.empty(B, max_id, 5, dtype=torch.int32, device=masks.device)
    check(lib.kd6d_aug_mask_stats(ops._ptr(masks), B, H, W, max_id, ops._ptr(st), ops._stream()), "kd6d_aug_mask_stats")
    return st


def occlude(frames, masks, stats, uniforms, n_inst, prob, key):
    """In place.  uniforms (B, MAX_GT, 5) host, n_inst (B,) host."""
    from .. import ops
    from ..ops import check, lib
    B, H, W, _ = frames.shape
    dev = frames.device
    u = _dev(np.asarray(uniforms, np.float64).reshape(B, MAX_GT, 5), torch.float64, dev)
    n = _dev(np.asarray(n_inst, np.int32).reshape(B), torch.int32, dev)
    check(lib.kd6d_aug_occlude(ops._ptr(frames), ops._ptr(masks), B, H, W, ops._ptr(stats), stats.shape[1], ops._ptr(u),
                               ops._ptr(n), float(prob), int(key), ops._stream()), "kd6d_aug_occlude")


def hsv(frames, factors):
    """In place.  factors (B,3) float32 host."""
    from .. import ops
    from ..ops import check, lib
    B, H, W, _ = frames.shape
    f = _dev(np.asarray(factors, np.float32).reshape(B, 3), torch.float32, frames.device)
    check(lib.kd6d_aug_hsv(ops._ptr(frames), B, H, W, ops._ptr(f), ops._stream()), "kd6d_aug_hsv")


def filt(frames, ksize=None, sigma=None, gray=False, key=0):
    """-> new buffer: blur (ksize (B,) or None), noise (sigma (B,) or None), grayscale."""
    from .. import ops
    from ..ops import check, lib
    B, H, W, _ = frames.shape
    dev = frames.device
    k = _dev(np.asarray(ksize, np.int32).reshape(B), torch.int32, dev) if ksize is not None else None
    s = _dev(np.asarray(sigma, np.float32).reshape(B), torch.float32, dev) if sigma is not None else None
    out = torch.empty_like(frames)
    check(lib.kd6d_aug_filter(ops._ptr(frames), ops._ptr(out), B, H, W, ops._ptr(k), ops._ptr(s), int(bool(gray)),
                              int(key), ops._stream()), "kd6d_aug_filter")
    return out


def background(frames, masks, pool, bg_index):
    """In place on frames (masks are read).  pool: a BackgroundPool on the frames' device; bg_index (B,) host ints, -1 =
    this image keeps its pixels, i = every mask == 0 pixel takes background i resized to the frame."""
    from .. import ops
    from ..ops import check, lib
    B, H, W, _ = frames.shape
    idx = np.asarray(bg_index, np.int64).reshape(B)
    if ((idx < -1) | (idx >= pool.n)).any():
        raise ValueError("background index outside [-1, %d): %s" % (pool.n, idx.tolist()))
    i = _dev(idx.astype(np.int32), torch.int32, frames.device)
    check(lib.kd6d_aug_background(ops._ptr(frames), ops._ptr(masks), B, H, W, ops._ptr(pool.pool), pool.nbytes,
                                  ops._ptr(pool.off), ops._ptr(pool.hw), pool.n, ops._ptr(i), ops._stream()),
          "kd6d_aug_background")


def sharpen(frames, ks, mode, alpha):
    """-> new buffer.  ks (B,) host ints in {0, 5, 7, 9, 11} (0 = copy), mode (B,) (non-zero = ratio), alpha (B,)."""
    from .. import ops
    from ..ops import check, lib
    B, H, W, _ = frames.shape
    dev = frames.device
    ks = np.asarray(ks, np.int32).reshape(B)
    if not np.isin(ks, (0,) + SHARPEN_KS).all():
        raise ValueError("sharpen box sizes must be 0 or one of %s (got %s)" % (SHARPEN_KS, ks.tolist()))
    km = _dev(np.concatenate([ks, np.asarray(mode, np.int32).reshape(B)]), torch.int32, dev)
    a = _dev(np.asarray(alpha, np.float64).reshape(B), torch.float64, dev)
    nws = int(lib.kd6d_aug_sharpen_ws_bytes(B))
    ws = torch.empty((nws + 7) // 8, dtype=torch.int64, device=dev)
    out = torch.empty_like(frames)
    check(lib.kd6d_aug_sharpen(ops._ptr(frames), ops._ptr(out), B, H, W, ops._ptr(km[:B]), ops._ptr(km[B:]), ops._ptr(a),
                               ops._ptr(ws), ws.numel() * 8, ops._stream()), "kd6d_aug_sharpen")
    return out


def relabel(masks, lut):
    """In place.  lut (B, max_id + 1) host float32."""
    from .. import ops
    from ..ops import check, lib
    B, H, W = masks.shape
    lut = np.asarray(lut, np.float32)
    L = _dev(lut, torch.float32, masks.device)
    check(lib.kd6d_aug_relabel(ops._ptr(masks), B, H, W, ops._ptr(L), lut.shape[1] - 1, ops._stream()),
          "kd6d_aug_relabel")


def _probe_background(path):
    """(h, w) of an image file from its header (Pillow opens lazily)."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return int(h), int(w)


def _decode_background(path):
    """One background as the frames are: Pillow decode + BOP_Dataset's frame clean-up -> (h, w, 3) BGR uint8."""
    from .dataset import load_image_cached, normalise_frame
    img = load_image_cached(path, None)
    if img is None:
        raise ValueError("background image %s cannot be decoded" % path)
    return np.ascontiguousarray(normalise_frame(img)[:, :, :3])


class BackgroundPool:
    """The backgrounds of RandomBackground on the device, decoded ONCE and kept at their native sizes in one packed
    uint8 buffer (`pool`, BGR, image after image, no padding) with an (n, 2) int32 table of (h, w) (`hw`) and an (n,)
    int64 table of byte offsets (`off`); kd6d_aug_background resizes while it samples.  Built once per process by
    AugmentFront (under torch.distributed every rank holds its own).  A pool over budget_bytes is refused before
    anything is decoded or allocated; a file that cannot be read is an error naming it (the reference draws another
    file instead).  probe(path) -> (h, w) and decode(path) -> (h, w, 3) uint8 can be replaced (tests)."""

    def __init__(self, directory, names, device, budget_bytes, probe=None, decode=None):
        probe, decode = probe or _probe_background, decode or _decode_background
        paths = [os.path.join(directory, n) for n in names]
        hw, off, total = self.plan(paths, budget_bytes, probe)
        buf = np.empty(total, np.uint8)
        for p, (h, w), o in zip(paths, hw, off):
            img = np.asarray(decode(p))
            if img.shape != (h, w, 3) or img.dtype != np.uint8:
                raise ValueError("background image %s decodes to %s %s, expected (%d, %d, 3) uint8"
                                 % (p, img.shape, img.dtype, h, w))
            buf[o:o + h * w * 3] = img.reshape(-1)
        self.n, self.nbytes, self.names = len(paths), int(total), list(names)
        self.hw_host, self.off_host = hw, off
        self.pool = torch.from_numpy(buf).to(device)
        self.hw = torch.from_numpy(hw).to(device)
        self.off = torch.from_numpy(off).to(device)

    @staticmethod
    def plan(paths, budget_bytes, probe):
        """-> ((n, 2) int32 sizes, (n,) int64 byte offsets, total bytes); raises when the total exceeds the budget."""
        if not paths:
            raise ValueError("a background pool needs at least one image")
        hw = np.zeros((len(paths), 2), np.int32)
        for i, p in enumerate(paths):
            try:
                h, w = probe(p)
            except Exception as e:
                raise ValueError("background image %s cannot be read: %s" % (p, e)) from e
            if h < 1 or w < 1:
                raise ValueError("background image %s has size %dx%d" % (p, w, h))
            hw[i] = (h, w)
        sizes = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64) * 3
        off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        total = int(sizes.sum())
        if total > int(budget_bytes):
            raise ValueError("the %d background images need %d bytes of device memory, over the budget of %d bytes: "
                             "raise --aug_background_gb" % (len(paths), total, int(budget_bytes)))
        return hw, off, total


class AugmentFront:
    """The GPU half of --augment, run by DziLoader on each training batch."""

    def __init__(self, ac, device):
        self.ac, self.device = ac, device
        self._box = None                     # (host copy, device copy) of the last box table kd6d_pose_remap read
        self.pool = None
        if ac.background_on:
            self.pool = BackgroundPool(ac.background_dir, ac.background_files, device,
                                       int(ac.background_gb * 2 ** 30))

    def _box_table(self, targets):
        """The (n_class, 8, 3) box corners the batch's class ids index, on the device (uploaded when they change).
        Every image of a batch must carry the same table."""
        kp = targets[0].keypoints_3d
        for t in targets[1:]:
            if t.keypoints_3d is not kp and not (t.keypoints_3d.shape == kp.shape and torch.equal(t.keypoints_3d, kp)):
                raise ValueError("--aug_pose_remap device needs one 3D-box table per batch: the images of this batch "
                                 "carry different ones")
        kp = kp.detach().to("cpu", torch.float32).reshape(-1, 8, 3)
        if self._box is None or self._box[0].shape != kp.shape or not torch.equal(self._box[0], kp):
            self._box = (kp.clone(), kp.to(self.device).contiguous())
        return self._box[1]

    def _launch_pose_remap(self, targets, params):
        """kd6d_pose_remap over the batch's instances on the current stream -> (pose, ok) in pinned memory (valid after
        the caller's wait), or None for a batch without instances."""
        from .. import ops
        src = params["pose_src"]
        n = int(src["inst_img"].shape[0])
        if n == 0:
            return None
        B = len(targets)
        box = self._box_table(targets)
        Ms = params["M_ssr"] if self.ac.ssr_on and "M_ssr" in params else None
        parts = [src["src_K"].reshape(-1), src["src_R"].reshape(-1), src["src_T"].reshape(-1),
                 np.asarray(params["M_resize"], np.float64).reshape(-1)]
        if Ms is not None:
            parts.append(np.asarray(Ms, np.float64).reshape(-1))
        f = _dev(np.concatenate(parts).astype(np.float64), torch.float64, self.device)
        i = _dev(np.concatenate([src["inst_img"], src["inst_cls"]]).astype(np.int32), torch.int32, self.device)
        cut = np.cumsum([0, B * 9, n * 9, n * 3, B * 6, B * 6])
        pose, ok = ops.pose_remap(i[:n], i[n:], f[cut[0]:cut[1]], f[cut[1]:cut[2]], f[cut[2]:cut[3]], box, self.ac.K,
                                  f[cut[3]:cut[4]], f[cut[4]:cut[5]] if Ms is not None else None)
        hp = torch.empty(pose.shape, dtype=torch.float32, pin_memory=True)
        ho = torch.empty(ok.shape, dtype=torch.int32, pin_memory=True)
        hp.copy_(pose, non_blocking=True)
        ho.copy_(ok, non_blocking=True)
        return hp, ho

    @staticmethod
    def _fill_poses(params, remap, ssr):
        """R_resize / T_resize / R / T of `params`, per image, from kd6d_pose_remap's readback (remap_poses' shapes)."""
        start = params["pose_src"]["start"]
        B = len(start) - 1
        if remap is None:
            pose, ok = np.zeros((0, 2, 12), np.float32), np.zeros((0, 2), np.int32)
        else:
            pose, ok = remap[0].numpy(), remap[1].numpy()
        # one line per remap the host chain would have run: without an SSR stage, stage 2 only repeats stage 1's flag
        stages = 2 if ssr else 1
        for _ in range(int((ok[:, :stages] == 0).sum())):
            print("Error in pose remapping!")
        for stage, (kr, kt) in enumerate((("R_resize", "T_resize"), ("R", "T"))):
            params[kr] = [pose[start[b]:start[b + 1], stage, :9].reshape(-1, 3, 3).copy() for b in range(B)]
            params[kt] = [pose[start[b]:start[b + 1], stage, 9:].reshape(-1, 3, 1).copy() for b in range(B)]

    def run(self, frames, masks, targets, params):
        """frames (B,H,W,3) uint8 / masks (B,H,W) float32 on the device, the items' original PoseAnnots, collated
        params -> (frames, masks at the internal size, per image (class_ids, R (n,3,3), T (n,3,1)) after
        remove_invalids + symmetry handling)."""
        ac = self.ac
        B, H, W, _ = frames.shape
        key = batch_key(params["key"])
        size = (ac.height, ac.width)
        # 0 the pose remaps of the whole batch (--aug_pose_remap device): first on the stream, read back with the areas
        remap = self._launch_pose_remap(targets, params) if "pose_src" in params else None
        # 1 Resize
        if (H, W) == size and all(is_identity_warp(np.vstack([m, [0, 0, 1]]), W, H) for m in params["M_resize"]):
            resized, resized_m = frames, masks
        else:
            resized, resized_m = warp(frames, masks, params["M_resize"], size)
        cur, cur_m = resized, resized_m
        n_inst = params["n"]
        max_id = max(int(n_inst.max()) if B else 0, 1)
        # 2 RandomOcclusion (visible boxes of the resized mask, taken once)
        if ac.occlusion_on:
            cur, cur_m = cur.clone(), cur_m.clone()          # the resized frame is kept for the fallback
            st = mask_stats(cur_m, max(max_id, MAX_GT))
            occlude(cur, cur_m, st, params["occl_u"], n_inst, ac.occlusion, key)
        # 2b RandomBackground (--aug_chain full): mask == 0 pixels of the images that drew one; no launch otherwise
        if ac.background_on and (np.asarray(params["bg"]) >= 0).any():
            if cur is resized:
                cur = cur.clone()                                # the resized frame is kept for the fallback
            background(cur, cur_m, self.pool, params["bg"])
        # 3 RandomShiftScaleRotate
        if ac.ssr_on:
            cur, cur_m = warp(cur, cur_m, params["M_ssr"], size)
        # 4 RandomHSV
        if ac.hsv_on:
            if cur is resized:
                cur = cur.clone()
            hsv(cur, params["hsv"])
        # 4b RandomPencilSharpen (--aug_chain full): a new buffer; no launch when no image of the batch drew it
        if ac.sharpen_on and (np.asarray(params["sharpen_ks"]) > 0).any():
            cur = sharpen(cur, params["sharpen_ks"], params["sharpen_mode"], params["sharpen_alpha"])
        # 5-7 RandomSmooth, RandomNoise, Grayscalize
        if ac.smooth_on or ac.noise_on or ac.gray:
            cur = filt(cur, params.get("ksize"), params.get("sigma"), ac.gray, key)
        if cur_m is resized_m:
            cur_m = cur_m.clone()
        # 8 remove_invalids: one small readback, waited on with an event of this stream
        st = mask_stats(cur_m, max_id)
        host = torch.empty(st.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(st, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        if "pose_src" in params:
            self._fill_poses(params, remap, self.ac.ssr_on and "M_ssr" in params)
        area = host[:, :, 0].numpy()
        lut = np.zeros((B, max_id + 1), np.float32)
        out = []
        fallback = []
        for b in range(B):
            n = int(n_inst[b])
            cls = targets[b].class_ids.numpy()[:n]
            keep = [i for i in range(n) if area[b, i] >= MIN_AREA]
            if keep:
                for j, i in enumerate(keep):
                    lut[b, i + 1] = j + 1
                R, T = params["R"][b][keep], params["T"][b][keep]
                cls = cls[keep]
            else:
                # deliberate deviation: the reference draws another image; this one falls back to Resize only
                fallback.append(b)
                lut[b, 1:n + 1] = np.arange(1, n + 1, dtype=np.float32)
                R, T = params["R_resize"][b], params["T_resize"][b]
            R = np.asarray(R, np.float32).copy()
            for i, c in enumerate(cls):
                k = "cls_" + str(int(c))
                if k in ac.symmetry_types:
                    from .evaluate import pose_symmetry_handling
                    R[i] = pose_symmetry_handling(R[i], ac.symmetry_types[k])
            out.append((cls.astype(np.int64), R, np.asarray(T, np.float32)))
        if fallback:
            idx = torch.tensor(fallback, dtype=torch.long, device=cur.device)
            if cur is resized:
                cur = cur.clone()
            cur[idx] = resized[idx]
            cur_m[idx] = resized_m[idx]
        relabel(cur_m, lut)
        return cur, cur_m, out
