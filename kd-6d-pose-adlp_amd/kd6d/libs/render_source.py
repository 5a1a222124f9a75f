"""Rendered frame source (train_kd.py / test.py --frame_source render): a device-resident store of frames that SHOW
their objects, drawn by csrc/render_frames.hip, in the shape of a frame cache (kd6d/libs/frame_cache.py).

`RenderedFrames` exposes what `CachedDziLoader` reads from a `DeviceFrameCache` -- frames (n, H, W, 3) uint8 BGR, masks
(n, H, W) uint8 (the VISIBLE instance image, i + 1 = the i-th object of the frame's row), the two annotation tables, the
3D boxes, metas, PoseAnnots without mask, DZI boxes, resolve / check_slots / gather -- and fills them by drawing scenes
on the host and rendering them on the device, one kd6d_render_frames call per chunk of frames:

    objects      1 ... `instances` per frame, of distinct classes (uniform), each with a uniform rotation (QR, as
                 synthetic._random_rotation) and a translation with z uniform in z_range (mm) and x, y uniform among the
                 positions that keep the projected 3D box inside the frame.  Objects may overlap: the mask carries the
                 occlusion.  An object without a visible pixel is dropped from the frame's row (like a BOP object without
                 a visible mask) and the mask ids of the objects behind it in the row move up.
    light        direction uniform on the camera-facing hemisphere, ambient uniform in [0.3, 0.7]
    background   uniform over a pool: `noise` = n_bg procedural low-frequency colour fields made on the host from the
                 seed; a directory = its .png / .jpg files (load_image_cached), which must already be H x W -- a file of
                 another size is REFUSED, nothing is resized here.

Every draw comes from the store's own numpy.random.Generator, seeded with the sequence (seed ..., 1, epoch) -- the noise
backgrounds with (seed ..., 0, 0); `seed` may itself be a sequence such as (seed, rank, list) --: building or refreshing a store
never touches the global `random`, numpy or torch streams (the samplers and the augmentation draw from those).
`refresh()` redraws and re-renders every slot from the next epoch's seed into the SAME allocations.  Memory: n * H * W * 4
bytes of frames + masks (plus n * H * W * 4 of depth when keep_depth), checked against the budget the way the cache checks
it.  Meshes: `dataset_meshes` (the PLYs of DATASETS.MESH_DIR with faces and per-vertex colours) or `surrogate_meshes`
(synthetic.surrogate_mesh: nothing is read from disk).

`render_fn(arrays, H, W) -> (frames, masks, depth)` (numpy) replaces the device call; the CPU tests inject the float64
restatement of the renderer there.
"""
import os
import time

import numpy as np
import torch

from .._lib import MAX_GT
from . import dataset as DS
from .frame_cache import _allocate, table_rows
from .poses import PoseAnnot

_CHUNK = 64                                  # frames per kd6d_render_frames call
ARRAY_ORDER = ("verts", "faces", "vcol", "voff", "vcnt", "foff", "fcnt", "item_frame", "item_slot", "R", "T", "K", "light",
               "ambient", "bg_index", "backgrounds")


class ColoredMesh(DS.Mesh):
    def __init__(self, vertices, faces, colors):
        super().__init__(vertices, faces)
        self.colors = colors                 # (n, 3) uint8 RGB


def dataset_meshes_colored(mesh_dir):
    """The BOP models of mesh_dir, sorted by file name like load_bop_meshes: vertices, faces, per-vertex colours."""
    files = sorted(f for f in os.listdir(mesh_dir) if f.endswith(".ply"))
    out = []
    for name in files:
        path = os.path.join(mesh_dir, name)
        faces = DS.load_ply_faces(path)
        if len(faces) == 0:
            raise ValueError("--render_meshes dataset: %s has no faces, nothing to draw" % path)
        out.append(ColoredMesh(DS.load_ply_vertices(path), faces, DS.load_ply_colors(path)))
    return out


def surrogate_meshes(n_class, level=4, diameters=None):
    """-> (meshes, kp3d (n_class, 8, 3) float32): synthetic.surrogate_mesh per class with cube_keypoints as the 3D boxes."""
    from .. import synthetic as S
    diameters = S.MESH_DIAMETERS if diameters is None else diameters
    n_class = min(int(n_class), len(diameters))
    meshes = [ColoredMesh(*S.surrogate_mesh(c, level, diameters)) for c in range(n_class)]
    return meshes, torch.from_numpy(S.cube_keypoints(diameters)[:n_class].copy())


def noise_backgrounds(n_bg, height, width, rng):
    """n_bg low-frequency colour fields (n_bg, height, width, 3) uint8: a coarse random grid, bilinearly enlarged, plus a
    little per-pixel noise."""
    cell = 32
    gh, gw = height // cell + 2, width // cell + 2
    ys, xs = np.arange(height) / float(cell), np.arange(width) / float(cell)
    y0, x0 = ys.astype(np.int64), xs.astype(np.int64)
    fy, fx = (ys - y0)[None, :, None, None], (xs - x0)[None, None, :, None]
    grid = rng.uniform(0.0, 255.0, (n_bg, gh, gw, 3))
    top = grid[:, y0][:, :, x0] * (1 - fx) + grid[:, y0][:, :, x0 + 1] * fx
    bot = grid[:, y0 + 1][:, :, x0] * (1 - fx) + grid[:, y0 + 1][:, :, x0 + 1] * fx
    field = top * (1 - fy) + bot * fy + rng.normal(0.0, 4.0, (n_bg, height, width, 3))
    return np.clip(np.rint(field), 0, 255).astype(np.uint8)


def directory_backgrounds(path, height, width):
    files = sorted(f for f in os.listdir(path) if f.lower().endswith((".png", ".jpg", ".jpeg")))
    if not files:
        raise ValueError("--render_backgrounds %s: no .png / .jpg file" % path)
    out = []
    for name in files:
        img = DS.load_image_cached(os.path.join(path, name), None)
        if img is None:
            raise ValueError("--render_backgrounds: %s cannot be read" % os.path.join(path, name))
        img = DS.normalise_frame(img)[:, :, :3]
        if img.shape[:2] != (height, width):
            raise ValueError("--render_backgrounds: %s is %dx%d, the frames are %dx%d (backgrounds are not resized; store "
                             "them at the frame size)" % (os.path.join(path, name), img.shape[1], img.shape[0], width, height))
        out.append(np.ascontiguousarray(img))
    return np.stack(out)


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _box_of(K, kp, R, T):
    cam = R @ kp.T + T.reshape(3, 1)
    if cam[2].min() <= 0:
        return None
    uv = K @ cam
    u, v = uv[0] / uv[2], uv[1] / uv[2]
    return u.min(), v.min(), u.max(), v.max()


def place(rng, K, kp, R, height, width, z_range):
    """A translation with z uniform in z_range and the projected 3D box (corners kp) inside the frame: x, y uniform in
    the frustum's cross-section at z, redrawn until the box fits; an object too large for the frame at its z moves away
    by 10 % per 32 failed draws."""
    z = float(rng.uniform(z_range[0], z_range[1]))
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    tries = 0
    while True:
        T = np.array([rng.uniform((0 - cx) * z / fx, (width - 1 - cx) * z / fx),
                      rng.uniform((0 - cy) * z / fy, (height - 1 - cy) * z / fy), z])
        box = _box_of(K, kp, R, T)
        if box is not None and box[0] >= 0 and box[1] >= 0 and box[2] <= width - 1 and box[3] <= height - 1:
            return T
        tries += 1
        if tries % 32 == 0:
            z *= 1.1


class _RenderedList(torch.utils.data.Dataset):
    """What `loader.dataset` is for a rendered list: item i is i (the sampler's indices are the slots); `meshes` and
    `bbox_3d` are what dataset_meshes / vsd_setup ask a BOP_Dataset for, `rendered_depth` is the frame's D_test."""

    def __init__(self, store):
        self.store = store
        self.meshes = store.meshes
        self.bbox_3d = store.kp3d_host
        self.training = store.training

    def __len__(self):
        return self.store.n

    def __getitem__(self, i):
        return int(i)

    def rendered_depth(self, meta):
        return self.store.depth_of(meta)


class RenderedFrames:
    def __init__(self, meshes, kp3d, n, K, height, width, device, seed=0, instances=1, classes=None, z_range=(600.0, 1400.0),
                 backgrounds="noise", n_bg=8, budget_bytes=64 * 2 ** 30, keep_depth=False, training=True, render_fn=None,
                 tag="render", log=print):
        """meshes: ColoredMesh per class id; kp3d (classes, 8, 3) tensor; n frames of height x width under K (3, 3).
        classes: the class ids frames may show (default: every class with a mesh).  keep_depth: keep the renderer's depth
        (what --bop_vsd scores a rendered list against).  log: where the one build line goes (None: nowhere)."""
        t0 = time.time()
        if not 1 <= int(instances) <= MAX_GT:
            raise ValueError("rendered frames: instances must be in 1..%d (got %r)" % (MAX_GT, instances))
        if int(n) < 1:
            raise ValueError("rendered frames: n=%r frames (>= 1)" % (n,))
        self.device = torch.device(device)
        self.meshes = list(meshes)
        self.kp3d_host = torch.as_tensor(kp3d, dtype=torch.float32).contiguous()
        self.classes = [int(c) for c in (range(len(self.meshes)) if classes is None else classes)]
        for c in self.classes:
            if not 0 <= c < min(len(self.meshes), len(self.kp3d_host)):
                raise ValueError("rendered frames: class %d has no mesh or no 3D box" % c)
        self.n = self.length = int(n)
        self.H, self.W = int(height), int(width)
        self.K = np.asarray(K, np.float64).reshape(3, 3)
        # an int or a sequence of ints, e.g. (seed, rank, list): the generators take the whole sequence as their entropy
        self.seed, self.epoch = tuple(int(x) for x in np.atleast_1d(seed)), 0
        self.instances, self.z_range = int(instances), (float(z_range[0]), float(z_range[1]))
        self.training, self.tag, self.render_fn = bool(training), str(tag), render_fn
        need = self.n * self.H * self.W * (8 if keep_depth else 4)
        if need > int(budget_bytes):
            raise ValueError("rendered frames: %d frames of %dx%d need %d bytes (%.3f GB) of device memory, "
                             "--frame_cache_gb allows %d (%.3f GB); raise it or render fewer frames"
                             % (self.n, self.W, self.H, need, need / 2.0 ** 30, int(budget_bytes), int(budget_bytes) / 2.0 ** 30))
        self.nbytes = need
        # pools
        self.voff = np.concatenate([[0], np.cumsum([len(m.vertices) for m in self.meshes])]).astype(np.int64)
        self.foff = np.concatenate([[0], np.cumsum([len(m.faces) for m in self.meshes])]).astype(np.int64)
        self.pool = dict(verts=np.concatenate([np.asarray(m.vertices, np.float32) for m in self.meshes]),
                         faces=np.concatenate([np.asarray(m.faces, np.int32) for m in self.meshes]),
                         vcol=np.concatenate([np.asarray(m.colors, np.uint8) for m in self.meshes]))
        if isinstance(backgrounds, str) and backgrounds == "noise":
            bgs = noise_backgrounds(int(n_bg), self.H, self.W, np.random.Generator(np.random.PCG64(list(self.seed) + [0, 0])))
        elif isinstance(backgrounds, str):
            bgs = directory_backgrounds(backgrounds, self.H, self.W)
        else:
            bgs = np.ascontiguousarray(backgrounds, np.uint8)
        assert bgs.ndim == 4 and bgs.shape[1:] == (self.H, self.W, 3)
        self.pool["backgrounds"] = bgs
        self.frames = _allocate((self.n, self.H, self.W, 3), torch.uint8, self.device)
        self.masks = _allocate((self.n, self.H, self.W), torch.uint8, self.device)
        self.depth = _allocate((self.n, self.H, self.W), torch.float32, self.device) if keep_depth else None
        self.kp3d_dev = self.kp3d_host.to(self.device)
        self.table_f_dev = torch.zeros(self.n, table_rows(self.K, [], [], [])[0].size, dtype=torch.float32, device=self.device)
        self.table_i_dev = torch.zeros(self.n, 1 + MAX_GT, dtype=torch.int32, device=self.device)
        self._pool_dev = None
        self.dataset = _RenderedList(self)
        self._fill()
        self.build_seconds = time.time() - t0
        if log is not None:
            log("rendered frames: %d frames of %dx%d on %s, 1..%d objects of %d classes, %d dropped as invisible, %d bytes "
                "(%.3f GB), drawn and rendered in %.1f s" % (self.n, self.W, self.H, self.device, self.instances,
                                                             len(self.classes), self.n_dropped, self.nbytes,
                                                             self.nbytes / 2.0 ** 30, self.build_seconds))

    # ---- drawing --------------------------------------------------------------------------------------------------------
    def _draw(self, rng):
        kp = self.kp3d_host.numpy().astype(np.float64)
        scenes = []
        for _ in range(self.n):
            g = int(rng.integers(1, min(self.instances, len(self.classes)) + 1))
            cls = [int(c) for c in rng.choice(self.classes, size=g, replace=False)]
            Rs = [_random_rotation(rng) for _ in cls]
            Ts = [place(rng, self.K, kp[c], R, self.H, self.W, self.z_range) for c, R in zip(cls, Rs)]
            light = rng.standard_normal(3)
            light /= np.linalg.norm(light)
            light[2] = -abs(light[2])                          # from the surface towards the camera's side
            scenes.append(dict(cls=cls, R=Rs, T=Ts, light=light, ambient=float(rng.uniform(0.3, 0.7)),
                               bg=int(rng.integers(0, len(self.pool["backgrounds"])))))
        return scenes

    def _arrays(self, scenes):
        items = [(f, g, c, R, T) for f, s in enumerate(scenes) for g, (c, R, T) in enumerate(zip(s["cls"], s["R"], s["T"]))]
        i32 = lambda xs: np.asarray(xs, np.int32).reshape(-1)  # noqa: E731
        return dict(voff=i32([self.voff[c] for _, _, c, _, _ in items]), vcnt=i32([len(self.meshes[c].vertices) for _, _, c, _, _ in items]),
                    foff=i32([self.foff[c] for _, _, c, _, _ in items]), fcnt=i32([len(self.meshes[c].faces) for _, _, c, _, _ in items]),
                    item_frame=i32([f for f, *_ in items]), item_slot=i32([g for _, g, *_ in items]),
                    R=np.asarray([R for *_, R, _ in items], np.float32).reshape(-1, 3, 3),
                    T=np.asarray([T for *_, T in items], np.float32).reshape(-1, 3),
                    K=np.tile(self.K.astype(np.float32).reshape(1, 3, 3), (len(scenes), 1, 1)),
                    light=np.asarray([s["light"] for s in scenes], np.float32).reshape(-1, 3),
                    ambient=np.asarray([s["ambient"] for s in scenes], np.float32),
                    bg_index=i32([s["bg"] for s in scenes]))

    def _render(self, lo, scenes):
        """Scenes of the slots lo ... -> their frames / masks / depth in place; -> visible pixels (len, MAX_GT) int64."""
        hi = lo + len(scenes)
        a = self._arrays(scenes)
        if self.render_fn is not None:
            full = dict(self.pool)
            full.update(a)
            fr, mk, dp = self.render_fn(full, self.H, self.W)
            self.frames[lo:hi].copy_(torch.from_numpy(np.ascontiguousarray(fr, np.uint8)))
            self.masks[lo:hi].copy_(torch.from_numpy(np.ascontiguousarray(mk, np.uint8)))
            if self.depth is not None:
                self.depth[lo:hi].copy_(torch.from_numpy(np.ascontiguousarray(dp, np.float32)))
        else:
            from .. import ops
            if self._pool_dev is None:
                self._pool_dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in self.pool.items()}
            d = dict(self._pool_dev)
            d.update({k: torch.from_numpy(np.ascontiguousarray(v)).to(self.device) for k, v in a.items()})
            ops.render_frames(*[d[k] for k in ARRAY_ORDER], self.H, self.W,
                              out=(self.frames[lo:hi], self.masks[lo:hi], None if self.depth is None else self.depth[lo:hi]))
        m = self.masks[lo:hi].reshape(len(scenes), -1).long()
        m = m + (MAX_GT + 1) * torch.arange(len(scenes), device=m.device).reshape(-1, 1)
        counts = torch.bincount(m.reshape(-1), minlength=(MAX_GT + 1) * len(scenes)).reshape(len(scenes), MAX_GT + 1)
        return counts[:, 1:].cpu().numpy()

    def _fill(self):
        rng = np.random.Generator(np.random.PCG64(list(self.seed) + [1, self.epoch]))
        scenes = self._draw(rng)
        self.metas, self.targets, self.boxes = [], [], []
        rows_f, rows_i = [], []
        self.n_dropped = 0
        Kf = self.K.copy()
        for lo in range(0, self.n, _CHUNK):
            part = scenes[lo:lo + _CHUNK]
            visible = self._render(lo, part)
            for j, s in enumerate(part):
                keep = [g for g in range(len(s["cls"])) if visible[j, g] > 0]
                if len(keep) != len(s["cls"]):                 # an object without a visible pixel leaves the row ...
                    self.n_dropped += len(s["cls"]) - len(keep)
                    lut = torch.zeros(MAX_GT + 1, dtype=torch.uint8)
                    for new, g in enumerate(keep):
                        lut[g + 1] = new + 1                   # ... and the mask ids behind it move up
                    self.masks[lo + j] = lut.to(self.masks.device)[self.masks[lo + j].long()]
                cls = [s["cls"][g] for g in keep]
                rot = [s["R"][g].copy() for g in keep]
                tra = [s["T"][g].reshape(3, 1).copy() for g in keep]
                meta = {"path": "%s/%s.%d/%06d" % (self.tag, "-".join(str(x) for x in self.seed), self.epoch, lo + j), "K": Kf.copy(), "width": self.W, "height": self.H,
                        "class_ids": cls, "rotations": rot, "translations": tra, "epoch": self.epoch, "slot": lo + j}
                rf, ri = table_rows(meta["K"], cls, rot, tra)
                rows_f.append(rf); rows_i.append(ri)
                self.metas.append(meta)
                t = PoseAnnot(self.kp3d_host, torch.tensor(meta["K"], dtype=torch.float32), None,
                              torch.tensor(cls, dtype=torch.long), torch.tensor(np.asarray(rot, np.float32).reshape(-1, 3, 3)),
                              torch.tensor(np.asarray(tra, np.float32).reshape(-1, 3, 1)), self.W, self.H)
                self.targets.append(t)
                self.boxes.append(DS.projected_box(t, 0) if cls else np.array([0.0, 0.0, float(self.W), float(self.H)]))
        self.table_f = np.stack(rows_f)
        self.table_i = np.stack(rows_i)
        self.table_f_dev.copy_(torch.from_numpy(self.table_f))
        self.table_i_dev.copy_(torch.from_numpy(self.table_i))

    def refresh(self):
        """Redraw and re-render every slot from the next epoch's seed, in place: same allocations, new frames."""
        self.epoch += 1
        self._fill()

    # ---- the cache's interface ------------------------------------------------------------------------------------------
    def __len__(self):
        return self.length

    def resolve(self, index):
        index = int(index)
        if not 0 <= index < self.n:
            raise IndexError("rendered frames: index %d outside the %d frames" % (index, self.n))
        return index

    def check_slots(self, slots):
        bad = [int(s) for s in slots if not 0 <= int(s) < self.n]
        if bad:
            raise IndexError("rendered frames: slots %s outside the %d frames" % (bad, self.n))

    def upload_slots(self, slots):
        self.check_slots(slots)
        return torch.tensor([int(s) for s in slots], dtype=torch.int32).to(self.device)

    def gather(self, slots):
        """-> (index on the device, frames (B,H,W,3) uint8, masks (B,H,W) float32): one upload, one launch."""
        from .. import ops
        index = self.upload_slots(slots)
        frames, masks = ops.cache_gather_frames(self.frames, self.masks, index)
        return index, frames, masks

    def depth_of(self, meta):
        """The depth the renderer wrote for the frame of `meta` (H, W) float32 numpy, mm, 0 = background."""
        if self.depth is None:
            raise ValueError("rendered frames: built without keep_depth, there is no depth to score VSD against")
        s = int(meta["slot"])
        if not (0 <= s < self.n and self.metas[s]["path"] == meta["path"] and self.metas[s]["epoch"] == meta["epoch"]):
            raise ValueError("rendered frames: %s is not a frame of this store (refreshed since?)" % meta["path"])
        return self.depth[s].cpu().numpy()

