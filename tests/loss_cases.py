"""TEST INFRASTRUCTURE ONLY -- seeded multi-instance targets and plain fp64 restatements of the loss-side operations
(csrc/losses.hip), used by tests/test_loss_cases_host.py (CPU: the restatements against the fp32 oracle and the
recorded goldens) and tests/test_losses_gpu.py (GPU: every kernel against the restatements).  Not collected as a test.

Rows are PACKED the way the kernels see them: level-major, then image, then row-major cells.  Every restatement takes
the same fp32-stored inputs the kernels take and computes in `dt` (torch.float64 for the reference; the GPU tolerances
are derived by running the SAME code with dt=torch.float32 on the CPU, see profiles/loss_kernel_tolerances.md and
`measure_deviations` below).  Selections (which cells) are only compared exactly where fp32 and fp64 cannot
legitimately disagree; the restatements assert those knife-edge conditions on their own inputs.

`python tests/loss_cases.py` prints the deviation table of profiles/loss_kernel_tolerances.md.
"""
import math

import numpy as np
import torch

from kd6d.libs.poses import PoseAnnot
from kd6d.synthetic import INTERNAL_K, LINEMOD_CLASSES, MESH_DIAMETERS, cube_keypoints

SIZES = [32.0, 64.0, 128.0, 256.0, 512.0]
STRIDES = [8.0, 16.0, 32.0, 64.0, 128.0]
F64 = torch.float64
FRAME_WH = (640.0, 480.0)


# --------------------------------------------------------------------------------------------------------------------
# geometry of the packed layout
# --------------------------------------------------------------------------------------------------------------------
def level_shapes(h, w, n_levels):
    out, hh, ww = [], h // 8, w // 8
    for _ in range(n_levels):
        out.append((hh, ww))
        hh, ww = (hh + 1) // 2, (ww + 1) // 2
    return out


class Layout:
    """Packed rows of `batch` images over `levels` [(h, w)]: row(l, b, cell) = row0[l] + b * hw[l] + cell."""

    def __init__(self, batch, levels):
        self.batch, self.levels = batch, [tuple(x) for x in levels]
        self.hw = [h * w for h, w in self.levels]
        self.row0 = [batch * sum(self.hw[:l]) for l in range(len(levels))]
        self.rows = batch * sum(self.hw)
        self.cells = sum(self.hw)

    def row(self, l, b, cell):
        return self.row0[l] + b * self.hw[l] + cell

    def locate(self, row):
        l = max(q for q in range(len(self.levels)) if row >= self.row0[q])
        r = row - self.row0[l]
        return l, r // self.hw[l], r % self.hw[l]

    def centre(self, l, cell):
        w = self.levels[l][1]
        return (cell % w) * STRIDES[l] + STRIDES[l] / 2.0, (cell // w) * STRIDES[l] + STRIDES[l] / 2.0

    def to_oracle(self):
        """index array: packed row -> b * cells + (cell index over the concatenated levels), the oracle's layout."""
        idx, off = [], 0
        for hw in self.hw:
            for b in range(self.batch):
                idx.append(torch.arange(hw) + b * self.cells + off)
            off += hw
        return torch.cat(idx)


# --------------------------------------------------------------------------------------------------------------------
# seeded multi-instance targets
# --------------------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def make_targets(batch, instances, seed, crop, mask_hw=None, affine="diag", same_class=(), absent=(), lone_pixel=None):
    """list[PoseAnnot] with instances[b] in 0..4 objects in image b.

    crop: int or (H, W) network input.  mask_hw: mask size, default the crop (smaller: the kernels clamp anchor centres
    into it).  Masks carry ids 1..G as non-overlapping rectangles, one per vertical strip; the last strip reaches the
    right edge (clamped centres land inside an instance), the last mask row stays free.  affine="general": rotation
    and shear, all four entries of the 2x2 non-zero with |b|, |c| >= 0.05 |a|.  same_class: images whose slot 1
    repeats slot 0's class.  absent: {(b, g)} listed in class_ids but not drawn (the reference's span-1 box).
    lone_pixel: {(b, g): flat mask index (negative: from the end)} -- the instance is that single pixel."""
    rng = np.random.default_rng(seed)
    H, W = (crop, crop) if isinstance(crop, int) else crop
    mh, mw = mask_hw or (H, W)
    lone_pixel = lone_pixel or {}
    K = np.asarray(INTERNAL_K, np.float64).reshape(3, 3)
    kp3d = cube_keypoints()
    out = []
    for b in range(batch):
        G = int(instances[b])
        assert 0 <= G <= 4
        classes = [int(c) for c in rng.permutation(LINEMOD_CLASSES)[:G]]
        if b in same_class and G >= 2:
            classes[1] = classes[0]
        R = np.stack([_rotation(rng) for _ in range(G)]) if G else np.zeros((0, 3, 3))
        T = np.stack([np.array([rng.normal(0, 60), rng.normal(0, 40), rng.uniform(700, 1600)]).reshape(3, 1)
                      for _ in range(G)]) if G else np.zeros((0, 3, 1))
        s = rng.uniform(0.8, 1.6) * min(H, W) / 256.0 if min(H, W) < 480 else rng.uniform(0.9, 1.1)
        if affine == "general":
            th, sh = -rng.uniform(0.15, 0.35), rng.uniform(0.1, 0.25)
            A = s * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]) @ np.array([[1, sh], [0, 1.0]])
            assert min(abs(A[0, 1]), abs(A[1, 0])) >= 0.05 * abs(A[0, 0]) and abs(A[1, 1]) > 0
        else:
            A = np.array([[s, 0.0], [0.0, s]])
        t = np.array([W / 2.0, H / 2.0]) - A @ np.array([K[0, 2], K[1, 2]])
        bt = np.concatenate([A, t[:, None]], 1)
        mask = np.zeros((mh, mw), np.float32)
        for g in range(G):
            if (b, g) in absent:
                continue
            if (b, g) in lone_pixel:
                mask.reshape(-1)[lone_pixel[(b, g)]] = g + 1
                continue
            x0, x1 = g * mw // G + 1, ((g + 1) * mw // G - 1 if g < G - 1 else mw)
            y0, y1 = int(rng.integers(0, max(mh // 4, 1))), mh - 1 - int(rng.integers(0, max(mh // 4, 1)))
            mask[y0:y1, x0:x1] = g + 1
        out.append(PoseAnnot(torch.from_numpy(kp3d.copy()), torch.from_numpy(K.astype(np.float32)),
                             torch.from_numpy(mask), torch.tensor(classes, dtype=torch.long),
                             torch.from_numpy(R.astype(np.float32)), torch.from_numpy(T.astype(np.float32)), W, H,
                             torch.tensor(float(s)), torch.from_numpy(bt.astype(np.float32))))
    return out


def make_keys(rows, seed):
    """Distinct multiples of 2^-24 in [0, 1): exact in fp32, so fp32 and fp64 order them alike."""
    rng = np.random.default_rng(seed)
    k = rng.choice(1 << 24, size=rows, replace=False).astype(np.float64) * 2.0 ** -24
    assert len(np.unique(k)) == rows and (k.astype(np.float32).astype(np.float64) == k).all()
    return k


def _rounded_count(x, what):
    """int(x + 0.5) with the knife-edge condition: x at least 1e-3 away from a k + 0.5 boundary."""
    assert abs((x % 1.0) - 0.5) >= 1e-3, "%s: %.6f is within 1e-3 of a rounding boundary -- choose another seed" % (what, x)
    return int(x + 0.5)


# --------------------------------------------------------------------------------------------------------------------
# SSC assignment (losses/loss.py:164-268), fp64
# --------------------------------------------------------------------------------------------------------------------
def projected_span(t, g):
    """Span of instance g's projected 3D box in crop coordinates (poses.py:264-304); 1 when absent from the mask."""
    mask = t.mask.numpy()
    if not (mask == g + 1).any():
        return 1.0
    c = int(t.class_ids[g])
    X = t.keypoints_3d[c].numpy().astype(np.float64)
    cam = t.rotations[g].numpy().astype(np.float64) @ X.T + t.translations[g].numpy().astype(np.float64).reshape(3, 1)
    pr = t.K.numpy().astype(np.float64) @ cam
    u, v = pr[0] / (pr[2] + 1e-8), pr[1] / (pr[2] + 1e-8)
    bt = t.bbox_trans.numpy().astype(np.float64)
    x, y = bt[0, 0] * u + bt[0, 1] * v + bt[0, 2], bt[1, 0] * u + bt[1, 1] * v + bt[1, 2]
    return max(x.max() - x.min() + 1.0, y.max() - y.min() + 1.0)


def ssc_reference(targets, levels, keys, positive_num=10.0, positive_lambda=1.0, cap=None):
    """labels (rows,) int64 in {-1, 0, c+1} and, per image, the positives [(row, g)] in ascending row order.
    keys (rows,) fp64, packed.  cap: the documented truncation (the cap smallest rows stay positive, the other picks keep
    the in-mask label -1); None = the reference itself, every pick."""
    lay = Layout(len(targets), levels)
    L = len(levels)
    labels = np.zeros(lay.rows, np.int64)
    pos, picked = [], []
    for b, t in enumerate(targets):
        mask = t.mask.numpy().astype(np.float64)
        mh, mw = mask.shape
        G = len(t.class_ids)
        at = []
        for l in range(L):
            cx, cy = np.array([lay.centre(l, c) for c in range(lay.hw[l])]).T
            ix = np.clip(cx, 0, mw - 1).astype(np.int64)
            iy = np.clip(cy, 0, mh - 1).astype(np.int64)
            at.append(mask[iy, ix])
        picks = []
        for g in range(G):
            span = projected_span(t, g)
            dk = np.abs(np.log2(span / np.asarray(SIZES[:L])))
            wl = np.exp(-positive_lambda * dk * dk)
            for l in range(L):
                n = _rounded_count(positive_num * wl[l] / wl.sum(), "ssc image %d gt %d level %d" % (b, g, l))
                cells = np.nonzero(at[l] == g + 1)[0]
                rows = np.array([lay.row(l, b, int(c)) for c in cells], np.int64)
                order = np.argsort(keys[rows], kind="stable")[:n] if len(rows) else []
                picks += [(int(rows[i]), g) for i in order]
        for l in range(L):
            inm = np.zeros(lay.hw[l], bool)
            for g in range(G):
                inm |= at[l] == g + 1
            labels[lay.row(l, b, 0):lay.row(l, b, 0) + lay.hw[l]] = np.where(inm, -1, 0)
        picks.sort()
        assert len({r for r, _ in picks}) == len(picks)
        picked.append(len(picks))
        if cap is not None:
            picks = picks[:cap]
        for r, g in picks:
            labels[r] = int(t.class_ids[g]) + 1
        pos.append(picks)
    return dict(labels=labels, pos=pos, picked=picked, layout=lay)


# --------------------------------------------------------------------------------------------------------------------
# teacher selection (postprocess_kd.py:22-203, PnP gate true)
# --------------------------------------------------------------------------------------------------------------------
def _rel_gap(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def teacher_reference(cls, reg, batch, levels, bbox_trans, th=0.1, positive_num=10.0, positive_lambda=1.0, cap=32,
                      frame_wh=FRAME_WH, class_of=None, dt=F64, check=True):
    """cls (rows,16) / reg (rows,240) packed fp32 tensors, bbox_trans (B,2,3).  Per image (class_of None: the first
    class with a cell above th; else class_of[b], a class id or None) a dict: rows, level, score (n,), kp (n,8,2)
    full-frame px, kp_norm, beta, emitted (before cap), nk.  Slot order: level ascending, score descending, ties by
    the smaller cell (the kernel's documented rule; torch.topk leaves it unspecified).  check: assert the knife-edge
    conditions (a) sigmoid vs th, (b) rounding of n_l, (c) gaps at the arg-max and the cut-off (bit-equal ties pass)."""
    lay = Layout(batch, levels)
    L = len(levels)
    out = []
    for b in range(batch):
        p = [torch.sigmoid(cls[lay.row(l, b, 0):lay.row(l, b, 0) + lay.hw[l], :15].to(dt)) for l in range(L)]
        if check:
            for l in range(L):
                assert float((p[l] - th).abs().min()) >= 1e-5, "a sigmoid within 1e-5 of the threshold"
        if class_of is None:
            above = [c for c in range(15) if any(bool((p[l][:, c] > th).any()) for l in range(L))]
            c = above[0] if above else None
        else:
            c = class_of[b]
            if c is not None and (c < 0 or c >= 15 or not any(bool((p[l][:, c] > th).any()) for l in range(L))):
                c = None
        res = dict(rows=[], level=[], score=[], kp=torch.zeros(0, 8, 2, dtype=dt), emitted=0, cls=c, nk=None)
        out.append(res)
        if c is None:
            continue
        A = bbox_trans[b, :, :2].to(dt)
        tr = bbox_trans[b, :, 2].to(dt)
        Ainv = torch.linalg.inv(A)
        ranked = []
        box_conf, box_size = 0.0, 0.0
        for l in range(L):
            sc = torch.sqrt(p[l][:, c])
            cells = torch.nonzero(p[l][:, c] > th).view(-1).tolist()
            order = sorted(cells, key=lambda i: (-float(sc[i]), i))
            ranked.append([(i, float(sc[i])) for i in order])
            if not order:
                continue
            best, bs = ranked[l][0]
            if check and len(order) > 1:
                g = _rel_gap(bs, ranked[l][1][1])
                assert g == 0.0 or g >= 1e-6, "per-level arg-max gap %g" % g
            if check and box_conf > 0:
                assert _rel_gap(bs, box_conf) >= 1e-6
            if bs > box_conf:
                box_conf = bs
                cx, cy = lay.centre(l, best)
                r = reg[lay.row(l, b, best), c * 16:(c + 1) * 16].to(dt)
                px, py = r[:8] * SIZES[l] + cx, r[8:] * SIZES[l] + cy
                size = float(torch.maximum(px.max() - px.min(), py.max() - py.min()))
                if size > box_size:
                    box_size = size
        dk = np.log2(box_size / np.asarray(SIZES))
        wl = np.exp(-positive_lambda * dk * dk)
        nk = [_rounded_count(positive_num * wl[l] / wl.sum(), "teacher image %d level %d" % (b, l)) for l in range(5)]
        res["nk"] = nk
        kps = []
        for l in range(L):
            n = min(nk[l], len(ranked[l]))
            if check and 0 < n < len(ranked[l]):
                g = _rel_gap(ranked[l][n - 1][1], ranked[l][n][1])
                assert g == 0.0 or g >= 1e-6, "cut-off gap %g" % g
            for cell, s in ranked[l][:n]:
                row = lay.row(l, b, cell)
                cx, cy = lay.centre(l, cell)
                r = reg[row, c * 16:(c + 1) * 16].to(dt)
                d = torch.stack([r[:8] * SIZES[l] + cx, r[8:] * SIZES[l] + cy], 1) - tr
                kps.append(d @ Ainv.T)
                res["rows"].append(row); res["level"].append(l)
                res["score"].append(torch.sqrt(p[l][cell, c]))
        res["emitted"] = len(res["rows"])
        n = min(res["emitted"], cap)
        res["rows"], res["level"] = res["rows"][:n], res["level"][:n]
        res["score"] = torch.stack(res["score"][:n]) if n else torch.zeros(0, dtype=dt)
        res["kp"] = torch.stack(kps[:n]) if n else res["kp"]
        res["kp_norm"] = res["kp"] / torch.tensor(frame_wh, dtype=dt)
        res["beta"] = res["score"] ** 2
    return out


# --------------------------------------------------------------------------------------------------------------------
# focal loss (losses/loss.py:20-40)
# --------------------------------------------------------------------------------------------------------------------
def focal_reference(cls, labels, gamma=2.0, alpha=0.25, dt=F64):
    """cls (rows,16) fp32 (column 15 is the pad), labels (rows,) in {-1, 0, c+1}.  SUM over the non-ignored rows and
    its gradient (rows,15) by autograd in `dt` (rows with label -1: zero)."""
    x = cls[:, :15].to(dt).clone().requires_grad_(True)
    t = labels.to(torch.int64).view(-1, 1)
    ids = torch.arange(1, 16, dtype=torch.int64).view(1, -1)
    p = torch.clamp(torch.sigmoid(x), 1e-4, 1 - 1e-4)
    hit = (t == ids).to(dt)
    miss = ((t != ids) & (t >= 0)).to(dt)
    loss = (-hit * alpha * (1 - p) ** gamma * torch.log(p) - miss * (1 - alpha) * p ** gamma * torch.log(1 - p)).sum()
    grad, = torch.autograd.grad(loss, x)
    return loss.detach(), grad


def focal_inputs(rows, seed, labels="mixed", saturated=0.1):
    """Logits |x| <= 8 (no sigmoid near the 1e-4 clamp, which sits at |x| = 9.21) with a `saturated` share at
    11 <= |x| <= 15 (clamped value in the loss, gradient exactly 0); the pad column carries garbage."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, 16, generator=g) * 3.0).clamp(-8.0, 8.0)
    sat = torch.rand(rows, 16, generator=g) < saturated
    big = (torch.rand(rows, 16, generator=g) * 4.0 + 11.0) * torch.where(torch.rand(rows, 16, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where(sat, big, x)
    x[:, 15] = 1e3
    if labels == "mixed":
        lab = torch.randint(-1, 16, (rows,), generator=g)
    elif labels == "ignored":
        lab = torch.full((rows,), -1)
    else:
        lab = torch.zeros(rows, dtype=torch.int64)
    return x.contiguous(), lab.to(torch.int32)


# --------------------------------------------------------------------------------------------------------------------
# student points, object-space loss and the chain into the logits (kd_loss.py:40-109, loss_libs.py:8-12)
# --------------------------------------------------------------------------------------------------------------------
def kinv_f32():
    """The inverse intrinsics as the host hands them to kd6d_student_points: inverted in double, rounded to fp32."""
    return np.linalg.inv(np.asarray(INTERNAL_K, np.float64).reshape(3, 3)).astype(np.float32)


def student_reference(cls, reg, targets, levels, pos, cap, dt=F64, frame_wh=FRAME_WH, upstream=None, weights=None,
                      valid=None, detach_alpha=False, seg_scale=None):
    """cls (rows,16) / reg (rows,240) packed fp32; pos[b] = [(row, g)] (ssc_reference).  Slot arrays are (B*cap, ...)
    with image b's positives at b*cap (unused slots zero).  Returns xs (n,8,2), alpha (n,8), g_reg_xy (n,8,2),
    loss_reg, branch statistics of the smooth-L1 terms, and -- with upstream = (g_kd_xs (n,8,2), g_kd_alpha (n,8)),
    weights (w_cls, w_reg, w_kd), valid (B,) -- the gradients of
        w_reg * loss_reg + (w_kd / n_valid) * sum over valid images (<g_kd_xs, xs> + <g_kd_alpha, alpha>)
    w.r.t. the class logit of every positive (`dz`), its 16 RAW regression outputs (`draw`; reg = raw * seg_scale[level])
    and seg_scale (`dscale`), by autograd in `dt`."""
    B = len(targets)
    lay = Layout(B, levels)
    n = B * cap
    idx = [(b, s, row, g) for b in range(B) for s, (row, g) in enumerate(pos[b])]
    P = len(idx)
    res = dict(xs=torch.zeros(n, 8, 2, dtype=dt), alpha=torch.zeros(n, 8, dtype=dt), g_reg_xy=torch.zeros(n, 8, 2, dtype=dt),
               loss_reg=torch.zeros((), dtype=dt), idx=idx, layout=lay)
    if P == 0:
        return res
    bi = torch.tensor([i[0] for i in idx])
    slot = torch.tensor([i[0] * cap + i[1] for i in idx])
    row = torch.tensor([i[2] for i in idx])
    gi = torch.tensor([i[3] for i in idx])
    ci = torch.stack([targets[b].class_ids[g] for b, _, _, g in idx]).to(torch.int64)
    loc = [lay.locate(r) for _, _, r, _ in idx]
    lv = torch.tensor([l for l, _, _ in loc])
    ctr = torch.tensor([lay.centre(l, c) for l, _, c in loc], dtype=dt)
    sz = torch.tensor([SIZES[l] for l, _, _ in loc], dtype=dt)
    scale = (torch.ones(5, dtype=dt) if seg_scale is None else seg_scale.to(dt)).clone().requires_grad_(True)
    cols = ci[:, None] * 16 + torch.arange(16)[None]
    raw = (reg[row[:, None], cols].to(dt) / scale.detach()[lv][:, None]).clone().requires_grad_(True)
    z = cls[row, ci].to(dt).clone().requires_grad_(True)
    pred = raw * scale[lv][:, None]
    bt = torch.stack([t.bbox_trans for t in targets]).to(dt)[bi]
    Ainv = torch.linalg.inv(bt[:, :, :2])
    d = torch.stack([pred[:, :8] * sz[:, None] + ctr[:, 0:1], pred[:, 8:] * sz[:, None] + ctr[:, 1:2]], -1) - bt[:, None, :, 2]
    pts = torch.einsum("pij,pkj->pki", Ainv, d)                                   # (P,8,2) full-frame px
    frame = torch.tensor(frame_wh, dtype=dt)
    xs = pts / frame
    sig = torch.sigmoid(z)
    alpha = torch.clamp(sig, 1e-3, 1 - 1e-3)
    kp = torch.stack([targets[b].keypoints_3d[int(c)] for (b, _, _, _), c in zip(idx, ci)]).to(dt)         # (P,8,3)
    R = torch.stack([targets[b].rotations[g] for b, _, _, g in idx]).to(dt)
    T = torch.stack([targets[b].translations[g].reshape(3) for b, _, _, g in idx]).to(dt)
    X = torch.einsum("pij,pkj->pki", R, kp) + T[:, None]
    dia = torch.tensor(MESH_DIAMETERS, dtype=torch.float32).to(dt)[ci].view(-1, 1, 1)
    Kinv = torch.from_numpy(kinv_f32()).to(dt)
    hom = torch.cat([pts, torch.ones_like(pts[..., :1])], -1)
    bb = hom @ Kinv.T
    proj = bb * ((bb * X).sum(-1, keepdim=True) / (bb * bb).sum(-1, keepdim=True))
    diff = 50.0 * proj / dia - 50.0 * X / dia
    ad = diff.abs()
    l1 = torch.where(ad < 1, 0.5 * diff * diff, ad - 0.5)
    loss_reg = l1.sum() / (24.0 * 50.0)
    g_pts, = torch.autograd.grad(loss_reg, pts, retain_graph=True)
    res["xs"][slot] = xs.detach()
    res["alpha"][slot] = alpha.detach()[:, None].expand(-1, 8)
    res["g_reg_xy"][slot] = g_pts
    res.update(loss_reg=loss_reg.detach(), quad_share=float((ad.detach() < 1).double().mean()),
               branch_gap=float((ad.detach() - 1).abs().min()), sigmoid=sig.detach(), rows=row, cls_of=ci, level=lv, slot=slot)
    if upstream is not None:
        g_xs, g_al = (u.to(dt) for u in upstream)
        nv = int((valid > 0).sum())
        a_used = alpha.detach() if detach_alpha else alpha
        total = weights[1] * loss_reg
        if nv > 0:
            on = (valid[bi] > 0).to(dt)
            total = total + (weights[2] / nv) * ((g_xs[slot] * xs).sum((1, 2)) * on
                                                 + (g_al[slot] * a_used[:, None]).sum(1) * on).sum()
        dz, draw, dscale = torch.autograd.grad(total, [z, raw, scale], allow_unused=True)
        res.update(dz=torch.zeros_like(z) if dz is None else dz, draw=draw, dscale=dscale)
    return res


def student_logits(targets, levels, pos, seed, near_share=0.5):
    """Packed head outputs for a student case: class logits |x| <= 6 (no sigmoid near the 1e-3 alpha clamp at
    |x| = 6.9) with every 5th positive's own class at +9 and every 7th at -9 (both clamps); regression outputs that
    decode `near_share` of the positives to within ~2 px of the instance's true projection (quadratic smooth-L1
    branch) and the rest tens of px away (linear branch)."""
    B = len(targets)
    lay = Layout(B, levels)
    g = torch.Generator().manual_seed(seed)
    cls = (torch.randn(lay.rows, 16, generator=g) * 2.0 - 1.0).clamp(-6.0, 6.0)
    reg = torch.randn(lay.rows, 240, generator=g) * 0.3
    i = 0
    for b, t in enumerate(targets):
        K = t.K.double()
        bt = t.bbox_trans.double()
        for row, gt in pos[b]:
            c = int(t.class_ids[gt])
            l, _, cell = lay.locate(row)
            cx, cy = lay.centre(l, cell)
            cam = t.rotations[gt].double() @ t.keypoints_3d[c].double().T + t.translations[gt].double().reshape(3, 1)
            pr = K @ cam
            uv = torch.stack([pr[0] / pr[2], pr[1] / pr[2]])
            xy = bt[:, :2] @ uv + bt[:, 2:3]                                                     # (2,8) crop px
            if float(torch.rand((), generator=g)) < near_share:
                noise = torch.randn(2, 8, generator=g).double() * 0.7
                reg[row, c * 16:c * 16 + 8] = ((xy[0] + noise[0] - cx) / SIZES[l]).float()
                reg[row, c * 16 + 8:c * 16 + 16] = ((xy[1] + noise[1] - cy) / SIZES[l]).float()
            if i % 5 == 1:
                cls[row, c] = 9.0
            elif i % 7 == 3:
                cls[row, c] = -9.0
            i += 1
    return cls.contiguous(), reg.contiguous()


def upstream_grads(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 8, 2, generator=g) * 0.1, torch.randn(n, 8, generator=g) * 0.05


def kd_mean_reference(loss_img, valid):
    v = [float(x) for x, ok in zip(loss_img.double().tolist(), valid.tolist()) if ok > 0]
    return (sum(v) / len(v) if v else 0.0), len(v)


# --------------------------------------------------------------------------------------------------------------------
# the seeded cases
# --------------------------------------------------------------------------------------------------------------------
# name: batch instances, seed, crop, levels, make_targets options, positive_lambda, positive_num
SSC_CASES = {
    "g01234_c128_l4_diag": dict(instances=(0, 1, 2, 3, 4), seed=11, crop=128, n_levels=4, affine="diag"),
    "mixed_c256_l5_general": dict(instances=(4, 2, 3, 1), seed=12, crop=256, n_levels=5, affine="general"),
    "full_640x480_l5_general_lam05": dict(instances=(3, 4), seed=13, crop=(480, 640), n_levels=5, affine="general", lam=0.5),
    # 33 x 47 = 1551 elements: 1551 % 4 = 3 and image 1 starts 6204 bytes in (not 16-byte aligned): scalar scan only; the
    # mask is smaller than the 128 px anchor grid (clamped centres); instance 0 of image 1 is the mask's LAST element
    "odd_mask_33x47_c128": dict(instances=(2, 1, 3), seed=14, crop=128, n_levels=4, affine="general", mask_hw=(33, 47),
                                lone_pixel={(1, 0): -1}),
    "odd_mask_33x47_c128_lam05": dict(instances=(3, 2), seed=15, crop=128, n_levels=4, affine="diag", mask_hw=(33, 47), lam=0.5,
                                      lone_pixel={(0, 2): -2}),
    # 136 x 128 = 4352 float4: one full 16 x 256 block of the unrolled scan, then 256 more; instance 1 of image 1 is the
    # last element (beyond the unrolled block), and the mask is smaller than the 256 px anchor grid
    "tail_block_136x128_c256": dict(instances=(2, 2), seed=16, crop=256, n_levels=5, affine="diag", mask_hw=(136, 128),
                                    lone_pixel={(1, 1): -1}),
    # 125 x 128 = 4000 float4: threads 0..159 take the unrolled block, the others the strided remainder
    "partial_block_125x128_c256": dict(instances=(3, 1), seed=17, crop=256, n_levels=5, affine="general", mask_hw=(125, 128),
                                       lone_pixel={(0, 2): -1}),
    "absent_same_class_c128_lam05": dict(instances=(3, 2), seed=18, crop=128, n_levels=4, affine="general", lam=0.5,
                                         absent={(0, 1)}, same_class=(1,)),
}
# the capacity case: four instances whose picks exceed the 32 slots the loss side used to have
CAPACITY_CASE = "mixed_c256_l5_general"


def ssc_case(name, positive_num=10.0):
    c = SSC_CASES[name]
    inst = c["instances"]
    crop = c["crop"]
    H, W = (crop, crop) if isinstance(crop, int) else crop
    levels = level_shapes(H, W, c["n_levels"])
    targets = make_targets(len(inst), inst, c["seed"], crop, c.get("mask_hw"), c["affine"], c.get("same_class", ()),
                           c.get("absent", ()), c.get("lone_pixel"))
    lay = Layout(len(inst), levels)
    return dict(name=name, targets=targets, levels=levels, layout=lay, keys=make_keys(lay.rows, c["seed"] + 100),
                positive_num=positive_num, positive_lambda=c.get("lam", 1.0))


def teacher_logits(batch, levels, seed, hot, n_hot=(9, 7, 5, 3, 2)):
    """Packed teacher outputs: background logits around -6 (sigmoid 0.0025, far below the 0.1 threshold); hot[b] is a
    list of (class, levels-with-cells) -- on those levels n_hot[l] cells get logits from a ladder in [-1.5, 3]
    whose steps keep every pair of scores >= 1e-4 apart."""
    lay = Layout(batch, levels)
    g = torch.Generator().manual_seed(seed)
    cls = torch.rand(lay.rows, 16, generator=g) - 6.5
    reg = torch.randn(lay.rows, 240, generator=g) * 0.3
    for b in range(batch):
        for c, lvls in hot[b]:
            total = sum(min(n_hot[l], lay.hw[l]) for l in lvls)
            ladder = (torch.linspace(-1.5, 3.0, total) + (torch.rand(total, generator=g) - 0.5) * 0.02)
            ladder = ladder[torch.randperm(total, generator=g)]
            k = 0
            for l in lvls:
                m = min(n_hot[l], lay.hw[l])
                cells = torch.randperm(lay.hw[l], generator=g)[:m]
                for cell in cells.tolist():
                    cls[lay.row(l, b, cell), c] = ladder[k]
                    k += 1
    return cls.contiguous(), reg.contiguous()


TEACHER_CASES = {
    # image 0: classes 3 and 7 above threshold (only 3 emits); image 1: nothing; image 2: class 0, one cell on level 1
    "c128_l4_general": dict(batch=3, crop=128, n_levels=4, seed=21, affine="general",
                            hot=[[(3, (0, 1, 2, 3)), (7, (0, 1))], [], [(0, (0, 1, 2))]], n_hot=(9, 1, 5, 3, 2)),
    "c256_l5_diag": dict(batch=2, crop=256, n_levels=5, seed=22, affine="diag",
                         hot=[[(14, (0, 1, 2, 3, 4))], [(5, (1, 2, 3))]]),
    "full_640x480_l5_general": dict(batch=2, crop=(480, 640), n_levels=5, seed=23, affine="general",
                                    hot=[[(1, (0, 1, 2, 3, 4))], [(9, (0, 2, 4))]]),
    "cap5_c256_l5_general": dict(batch=2, crop=256, n_levels=5, seed=24, affine="general", cap=5,
                                 hot=[[(2, (0, 1, 2, 3, 4))], [(2, (1, 2))]]),
}


def teacher_case(name, tie=None):
    """tie: None, "inside" (ranks 1 and 2 of a level with n_l >= 3 share one logit: both selected, order unspecified in
    the reference) or "straddle" (ranks n_l - 1 and n_l share one: the smaller cell index is selected)."""
    c = TEACHER_CASES[name]
    crop = c["crop"]
    H, W = (crop, crop) if isinstance(crop, int) else crop
    levels = level_shapes(H, W, c["n_levels"])
    B = c["batch"]
    targets = make_targets(B, (1,) * B, c["seed"], crop, None, c["affine"])
    bt = torch.stack([t.bbox_trans for t in targets])
    cls, reg = teacher_logits(B, levels, c["seed"] + 100, c["hot"], c.get("n_hot", (9, 7, 5, 3, 2)))
    case = dict(name=name, batch=B, levels=levels, bbox_trans=bt, cls=cls, reg=reg, cap=c.get("cap", 32), th=0.1,
                positive_num=10.0, positive_lambda=1.0, tie_level=None)
    if tie:
        lay = Layout(B, levels)
        ref = teacher_reference(cls, reg, B, levels, bt, cap=64)[0]
        cl = ref["cls"]
        for l in range(len(levels)):
            rows = [r for r, q in zip(ref["rows"], ref["level"]) if q == l]
            p = cls[lay.row(l, 0, 0):lay.row(l, 0, 0) + lay.hw[l], cl]
            order = sorted(range(lay.hw[l]), key=lambda i: -float(p[i]))
            n_above = int((torch.sigmoid(p.double()) > 0.1).sum())
            n = len(rows)
            if tie == "inside" and n >= 3:
                a, bcell = order[1], order[2]
            elif tie == "straddle" and n >= 2 and n_above > n:
                a, bcell = order[n - 1], order[n]
            else:
                continue
            cls[lay.row(l, 0, bcell), cl] = cls[lay.row(l, 0, a), cl]
            case["tie_level"] = l
            break
        assert case["tie_level"] is not None, "no level fits the tie construction -- choose another seed"
    return case


STUDENT_CASES = {      # ssc case -> logits seed
    "g01234_c128_l4_diag": 31, "mixed_c256_l5_general": 32, "full_640x480_l5_general_lam05": 33,
    "absent_same_class_c128_lam05": 34,
}


def student_case(name, cap=48, every_level=True):
    """Positives of the ssc case's fp64 assignment; every_level: a level the assignment left empty (the 512 px anchors
    need a span these objects do not reach) gets its cell 0 of the first non-empty image, for that image's instance 0 --
    the kernels under test take any (row, instance) list."""
    sc = ssc_case(name)
    ref = ssc_reference(sc["targets"], sc["levels"], sc["keys"], sc["positive_num"], sc["positive_lambda"], cap=cap)
    if every_level:
        lay = sc["layout"]
        used = {lay.locate(r)[0] for p in ref["pos"] for r, _ in p}
        b = next(i for i, t in enumerate(sc["targets"]) if len(t.class_ids))
        for l in range(len(sc["levels"])):
            if l not in used:
                ref["pos"][b] = sorted(ref["pos"][b] + [(lay.row(l, b, 0), 0)])
        assert all(len(p) <= cap for p in ref["pos"])
    cls, reg = student_logits(sc["targets"], sc["levels"], ref["pos"], STUDENT_CASES[name])
    return dict(name=name, targets=sc["targets"], levels=sc["levels"], pos=ref["pos"], cap=cap, cls=cls, reg=reg)


# (dtype is the GPU side's business) detach_alpha, seg: None | "grad" | "nograd", valid pattern
BACKWARD_VARIANTS = [
    dict(detach=0, seg=None, valid="all"), dict(detach=1, seg=None, valid="all"),
    dict(detach=0, seg="grad", valid="one_invalid"), dict(detach=0, seg="nograd", valid="all"),
    dict(detach=0, seg="grad", valid="none"), dict(detach=1, seg="grad", valid="one_invalid"),
]
BACKWARD_WEIGHTS = (0.1, 1.0, 5.0)
SEG_SCALE = (1.25, 0.8, 1.5, 0.6, 1.1)


def valid_pattern(kind, batch):
    v = torch.ones(batch, dtype=torch.int32)
    if kind == "one_invalid":
        v[batch // 2] = 0
    elif kind == "none":
        v[:] = 0
    return v


FOCAL_CASES = [  # rows, gamma, labels
    (1, 2.0, "mixed"), (17, 2.0, "ignored"), (17, 2.0, "background"), (17, 1.5, "mixed"), (2184, 2.0, "mixed"),
    (2185, 1.5, "mixed"), (40000, 2.0, "mixed"), (128 * 1364, 2.0, "mixed"),
]


# --------------------------------------------------------------------------------------------------------------------
# fp32-vs-fp64 deviation of the restatements themselves: the yardstick of the GPU tolerances
# --------------------------------------------------------------------------------------------------------------------
def _rel_dev(a32, a64):
    a64 = a64.double()
    m = float(a64.abs().max()) if a64.numel() else 0.0
    return 0.0 if m == 0.0 else float((a32.double() - a64).abs().max()) / m


def measure_deviations(focal_cases=FOCAL_CASES):
    """{output: max over the seeded cases of max|fp32 - fp64| / max|fp64|}, both sides on the CPU."""
    dev = {}

    def note(k, v):
        dev[k] = max(dev.get(k, 0.0), v)

    for name in TEACHER_CASES:
        c = teacher_case(name)
        args = (c["cls"], c["reg"], c["batch"], c["levels"], c["bbox_trans"], c["th"], c["positive_num"], c["positive_lambda"], c["cap"])
        r64 = teacher_reference(*args)
        r32 = teacher_reference(*args, dt=torch.float32, check=False)
        for a, b in zip(r32, r64):
            assert a["rows"] == b["rows"]
            for k in ("kp", "score", "kp_norm", "beta"):
                if b["emitted"]:
                    note("t_" + k, _rel_dev(a[k], b[k]))
    for rows, gamma, labels in focal_cases:
        x, lab = focal_inputs(rows, rows + 7, labels)
        l64, g64 = focal_reference(x, lab, gamma)
        l32, g32 = focal_reference(x, lab, gamma, dt=torch.float32)
        note("loss_cls", _rel_dev(l32.view(1), l64.view(1)))
        note("dcls_focal", _rel_dev(g32, g64))
    for name in STUDENT_CASES:
        c = student_case(name)
        B = len(c["targets"])
        up = upstream_grads(B * c["cap"], 5)
        for v in BACKWARD_VARIANTS:
            kw = dict(upstream=up, weights=BACKWARD_WEIGHTS, valid=valid_pattern(v["valid"], B), detach_alpha=bool(v["detach"]),
                      seg_scale=None if v["seg"] is None else torch.tensor(SEG_SCALE))
            r64 = student_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], c["cap"], **kw)
            r32 = student_reference(c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], c["cap"], dt=torch.float32, **kw)
            for k in ("xs", "alpha", "g_reg_xy"):
                note(k, _rel_dev(r32[k], r64[k]))
            note("loss_reg", _rel_dev(r32["loss_reg"].view(1), r64["loss_reg"].view(1)))
            note("dreg", _rel_dev(r32["draw"], r64["draw"]))
            note("dcls_kd", _rel_dev(r32["dz"], r64["dz"]))
            if v["seg"] == "grad":
                note("dseg_scale", _rel_dev(r32["dscale"], r64["dscale"]))
    g = torch.Generator().manual_seed(3)
    li = torch.rand(16, generator=g)
    note("loss_kd", abs(float(li.sum() / 16) - kd_mean_reference(li, torch.ones(16))[0]) / float(li.mean()))
    return dev


FACTOR = 8.0
FLOOR = 4.0 * 2.0 ** -23          # 4 fp32 ulps of the output's largest magnitude


# profiles/loss_kernel_tolerances.md: what measure_deviations() returned when the cases were fixed (the host test
# checks that a fresh measurement does not exceed it)
RECORDED_DEV = {
    "t_kp": 1.339e-07, "t_score": 4.616e-08, "t_kp_norm": 1.407e-07, "t_beta": 8.965e-08,
    "loss_cls": 5.492e-06, "dcls_focal": 8.481e-07,
    "xs": 1.732e-07, "alpha": 6.507e-08, "g_reg_xy": 6.644e-05, "loss_reg": 9.909e-08,
    "loss_kd": 8.559e-08, "dreg": 1.937e-05, "dcls_kd": 1.595e-07, "dseg_scale": 4.169e-05,
}


def bound(name):
    """Relative-to-largest-magnitude bound of GPU output `name` (profiles/loss_kernel_tolerances.md)."""
    return max(FACTOR * RECORDED_DEV[name], FLOOR)


def assert_within(got, ref, name, what=""):
    """max|got - ref| <= bound(name) * max|ref| (fp64 comparison); prints the figure first."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (name, what)
    m = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    print("  %-10s %-40s max|err| %.3e  max|ref| %.3e  rel %.3e  bound %.3e" % (name, what, err, m, err / max(m, 1e-300), bound(name)))
    assert err <= bound(name) * m, "%s %s: max|err| %.3e > %.3e x %.3e" % (name, what, err, bound(name), m)


def assert_bf16_within_one_ulp(got, ref, what=""):
    """got (bf16 tensor) vs the fp64 value rounded to bf16, one bf16 ulp allowed."""
    ref = torch.as_tensor(ref).double().cpu()
    want = ref.to(torch.bfloat16).double()
    g = got.double().cpu()
    ulp = torch.where(want == 0, torch.zeros_like(want), 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(1e-300))) - 7))
    bad = (g - want).abs() > ulp
    print("  bf16       %-40s max|err|/ulp %.3f" % (what, float(((g - want).abs() / ulp.clamp_min(1e-300)).max()) if g.numel() else 0.0))
    assert bool(torch.isfinite(g).all()) and not bool(bad.any()), "%s: %d elements more than one bf16 ulp off" % (what, int(bad.sum()))


if __name__ == "__main__":
    d = measure_deviations()
    print("| output | fp32-vs-fp64 deviation of the restatement | x %g | bound used (relative to max magnitude) |" % FACTOR)
    print("|---|---|---|---|")
    for k in sorted(d):
        print("| %s | %.3e | %.3e | %.3e |" % (k, d[k], FACTOR * d[k], max(FACTOR * d[k], FLOOR)))
