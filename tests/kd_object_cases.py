"""TEST INFRASTRUCTURE ONLY -- cases and fp64 restatement of the per-object KD term (--kd_per_object), used by
tests/test_kd_per_object_host.py (CPU) and tests/test_kd_per_object_gpu.py (GPU).  Not collected as a test.

Object o = b*MAX_GT + g exists for every ground-truth slot g < n_gt[b].  Its teacher set is
loss_cases.teacher_reference(class_of=class of slot g); its student set the positives of image b with pos_gt == g in
ascending packed-row order (points and weights from loss_cases.student_reference); the OT is oracle.sinkhorn_ref with
the eight keypoint problems of an object as one batch (joint diameter).  loss_kd = mean over the valid objects, and the
chain into the logits is loss_cases.student_reference's autograd with a per-slot validity mask.

`python tests/kd_object_cases.py` prints the deviation table of profiles/kd_per_object_tolerances.md.
"""
import numpy as np
import torch

import loss_cases as C
from oracle import sinkhorn_ref as S

MAX_GT = 4
T_CAP = 32                         # kd_losses.CAP: teacher slots per object
OT = dict(blur=0.001, scaling=0.5, reach=0.5)
WEIGHTS = (0.0, 1.0, 5.0)          # w_cls = 0: dcls holds the KD chain alone
F64 = torch.float64


# --------------------------------------------------------------------------------------------------------------------
# teacher side
# --------------------------------------------------------------------------------------------------------------------
def slot_class(targets, b, g):
    t = targets[b]
    return int(t.class_ids[g]) if g < min(len(t.class_ids), MAX_GT) else None


def object_teacher_logits(targets, levels, seed, distractor=True):
    """Teacher outputs in which every class of every image emits (several classes per image), plus -- distractor -- one
    class that no instance of the image has, with a LOWER id than the image's classes where one is free (the per-image
    rule would pick it)."""
    hot = []
    L = len(levels)
    for b, t in enumerate(targets):
        classes = sorted({int(c) for c in t.class_ids})
        h = [(c, tuple(range(L)) if i % 2 == 0 else tuple(range(0, L, 2))) for i, c in enumerate(classes)]
        if distractor:
            free = [c for c in range(15) if c not in classes]
            h.append((free[0], tuple(range(min(2, L)))))
        hot.append(h)
    return C.teacher_logits(len(targets), levels, seed, hot)


def teacher_objects(cls, reg, targets, levels, cap=T_CAP, dt=F64, check=True, th=0.1, positive_num=10.0, positive_lambda=1.0):
    """[B*MAX_GT] teacher_reference results, entry o = b*MAX_GT + g (cls None / no rows where the slot does not exist or
    its class emits nothing)."""
    B = len(targets)
    bt = torch.stack([t.bbox_trans for t in targets])
    out = [None] * (B * MAX_GT)
    for g in range(MAX_GT):
        class_of = [slot_class(targets, b, g) for b in range(B)]
        res = C.teacher_reference(cls, reg, B, levels, bt, th, positive_num, positive_lambda, cap, class_of=class_of,
                                  dt=dt, check=check)
        for b in range(B):
            out[b * MAX_GT + g] = res[b]
    return out


def teacher_images(cls, reg, targets, levels, cap=T_CAP, dt=F64, check=True):
    """The per-image rule (first class that emits): [B] teacher_reference results."""
    bt = torch.stack([t.bbox_trans for t in targets])
    return C.teacher_reference(cls, reg, len(targets), levels, bt, cap=cap, dt=dt, check=check)


# --------------------------------------------------------------------------------------------------------------------
# grouping: a stable partition of an image's positive slots by instance
# --------------------------------------------------------------------------------------------------------------------
def group_reference(cnt, gt, batch, cap):
    """cnt (B,), gt (B*cap,) -> obj_start (B*MAX_GT), obj_cnt (B*MAX_GT), dest (B*cap; -1 beyond cnt) by numpy's stable
    sort; slots whose gt is outside 0..MAX_GT-1 follow the last object."""
    cnt, gt = np.asarray(cnt), np.asarray(gt).reshape(batch, cap)
    start = np.zeros(batch * MAX_GT, np.int64)
    num = np.zeros(batch * MAX_GT, np.int64)
    dest = np.full(batch * cap, -1, np.int64)
    for b in range(batch):
        n = int(cnt[b])
        key = np.array([g if 0 <= g < MAX_GT else MAX_GT for g in gt[b, :n]], np.int64)
        order = np.argsort(key, kind="stable")                   # order[j] = slot that lands at position j
        dest[b * cap + order] = b * cap + np.arange(n)
        base = 0
        for g in range(MAX_GT):
            start[b * MAX_GT + g] = b * cap + base
            num[b * MAX_GT + g] = int((key == g).sum())
            base += num[b * MAX_GT + g]
    return start, num, dest


# --------------------------------------------------------------------------------------------------------------------
# the KD term, fp64 (or fp32 for the tolerance measurement)
# --------------------------------------------------------------------------------------------------------------------
def _problems(targets, pos, cap, tsets, per_object):
    """[(key, image, student slots, teacher result)]: one per (image, slot) or one per image."""
    out = []
    for b in range(len(targets)):
        if per_object:
            for g in range(MAX_GT):
                slots = [b * cap + s for s, (_, gg) in enumerate(pos[b]) if gg == g]
                out.append((b * MAX_GT + g, b, slots, tsets[b * MAX_GT + g] if slot_class(targets, b, g) is not None else None))
        else:
            out.append((b, b, [b * cap + s for s in range(len(pos[b]))], tsets[b]))
    return out


def kd_reference(cls, reg, targets, levels, pos, cap, tsets, per_object=True, weights=WEIGHTS, dt=F64, detach_alpha=False,
                 slot_mask=None):
    """The KD term and its chain into the logits.  tsets: teacher_objects() (per_object) or teacher_images().
    slot_mask (optional, bool (B*cap,)): the per-slot validity mask -- slots outside it get no KD gradient.
    Returns loss_kd, loss (per problem), valid (per problem), g_xs (n,8,2), g_alpha (n,8) (zero on the slots of invalid
    problems), n_valid, and student_reference's dz / draw / rows / cls_of."""
    npdt = np.float64 if dt == F64 else np.float32
    B = len(targets)
    n = B * cap
    st = C.student_reference(cls, reg, targets, levels, pos, cap, dt=dt)
    probs = _problems(targets, pos, cap, tsets, per_object)
    loss = np.zeros(len(probs), np.float64)
    valid = np.zeros(len(probs), np.int64)
    g_xs, g_al = torch.zeros(n, 8, 2, dtype=dt), torch.zeros(n, 8, dtype=dt)
    img_valid = np.zeros(B, np.int64)
    for i, (_, b, slots, t) in enumerate(probs):
        if not slots or t is None or len(t["rows"]) == 0:
            continue
        x = st["xs"][slots].numpy().astype(npdt).transpose(1, 0, 2)                 # (8,N,2)
        a = st["alpha"][slots].numpy().astype(npdt).T                              # (8,N)
        y = t["kp_norm"].numpy().astype(npdt).transpose(1, 0, 2)
        be = np.repeat(t["beta"].numpy().astype(npdt)[None], 8, 0)
        Sv, gx, fa = S.sinkhorn_divergence(a, x, be, y, OT["blur"], OT["scaling"], OT["reach"], with_grad=True, dtype=npdt)
        loss[i], valid[i] = float(Sv.astype(np.float64).sum()), 1
        img_valid[b] = 1
        g_xs[slots] = torch.from_numpy(np.ascontiguousarray(gx.transpose(1, 0, 2))).to(dt)
        g_al[slots] = torch.from_numpy(np.ascontiguousarray(fa.T)).to(dt)
    if slot_mask is not None:
        g_xs[~slot_mask] = 0
        g_al[~slot_mask] = 0
    nv = int(valid.sum())
    loss_kd = float(loss[valid > 0].sum() / nv) if nv else 0.0
    # the weight of a cell's KD gradient, applied HERE: w_kd / n_valid problems for the cells of a valid problem, 0 for
    # every other cell (g_xs / g_al are zero there).  student_reference then gets every image marked valid and
    # weights[2] = B, so that its own factor weights[2] / (number of valid images) is exactly 1.
    scale = (weights[2] / nv) if nv else 0.0
    ch = C.student_reference(cls, reg, targets, levels, pos, cap, dt=dt, upstream=(g_xs * scale, g_al * scale),
                             weights=(weights[0], weights[1], float(B)), valid=torch.ones(B, dtype=torch.int32),
                             detach_alpha=detach_alpha)
    return dict(loss_kd=loss_kd, loss=loss, valid=valid, g_xs=g_xs, g_alpha=g_al, n_valid=nv, img_valid=img_valid,
                dz=ch.get("dz"), draw=ch.get("draw"), rows=ch.get("rows"), cls_of=ch.get("cls_of"), slot=ch.get("slot"),
                xs=st["xs"], alpha=st["alpha"])


# --------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------
def object_case(name):
    """A loss_cases student case (0..4 instances per image, `absent_same_class` among them) plus teacher outputs in
    which every class of the image and a distractor emit."""
    c = C.student_case(name)
    tcls, treg = object_teacher_logits(c["targets"], c["levels"], C.STUDENT_CASES[name] + 500)
    c.update(tcls=tcls, treg=treg)
    return c


def single_instance_case(seed=42, batch=3, crop=128, n_levels=4):
    """One instance per image, the teacher emits the ground-truth class only: per-object and per-image KD coincide."""
    levels = C.level_shapes(crop, crop, n_levels)
    targets = C.make_targets(batch, (1,) * batch, seed, crop)
    lay = C.Layout(batch, levels)
    ref = C.ssc_reference(targets, levels, C.make_keys(lay.rows, seed + 100), cap=48)
    cls, reg = C.student_logits(targets, levels, ref["pos"], seed + 1)
    tcls, treg = object_teacher_logits(targets, levels, seed + 2, distractor=False)
    return dict(name="single_%d" % seed, targets=targets, levels=levels, pos=ref["pos"], cap=48, cls=cls, reg=reg,
                tcls=tcls, treg=treg)


def two_object_case(seed=44, crop=128, n_levels=4):
    """Two images with two objects each; object A = the instance with the lower class id (the per-image rule's pick)."""
    levels = C.level_shapes(crop, crop, n_levels)
    targets = C.make_targets(2, (2, 2), seed, crop)
    lay = C.Layout(2, levels)
    keys = C.make_keys(lay.rows, seed + 100)
    ref = C.ssc_reference(targets, levels, keys, cap=48)
    cls, reg = C.student_logits(targets, levels, ref["pos"], seed + 1)
    tcls, treg = object_teacher_logits(targets, levels, seed + 2, distractor=False)
    return dict(name="two_%d" % seed, targets=targets, levels=levels, pos=ref["pos"], cap=48, cls=cls, reg=reg,
                tcls=tcls, treg=treg, keys=keys)


# --------------------------------------------------------------------------------------------------------------------
# tolerances of the chained gradients: fp32-vs-fp64 deviation of the restatement itself (loss_cases.FACTOR / FLOOR rule)
# --------------------------------------------------------------------------------------------------------------------
def measure_deviations(names=None):
    dev = {}
    for name in names or sorted(C.STUDENT_CASES):
        c = object_case(name)
        args = (c["cls"], c["reg"], c["targets"], c["levels"], c["pos"], c["cap"])
        t64 = teacher_objects(c["tcls"], c["treg"], c["targets"], c["levels"])
        t32 = teacher_objects(c["tcls"], c["treg"], c["targets"], c["levels"], dt=torch.float32, check=False)
        r64 = kd_reference(*args, t64)
        r32 = kd_reference(*args, t32, dt=torch.float32)
        assert (r64["valid"] == r32["valid"]).all()
        for k, key in (("dreg", "draw"), ("dcls", "dz")):
            dev[k] = max(dev.get(k, 0.0), C._rel_dev(r32[key], r64[key]))
    return dev


# profiles/kd_per_object_tolerances.md: what measure_deviations() returned when the cases were fixed
RECORDED_DEV = {"dreg": 9.897e-04, "dcls": 2.601e-07}


def bound(name):
    return max(C.FACTOR * RECORDED_DEV[name], C.FLOOR)


if __name__ == "__main__":
    d = measure_deviations()
    print("| output | fp32-vs-fp64 deviation of the restatement | x %g | bound used (relative to max magnitude) |" % C.FACTOR)
    print("|---|---|---|---|")
    for k in sorted(d):
        print("| %s | %.3e | %.3e | %.3e |" % (k, d[k], C.FACTOR * d[k], max(C.FACTOR * d[k], C.FLOOR)))
