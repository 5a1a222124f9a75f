"""Darknet-53 as a TRAINED network (the reference's teacher recipe, the third line of its train.sh: train_kd.py
--backbone darknet53 --kd_weight 0.): the BatchNorm forward with the DarkUnit's residual against torch, every
Darknet-53 layer's data and weight gradient at its training shape, one DarkUnit and one stage against the oracle's
autograd, the whole step against oracle/kd_step_ref.py in every launch mode, the train_kd.py recipe end to end, and the
bench.py surface.

Every GPU subprocess below carries a time limit."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_step_gpu import build, ref_to_packed_rows
from util_pack import pack_levels, round_to, unpack_levels, w_to_dgrad, w_to_krsc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
BIAS = [1.0] + [-6.0] * 14


def _accs(n, dev):
    return torch.zeros(n * 4, device=dev)


# ---------------------------------------------------------------------------------------------------------
# 1. BatchNorm train forward with the DarkUnit residual
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,xf32", [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False)])
@pytest.mark.parametrize("C,rows", [(32, 70001), (64, 777), (128, 40001), (256, 301), (512, 65), (1024, 33)])
def test_bn_train_fwd_residual_vs_torch(gpu_device, dtype, xf32, C, rows):
    """y = LeakyReLU(BN(x)) + res (odd row counts; 70001 and 40001 rows are above ConvBlock.FUSE_STATS_MAX_ROWS): y, the
    running buffers, save_mean / save_invstd against torch in double; two launches are bitwise equal."""
    from kd6d import ops
    from kd6d.engine import ConvBlock
    assert max(r for r in (70001, 40001)) > ConvBlock.FUSE_STATS_MAX_ROWS
    dev = gpu_device
    g = torch.Generator().manual_seed(C * 7 + rows)
    x = round_to(torch.randn(rows, C, generator=g) * 2 + 0.5, torch.float32 if xf32 else dtype)
    res = round_to(torch.randn(rows, C, generator=g), dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    rmr, rvr = rm0.double().clone(), rv0.double().clone()
    yr = F.leaky_relu(F.batch_norm(x.double(), rmr, rvr, gamma.double(), beta.double(), True, 0.1, 1e-5), 0.1) + res.double()
    mean_r = x.double().mean(0)
    invstd_r = 1.0 / torch.sqrt(x.double().var(0, unbiased=False) + 1e-5)
    xd, resd = x.to(dev), res.to(dtype).to(dev)
    s1, s2 = _accs(C, dev), _accs(C, dev)
    ops.colstats(xd, s1, s2)
    outs = []
    for _ in range(2):
        y = torch.empty(rows, C, dtype=dtype, device=dev)
        rm_d, rv_d = rm0.to(dev), rv0.to(dev)
        mean = torch.empty(C, device=dev)
        invstd = torch.empty(C, device=dev)
        ops.bn_train_fwd_res(xd, resd, y, s1, s2, gamma.to(dev), beta.to(dev), 1e-5, 0.1, rm_d, rv_d, mean, invstd,
                             ops.ACT_LEAKY)
        outs.append((y, rm_d, rv_d, mean, invstd))
    torch.cuda.synchronize()
    y, rm_d, rv_d, mean, invstd = outs[0]
    tol = dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32 else dict(rtol=1.2e-2, atol=1.2e-2)
    torch.testing.assert_close(y.cpu().double(), yr, **tol)
    torch.testing.assert_close(rm_d.cpu().double(), rmr, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rv_d.cpu().double(), rvr, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(mean.cpu().double(), mean_r, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(invstd.cpu().double(), invstd_r, rtol=1e-4, atol=1e-5)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b), "two launches differ"


# ---------------------------------------------------------------------------------------------------------
# 2. every Darknet-53 layer at its training shape (B = 16, bf16)
# ---------------------------------------------------------------------------------------------------------
def _teacher_layers():
    import step_layers as BC
    return list(BC.TEACHER)


TEACHER_LAYERS = _teacher_layers()


@pytest.mark.parametrize("layer", TEACHER_LAYERS, ids=[l[0] for l in TEACHER_LAYERS])
def test_darknet53_layer_gradients_at_training_shape(gpu_device, layer):
    """dgrad and wgrad (the whole device and cu_budget=128) of every Darknet-53 convolution at B = 16 against torch's CPU
    convolution; the bounds and bf16-representable inputs of test_fullsize_gpu.py::test_conv_layer_at_benchmark_shape.
    The stride-2 layers also run the training forward with the BatchNorm-statistics epilogue wherever the engine asks
    for it (rows <= ConvBlock.FUSE_STATS_MAX_ROWS)."""
    from kd6d import ops
    from kd6d.engine import ConvBlock, PoseNet
    name, cin, cout, k, stride, levels = layer
    B, dev, dtype, pad = 16, gpu_device, torch.bfloat16, k // 2
    g = torch.Generator().manual_seed(len(name) * 131 + cin + cout)
    geom = ops.Geom(B, cin, cout, k, stride, pad, levels)
    xs = [round_to(torch.randn(B, cin, h, w, generator=g), dtype) for (h, w) in levels]
    w = round_to(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, dtype)
    ws = torch.empty(PoseNet.WORKSPACE_BYTES // 4, dtype=torch.float32, device=dev)
    xp = pack_levels(xs, dtype).to(dev)
    dys = [round_to(torch.randn(B, cout, h, w_, generator=g), dtype) for (h, w_) in geom.levels_out]
    dyp = pack_levels(dys, dtype).to(dev)
    dx = ops.conv2d_dgrad(geom, dyp, w_to_dgrad(w, dtype).to(dev))
    dw = ops.conv2d_wgrad_f32(geom, xp, dyp)[0].view(cout, k, k, cin)
    dw_half = ops.conv2d_wgrad_f32(geom, xp, dyp, cu_budget=128)[0].view(cout, k, k, cin)
    fused = stride == 2 and geom.rows_out <= ConvBlock.FUSE_STATS_MAX_ROWS
    if fused:
        stats = _accs(2 * cout, dev)
        y = ops.conv2d_fwd(geom, xp, w_to_krsc(w, dtype).to(dev), out_f32=True, stats=stats, stats_groups=0, workspace=ws)
        st = ops.acc_read(stats, 2 * cout, ops.ACC_ACT)
    torch.cuda.synchronize()
    ref_w = torch.zeros(cout, cin, k, k)
    for (h, w_), x, dy, gl in zip(levels, xs, dys, unpack_levels(dx.cpu(), B, levels)):
        ref = torch.nn.grad.conv2d_input((B, cin, h, w_), w, dy, stride=stride, padding=pad)
        torch.testing.assert_close(gl, ref, rtol=1.2e-2, atol=1.2e-2)
        ref_w += torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dy, stride=stride, padding=pad)
    scale = max(float(ref_w.abs().max()), 1.0)
    for got in (dw, dw_half):
        torch.testing.assert_close(got.cpu().permute(0, 3, 1, 2), ref_w, rtol=2e-4, atol=2e-4 * scale)
    if fused:
        refs = [F.conv2d(x, w, stride=stride, padding=pad) for x in xs]
        got_y = unpack_levels(y.cpu(), B, geom.levels_out)
        for gl, ref in zip(got_y, refs):
            torch.testing.assert_close(gl, ref, rtol=2e-4, atol=2e-4)
        s1 = sum(t.double().sum(dim=(0, 2, 3)) for t in got_y)
        s2 = sum((t.double() ** 2).sum(dim=(0, 2, 3)) for t in got_y)
        want = torch.cat([s1, s2])
        torch.testing.assert_close(st.cpu().double(), want, rtol=1e-4, atol=1e-4 * max(float(want.abs().max()), 1.0))
    assert ops.lib.kd6d_barrier_timeouts() == 0


# ---------------------------------------------------------------------------------------------------------
# 3. one DarkUnit and one whole stage against the oracle's autograd (fp32)
# ---------------------------------------------------------------------------------------------------------
def _to_nchw(packed, B, h, w, c):
    return packed.float().cpu().reshape(B, h, w, -1)[..., :c].permute(0, 3, 1, 2)


def _to_nhwc(x):
    B, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * h * w, c).contiguous()


@pytest.mark.parametrize("what", ["unit", "stage"])
def test_darkunit_and_stage_vs_oracle_autograd(gpu_device, what):
    """Stage 3 of Darknet-53 (its down-sampling block and 8 DarkUnits; 'unit': its second unit alone) on B = 2, 16x16
    input, fp32, seeded weights: output, input gradient, every parameter gradient and the running statistics against
    oracle.kd_step_ref.ConvBlockRef / DarkUnitRef under torch autograd."""
    from kd6d.engine import UnitRec
    from oracle import kd_step_ref as O
    dev = gpu_device
    B = 2
    module = build("darknet53", "fp32", 3, dev).train()
    net = module.net
    ref = O.PoseNetRef("darknet53")
    ref.load_state_dict(O.seeded_state_dict(ref, 3))
    ref.train()
    stage_ref = ref.backbone.features.stage3
    prefix = "backbone.features.stage3."
    units = net.stages[2]
    if what == "unit":
        mods, units = [stage_ref.unit2], [units[1]]
        cin, h = 256, 8
        prefix += "unit2."
    else:
        mods = list(stage_ref.children())
        cin, h = 128, 16
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, h, h, generator=g)
    xr = x.clone().requires_grad_(True)
    y_ref = xr
    for m in mods:
        y_ref = m(y_ref)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy)

    net.prepare_weights(need_dgrad=True)
    module.zero_grad()
    net.tape = []
    lv = [(h, h)]
    xd = _to_nhwc(x).to(dev)
    y = xd
    for u in units:
        if u[0] == "down":
            y, lv = u[1].fwd_train(y, B, lv, net.tape)
        else:
            y, lv = net.unit_fwd_train(u, y, B, lv)
    (ho, wo), = lv
    grad = _to_nhwc(dy).to(dev)
    for rec in reversed(net.tape):
        if isinstance(rec, UnitRec):
            grad = net.unit_bwd(rec, grad)
        else:
            grad = rec.block.bwd(rec, grad, dx=net.buf(rec.block.name + ".dx", rec.x.shape))
    net.store.resolve_grads()
    torch.cuda.synchronize()
    cout = y_ref.shape[1]
    torch.testing.assert_close(_to_nchw(y, B, ho, wo, cout), y_ref.detach(), rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(_to_nchw(grad, B, h, h, cin), xr.grad, rtol=1e-3, atol=1e-3 * float(xr.grad.abs().max()))
    got = dict(module.named_parameters())
    bufs = dict(module.named_buffers())
    n = 0
    for m in mods:
        mname = [k for k, v in stage_ref.named_children() if v is m][0]
        for k, p in m.named_parameters():
            full = "backbone.features.stage3.%s.%s" % (mname, k)
            r = p.grad
            torch.testing.assert_close(got[full].grad.cpu(), r, rtol=1e-3, atol=1e-3 * max(float(r.abs().max()), 1e-6),
                                       msg=lambda s, full=full: "%s: %s" % (full, s))
            n += 1
        for k, b in m.named_buffers():
            full = "backbone.features.stage3.%s.%s" % (mname, k)
            if k.endswith("num_batches_tracked"):
                continue
            torch.testing.assert_close(bufs[full].cpu(), b, rtol=1e-4, atol=1e-5, msg=lambda s, full=full: "%s: %s" % (full, s))
    assert n == (6 if what == "unit" else 3 + 8 * 6)


# ---------------------------------------------------------------------------------------------------------
# 4. the whole step against the oracle, Darknet-53 student (B = 2, 128 x 128)
# ---------------------------------------------------------------------------------------------------------
def _levels(crop, n=5):
    return [(max(crop // 8 // (2 ** i), 1),) * 2 for i in range(n)]


def _chooser(keys_ref, levels):
    cells = sum(h * w for h, w in levels)
    counts = [h * w for h, w in levels]

    def choose(vp, n, im, l, g):
        off = im * cells + sum(counts[:l])
        return torch.argsort(keys_ref[off + vp], stable=True)[:n]
    return choose


@pytest.mark.parametrize("kd_weight", [0.0, 5.0])
def test_darknet53_student_step_vs_oracle_fp32_with_optimizer(gpu_device, kd_weight):
    """The teacher recipe's step (Darknet-53 student) incl. the fused clip + AdamW + OneCycle update against the CPU
    oracle, element-wise on every gradient tensor and updated weight with the bounds of
    test_step_gpu.py::test_step_against_oracle_fp32_with_optimizer; a second execution of the step from the same state is
    bitwise equal.  At kd_weight 0 the teacher still runs and loss_kd is still computed (train_kd.py:104-137)."""
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.optim import FusedClipAdamW
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS, make_batch
    from oracle import kd_step_ref as O
    dev = gpu_device
    B, crop, arch = 2, 128, "darknet53"
    images, targets = make_batch(B, 21, crop=crop)
    img = ImageList(images.tensors.to(dev), images.sizes)
    tgt = PackedTargets(targets, dev)
    levels = _levels(crop)
    cells = sum(h * w for h, w in levels)
    keys_ref = torch.rand(B * cells, generator=torch.Generator().manual_seed(100))
    choose = _chooser(keys_ref, levels)
    step = O.KDStepRef(arch, "darknet53", K=INTERNAL_K, diameters=MESH_DIAMETERS, kd_weight=kd_weight,
                       teacher_cls_bias=BIAS)
    res, _ = step.step(images.tensors, [t.as_dict() for t in targets], choose=choose, return_extras=True)
    ref_grads = {k: p.grad.clone() for k, p in step.student.named_parameters() if p.grad is not None}
    teacher = build("darknet53", "fp32", 2, dev, BIAS).eval()

    def run():
        student = build(arch, "fp32", 1, dev).train()
        student._debug_keys = keys_ref[ref_to_packed_rows(B, levels)].to(dev)
        opt = FusedClipAdamW(student, lr=1e-3, weight_decay=1e-4, eps=1e-8, max_norm=1.0)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, 1e-3, 10100, pct_start=0.05, cycle_momentum=False,
                                                    anneal_strategy="linear")
        with torch.no_grad():
            pred_t = teacher(img, targets=tgt, is_teacher=True)
        student.zero_grad()
        _, ld = student(img, targets=tgt, pred_t=pred_t)
        loss = ld["loss_cls"] * 0.1 + ld["loss_reg"] * 1.0
        if kd_weight > 0:
            loss = loss + ld["loss_kd"] * kd_weight
        loss.backward()
        grads = {k: p.grad.detach().clone().cpu() for k, p in student.named_parameters() if p.grad is not None}
        opt.step(); sched.step()
        torch.cuda.synchronize()
        return {k: float(v) for k, v in ld.items()}, float(opt.grad_norm()), grads, student.state_dict()

    ld, gn, got_grads, sd = run()
    ld2, gn2, got_grads2, sd2 = run()
    assert ld == ld2 and gn == gn2
    for k in got_grads:
        assert torch.equal(got_grads[k], got_grads2[k]), "two executions differ: %s" % k
    assert ld["loss_cls"] == pytest.approx(res["loss_cls"], rel=1e-3)
    assert ld["loss_reg"] == pytest.approx(res["loss_reg"], rel=1e-3)
    assert ld["loss_kd"] == pytest.approx(res["loss_kd"], rel=2e-3)
    assert res["loss_kd"] > 0, "the teacher runs and loss_kd is computed also at kd_weight 0"
    assert gn == pytest.approx(res["grad_norm"], rel=5e-3)
    assert set(got_grads) == set(ref_grads) and len(ref_grads) == 213       # 52 blocks x 3, FPN, head
    clip = min(1.0, 1.0 / (res["grad_norm"] + 1e-6))
    # element-wise deviation per tensor, in units of the tensor's largest gradient.  The tiny student's bound is 2e-2;
    # at 128 x 128 this network's stage 5 normalises over 2 x 4 x 4 values per channel, and fp32 summation-order
    # differences through 52 batch-statistics backwards reach a few percent on single elements of the deepest tensors
    # (one unit and one stage alone agree to 1e-3: test_darkunit_and_stage_vs_oracle_autograd)
    dev_e = {k: float((got_grads[k] - g / clip).abs().max()) / (float((g / clip).abs().max()) + 1e-6 * res["grad_norm"])
             for k, g in ref_grads.items()}
    worst = sorted(dev_e.items(), key=lambda kv: -kv[1])[:5]
    print("[darknet53 fp32 kd=%g] worst element-wise gradient deviation: %s" % (kd_weight, worst))
    assert sum(v > 2e-2 for v in dev_e.values()) <= 0.05 * len(dev_e), worst
    assert worst[0][1] <= 0.1, worst
    bad = total = 0
    for k, v in step.student.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v)
            continue
        d = (sd[k].cpu() - v).abs()
        bad += int((d > 2e-4 + 2e-3 * v.abs()).sum())
        total += v.numel()
    # the first AdamW update is lr * sign(g): where a gradient is near zero its sign may differ
    print("[darknet53 fp32 kd=%g] updated weights outside rtol 2e-3 / atol 2e-4: %d of %d" % (kd_weight, bad, total))
    assert bad <= 1e-3 * total, (bad, total)


def test_darknet53_student_step_vs_oracle_bf16(gpu_device):
    """bf16 step of the Darknet-53 student against the oracle under bf16-storage emulation, with the bf16 bounds of
    test_step_gpu.py (losses 1e-2 / KD 0.1, per-tensor gradient-norm deviation BF16_EMU_WORST at 128 x 128, global norm
    3e-3); two executions bitwise equal."""
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS, make_batch
    from oracle import kd_step_ref as O
    from test_step_gpu import BF16_EMU_WORST
    dev = gpu_device
    B, crop, arch = 2, 128, "darknet53"
    images, targets = make_batch(B, 22, crop=crop)
    img = ImageList(images.tensors.to(dev), images.sizes)
    tgt = PackedTargets(targets, dev)
    levels = _levels(crop)
    cells = sum(h * w for h, w in levels)
    keys_ref = torch.rand(B * cells, generator=torch.Generator().manual_seed(101))
    emu = O.KDStepRef(arch, "darknet53", K=INTERNAL_K, diameters=MESH_DIAMETERS, kd_weight=5.0, teacher_cls_bias=BIAS,
                      emulate_bf16=True)
    out, _ = emu.forward_backward(images.tensors, [t.as_dict() for t in targets], choose=_chooser(keys_ref, levels))
    eg = {k: p.grad for k, p in emu.student.named_parameters() if p.grad is not None}
    egn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in eg.values())))
    teacher = build("darknet53", "bf16", 2, dev, BIAS).eval()
    runs = []
    for _ in range(2):
        student = build(arch, "bf16", 1, dev).train()
        student._debug_keys = keys_ref[ref_to_packed_rows(B, levels)].to(dev)
        with torch.no_grad():
            pred_t = teacher(img, targets=tgt, is_teacher=True)
        student.zero_grad()
        _, ld = student(img, targets=tgt, pred_t=pred_t)
        (ld["loss_cls"] * 0.1 + ld["loss_reg"] * 1.0 + ld["loss_kd"] * 5.0).backward()
        torch.cuda.synchronize()
        runs.append(({k: float(v) for k, v in ld.items()},
                     {k: p.grad.detach().float().cpu().clone() for k, p in student.named_parameters() if p.grad is not None}))
    (ld, got), (ld2, got2) = runs
    assert ld == ld2 and all(torch.equal(got[k], got2[k]) for k in got), "two executions differ"
    dev_e = {k: abs(float(got[k].norm()) - float(eg[k].norm())) / max(float(eg[k].norm()), 1e-6 * egn) for k in eg}
    worst = max(dev_e.values())
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in got.values())))
    print("[darknet53 bf16] vs emulation: worst %.4f (%s), total %.2e, losses %s / %s" % (
        worst, max(dev_e, key=dev_e.get), abs(total - egn) / egn, ld, {k: float(v) for k, v in out.items()
                                                                        if torch.is_tensor(v) and v.numel() == 1}))
    for k in ("loss_cls", "loss_reg"):
        assert ld[k] == pytest.approx(float(out[k]), rel=1e-2)
    assert ld["loss_kd"] == pytest.approx(float(out["loss_kd"]), rel=0.1)
    assert worst <= BF16_EMU_WORST[crop], (worst, max(dev_e, key=dev_e.get))
    assert total == pytest.approx(egn, rel=3e-3)


def test_darknet53_student_launch_modes_bitwise_equal(gpu_device):
    """Three fp32 steps of the Darknet-53 student: eager launches, GraphedKDStep(pipeline=True) and
    GroupedTeacherKDStep(group=3) end with bitwise-equal parameters and losses; an eval forward after the replays sees the
    current weights (the cached BatchNorm folds are refreshed after the optimiser steps)."""
    from kd6d.graph import GraphedKDStep, GroupedTeacherKDStep
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.optim import FusedClipAdamW
    from kd6d.synthetic import make_batch
    dev = gpu_device
    B, crop, n = 2, 64, 3
    batches = []
    for i in range(n):
        images, targets = make_batch(B, 60 + i, crop=crop)
        batches.append((ImageList(images.tensors.to(dev), images.sizes), PackedTargets(targets, dev)))
    levels = _levels(crop)
    keys = torch.rand(B * sum(h * w for h, w in levels), generator=torch.Generator().manual_seed(4)).to(dev)
    names = ("loss_cls", "loss_reg", "loss_kd")
    w = (0.1, 1.0, 5.0)

    def make():
        teacher = build("darknet53", "fp32", 2, dev, BIAS).eval()
        student = build("darknet53", "fp32", 1, dev).train()
        student._debug_keys = keys
        return teacher, student, FusedClipAdamW(student, lr=1e-3)

    def eval_logits(m):
        m.eval()
        cls, reg = m.net.forward(batches[0][0].tensors)
        out = (cls.clone(), reg.clone())
        m.train()
        return out

    results = {}
    teacher, student, opt = make()
    eager = []
    for img, tgt in batches:
        student.zero_grad()
        with torch.no_grad():
            pred_t = teacher(img, targets=tgt, is_teacher=True)
        _, ld = student(img, targets=tgt, pred_t=pred_t)
        (ld["loss_cls"] * w[0] + ld["loss_reg"] * w[1] + ld["loss_kd"] * w[2]).backward()
        opt.step()
        eager.append([float(ld[k]) for k in names])
    results["eager"] = (eager, student.net.store.params.detach().clone(), student.net.store.bufs.detach().clone())
    for mode in ("pipeline", "grouped"):
        teacher, student, opt = make()
        gs = (GraphedKDStep(teacher, student, opt, w, pipeline=True) if mode == "pipeline"
              else GroupedTeacherKDStep(teacher, student, opt, w, group=3))
        got = []
        for b in batches:
            ld = gs(*b)
            if ld is not None:
                got.append([float(ld[k]) for k in names])
        while True:
            ld = gs.flush()
            if ld is None:
                break
            got.append([float(ld[k]) for k in names])
        assert opt.steps == n
        results[mode] = (got, student.net.store.params.detach().clone(), student.net.store.bufs.detach().clone())
        if mode == "grouped":
            after = eval_logits(student)
            fresh = build("darknet53", "fp32", 1, dev)
            fresh.load_state_dict(student.state_dict())
            want = eval_logits(fresh)
    torch.cuda.synchronize()
    for mode in ("pipeline", "grouped"):
        assert results[mode][0] == results["eager"][0], (mode, results[mode][0], results["eager"][0])
        assert torch.equal(results[mode][1], results["eager"][1]), "%s: parameters differ from eager" % mode
        assert torch.equal(results[mode][2], results["eager"][2]), "%s: running statistics differ from eager" % mode
    torch.testing.assert_close(after[0], want[0], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(after[1], want[1], rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------
# 5. one step at the benchmark shape (grouped launch mode, bf16)
# ---------------------------------------------------------------------------------------------------------
def test_darknet53_student_benchmark_shape_grouped_vs_oracle(gpu_device):
    """B = 16, 256 x 256, bf16, GroupedTeacherKDStep(group=3), kd_weight 5: the first step against the oracle under
    bf16-storage emulation with the bf16 bounds of test_fullsize_gpu.py::test_benchmark_config_grouped_teacher_vs_oracle
    (losses, global gradient norm, per-tensor norm worst / >= 1024 elements / weighted mean).  The gradient direction
    gets its own bound: 52 BatchNorm layers of bf16 roundings in the backward (the tiny student has 15) put 1 - cosine
    at 6.0e-4 on MI355X against the tiny student's 8e-5; bound 2x measured."""
    from kd6d import ops
    from kd6d.graph import GroupedTeacherKDStep
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.optim import FusedClipAdamW
    from kd6d.synthetic import INTERNAL_K, MESH_DIAMETERS, make_batch
    from oracle import kd_step_ref as O
    from test_fullsize_gpu import TOL, _grad_report
    dev = gpu_device
    B, crop, group = 16, 256, 3
    tol = TOL["bf16"]
    levels = _levels(crop)
    cells = sum(h * w for h, w in levels)
    keys_ref = torch.rand(B * cells, generator=torch.Generator().manual_seed(17))
    cpu_batches, batches = [], []
    for i in range(2):
        images, targets = make_batch(B, 41 + i, crop=crop)
        cpu_batches.append((images.tensors, [t.as_dict() for t in targets]))
        batches.append((ImageList(images.tensors.to(dev), images.sizes), PackedTargets(targets, dev)))
    teacher = build("darknet53", "bf16", 2, dev, BIAS).eval()
    student = build("darknet53", "bf16", 1, dev).train()
    student._debug_keys = keys_ref[ref_to_packed_rows(B, levels)].to(dev)
    opt = FusedClipAdamW(student, lr=1e-3, weight_decay=1e-4, eps=1e-8, max_norm=1.0)
    gs = GroupedTeacherKDStep(teacher, student, opt, (0.1, 1.0, 5.0), group=group)
    for i in range(2 * group):
        assert gs(*batches[i % 2]) is None
    ld = gs(*batches[0])
    torch.cuda.synchronize()
    got = {k: float(v) for k, v in ld.items()}
    gn = float(opt.grad_norm())
    assert int(ops.lib.kd6d_barrier_timeouts()) == 0
    ref = O.KDStepRef("darknet53", "darknet53", K=INTERNAL_K, diameters=MESH_DIAMETERS, kd_weight=5.0,
                      teacher_cls_bias=BIAS, emulate_bf16=True)
    res = ref.step(*cpu_batches[0], choose=_chooser(keys_ref, levels))
    ref_grads = {k: p.grad.clone() for k, p in ref.student.named_parameters() if p.grad is not None}
    clip = min(1.0, 1.0 / (res["grad_norm"] + 1e-6))
    rep = _grad_report(student, ref_grads, clip, res["grad_norm"])
    rep.update({"d_" + k: abs(got[k] - res[k]) / max(abs(res[k]), 1e-6) for k in got},
               d_grad_norm=abs(gn - res["grad_norm"]) / res["grad_norm"])
    print("[darknet53 student, B=16 256x256 bf16 grouped] %s" % json.dumps(rep, default=str))
    assert res["loss_kd"] > 0
    assert rep["d_loss_cls"] <= tol["loss"] and rep["d_loss_reg"] <= tol["loss"], rep
    assert rep["d_loss_kd"] <= tol["kd"], rep
    assert rep["d_grad_norm"] <= tol["gn"] and rep["total"] <= tol["gn"], rep
    assert rep["worst_norm"] <= tol["worst"] and rep["wmean_norm"] <= tol["wmean"], rep
    assert rep["worst_norm_1k"] <= tol["worst1k"], rep
    assert 1.0 - rep["cosine"] <= 1.2e-3, rep


# ---------------------------------------------------------------------------------------------------------
# 6. the teacher recipe through train_kd.py, its final.pth as the KD teacher
# ---------------------------------------------------------------------------------------------------------
def test_teacher_recipe_trains_and_its_checkpoint_is_the_kd_teacher(gpu_device, tmp_path):
    """train.sh's third recipe (--backbone darknet53 --kd_weight 0.) with --synthetic --max_iters 3, pipelined grouped
    launch: exits 0, writes final.pth and latest.pth with the reference's key names.  That final.pth as --weight_file_t
    of the KD recipe (darknet_tiny_h student) loads, and the teacher built from it computes bitwise the eval-mode logits
    of the Darknet-53 network built from the same file."""
    from kd6d.libs.train_libs import build_model_teacher
    from kd6d.models.model_kd import PoseModuleKD
    from kd6d.arguments.argument_kd import get_args
    from kd6d.synthetic import make_batch
    from oracle import kd_step_ref as O
    cfgf = os.path.join(ROOT, "configs", "ape.yaml")
    wd = str(tmp_path / "darknet53")
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "train_kd.py"),
           "--config_file", cfgf, "--config_file_t", cfgf, "--backbone", "darknet53", "--backbone_t", "darknet53",
           "--weight_file_t", "None", "--kd_weight", "0.", "--working_dir", wd, "--synthetic", "--max_iters", "3",
           "--launch", "pipeline", "--teacher_group", "3", "--batch_size", "2", "--image_size", "128",
           "--skip_teacher_eval", "--val_freq", "3", "--num_workers", "0"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    final = os.path.join(wd, "final.pth")
    assert os.path.exists(final) and os.path.exists(os.path.join(wd, "latest.pth"))
    sd = torch.load(final, map_location="cpu")
    ref_keys = set(O.PoseNetRef("darknet53").state_dict())
    assert ref_keys <= set(sd), sorted(ref_keys - set(sd))[:5]
    assert int(sd["backbone.features.stage3.unit2.conv2.bn.num_batches_tracked"]) == 3

    _, cfg_t = get_args(["--config_file", cfgf, "--config_file_t", cfgf, "--backbone", "darknet_tiny_h",
                         "--backbone_t", "darknet53", "--weight_file_t", final, "--synthetic"])
    import io
    import contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model_t = build_model_teacher(cfg_t, PoseModuleKD, gpu_device)
    assert "Weights are loaded from " + final in buf.getvalue(), buf.getvalue()
    model_t.eval()
    direct = build("darknet53", cfg_t["RUNTIME"]["PRECISION"], 1, gpu_device)
    direct.load_state_dict(sd)
    direct.eval()
    images, _ = make_batch(2, 77, crop=128)
    x = images.tensors.to(gpu_device)
    with torch.no_grad():
        a = [t.clone() for t in model_t.net.forward(x)]
        b = [t.clone() for t in direct.net.forward(x)]
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------
# 7. the benchmark surface (bench.py unchanged)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3])
def test_bench_runs_with_a_darknet53_student(gpu_device, group):
    """`bench.py --student darknet53` prints one valid JSON line and exits 0 (flop_per_step falls back when
    FLOP_PER_IMG has no entry for the student)."""
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5",
           "--warmup", "2", "--student", "darknet53", "--teacher-group", str(group)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    rec = json.loads(lines[0])
    print("[bench darknet53 student, teacher-group %d] %s" % (group, lines[0]))
    assert rec["unit"] == "images/s" and rec["value"] > 0 and rec["finite"], rec
    assert rec["config"]["teacher_group"] == group and rec["barrier_timeouts"] == 0, rec
