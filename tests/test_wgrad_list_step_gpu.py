"""Option wgrad.list changes WHEN the reverse sweep's per-layer weight gradients are launched and how many share a launch,
never what they compute: three replayed steps of the smallest student of the step tests (darknet_tiny_h, B = 2, 64x64
crops, bf16) with a fork per layer (wgrad.list = 0) and with the lists of the library's default give equal losses,
gradient norms and parameters, element for element."""
import os

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(arch, precision):
    from kd6d.arguments.argument import custom_cfg
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["RUNTIME"] = {"PRECISION": precision}
    cfg["MODEL"]["BACKBONE"] = arch
    cfg = custom_cfg(cfg)
    cfg["KD"] = dict(LOSS_WEIGHT_KD=5.0, LEVEL="pred", GLEVEL="point", GTYPE="sinkhorn", GP=2.0, GBLUR=0.001, GnD=2,
                     WEIGHTED_OT=True, DETACH=False, SCALING=0.5, REACH=0.5)
    return cfg


def _build(arch, precision, seed, dev, cls_bias=None):
    from kd6d import backbone as BB
    from kd6d.models.model_kd import PoseModuleKD
    from oracle import kd_step_ref as O
    m = PoseModuleKD(_cfg(arch, precision), getattr(BB, arch)())
    sd = O.seeded_state_dict(O.PoseNetRef(arch), seed)
    if cls_bias is not None:
        sd["head.cls_logits.bias"] = torch.as_tensor(cls_bias, dtype=torch.float32)
    m.load_state_dict(sd)
    return m.to(dev)


def test_replayed_steps_do_not_depend_on_wgrad_list(gpu_device):
    from kd6d import ops
    from kd6d.graph import GraphedKDStep
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import ImageList
    from kd6d.optim import FusedClipAdamW
    from kd6d.synthetic import make_batch
    dev = gpu_device
    B, crop, arch = 2, 64, "darknet_tiny_h"
    teacher = _build("darknet53", "bf16", 2, dev, [1.0] + [-6.0] * 14).eval()
    batches = []
    for i in range(2):
        images, targets = make_batch(B, 10 + i, crop=crop)
        batches.append((ImageList(images.tensors.to(dev), images.sizes), PackedTargets(targets, dev)))
    rows = B * sum((crop // 8 // 2 ** i) ** 2 for i in range(4))
    keys = torch.rand(rows, generator=torch.Generator().manual_seed(3)).to(dev)
    chosen = ops.get_option("wgrad.list")          # the library's default: what the product path runs

    def run(value):
        forks = []
        with ops.option("wgrad.list", value):
            student = _build(arch, "bf16", 1, dev).train()
            student._debug_keys = keys
            opt = FusedClipAdamW(student, lr=1e-3)
            gs = GraphedKDStep(teacher, student, opt, (0.1, 1.0, 5.0), pipeline=False)
            flush = student.net.wgrad.flush_list

            def counted():
                forks.append(len(student.net.wgrad.pending))
                flush()
            student.net.wgrad.flush_list = counted
            hist = []
            for it in range(3):
                ld = gs(*batches[it % 2])
                hist.append([ld[k].clone() for k in ("loss_cls", "loss_reg", "loss_kd")] + [torch.as_tensor(opt.grad_norm()).clone()])
            torch.cuda.synchronize()
        return hist, student.net.store.params.clone(), [n for n in forks if n]

    h0, p0, f0 = run(0)
    h1, p1, f1 = run(chosen if chosen > 1 else 3)
    assert not f0, "wgrad.list = 0 must not collect anything"
    assert f1 and max(f1) > 1, "the lists were never used: the test compares the same path twice"
    for it, (a, b) in enumerate(zip(h0, h1)):
        for name, x, y in zip(("loss_cls", "loss_reg", "loss_kd", "grad_norm"), a, b):
            assert torch.equal(x, y), (it, name, float(x), float(y))
    assert float(h0[-1][2]) > 0, "the KD term must be active"
    assert torch.equal(p0, p1)
    assert ops.lib.kd6d_barrier_timeouts() == 0
