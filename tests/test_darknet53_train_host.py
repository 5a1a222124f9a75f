"""CPU: the pieces of Darknet-53 training (the reference's teacher recipe, train.sh) that need no device -- the C entry
point of the BatchNorm forward with the DarkUnit residual is exported, bound and rejects bad input before it touches a
device, and the recipe's command line configures a Darknet-53 student."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's train.sh, third recipe: the teacher is trained by train_kd.py with --kd_weight 0.
TEACHER_RECIPE = ["--config_file", os.path.join(ROOT, "configs", "ape.yaml"),
                  "--config_file_t", os.path.join(ROOT, "configs", "ape.yaml"),
                  "--backbone", "darknet53", "--backbone_t", "darknet53", "--weight_file_t", "None",
                  "--kd_weight", "0.", "--working_dir", "outputs/ape/darknet53"]


def test_bn_train_fwd_res_is_exported_and_bound():
    from kd6d import _lib, ops
    assert hasattr(_lib.lib, "kd6d_bn_train_fwd_res")
    assert "kd6d_bn_train_fwd_res" in _lib.SIGNATURES
    assert callable(ops.bn_train_fwd_res)


def test_bn_train_fwd_res_argument_checks_fail_loudly_without_gpu():
    from kd6d import _lib
    lib = _lib.lib
    p = 64          # never dereferenced: every call below fails its argument checks on the host

    def call(dtype=_lib.KD6D_BF16, x=p, res=p, y=p, rows=16, C=64):
        return lib.kd6d_bn_train_fwd_res(dtype, 1, x, res, y, rows, C, p, p, p, p, 1e-5, 0.1, p, p, p, p,
                                         _lib.ACT_LEAKY, None)

    assert call(C=12) == -1 and b"C=12" in lib.kd6d_last_error()
    assert call(dtype=_lib.KD6D_F32, C=6) == -1 and b"C=6" in lib.kd6d_last_error()
    assert call(dtype=7) == -1 and b"bad dtype" in lib.kd6d_last_error()
    assert call(res=None) == -1 and b"null residual" in lib.kd6d_last_error()
    assert call(rows=0) == -1 and b"bad arguments" in lib.kd6d_last_error()
    assert call(rows=-3) == -1 and b"bad arguments" in lib.kd6d_last_error()
    assert call(x=None) == -1 and b"bad arguments" in lib.kd6d_last_error()
    assert call(y=None) == -1 and b"bad arguments" in lib.kd6d_last_error()


def test_teacher_recipe_configures_a_darknet53_student():
    from kd6d.arguments.argument_kd import get_args
    from kd6d.engine import BACKBONE_CFG
    cfg, cfg_t = get_args(TEACHER_RECIPE)
    assert cfg["MODEL"]["BACKBONE"] == "darknet53"
    assert list(cfg["MODEL"]["FEAT_CHANNELS"]) == [0, 0, 256, 512, 1024]
    assert cfg["MODEL"]["OUT_CHANNEL"] == 256
    assert cfg_t["MODEL"]["BACKBONE"] == "darknet53"
    assert cfg["KD"]["LOSS_WEIGHT_KD"] == 0.0
    assert BACKBONE_CFG["darknet53"] == ([0, 0, 256, 512, 1024], 256)


def test_darknet53_student_network_layout():
    """The trainable Darknet-53 built on the host: 52 BatchNorm blocks, five pyramid levels, every convolution in the
    dgrad-packed weight set, and the reference's parameter names (what final.pth carries)."""
    import torch
    from kd6d.engine import PoseNet
    from oracle import kd_step_ref as O
    net = PoseNet("darknet53", torch.float32)
    assert len(net.bns) == 52 and net.n_levels == 5
    assert all(c.w.trainable for c in net.convs if c.name.startswith("backbone."))
    assert sum(1 for c in net.convs if c.name.startswith("backbone.")) == 52
    ref_names = set(O.PoseNetRef("darknet53").state_dict())
    ours = {n for n, _, _ in net.named_logical()}
    missing = {n for n in ref_names - ours if not n.endswith("num_batches_tracked") and "anchor" not in n}
    assert not missing, sorted(missing)[:5]
