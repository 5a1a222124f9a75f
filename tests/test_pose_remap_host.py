"""CPU side of --aug_pose_remap device (kd6d_pose_remap, csrc/pnp.hip): the item's draws do not depend on the mode, the
device mode solves nothing on the host, the collated layout is the header's, the flag, the argument checks of the C
entry, and the self-consistency of the expected values in tests/pose_remap_cases.py."""
import ctypes
import itertools
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pose_remap_cases as C  # noqa: E402


def _cfg(mode, occlusion=True, ssr=True, hsv=True, smooth=True, noise=True):
    solver = dict(AUGMENTATION_OCCLUSION=0.5 if occlusion else 0, AUGMENTATION_SHIFT=0.05 if ssr else 0,
                  AUGMENTATION_SCALE=0.05 if ssr else 0, AUGMENTATION_ROTATION=10 if ssr else 0,
                  AUGMENTATION_ColorH=0.1 if hsv else 0, AUGMENTATION_ColorS=0.2 if hsv else 0,
                  AUGMENTATION_ColorV=0.2 if hsv else 0, AUGMENTATION_Smooth=5 if smooth else 0,
                  AUGMENTATION_Noise=0.05 if noise else 0)
    cfg = {"SOLVER": solver, "DATASETS": {},
           "INPUT": {"INTERNAL_K": C.internal_k().reshape(-1).tolist(), "INTERNAL_WIDTH": C.W, "INTERNAL_HEIGHT": C.H}}
    if mode is not None:
        cfg["RUNTIME"] = {"AUG_POSE_REMAP": mode}
    return cfg


def _item(seed=0, n=2):
    rng = np.random.default_rng(seed)
    Rs, Ts = C.poses(rng, n)
    K = C.other_camera(C.internal_k(), 0.8, 5.0, -3.0)
    return K, [1, 0, 2][:n], [r.tolist() for r in Rs], [t.tolist() for t in Ts], C.BOXES


POSE_KEYS = ("R_resize", "T_resize", "R", "T", "pose_src")


@pytest.mark.parametrize("stages", list(itertools.product((False, True), repeat=5)),
                         ids=lambda s: "".join("osHbn"[i] if on else "-" for i, on in enumerate(s)))
def test_device_mode_draws_what_host_mode_draws(stages):
    from kd6d.libs.augment import AugConfig, draw_params
    got = {}
    for mode in ("host", "device"):
        ac = AugConfig(_cfg(mode, *stages))
        random.seed(1234)
        p = draw_params(ac, *_item())
        got[mode] = (p, random.random())
    (ph, nh), (pd, nd) = got["host"], got["device"]
    assert nh == nd, "the two modes consumed `random` differently"
    keys_h, keys_d = set(ph) - set(POSE_KEYS), set(pd) - set(POSE_KEYS)
    assert keys_h == keys_d and {"M_resize", "key", "n"} <= keys_h
    assert ("M_ssr" in keys_h) == stages[1] and ("occl_u" in keys_h) == stages[0]
    for k in keys_h:
        a, b = np.asarray(ph[k]), np.asarray(pd[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert set(ph) & set(POSE_KEYS) == {"R_resize", "T_resize", "R", "T"}
    assert set(pd) & set(POSE_KEYS) == {"pose_src"}


def test_default_mode_is_host_and_unknown_modes_are_refused():
    from kd6d.libs.augment import AugConfig
    assert AugConfig(_cfg(None)).pose_remap == "host"
    assert AugConfig(_cfg("device")).pose_remap == "device"
    with pytest.raises(ValueError, match="AUG_POSE_REMAP"):
        AugConfig(_cfg("gpu"))


def test_device_mode_calls_no_solver(monkeypatch):
    from kd6d.libs import augment as A

    def boom(*a, **k):
        raise AssertionError("the host solver was called")
    monkeypatch.setattr(A, "remap_pose", boom)
    K, cls, Rs, Ts, boxes = _item()
    p = A.draw_params(A.AugConfig(_cfg("device")), K, cls, Rs, Ts, boxes)
    src = p["pose_src"]
    assert all(src[k].dtype == np.float64 for k in ("K", "rotations", "translations"))
    assert np.array_equal(src["K"], K) and np.array_equal(src["rotations"], np.asarray(Rs))
    assert np.array_equal(src["translations"], np.asarray(Ts)) and src["class_ids"].tolist() == cls
    with pytest.raises(AssertionError, match="host solver"):
        A.draw_params(A.AugConfig(_cfg("host")), K, cls, Rs, Ts, boxes)


def test_collate_params_lays_the_instances_out_for_the_kernel():
    from kd6d.libs import augment as A
    ac = A.AugConfig(_cfg("device"))
    items = [_item(seed=s, n=n) for s, n in ((1, 2), (2, 0), (3, 3), (4, 1))]
    random.seed(7)
    ps = [A.draw_params(ac, *it) for it in items]
    out = A.collate_params(ps)
    assert not set(out) & {"R_resize", "T_resize", "R", "T"}
    src = out["pose_src"]
    assert src["inst_img"].dtype == np.int32 and src["inst_img"].tolist() == [0, 0, 2, 2, 2, 3]
    assert src["inst_cls"].dtype == np.int32 and src["inst_cls"].tolist() == [1, 0, 1, 0, 2, 1]
    assert src["start"].tolist() == [0, 2, 2, 5, 6]
    assert src["src_K"].shape == (4, 9) and src["src_R"].shape == (6, 9) and src["src_T"].shape == (6, 3)
    assert all(src[k].dtype == np.float64 and src[k].flags["C_CONTIGUOUS"] for k in ("src_K", "src_R", "src_T"))
    for b, it in enumerate(items):
        assert np.array_equal(src["src_K"][b], np.asarray(it[0]).reshape(9))
        lo, hi = src["start"][b], src["start"][b + 1]
        assert np.array_equal(src["src_R"][lo:hi], np.asarray(it[2], np.float64).reshape(-1, 9))
        assert np.array_equal(src["src_T"][lo:hi], np.asarray(it[3], np.float64).reshape(-1, 3))
    assert out["M_resize"].shape == (4, 2, 3) and out["M_ssr"].shape == (4, 2, 3) and out["n"].tolist() == [2, 0, 3, 1]
    # host mode keeps its layout
    random.seed(7)
    host = A.collate_params([A.draw_params(A.AugConfig(_cfg("host")), *it) for it in items[:1]])
    assert "pose_src" not in host and host["R"][0].shape == (2, 3, 3) and host["T_resize"][0].shape == (2, 3, 1)


def test_flag_defaults_to_host_and_needs_augment():
    from kd6d.arguments.argument_kd import get_argparser, get_args
    assert get_argparser().parse_args([]).aug_pose_remap == "host"
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    base = ["--config_file", ape, "--config_file_t", ape]
    cfg, _ = get_args(base)
    assert cfg["RUNTIME"]["AUG_POSE_REMAP"] == "host"
    cfg, _ = get_args(base + ["--augment"])
    assert cfg["RUNTIME"]["AUG_POSE_REMAP"] == "host"
    cfg, _ = get_args(base + ["--augment", "--aug_pose_remap", "device"])
    assert cfg["RUNTIME"]["AUG_POSE_REMAP"] == "device" and cfg["RUNTIME"]["AUGMENT"] is True
    from kd6d.libs.augment import AugConfig
    assert AugConfig(cfg).pose_remap == "device"
    with pytest.raises(ValueError) as e:
        get_args(base + ["--aug_pose_remap", "device"])
    assert "--aug_pose_remap" in str(e.value) and "--augment" in str(e.value)
    with pytest.raises(SystemExit):
        get_argparser().parse_args(["--aug_pose_remap", "gpu"])


def _remap(lib, n_inst=4, n_images=2, n_class=3, null=None, ssr=True):
    p = ctypes.c_void_p(16)                  # never dereferenced: every call below fails its checks first
    K = (ctypes.c_double * 9)(*C.internal_k().reshape(-1))
    a = {k: p for k in ("inst_img", "inst_cls", "src_K", "src_R", "src_T", "box", "M_resize", "M_ssr", "pose", "ok")}
    a["dst_K"] = K
    if not ssr:
        a["M_ssr"] = None
    if null:
        a[null] = None
    return lib.kd6d_pose_remap(n_inst, n_images, n_class, a["inst_img"], a["inst_cls"], a["src_K"], a["src_R"], a["src_T"],
                               a["box"], a["dst_K"], a["M_resize"], a["M_ssr"], a["pose"], a["ok"], None)


def test_pose_remap_argument_checks_fail_loudly_without_gpu():
    from kd6d import _lib
    lib = _lib.lib
    src = open(os.path.join(ROOT, "include", "kd6d.h")).read()
    assert "kd6d_pose_remap" in src and "kd6d_pose_remap" in _lib.SIGNATURES
    assert _lib.lib.kd6d_abi_version() == _lib.ABI_VERSION
    for null in ("inst_img", "inst_cls", "src_K", "src_R", "src_T", "box", "dst_K", "M_resize", "pose", "ok"):
        assert _remap(lib, null=null) == -1, null
        assert b"kd6d_pose_remap: null pointer" in lib.kd6d_last_error(), null
    for kw, msg in ((dict(n_inst=0), b"n_inst=0"), (dict(n_inst=-3), b"n_inst=-3"), (dict(n_class=0), b"n_class=0"),
                    (dict(n_images=0), b"n_images=0"), (dict(n_inst=0, ssr=False), b"n_inst=0")):
        assert _remap(lib, **kw) == -1, kw
        assert msg in lib.kd6d_last_error(), (kw, lib.kd6d_last_error())
    with pytest.raises(_lib.Kd6dError, match="n_class=0"):
        _lib.check(_remap(lib, n_class=0), "kd6d_pose_remap")


def test_case_file_covers_what_it_must():
    names = [c["name"] for c in C.CASES]
    assert len(set(names)) == len(names)
    K = C.internal_k()
    assert np.array_equal(K.reshape(-1), [572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1])
    for c in C.CASES:
        assert np.array_equal(c["dst_K"], K)
        n = len(c["inst_img"])
        assert c["src_R"].shape == (n, 3, 3) and c["src_T"].shape == (n, 3) and c["box"].dtype == np.float32
        assert c["src_K"].shape[0] == c["M_resize"].shape[0] and int(c["inst_img"].max()) < c["src_K"].shape[0]
        z = c["src_T"][:, 2]
        assert np.all((z >= 300) & (z <= 2000))
    for b in C.BOXES:
        ext = b.max(0) - b.min(0)
        assert 100 - 1e-3 <= np.linalg.norm(ext) <= 290 + 1e-3 and len(set(np.round(ext, 3))) == 3
    assert C.by_name("pool")["src_R"].shape[0] == max(C.SIZES) == 256 and set(C.SIZES) == {1, 63, 64, 65, 256}
    assert len(set(C.by_name("pool")["inst_img"].tolist())) == 3 and len(set(C.by_name("pool")["inst_cls"].tolist())) == 3
    assert C.by_name("no_ssr_matrix")["M_ssr"] is None and C.by_name("two_images")["src_K"].shape[0] == 2
    fb = C.by_name("failures")["box"]
    assert len(np.unique(fb[1], axis=0)) == 1 and len(np.unique(fb[2], axis=0)) == 4
    # the SSR cases sit where they claim: the extreme draws of the limits
    M = C.by_name("ssr_ape_limits_a")["M_ssr"][0]
    assert abs(np.hypot(M[0, 0], M[0, 1]) - 1.05) < 1e-6 and abs(np.degrees(np.arctan2(M[0, 1], M[0, 0])) - 10.0) < 1e-4
    M = C.by_name("ssr_wide_a")["M_ssr"][0]
    assert abs(np.hypot(M[0, 0], M[0, 1]) - 0.7) < 1e-6 and abs(np.degrees(np.arctan2(M[0, 1], M[0, 0])) - 45.0) < 1e-4


@pytest.mark.parametrize("name", [c["name"] for c in C.CASES if c["name"] != "pool"] + ["pool[:65]"])
def test_expected_values_are_self_consistent(name):
    case = C.prefix(C.by_name("pool"), 65) if name == "pool[:65]" else C.by_name(name)
    pose, ok = C.expected(case)
    failing = C.FAILING.get(name, {})
    K = case["dst_K"]
    for i in range(len(case["inst_img"])):
        c = int(case["inst_cls"][i])
        if i in failing:
            assert ok[i].tolist() == [0, 0], (i, failing[i])
            want = C.source_pose32(case, i) if 0 <= c < len(case["box"]) else np.zeros(12, np.float32)
            assert np.array_equal(pose[i, 0].view(np.int32), want.view(np.int32)), (i, failing[i])
            assert np.array_equal(pose[i, 1].view(np.int32), want.view(np.int32)), (i, failing[i])
            continue
        assert ok[i].tolist() == [1, 1], i
        for s in range(2):
            R = pose[i, s, :9].astype(np.float64).reshape(3, 3)
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and np.linalg.det(R) > 0, (i, s)
        # Resize alone (and the identity) moves no projected point: the remapped pose is the source pose
        X = case["box"][c]
        gap = C.pixel_gap(K, X, pose[i, 0], np.concatenate([case["src_R"][i].reshape(9), case["src_T"][i]]))
        assert gap <= C.TOL_PX, (i, gap)
        if case["M_ssr"] is None:
            assert np.array_equal(pose[i, 1], pose[i, 0])


def test_front_end_refuses_a_batch_with_different_box_tables():
    import torch
    from kd6d.libs import augment as A
    from kd6d.libs.poses import PoseAnnot
    front = A.AugmentFront(A.AugConfig(_cfg("device")), "cpu")
    K = torch.eye(3)
    mk = lambda boxes: PoseAnnot(torch.from_numpy(boxes.copy()), K, None, torch.tensor([0]), torch.eye(3)[None],  # noqa: E731
                                 torch.zeros(1, 3, 1), C.W, C.H)
    same = [mk(C.BOXES), mk(C.BOXES)]
    table = front._box_table(same)
    assert table.shape == (3, 8, 3) and table.dtype == torch.float32 and front._box_table(same) is table
    with pytest.raises(ValueError, match="one 3D-box table per batch"):
        front._box_table([mk(C.BOXES), mk(C.BOXES[::-1])])
