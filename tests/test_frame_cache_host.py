"""CPU side of the device-resident frame cache (kd6d/libs/frame_cache.py, --frame_cache device): the flags, the
refusals (budget, mixed frame sizes, too many instances, out-of-range slots), the host annotation table against
PackedTargets, the resample rule against BOP_Dataset.__getitem__, and the C entry points' argument checks.  The cache
itself is built on the CPU device here: the gather kernels are what tests/test_frame_cache_gpu.py covers."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import frame_cache_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return C.write_cache_tree(str(tmp_path_factory.mktemp("frame_cache")))


def test_flags_defaults_parsing_and_synthetic_refusal():
    from kd6d.arguments import argument, argument_kd
    ape = os.path.join(ROOT, "configs", "ape.yaml")
    base = ["--config_file", ape, "--config_file_t", ape]
    cfg, cfg_t = argument_kd.get_args(base)
    assert cfg["RUNTIME"]["FRAME_CACHE"] == "off" and cfg["RUNTIME"]["FRAME_CACHE_GB"] == 64.0
    cfg, _ = argument_kd.get_args(base + ["--frame_cache", "device", "--frame_cache_gb", "1.5"])
    assert cfg["RUNTIME"]["FRAME_CACHE"] == "device" and cfg["RUNTIME"]["FRAME_CACHE_GB"] == 1.5
    with pytest.raises(SystemExit) as e:
        argument_kd.get_args(base + ["--frame_cache", "device", "--synthetic"])
    assert "--frame_cache device" in str(e.value) and "--synthetic" in str(e.value)
    with pytest.raises(SystemExit):
        argument_kd.get_args(base + ["--frame_cache", "host"])            # not a choice
    # test.py's parser
    cfg = argument.get_args(["--config_file", ape])
    assert cfg["RUNTIME"]["FRAME_CACHE"] == "off" and cfg["RUNTIME"]["FRAME_CACHE_GB"] == 64.0
    cfg = argument.get_args(["--config_file", ape, "--frame_cache", "device", "--frame_cache_gb", "2"])
    assert cfg["RUNTIME"]["FRAME_CACHE"] == "device" and cfg["RUNTIME"]["FRAME_CACHE_GB"] == 2.0
    with pytest.raises(SystemExit) as e:
        argument.get_args(["--config_file", ape, "--frame_cache", "device", "--synthetic"])
    assert "--synthetic" in str(e.value)
    # the help text says that every rank caches the whole list
    text = argument_kd.get_argparser().format_help()
    assert re.search(r"rank\s+caches\s+the\s+whole\s+list", text, re.I)


def test_budget_refusal_names_both_sizes_and_allocates_nothing(tree, monkeypatch):
    from kd6d.libs import frame_cache as FC
    calls = []
    real = FC._allocate
    monkeypatch.setattr(FC, "_allocate", lambda *a, **k: calls.append(a) or real(*a, **k))
    need = 7 * C.H * C.W * 4
    with pytest.raises(ValueError) as e:
        FC.DeviceFrameCache(C.datasets(tree), "cpu", need - 1, log=None)
    assert str(need) in str(e.value) and str(need - 1) in str(e.value)
    assert calls == []
    cache = FC.DeviceFrameCache(C.datasets(tree), "cpu", need, log=None)      # exactly enough
    assert calls and cache.nbytes == 6 * C.H * C.W * 4
    # build_dataset passes --frame_cache_gb on (GiB -> bytes) and does not fall back to the host loader
    from kd6d.libs.train_libs import build_dataset
    with pytest.raises(ValueError, match="frame_cache_gb"):
        build_dataset(C.make_cfg(tree), "cpu", frame_cache="device", frame_cache_gb=(need - 1) / 2.0 ** 30)
    with pytest.raises(ValueError, match="frame_cache must be"):
        build_dataset(C.make_cfg(tree), "cpu", frame_cache="host")


def test_mixed_frame_sizes_raise_naming_both_paths(tree):
    from torch.utils.data import ConcatDataset
    from kd6d.libs.frame_cache import DeviceFrameCache
    both = ConcatDataset([C.datasets(tree, training=False), C.datasets(tree, training=False, key="small_list")])
    with pytest.raises(ValueError) as e:
        DeviceFrameCache(both, "cpu", 1 << 30, log=None)
    first = os.path.join(tree["scene"], "rgb", "000001.png")
    assert first in str(e.value) and tree["small_path"] in str(e.value)
    assert "52x37" in str(e.value) and "24x20" in str(e.value)


def test_too_many_instances_raise_like_packed_targets():
    from kd6d.kd_losses import MAX_GT, PackedTargets
    from kd6d.libs.frame_cache import table_rows
    from kd6d.libs.poses import PoseAnnot
    g = MAX_GT + 1
    with pytest.raises(ValueError) as e:
        table_rows(np.eye(3), [0] * g, [np.eye(3)] * g, [np.zeros((3, 1))] * g)
    t = PoseAnnot(torch.zeros(2, 8, 3), torch.eye(3), torch.zeros(4, 4), torch.zeros(g, dtype=torch.long),
                  torch.zeros(g, 3, 3), torch.zeros(g, 3, 1), 4, 4, torch.ones(()), torch.zeros(2, 3))
    with pytest.raises(ValueError) as e2:
        PackedTargets([t], "cpu")
    assert str(e.value) == str(e2.value)


@pytest.mark.parametrize("training", [True, False])
def test_table_rows_equal_packed_targets(tree, training):
    """Every frame's row of the host table (and of its device copy) is what PackedTargets([item target]) holds."""
    from kd6d._lib import MAX_GT
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.frame_cache import DeviceFrameCache
    ds = C.datasets(tree, training=training)
    cache = DeviceFrameCache(ds, "cpu", 1 << 30, log=None)
    assert cache.table_f.shape == (cache.n, 9 + MAX_GT * 12) and cache.table_i.shape == (cache.n, 1 + MAX_GT)
    assert cache.frames.shape == (cache.n, C.H, C.W, 3) and cache.frames.dtype == torch.uint8
    assert cache.masks.shape == (cache.n, C.H, C.W) and cache.masks.dtype == torch.uint8
    assert cache.n == (6 if training else 7) and cache.n_invalid == (1 if training else 0) and len(cache) == 7
    seen_counts = set()
    for i in range(len(ds)):
        item = ds.getitem1(i)
        slot = cache.slot_of[i]
        if item is None:
            assert slot < 0 and ds.img_files[i].endswith("%06d.png" % C.UNKNOWN_ONLY)
            continue
        frame, target, meta = item
        target.bbox_trans = torch.zeros(2, 3)
        pt = PackedTargets([target], "cpu")
        rf, ri = cache.table_f[slot], cache.table_i[slot]
        assert np.array_equal(rf[0:9], pt.K.numpy().reshape(-1))
        assert np.array_equal(rf[9:9 + MAX_GT * 9], pt.rot.numpy().reshape(-1))             # padding included
        assert np.array_equal(rf[9 + MAX_GT * 9:], pt.trans.numpy().reshape(-1))
        assert ri[0] == int(pt.n_gt[0]) and np.array_equal(ri[1:], pt.class_ids.numpy().reshape(-1))
        assert np.array_equal(cache.table_f_dev.numpy()[slot], rf) and np.array_equal(cache.table_i_dev.numpy()[slot], ri)
        assert torch.equal(cache.kp3d_dev, pt.kp3d[0])
        # the stored frame and mask are the item's, and the meta keeps its shape
        assert torch.equal(cache.frames[slot], frame)
        assert torch.equal(cache.masks[slot].to(torch.float32), target.mask)
        m = cache.metas[slot]
        assert set(m) == set(meta) and m["path"] == meta["path"] and np.array_equal(m["K"], meta["K"])
        assert m["class_ids"] == meta["class_ids"]
        assert all(np.array_equal(a, b) for a, b in zip(m["rotations"] + m["translations"],
                                                        meta["rotations"] + meta["translations"]))
        seen_counts.add(int(ri[0]))
    assert seen_counts == ({1, 2, 3} if training else {0, 1, 2, 3})


def test_invalid_frame_has_no_slot_and_is_resampled_like_getitem(tree):
    from kd6d.libs.frame_cache import DeviceFrameCache
    random.seed(3)
    ds = C.datasets(tree, training=True)                  # (shuffles its list with `random`)
    cache = DeviceFrameCache(ds, "cpu", 1 << 30, log=None)
    bad = [i for i in range(len(ds)) if cache.slot_of[i] < 0]
    assert len(bad) == 1 and sorted(s for s in cache.slot_of if s >= 0) == list(range(6))
    state = random.getstate()
    for seed in range(6):
        random.seed(seed)
        want = [ds[i][2]["path"] for i in (bad[0], 0, bad[0], bad[0], 3)]
        after = random.getstate()
        random.seed(seed)
        got = [cache.metas[cache.resolve(i)]["path"] for i in (bad[0], 0, bad[0], bad[0], 3)]
        assert got == want and random.getstate() == after
    random.setstate(state)
    with pytest.raises(IndexError):
        cache.resolve(len(ds))
    # the host-side validation of gather indices
    cache.check_slots([0, 5, 5])
    for slots in ([6], [-1], [0, 7]):
        with pytest.raises(IndexError):
            cache.check_slots(slots)
        with pytest.raises(IndexError):
            cache.upload_slots(slots)


def test_from_packed_refuses_other_layouts():
    from kd6d.kd_losses import PackedTargets
    with pytest.raises(ValueError, match="packed layout"):
        PackedTargets.from_packed(torch.zeros(2, 4, 4), torch.zeros(10), torch.zeros(12, dtype=torch.int32), 2)


def test_entry_points_check_arguments_without_a_device():
    from kd6d import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(64)             # never dereferenced: the argument checks come first
    rc = lib.kd6d_cache_gather_frames(None, None, 7, 37, 52, None, 5, None, None, None)
    assert rc == -1 and b"kd6d_cache_gather_frames: null pointer" in lib.kd6d_last_error()
    rc = lib.kd6d_cache_gather_frames(one, one, 7, 37, 52, one, 5, one, None, None)
    assert rc == -1 and b"null pointer" in lib.kd6d_last_error()
    for B in (0, -3):
        rc = lib.kd6d_cache_gather_frames(one, one, 7, 37, 52, one, B, one, one, None)
        assert rc == -1 and b"bad sizes" in lib.kd6d_last_error() and (b"B=%d" % B) in lib.kd6d_last_error()
    rc = lib.kd6d_cache_gather_frames(one, one, 0, 37, 52, one, 5, one, one, None)
    assert rc == -1 and b"bad sizes" in lib.kd6d_last_error()
    rc = lib.kd6d_cache_gather_frames(one, one, 7, 37, 52, one, 5, one, ctypes.c_void_p(66), None)
    assert rc == -1 and b"aligned" in lib.kd6d_last_error()
    rc = lib.kd6d_cache_gather_targets(None, None, None, 48, 7, None, 5, None, None, None, None)
    assert rc == -1 and b"kd6d_cache_gather_targets: null pointer" in lib.kd6d_last_error()
    rc = lib.kd6d_cache_gather_targets(one, one, one, 48, 7, one, 5, None, one, one, None)
    assert rc == -1 and b"null pointer" in lib.kd6d_last_error()
    for B in (0, -1):
        rc = lib.kd6d_cache_gather_targets(one, one, one, 48, 7, one, B, one, one, one, None)
        assert rc == -1 and b"bad sizes" in lib.kd6d_last_error()
    rc = lib.kd6d_cache_gather_targets(one, one, one, 46, 7, one, 5, one, one, one, None)     # kp_elems % 4
    assert rc == -1 and b"kp_elems=46" in lib.kd6d_last_error()
    with pytest.raises(_lib.Kd6dError, match="bad sizes"):
        _lib.check(rc, "kd6d_cache_gather_targets")


def test_header_symbols_bound_and_abi_version_matches():
    from kd6d import _lib
    src = open(os.path.join(ROOT, "include", "kd6d.h")).read()
    for name in ("kd6d_cache_gather_frames", "kd6d_cache_gather_targets"):
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    ver = int(re.search(r"#define KD6D_ABI_VERSION (\d+)", src).group(1))
    assert ver == _lib.ABI_VERSION == _lib.lib.kd6d_abi_version()
    assert re.search(r"#define KD6D_CACHE_ROW_F \(9 \+ KD6D_MAX_GT \* 12\)", src) and _lib.CACHE_ROW_F == 9 + _lib.MAX_GT * 12
    assert re.search(r"#define KD6D_CACHE_ROW_I \(1 \+ KD6D_MAX_GT\)", src) and _lib.CACHE_ROW_I == 1 + _lib.MAX_GT
    # packed sizes agree with PackedTargets' own layout
    from kd6d import ops
    from kd6d.kd_losses import PackedTargets
    from kd6d.libs.poses import PoseAnnot
    t = PoseAnnot(torch.zeros(2, 8, 3), torch.eye(3), torch.zeros(4, 4), torch.zeros(1, dtype=torch.long),
                  torch.zeros(1, 3, 3), torch.zeros(1, 3, 1), 4, 4, torch.ones(()), torch.zeros(2, 3))
    for B in (1, 3, 5):
        pt = PackedTargets([t] * B, "cpu")
        assert (pt.flat_f.numel(), pt.flat_i.numel()) == ops.cache_target_sizes(B, 48)
