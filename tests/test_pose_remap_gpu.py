"""GPU side of --aug_pose_remap device: kd6d_pose_remap (csrc/pnp.hip) on every case of tests/pose_remap_cases.py
against the host chain of kd6d.libs.pnp.remap_pose, its reproducibility and independence from the batch, the augmentation
front-end and the cached loader in both modes from the same seeds, and a short train_kd.py run.

Agreement criterion (tests/pose_remap_cases.py): the 8 box corners projected through INTERNAL_K with the device pose and
with the host pose differ by at most 1e-3 px."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import pose_remap_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                                # rows behind row n_inst that no launch may touch
NAN_BITS = 0x7FC5A5A5                    # the prefill of pose_out: a NaN no arithmetic produces
OK_FILL = -77
CHILD_TIMEOUT = 420


def _launch(case, dev, with_guards=True):
    """-> pose (n, 2, 12) float32, ok (n, 2) int32 as numpy, after checking the guard rows."""
    from kd6d import ops
    n = len(case["inst_img"])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()  # noqa: E731
    rows = n + (GUARD if with_guards else 0)
    pose = torch.full((rows, 2, 12), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    ok = torch.full((rows, 2), OK_FILL, dtype=torch.int32, device=dev)
    ops.pose_remap(t(case["inst_img"], torch.int32), t(case["inst_cls"], torch.int32), t(case["src_K"], torch.float64),
                   t(case["src_R"], torch.float64), t(case["src_T"], torch.float64), t(case["box"], torch.float32),
                   case["dst_K"], t(case["M_resize"], torch.float64),
                   None if case["M_ssr"] is None else t(case["M_ssr"], torch.float64), pose_out=pose, ok_out=ok)
    torch.cuda.synchronize()
    bits = pose.view(torch.int32).cpu().numpy()
    okh = ok.cpu().numpy()
    assert (bits[n:] == NAN_BITS).all() and (okh[n:] == OK_FILL).all(), "rows behind n_inst were written"
    assert not (bits[:n] == NAN_BITS).any(), "a row below n_inst was left unwritten"
    assert np.isin(okh[:n], (0, 1)).all()
    return bits[:n].view(np.float32), okh[:n]


def _case(name):
    if name.startswith("pool[:"):
        return C.prefix(C.by_name("pool"), int(name[6:-1]))
    return C.by_name(name)


NAMES = [c["name"] for c in C.CASES if c["name"] != "pool"] + ["pool[:%d]" % n for n in C.SIZES]


@pytest.mark.parametrize("name", NAMES)
def test_cases_agree_with_the_host_chain(gpu_device, name):
    case = _case(name)
    want, want_ok = C.expected(case)
    got, ok = _launch(case, gpu_device)
    assert np.array_equal(ok, want_ok), (ok.tolist(), want_ok.tolist())
    worst = 0.0
    for i in range(len(ok)):
        c = int(case["inst_cls"][i])
        for s in range(2):
            if not want_ok[i, s]:
                # no pose: the stage's source pose as its fp32 rounding, bit for bit (zeros for a class outside the table)
                if not 0 <= c < len(case["box"]):
                    src = np.zeros(12, np.float32)
                else:
                    src = C.source_pose32(case, i) if s == 0 else got[i, 0]
                assert np.array_equal(got[i, s].view(np.int32), src.view(np.int32)), (i, s)
                if s == 0 or not want_ok[i, 0]:              # the host's chain went on from the same bits
                    assert np.array_equal(got[i, s].view(np.int32), want[i, s].view(np.int32)), (i, s)
                continue
            gap = C.pixel_gap(case["dst_K"], case["box"][c], got[i, s], want[i, s])
            worst = max(worst, gap)
            assert gap <= C.TOL_PX, (i, s, gap)
    print("pose_remap %s: worst corner gap %.3e px over %d instances" % (name, worst, len(ok)))


def test_two_launches_are_bitwise_equal(gpu_device):
    case = C.by_name("pool")
    a, oa = _launch(case, gpu_device)
    b, ob = _launch(case, gpu_device)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(oa, ob)


def test_an_instance_does_not_depend_on_its_batch(gpu_device):
    """Alone, and at another position of another batch (other neighbours, the images listed in another order), an
    instance gets the bits it gets in the full launch."""
    pool = C.by_name("pool")
    full, full_ok = _launch(pool, gpu_device)
    for i in (0, 63, 64, 200):
        one = C.prefix(pool, 1)
        for k in ("inst_img", "inst_cls", "src_R", "src_T"):
            one[k] = pool[k][i:i + 1].copy()
        got, ok = _launch(one, gpu_device)
        assert np.array_equal(got[0].view(np.int32), full[i].view(np.int32)) and np.array_equal(ok[0], full_ok[i]), i
    # another batch: 70 instances in reverse order, behind 5 instances of the failure case's kind, images permuted
    pick = np.arange(199, 129, -1)
    perm = np.array([2, 0, 1])                       # new image index of old image b
    other = dict(pool, name="other")
    inv = np.argsort(perm)
    other["src_K"], other["M_resize"], other["M_ssr"] = pool["src_K"][inv], pool["M_resize"][inv], pool["M_ssr"][inv]
    other["inst_img"] = np.concatenate([np.zeros(5, np.int32), perm[pool["inst_img"][pick]].astype(np.int32)])
    other["inst_cls"] = np.concatenate([np.array([9, 0, 1, 2, -4], np.int32), pool["inst_cls"][pick]])
    other["src_R"] = np.concatenate([pool["src_R"][:5], pool["src_R"][pick]])
    other["src_T"] = np.concatenate([pool["src_T"][:5], pool["src_T"][pick]])
    got, ok = _launch(other, gpu_device)
    assert np.array_equal(got[5:].view(np.int32), full[pick].view(np.int32)) and np.array_equal(ok[5:], full_ok[pick])


# ---- the augmentation front-end in both modes ---------------------------------------------------------------------------
FH, FW = 60, 80                           # source frames
IH, IW = 48, 64                           # INTERNAL_HEIGHT / _WIDTH of the front-end test


def _front_cfg(mode):
    K = [560.3, 0, 31.47, 0, 561.1, 23.53, 0, 0, 1]       # not exact in fp32: the device solver's K is rounded
    solver = dict(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_SHIFT=0.05, AUGMENTATION_SCALE=0.05, AUGMENTATION_ROTATION=10,
                  AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2, AUGMENTATION_ColorV=0.2, AUGMENTATION_Smooth=3,
                  AUGMENTATION_Noise=0.05, AUGMENTATION_Grayscalize=False)
    return {"SOLVER": solver, "DATASETS": {"SYMMETRY_TYPES": {}}, "RUNTIME": {"AUG_POSE_REMAP": mode},
            "INPUT": {"INTERNAL_K": K, "INTERNAL_WIDTH": IW, "INTERNAL_HEIGHT": IH}}


def _front_batch():
    """3 frames: (0) two instances that stay, (1) one that stays and one of 4 px that remove_invalids drops, (2) two of
    4 px each: no instance is left and the frame falls back to its Resize-only pose."""
    from kd6d.libs.poses import PoseAnnot
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (3, FH, FW, 3), dtype=np.uint8)
    masks = np.zeros((3, FH, FW), np.float32)
    masks[0, 8:34, 6:36] = 1; masks[0, 30:54, 44:74] = 2
    masks[1, 10:44, 20:62] = 1; masks[1, 50:52, 4:6] = 2
    masks[2, 20:22, 30:32] = 1; masks[2, 40:42, 50:52] = 2
    boxes = torch.from_numpy(C.BOXES.copy())
    items = []
    for b, cls in enumerate(([0, 2], [1, 0], [2, 1])):
        K = np.array([[600.0 + 10 * b, 0, 0.5 * FW + b], [0, 598.0, 0.5 * FH - b], [0, 0, 1.0]])
        Rs, Ts = C.poses(rng, 2)
        Ts[:, :2] *= 0.05                 # the small frames see +-3 degrees: keep the objects near the axis
        t = PoseAnnot(boxes, torch.tensor(K, dtype=torch.float32), torch.from_numpy(masks[b]), torch.tensor(cls),
                      torch.tensor(Rs, dtype=torch.float32), torch.tensor(Ts.reshape(-1, 3, 1), dtype=torch.float32), FW, FH)
        items.append((t, K, cls, Rs.tolist(), Ts.tolist()))
    return frames, masks, items


def _run_front(mode, dev):
    from kd6d.libs import augment as A
    ac = A.AugConfig(_front_cfg(mode))
    frames, masks, items = _front_batch()
    random.seed(77)
    params = A.collate_params([A.draw_params(ac, K, cls, Rs, Ts, C.BOXES) for _, K, cls, Rs, Ts in items])
    front = A.AugmentFront(ac, dev)
    f, m, out = front.run(torch.from_numpy(frames).to(dev), torch.from_numpy(masks).to(dev), [it[0] for it in items], params)
    torch.cuda.synchronize()
    return f.cpu(), m.cpu(), out, params


def test_front_end_host_mode_against_device_mode(gpu_device, capsys):
    fh, mh, oh, ph = _run_front("host", gpu_device)
    fd, md, od, pd = _run_front("device", gpu_device)
    assert "Error in pose remapping!" not in capsys.readouterr().out
    assert fh.shape == (3, IH, IW, 3) and torch.equal(fh, fd), "frames depend on matrices and areas, not on poses"
    assert torch.equal(mh.view(torch.int32), md.view(torch.int32))
    # the situations the batch was built for
    assert [len(o[0]) for o in oh] == [2, 1, 2]
    assert oh[1][0].tolist() == [1]
    assert np.array_equal(oh[2][1], ph["R_resize"][2]) and not np.array_equal(oh[2][1], ph["R"][2])
    K = np.array(_front_cfg("host")["INPUT"]["INTERNAL_K"]).reshape(3, 3)
    worst = 0.0
    for b in range(3):
        assert oh[b][0].tolist() == od[b][0].tolist() and oh[b][0].dtype == od[b][0].dtype
        assert oh[b][1].shape == od[b][1].shape and oh[b][2].shape == od[b][2].shape
        assert oh[b][1].dtype == od[b][1].dtype == np.float32 and oh[b][2].dtype == od[b][2].dtype == np.float32
        for i, c in enumerate(oh[b][0]):
            a = np.concatenate([oh[b][1][i].reshape(9), oh[b][2][i].reshape(3)])
            d = np.concatenate([od[b][1][i].reshape(9), od[b][2][i].reshape(3)])
            worst = max(worst, C.pixel_gap(K, C.BOXES[int(c)], a, d))
        for k in ("R_resize", "T_resize", "R", "T"):
            assert pd[k][b].shape == ph[k][b].shape and pd[k][b].dtype == ph[k][b].dtype, (k, b)
    print("front end: worst corner gap %.3e px" % worst)
    assert worst <= C.TOL_PX
    for k in ("M_resize", "M_ssr", "occl_u", "hsv", "ksize", "sigma", "key"):
        assert np.array_equal(ph[k], pd[k]), k


# ---- the cached loader on the BOP fixture tree ---------------------------------------------------------------------------
def test_front_end_reports_failed_remaps_like_the_host(gpu_device, capsys):
    """One instance with a non-finite translation: the host chain prints its line once per remap it runs -- once
    without an SSR stage, twice with one (stage 2 starts from the unusable pose) -- and so does the device mode."""
    from kd6d.libs import augment as A
    for ssr in (False, True):
        lines = {}
        for mode in ("host", "device"):
            cfg = _front_cfg(mode)
            if not ssr:
                cfg["SOLVER"].update(AUGMENTATION_SHIFT=0, AUGMENTATION_SCALE=0, AUGMENTATION_ROTATION=0)
            ac = A.AugConfig(cfg)
            frames, masks, items = _front_batch()
            items[0][4][1][0] = float("inf")
            capsys.readouterr()
            random.seed(78)
            params = A.collate_params([A.draw_params(ac, K, cls, Rs, Ts, C.BOXES) for _, K, cls, Rs, Ts in items])
            assert ("M_ssr" in params) == ssr
            A.AugmentFront(ac, gpu_device).run(torch.from_numpy(frames).to(gpu_device), torch.from_numpy(masks).to(gpu_device),
                                               [it[0] for it in items], params)
            torch.cuda.synchronize()
            lines[mode] = capsys.readouterr().out.count("Error in pose remapping!")
            assert np.isinf(params["T"][0][1]).any() and np.isfinite(params["T"][0][0]).all()
        assert lines["host"] == (2 if ssr else 1) and lines["device"] == lines["host"], (ssr, lines)


def _tree_cfg(tree, mode, workers=0):
    from test_step_gpu import make_cfg
    cfg = make_cfg("darknet_tiny_h", "fp32")
    cfg["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], MESH_DIR=tree["models"], BBOX_FILE=tree["bbox"],
                           N_CLASS=3, SYMMETRY_TYPES={})
    # close to the fixture's cameras (fx 572.4, cx 15..21, cy 10) but not equal: Resize is a real warp; not exact in fp32
    cfg["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=[565.3, 0, 13.47, 0, 566.1, 10.53, 0, 0, 1])
    cfg["SOLVER"].update(IMS_PER_BATCH=2, AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_SHIFT=0.05, AUGMENTATION_SCALE=0.05,
                         AUGMENTATION_ROTATION=10, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2, AUGMENTATION_ColorV=0.2,
                         AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05, AUGMENTATION_Grayscalize=False)
    cfg["RUNTIME"].update(N_GPU=1, DISTRIBUTED=False, NUM_WORKERS=workers, AUG_POSE_REMAP=mode)
    return cfg


@pytest.mark.parametrize("frame_cache,workers", [("device", 0), ("off", 1)], ids=["cached", "host_loader_1_worker"])
def test_loader_host_mode_against_device_mode(gpu_device, tmp_path, frame_cache, workers):
    """One batch of the BOP fixture tree in both modes from the same seeds: through CachedDziLoader (items drawn in the main
    process), and through DziLoader with a worker process (items drawn, collated and pickled there; the worker seeds
    `random` from torch's seed, the same in both modes)."""
    from bop_fixture import write_tree
    from kd6d.libs.train_libs import CachedDziLoader, DziLoader, build_dataset
    tree = write_tree(str(tmp_path))
    got = {}
    for mode in ("host", "device"):
        cfg = _tree_cfg(tree, mode, workers)
        random.seed(9); np.random.seed(9); torch.manual_seed(9)
        train, _ = build_dataset(cfg, gpu_device, augment=True, frame_cache=frame_cache)
        assert type(train) is (CachedDziLoader if frame_cache == "device" else DziLoader)
        assert train.front.ac.pose_remap == mode
        images, tgt, metas = next(iter(train))
        torch.cuda.synchronize()
        got[mode] = (images.tensors.cpu().numpy(), tgt.mask.cpu().numpy(), tgt.bbox_trans.cpu().numpy(),
                     tgt.rot.cpu().numpy(), tgt.trans.cpu().numpy(), tgt.class_ids.cpu().numpy(), tgt.n_gt.cpu().numpy(),
                     tgt.kp3d.cpu().numpy(), [m["path"] for m in metas])
    (ih, mh, bh, rh, th, ch, nh, kh, ph), (id_, md, bd, rd, td, cd, nd, kd, pd) = got["host"], got["device"]
    assert ph == pd and np.array_equal(ch, cd) and np.array_equal(nh, nd) and int(nh.sum()) >= 2
    K = np.array(_tree_cfg(tree, "host")["INPUT"]["INTERNAL_K"]).reshape(3, 3)
    B = ih.shape[0]
    worst = 0.0
    for b in range(B):
        for g in range(int(nh.reshape(-1)[b])):
            X = kh.reshape(B, -1, 8, 3)[b, int(ch.reshape(B, -1)[b, g])]
            a = np.concatenate([rh.reshape(B, -1, 9)[b, g], th.reshape(B, -1, 3)[b, g]])
            d = np.concatenate([rd.reshape(B, -1, 9)[b, g], td.reshape(B, -1, 3)[b, g]])
            worst = max(worst, C.pixel_gap(K, X, a, d))
    dt = float(np.abs(bh.reshape(B, 2, 3)[:, :, 2] - bd.reshape(B, 2, 3)[:, :, 2]).max())
    dimg = float(np.abs(ih - id_).max())
    dmask = float((mh != md).mean())
    print(frame_cache, "loader: corner gap %.3e px, bbox_trans %.3e px, crop %.3e, mask pixels %.3e" % (worst, dt, dimg, dmask))
    assert worst <= C.TOL_PX
    assert dt <= 1e-3
    assert dimg <= 1e-2
    assert dmask <= 1e-3


def test_train_entry_with_device_pose_remap(gpu_device, tmp_path):
    """train_kd.py --augment --frame_cache device --aug_pose_remap device --launch pipeline on the BOP fixture tree."""
    import yaml
    from bop_fixture import write_tree
    tree = write_tree(str(tmp_path / "data"))
    with open(os.path.join(ROOT, "configs", "ape.yaml")) as f:
        y = yaml.safe_load(f)
    y["DATASETS"].update(TRAIN=tree["list_file"], VALID=tree["list_file"], TEST=tree["list_file"],
                         MESH_DIR=tree["models"], BBOX_FILE=tree["bbox"])
    y["INPUT"].update(INTERNAL_WIDTH=tree["W"], INTERNAL_HEIGHT=tree["H"], INTERNAL_K=[565.3, 0, 13.47, 0, 566.1, 10.53, 0, 0, 1])
    y["SOLVER"].update(AUGMENTATION_OCCLUSION=0.5, AUGMENTATION_ColorH=0.1, AUGMENTATION_ColorS=0.2, AUGMENTATION_ColorV=0.2,
                       AUGMENTATION_Smooth=3, AUGMENTATION_Noise=0.05)
    cfgp = str(tmp_path / "aug.yaml")
    with open(cfgp, "w") as f:
        yaml.safe_dump(y, f)
    cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.join(ROOT, "train_kd.py"), "--config_file", cfgp,
           "--config_file_t", cfgp, "--backbone", "darknet_tiny_h", "--backbone_t", "darknet53", "--kd_weight", "5.",
           "--working_dir", str(tmp_path / "out") + "/", "--augment", "--frame_cache", "device", "--aug_pose_remap", "device",
           "--skip_teacher_eval", "--num_workers", "0", "--max_iters", "4", "--val_freq", "1000", "--batch_size", "2",
           "--launch", "pipeline"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 30)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "Training finished" in r.stdout and "frame cache: " in r.stdout
    steps = re.findall(r"steps: \d+/4, lr:\S+, cls:(\S+), reg:(\S+), kd:(\S+) ", r.stdout)
    assert steps, r.stdout[-3000:]
    assert all(np.isfinite(float(v.rstrip(","))) for row in steps for v in row), steps
