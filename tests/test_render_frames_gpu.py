"""GPU: kd6d_render_frames (csrc/render_frames.hip) against the float64 restatement of tests/render_cases.py -- the mask
exactly, the depth within eps_d and the colour by the rounding rule outside the reference's own ambiguous pixels --
against the closed forms (exactly), against kd6d_render_depth (bit for bit), its bitwise properties (two calls, batch,
order of the frames, of the items, of a mesh's faces, a duplicated face) and its edges (malformed items, no frame).
Tolerances: eps_d of bop_vsd_cases, eps_c = 4 x the float32 restatement's own deviation (render_cases.tolerances(),
profiles/render_frames.md)."""
import numpy as np
import pytest
import torch

import bop_vsd_cases as C
import render_cases as RC

pytestmark = pytest.mark.gpu

H, W = C.PLATE_HW


def _t(x, dev):
    x = np.asarray(x)
    return torch.from_numpy(np.ascontiguousarray(x, np.float32 if x.dtype == np.float64 else x.dtype)).to(dev)


def _call(a, h, w, dev, depth=True, **kw):
    """The packed arrays of render_cases.pack -> (frames, masks, depth) numpy."""
    from kd6d import ops
    fr, mk, dp = ops.render_frames(*[_t(a[k], dev) for k in RC.ARG_ORDER], h, w, want_depth=depth, **kw)
    return fr.cpu().numpy(), mk.cpu().numpy(), None if dp is None else dp.cpu().numpy()


def _plate_frames(objs, light=RC.LIGHT_AXIS, ambient=0.5, bg=0):
    """objs: (slot, T, rgb) plates under K_PLATE -> (frames, mesh list) for render_cases.pack."""
    ms = [(C.plate(), RC.uniform_colors(C.plate(), rgb)) for _, _, rgb in objs]
    return [RC._frame(C.K_PLATE, [(i, g, np.eye(3), T) for i, (g, T, _) in enumerate(objs)], light, ambient, bg)], ms


def test_cases_against_float64(gpu_device):
    eps_c = RC.tolerances()["eps_c"]
    for (name, h, w, frames), refs in zip(RC.cases(), RC.references()):
        fr, mk, dp = _call(RC.pack(frames, h, w), h, w, gpu_device)
        assert fr.shape == (len(frames), h, w, 3) and fr.dtype == np.uint8 and mk.dtype == np.uint8 and dp.dtype == np.float32
        for i, (ref, amb) in enumerate(refs):
            sure = ~amb
            cov = ref["owner"] >= 0
            wrong_mask = int((mk[i] != ref["mask"])[sure].sum())
            both = sure & cov & (mk[i] > 0)
            worst_d = float(np.abs(dp[i].astype(np.float64) - ref["depth"])[both].max()) if both.any() else 0.0
            own = sure & cov & (mk[i] == ref["mask"])
            wrong_c, far_c, worst_c = RC.colour_verdict(fr[i], ref["colour"], own, eps_c)
            bg_wrong = int((fr[i] != ref["frame"])[sure & ~cov].sum())
            print("%-52s frame %d covered %5d ambiguous %3d mask mismatches %d worst depth deviation %.3e mm (eps_d %.3e) "
                  "colour: %d channels off where exact, %d further than 1 level, worst |got - c64| %.3f; background "
                  "mismatches %d" % (name, i, int(cov.sum()), int((amb & cov).sum()), wrong_mask, worst_d, RC.EPS_D, wrong_c,
                                     far_c, worst_c, bg_wrong))
            assert wrong_mask == 0, name
            assert worst_d <= RC.EPS_D, name
            assert (dp[i][sure & ~cov] == 0).all(), name
            assert wrong_c == 0 and far_c == 0, name
            assert bg_wrong == 0, name


def test_closed_forms_are_exact_on_the_device(gpu_device):
    albedo = (200, 120, 40)
    bg = RC.backgrounds(H, W)[0]
    rect = np.zeros((H, W), bool)
    rect[9:29, 11:41] = True
    # axial light: the albedo itself, the rest is the background
    frames, ms = _plate_frames([(2, [0.0, 0, 1000.0], albedo)], ambient=0.3)
    fr, mk, dp = _call(RC.pack(frames, H, W, ms), H, W, gpu_device)
    assert np.array_equal(mk[0] == 3, rect) and (mk[0] > 0).sum() == 600 and (mk[0][~rect] == 0).all()
    assert (fr[0][rect] == np.array(albedo[::-1], np.uint8)).all() and np.array_equal(fr[0][~rect], bg[~rect])
    assert np.array_equal(dp[0], np.where(rect, np.float32(1000), np.float32(0)))
    # light at 60 degrees: a * (w + (1 - w) / 2); albedo and ambient chosen so that no product lies near k + 0.5
    w_amb = 0.5
    frames, ms = _plate_frames([(0, [0.0, 0, 1000.0], albedo)], light=[np.sqrt(3.0) / 2.0, 0.0, -0.5], ambient=w_amb)
    fr, mk, _ = _call(RC.pack(frames, H, W, ms), H, W, gpu_device)
    want = np.asarray(albedo[::-1], np.float64) * (w_amb + (1 - w_amb) / 2)
    assert (np.abs((want + 0.5) - np.rint(want + 0.5)) > 0.1).all()
    assert np.array_equal(mk[0] == 1, rect) and (fr[0][rect] == np.floor(want + 0.5).astype(np.uint8)).all()
    # two plates: the nearer one's id and colour in the overlap, in both list orders
    near, far = (1, [16.0, 6.0, 900.0], (10, 250, 90)), (0, [0.0, 0, 1000.0], albedo)
    frames, ms = _plate_frames([near])
    only_near = _call(RC.pack(frames, H, W, ms), H, W, gpu_device)[1][0] > 0
    assert (only_near & rect).sum() > 50
    for objs in ([near, far], [far, near]):
        frames, ms = _plate_frames(objs)
        fr, mk, dp = _call(RC.pack(frames, H, W, ms), H, W, gpu_device)
        assert (mk[0][only_near] == 2).all() and (dp[0][only_near] == 900).all()
        assert (fr[0][only_near] == np.array([90, 250, 10], np.uint8)).all()
        assert (mk[0][rect & ~only_near] == 1).all() and (mk[0][~rect & ~only_near] == 0).all()
    # an identical plate in slots 0 and 1 at one depth: slot 0 owns every pixel
    a, b = (0, [0.0, 0, 1000.0], (1, 2, 3)), (1, [0.0, 0, 1000.0], (200, 200, 200))
    for objs in ([a, b], [b, a]):
        frames, ms = _plate_frames(objs)
        fr, mk, _ = _call(RC.pack(frames, H, W, ms), H, W, gpu_device)
        assert np.array_equal(mk[0] == 1, rect) and (mk[0][~rect] == 0).all()
        assert (fr[0][rect] == np.array([3, 2, 1], np.uint8)).all()


def test_depth_is_render_depth_bit_for_bit(gpu_device):
    from kd6d import ops
    for ci in RC.SINGLE_OBJECT_CASES:
        name, h, w, frames = RC.cases()[ci]
        a = RC.pack(frames, h, w)
        _, mk, dp = _call(a, h, w, gpu_device)
        d = {k: _t(a[k], gpu_device) for k in a}
        want = ops.render_depth(d["verts"], d["faces"], d["voff"], d["vcnt"], d["foff"], d["fcnt"], d["K"], d["R"], d["T"], h,
                                w).cpu().numpy()
        assert (want > 0).sum() > 500, name
        assert np.array_equal(dp.view(np.uint32), want.view(np.uint32)), name
        assert np.array_equal(mk > 0, dp > 0), name
    # without the depth pointer: the same frames and masks
    name, h, w, frames = RC.cases()[8]
    a = RC.pack(frames, h, w)
    f1, m1, d1 = _call(a, h, w, gpu_device)
    f2, m2, d2 = _call(a, h, w, gpu_device, depth=False)
    assert d2 is None and np.array_equal(f1, f2) and np.array_equal(m1, m2) and np.array_equal(m1 > 0, d1 > 0)


def _same_size_frames():
    out = []
    for ci in (3, 7, 9):
        name, h, w, frames = RC.cases()[ci]
        assert (h, w) == (97, 130)
        out += frames
    return out                                               # 5 frames: 1, 2, 3, 0 and 1 objects


def test_bitwise_across_calls_batches_and_orders(gpu_device):
    h, w = 97, 130
    frames = _same_size_frames()
    base = _call(RC.pack(frames, h, w), h, w, gpu_device)
    again = _call(RC.pack(frames, h, w), h, w, gpu_device)
    for x, y in zip(base, again):
        assert np.array_equal(x, y)                                                     # two calls
    rev = _call(RC.pack(frames[::-1], h, w), h, w, gpu_device)
    for x, y in zip(base, rev):
        assert np.array_equal(x, y[::-1])                                               # a reversed batch
    for i, fr in enumerate(frames):
        alone = _call(RC.pack([fr], h, w), h, w, gpu_device)
        for x, y in zip(base, alone):
            assert np.array_equal(x[i], y[0]), i                                        # a frame alone
    n_items = sum(len(fr["objs"]) for fr in frames)
    order = np.random.default_rng(3).permutation(n_items)
    assert not np.array_equal(order, np.arange(n_items))
    mixed = _call(RC.pack(frames, h, w, order=order), h, w, gpu_device)
    for x, y in zip(base, mixed):
        assert np.array_equal(x, y)                                                     # the items in another order


def test_bitwise_under_face_order_and_a_duplicated_face(gpu_device):
    name, h, w, frames = RC.cases()[7]                       # cube and ellipsoid, interpenetrating
    ms = list(RC.meshes())
    base = _call(RC.pack(frames, h, w, ms), h, w, gpu_device)
    rng = np.random.default_rng(5)
    perm = [(C.Mesh(m.vertices, m.faces[rng.permutation(len(m.faces))]), c) for m, c in ms]
    got = _call(RC.pack(frames, h, w, perm), h, w, gpu_device)
    # coverage and depth are minima over the faces; the owner -- hence the colour -- can depend on the order only where two
    # distinct faces tie in depth bit for bit.  This case has no such pixel: the whole frame is equal, colour included
    for x, y in zip(base, got):
        assert np.array_equal(x, y)
    dup = [(C.Mesh(m.vertices, np.concatenate([m.faces, m.faces[[0, len(m.faces) // 2, len(m.faces) - 1]]])), c) for m, c in ms]
    got = _call(RC.pack(frames, h, w, dup), h, w, gpu_device)
    for x, y in zip(base, got):
        assert np.array_equal(x, y)                          # the copy ties with its original everywhere: the lower index wins


def test_malformed_items_leave_their_frame_as_background(gpu_device):
    name, h, w, frames = RC.cases()[9]                       # 3, 0 and 1 objects
    good = RC.pack(frames, h, w)
    base = _call(good, h, w, gpu_device)
    bgs = RC.backgrounds(h, w)
    n_v, n_f = len(good["verts"]), len(good["faces"])
    ms = list(RC.meshes())
    cube_v = len(ms[1][0].vertices)

    def broken(**kw):
        a = dict(good)
        for k, (i, v) in kw.items():
            a[k] = good[k].copy()
            a[k][i] = v
        return a
    # item 3 is frame 2's only object; each of these takes it out
    for what in (dict(voff=(3, n_v - 2)), dict(foff=(3, n_f - 1)), dict(vcnt=(3, 0)), dict(fcnt=(3, -5)),
                 dict(item_frame=(3, 3)), dict(item_frame=(3, -1)), dict(item_slot=(3, 4)), dict(item_slot=(3, -1))):
        a = broken(**what)
        with pytest.raises(ValueError):
            _call(a, h, w, gpu_device)
        fr, mk, dp = _call(a, h, w, gpu_device, validate=False)
        assert (mk[2] == 0).all() and (dp[2] == 0).all() and np.array_equal(fr[2], bgs[frames[2]["bg"]]), what
        for x, y in zip(base, (fr, mk, dp)):
            assert np.array_equal(x[:2], y[:2]), what                                  # the other frames are untouched
    # a face index = vcnt: that face is skipped, the rest of the object is drawn -- as if the mesh did not have the face
    cube_f0 = len(ms[0][0].faces)
    a = dict(good)
    a["faces"] = good["faces"].copy()
    own = RC.references()[9][2][0]["owner"]
    k = int(np.bincount(own[own >= 0] & ((1 << RC.FACE_BITS) - 1)).argmax())             # a face frame 2 shows
    a["faces"][cube_f0 + k, 1] = cube_v
    with pytest.raises(ValueError, match="face index"):
        _call(a, h, w, gpu_device)
    got = _call(a, h, w, gpu_device, validate=False)
    less = [ms[0], (C.Mesh(ms[1][0].vertices, np.delete(ms[1][0].faces, k, axis=0)), ms[1][1]), ms[2]]
    want = _call(RC.pack(frames, h, w, less), h, w, gpu_device)
    assert not np.array_equal(want[2][2], base[2][2])                                    # the face was visible
    for x, y in zip(want, got):
        assert np.array_equal(x, y)
    # two items in one slot, a background outside the pool
    a = broken(item_slot=(1, 0))
    with pytest.raises(ValueError, match="claim slot"):
        _call(a, h, w, gpu_device)
    a = broken(bg_index=(1, 2))
    with pytest.raises(ValueError, match="backgrounds"):
        _call(a, h, w, gpu_device)
    fr, mk, _ = _call(a, h, w, gpu_device, validate=False)
    assert (fr[1] == 0).all() and (mk[1] == 0).all()


def test_no_frames_launches_nothing(gpu_device):
    h, w = 48, 64
    from kd6d import ops
    dev = gpu_device
    e = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    fr, mk, dp = ops.render_frames(e((0, 3), torch.float32), e((0, 3), torch.int32), e((0, 3), torch.uint8),
                                   *[e((0,), torch.int32) for _ in range(6)], e((0, 3, 3), torch.float32),
                                   e((0, 3), torch.float32), e((0, 3, 3), torch.float32), e((0, 3), torch.float32),
                                   e((0,), torch.float32), e((0,), torch.int32), e((0, h, w, 3), torch.uint8), h, w,
                                   want_depth=True)
    assert fr.shape == (0, h, w, 3) and mk.shape == (0, h, w) and dp.shape == (0, h, w)
