"""The device PnP-RANSAC (csrc/pnp.hip: pnp_hyp_kernel, pnp_pick_kernel behind kd6d_pnp_ransac and
kd6d_teacher_pnp_gate) hypothesis by hypothesis against the fp64 reference of tests/pnp_ransac_cases.py.

Every launch owns its workspace, prefilled with a NaN no arithmetic produces: each hypothesis slot {count, R, T} is
compared with the reference wherever the reference alone calls the hypothesis decidable (same count; a zero pose
without one; the 8 corners within 1e-3 px; |det R - 1| <= 1e-5), and the pick is compared bit for bit with the winner
(count desc, h asc) of the launch's own slots."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pnp_ransac_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC5A5A5                    # the prefill of the workspace and of the guard behind it
GUARD = 64                               # floats behind the last slot that no launch may touch
RANSAC = [c["name"] for c in C.CASES if c["kind"] == "ransac"]
GATES = [c["name"] for c in C.CASES if c["kind"] == "gate"]


def _t(a, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt).contiguous()


def _fresh_ws(P, iters, dev):
    return torch.full((P * iters * C.SLOT + GUARD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def _ws_bits(ws, P, iters):
    bits = ws.view(torch.int32).cpu().numpy()
    assert (bits[P * iters * C.SLOT:] == NAN_BITS).all(), "floats behind the last slot were written"
    return bits[:P * iters * C.SLOT].reshape(P, iters, C.SLOT)


def _launch(case, dev, ws=None, rows=None):
    """One kd6d_pnp_ransac launch of the case (rows: only these problems) -> slot bits (P, iters, 16) int32, ok, R, T,
    n_inliers as numpy, and the workspace tensor."""
    from kd6d import ops
    rows = list(range(len(case["cnt"]))) if rows is None else list(rows)
    P, cap, iters = len(rows), case["cap"], case["iters"]
    ws = _fresh_ws(P, iters, dev) if ws is None else ws
    ok, R, T, ni = ops.pnp_ransac(_t(case["kp"][rows].reshape(P * cap, 8, 2), dev), _t(case["cnt"][rows], dev, torch.int32),
                                  _t(case["box"][rows], dev), _t(case["K"][rows], dev), reproj_err=case["reproj_err"],
                                  iters=iters, seed=case["seed"], workspace=ws)
    torch.cuda.synchronize()
    return _ws_bits(ws, P, iters), ok.cpu().numpy(), R.cpu().numpy(), T.cpu().numpy(), ni.cpu().numpy(), ws


def _check_fill(bits, cnt):
    """Slots of cnt = 0 problems keep the prefill (the pick reads none of them); floats 0-12 of every other slot are
    written."""
    for p, n in enumerate(cnt):
        if n <= 0:
            assert (bits[p] == NAN_BITS).all(), (p, "a slot of a problem without cells was written")
        else:
            assert not (bits[p, :, :13] == NAN_BITS).any(), (p, "a slot was left unwritten")


@pytest.mark.parametrize("name", RANSAC)
def test_slots_and_pick_against_the_reference(gpu_device, name):
    case = C.by_name(name)
    bits, ok, R, T, ni, _ = _launch(case, gpu_device)
    _check_fill(bits, case["cnt"])
    ws = bits.view(np.float32)
    C.check_slots(ws, case)
    win = C.check_pick(ws, ok, R, T, ni, case["cnt"])
    assert np.isin(ok, (0, 1)).all() and np.isfinite(R).all() and np.isfinite(T).all()
    print("pnp_ransac %s: ok %s, winners %s, n_inliers %s" % (name, ok.tolist(), win.tolist(), ni.tolist()))
    # problems that are the same problem (cnt above the capacity clamps to it) agree slot for slot
    for p in range(len(case["cnt"])):
        for q in range(p):
            if case["cnt"][p] > 0 and case["cnt"][q] > 0 and C.problem_of(case, p) == C.problem_of(case, q):
                assert np.array_equal(bits[p, :, :13], bits[q, :, :13]), (p, q)
                assert ok[p] == ok[q] and ni[p] == ni[q] and np.array_equal(R[p].view(np.int32), R[q].view(np.int32))


def test_expected_outcomes_of_the_edge_problems(gpu_device):
    """What the reference's decidable hypotheses already settle about the launch's outputs."""
    _, ok, _, _, ni, _ = _launch(C.by_name("invalid_among_valid"), gpu_device)
    assert ok.tolist() == [1, 0, 0, 0, 0, 1, 1] and ni.tolist()[1:5] == [0, 0, 0, 0] and ni[5] == 80
    _, ok, _, _, ni, _ = _launch(C.by_name("batch8_cnt_edges"), gpu_device)
    assert ok.tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and ni.tolist()[:3] == [8, 16, 48] and ni[4] == ni[5] == 80
    lw = C.by_name("late_winner")
    bits, ok, _, _, ni, _ = _launch(lw, gpu_device)
    win = C.host_pick(bits.view(np.float32), lw["cnt"])[4]
    res = C.case_results(lw)
    cs = np.array([res[0, h].count for h in range(lw["iters"])])
    assert ok[0] == 1 and win[0] == int(np.argmax(cs)) >= 64 and ni[0] == cs.max()


def test_a_used_workspace_changes_nothing(gpu_device):
    """The same launch over a workspace that holds another call's contents: bitwise the same slots and outputs."""
    case = C.by_name("noise_half_r12")
    a = _launch(case, gpu_device)
    other = dict(case, seed=0, reproj_err=5.0)
    ws = _launch(other, gpu_device)[5]
    b = _launch(case, gpu_device, ws=ws)
    assert np.array_equal(a[0][:, :, :13], b[0][:, :, :13])
    for x, y in zip(a[1:5], b[1:5]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    c = _launch(case, gpu_device, ws=a[5])
    assert np.array_equal(a[0], c[0])


@pytest.mark.parametrize("name", ["batch8_cnt_edges", "invalid_among_valid"])
def test_a_problem_alone_equals_its_rows_in_the_batch(gpu_device, name):
    case = C.by_name(name)
    bits, ok, R, T, ni, _ = _launch(case, gpu_device)
    for p in range(len(case["cnt"])):
        b1, ok1, R1, T1, ni1, _ = _launch(case, gpu_device, rows=[p])
        assert np.array_equal(b1[0], bits[p]), p
        assert ok1[0] == ok[p] and ni1[0] == ni[p], p
        assert np.array_equal(R1[0].view(np.int32), R[p].view(np.int32)), p
        assert np.array_equal(T1[0].view(np.int32), T[p].view(np.int32)), p
    # another order and another batch size
    rows = list(range(len(case["cnt"])))[::-2]
    b2, ok2, R2, T2, ni2, _ = _launch(case, gpu_device, rows=rows)
    assert np.array_equal(b2, bits[rows]) and np.array_equal(ok2, ok[rows]) and np.array_equal(ni2, ni[rows])
    assert np.array_equal(R2.view(np.int32), R[rows].view(np.int32))
    assert np.array_equal(T2.view(np.int32), T[rows].view(np.int32))


def test_fewer_iterations_are_a_prefix(gpu_device):
    """iters63_r12 holds noise_half_r12's problems in the other order with 63 of its 130 hypotheses: a hypothesis is a
    function of (problem, seed, h), so its slots are the first 63 of the longer launch, at the other stride."""
    long_, short = C.by_name("noise_half_r12"), C.by_name("iters63_r12")
    assert C.problem_of(long_, 0) == C.problem_of(short, 1) and C.problem_of(long_, 1) == C.problem_of(short, 0)
    a, b = _launch(long_, gpu_device)[0], _launch(short, gpu_device)[0]
    assert np.array_equal(b[0, :, :13], a[1, :63, :13]) and np.array_equal(b[1, :, :13], a[0, :63, :13])


@pytest.mark.parametrize("name", GATES)
def test_gate_against_the_reference(gpu_device, name):
    from kd6d import ops
    case = C.by_name(name)
    dev = gpu_device
    B, cap, iters = len(case["cnt"]), case["cap"], case["iters"]
    want = C.gate_expected(case)
    assert None not in want
    ws = _fresh_ws(B, iters, dev)
    t_cnt = _t(case["cnt"], dev, torch.int32)
    ops.teacher_pnp_gate(_t(case["cls"], dev), case["n_cls"], case["threshold"], _t(case["t_row"].reshape(-1), dev, torch.int32),
                         t_cnt, _t(case["kp"].reshape(B * cap, 8, 2), dev), cap, _t(case["kp3d"], dev), _t(case["K"], dev),
                         reproj_err=case["reproj_err"], iters=iters, seed=case["seed"], workspace=ws)
    torch.cuda.synchronize()
    bits = _ws_bits(ws, B, iters)
    _check_fill(bits, case["cnt"])
    C.check_slots(bits.view(np.float32), case)          # against the box of the class the reference's gate chooses
    got = t_cnt.cpu().tolist()
    print("gate %s: t_cnt %s -> %s" % (name, case["cnt"].tolist(), got))
    assert got == want, (got, want)
    # the gate's slots are the general entry's slots for the chosen boxes
    assert np.array_equal(_launch(case, dev)[0][:, :, :13], bits[:, :, :13])
