"""CPU: the cases of tests/sinkhorn_cases.py (the inputs and references of tests/test_sinkhorn_small_gpu.py) satisfy
the conditions their tolerances rest on -- size classes and residues, schedule lengths, knife-edge margins, spread
caps, recorded deviations -- and the oracle has the properties the GPU tests lean on: the reference is bitwise
kd_loss_images', permuting the keypoints permutes the results, the divergence is symmetric and S(a, a) = 0, and
coincident points give finite values with a zero point gradient."""
import numpy as np
import pytest

import sinkhorn_cases as C


def test_case_table_covers_every_size_class_and_residue():
    plain = {(c.N, c.M, c.regime) for c in C.CASES.values() if c.kind == "plain"}
    assert plain == {(n, m, r) for n, m in C.SIZES for r in C.REGIMES}
    assert len(C.SIZES) == 19
    for lo, hi in ((1, 16), (17, 64), (65, 128)):                  # lane path / one strided pass / two
        assert any(lo <= n <= hi and lo <= m <= hi for n, m in C.SIZES)
    for pair in ((16, 17), (17, 16), (64, 65), (65, 64), (128, 128), (128, 1), (3, 128), (1, 1)):
        assert pair in C.SIZES
    # the general path sees every residue mod 4 of the row count and of the column count (lse_row's 4-wide loop and
    # scalar tail): sizes above 16 by themselves, sizes up to 16 with sinkhorn.lanes = 0
    general = C.SIZES                                                # every size runs on it in one of the two modes
    assert {n % 4 for n, _ in general} == {m % 4 for _, m in general} == {0, 1, 2, 3}
    small = [(n, m) for n, m in C.SIZES if n <= C.LANE_MAX and m <= C.LANE_MAX]
    assert {n for n, _ in small} | {m for _, m in small} >= {1, 2, 3, 4, 5, 15, 16}      # tail only, empty tail
    for sizes in (C.SCHED_SIZES, C.ZERO_SIZES, C.COINCIDENT_SIZES):
        assert max(sizes[0]) <= C.LANE_MAX < max(sizes[1]) <= C.CAP
    for kind in ("zero", "coincident"):
        assert {(c.N, c.regime) for c in C.CASES.values() if c.kind == kind} == \
            {(n, r) for n, _ in (C.ZERO_SIZES if kind == "zero" else C.COINCIDENT_SIZES) for r in C.REGIMES}


def test_input_conditions_and_schedule_lengths():
    lengths = {}
    for name, c in C.CASES.items():
        inp = C.inputs(name)
        steps, margin = C.check_conditions(inp)
        assert C.KNIFE <= margin, name
        assert inp["blur"] == float(np.float32(inp["blur"])) and inp["scaling"] == float(np.float32(inp["scaling"]))
        for a in (inp["xs"], inp["al"], inp["yt"], inp["be"]):
            assert a.dtype == np.float32 and np.isfinite(a).all()
        if c.N > 1 and c.M > 1:                                    # weights differ from keypoint to keypoint
            assert (inp["al"].std(1) > 0).all() and (inp["be"].std(1) > 0).all()
        if c.kind == "sched":
            assert inp["scaling"] != 0.5
            lengths.setdefault((c.N, c.M), []).append(steps)
        else:
            assert inp["scaling"] == 0.5 and steps <= 16
    assert sorted(lengths) == sorted(C.SCHED_SIZES)
    for got in lengths.values():
        assert got[0] == C.SCHED_TABLE == 128 and got[1] == 129 and 180 <= got[2] <= 230
    # the sizes that left blur 0.001 are few, named, and still unbalanced
    assert set(C.BLUR_OVERRIDE) == {"plain_1x5_unb", "plain_3x128_unb"}
    assert all(C.inputs(n)["blur"] == float(np.float32(0.01)) and C.inputs(n)["reach"] == 0.5 for n in C.BLUR_OVERRIDE)


def test_spread_caps_and_recorded_deviations():
    dev, each = C.measure_deviations(per_case=True)
    assert sorted(dev) == sorted(C.RECORDED_DEV)
    for k, v in dev.items():
        assert v <= C.RECORDED_DEV[k] * 1.001 + 1e-12, (k, v, C.RECORDED_DEV[k])
    for name, c in C.CASES.items():
        for o in C.OUTPUTS:
            if c.kind == "coincident":                             # compared absolutely against the regime's bound
                assert each[name][o] <= C.bound(c.regime, o), (name, o, each[name][o])
            else:
                assert 8.0 * each[name][o] <= C.caps(c)[o], (name, o, each[name][o])
    for grp in ("unb", "bal", "sched"):
        for o in C.OUTPUTS:
            assert C.FLOOR <= C.bound(grp, o) <= (C.CAPS_SCHED if grp == "sched" else C.CAPS)[o], (grp, o)
    assert all(C.seed_passes(n, c.seed) for n, c in C.CASES.items())


def test_reference_is_kd_loss_images():
    for name in C.CASES:
        ref = C.reference(name)
        loss, valid, gx, ga = C.kd_loss_images_reference(name)
        assert valid.tolist() == [1]
        assert loss[0] == ref["loss_img"] == ref["loss_kp"].sum()
        assert np.array_equal(gx, ref["gx"]) and np.array_equal(ga, ref["ga"])


@pytest.mark.parametrize("name", ["plain_4x4_unb", "plain_19x33_bal", "zero_12x16_unb", "plain_65x64_unb"])
def test_oracle_is_equivariant_under_keypoint_permutation(name):
    i, ref = C.inputs(name), C.reference(name)
    perm = np.random.default_rng(3).permutation(8)
    got = C.ot_reference(i["xs"][:, perm], i["al"][:, perm], i["yt"][:, perm], i["be"][:, perm], i["blur"], i["scaling"],
                         i["reach"])
    for o, want in (("loss_kp", ref["loss_kp"][perm]), ("gx", ref["gx"][:, perm]), ("ga", ref["ga"][:, perm])):
        np.testing.assert_allclose(got[o], want, rtol=0, atol=1e-11 * np.abs(want).max())
    assert got["loss_img"] == pytest.approx(ref["loss_img"], rel=1e-12)


@pytest.mark.parametrize("name", ["plain_4x4_unb", "plain_16x17_bal", "zero_39x68_unb", "plain_3x128_bal"])
def test_oracle_symmetry_and_identity(name):
    i, ref = C.inputs(name), C.reference(name)
    swapped = C.ot_reference(i["yt"], i["be"], i["xs"], i["al"], i["blur"], i["scaling"], i["reach"])
    np.testing.assert_allclose(swapped["loss_kp"], ref["loss_kp"], rtol=1e-9, atol=1e-18)
    same = C.ot_reference(i["xs"], i["al"], i["xs"], i["al"], i["blur"], i["scaling"], i["reach"])
    assert np.abs(same["loss_kp"]).max() == 0.0 and np.abs(same["gx"]).max() == 0.0


@pytest.mark.parametrize("name", [n for n, c in C.CASES.items() if c.kind == "coincident"])
def test_oracle_on_coincident_points(name):
    c = C.CASES[name]
    for dtype in (np.float64, np.float32):
        ref = C.reference(name, dtype)
        assert all(np.isfinite(ref[o]).all() for o in C.OUTPUTS)
        assert np.abs(ref["gx"]).max() == 0.0
        if c.regime == "unb":         # only the mass mismatch of the eight problems is left, of the order of eps
            assert np.abs(ref["loss_kp"]).max() < 1e-4 and ref["loss_img"] > 0
        else:
            assert np.abs(ref["loss_kp"]).max() < 1e-9


def test_launch_layout():
    for regime in C.REGIMES:
        L = C.layout(regime)
        B = len(L["sizes"])
        sample = C.launch_sample(regime)
        assert [max(L["sizes"][b]) > 16 for b, _, _ in sample] == [False, False, True, True, True]
        assert max(L["sizes"][sample[-1][0]]) > 64
        assert B >= 300 and int((L["valid"] == 1).sum()) >= 280
        assert int((L["valid"] == 0).sum()) >= 18 and int((L["valid"] == -1).sum()) >= 4
        kinds = {(n == 0, m == 0) for n, m in L["sizes"] if n == 0 or m == 0}
        assert kinds == {(True, True), (True, False), (False, True)}
        assert {129, 200} <= {max(n, m) for n, m in L["sizes"]}
        assert max(max(n, m) for (n, m), v in zip(L["sizes"], L["valid"]) if v == 1) == C.CAP
        for start, cnt, rows in ((L["s_start"], L["s_cnt"], len(L["xs"])), (L["t_start"], L["t_cnt"], len(L["yt"]))):
            assert (np.diff(start) < 0).sum() > B // 4                 # shuffled, not ascending
            use = np.zeros(rows + 1, int)
            for s, n in zip(start, cnt):
                use[s:s + n] += 1
                assert use[s - 1] == 0 and use[s + n] == 0 and s >= 1 and s + n < rows + 1       # a gap on both sides
            assert use.max() == 1 and use[:rows].min() == 0
        own = np.zeros(len(L["xs"]), bool)
        for b in range(B):
            if L["valid"][b] == 1:
                own[L["s_start"][b]:L["s_start"][b] + L["s_cnt"][b]] = True
                x, a, y, w = C.layout_problem(L, b)[:4]
                assert all(np.isfinite(v).all() for v in (x, a, y, w)) and (a.max(0) > 0).all() and (w.max(0) > 0).all()
        assert np.array_equal(own, L["owned"]) and np.isnan(L["xs"][~own]).any()
