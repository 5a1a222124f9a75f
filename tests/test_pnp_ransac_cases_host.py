"""CPU side of the hypothesis-by-hypothesis tests of the device PnP-RANSAC (csrc/pnp.hip): what
tests/pnp_ransac_cases.py promises of its own reference, cases and comparisons, without a GPU and without libkd6d.

  * decidability: in every case at most 10 % of the hypotheses are undecidable, by the reference alone;
  * coverage: every branch a valid input can reach ends at least 5 decidable hypotheses, the late-winner and tie
    situations exist, every cnt / cap / iters / seed / reproj_err value of the list occurs;
  * teeth: the reference with one stage changed (MUTATIONS), packed as the kernel packs its workspace, fails
    check_slots / check_pick on at least one case -- or is shown to be unobservable on decidable hypotheses;
  * the winner of the clear-cut problems agrees with kd6d.libs.pnp.solve_pnp_ransac within 1 degree / 10 mm."""
import collections
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pnp_ransac_cases as C  # noqa: E402
import pose_remap_cases as PR  # noqa: E402

NAMES = [c["name"] for c in C.CASES]


def test_sampling_hash_is_splitmix64():
    assert C.splitmix64(0) == 0xE220A8397B1DCDAF                     # the generator's first output from state 0
    assert C.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4   # and its second
    seen = collections.Counter(C.sample_cell(2 ** 40 + 3, h, k, 7) for h in range(300) for k in range(8))
    assert set(seen) == set(range(7)) and min(seen.values()) > 250
    assert C.sample_cell(0, 5, 3, 10) != C.sample_cell(0, 5, 3, 10, swapped=True) or \
        C.sample_cell(0, 6, 3, 10) != C.sample_cell(0, 6, 3, 10, swapped=True)
    assert all(C.sample_cell(7, h, k, 1) == 0 for h in range(4) for k in range(8))


def test_tolerances_are_the_issue_s():
    assert C.TOL_PX is PR.TOL_PX and C.TOL_PX == 1e-3
    assert C.DELTA_PX == 0.01 and C.DELTA_Z_MM == 1.0 and C.MAX_UNDECIDABLE == 0.10
    assert C.PERTURB_REL == 1e-10 and C.PERTURB_PX == 1e-6 and C.DET_TOL == 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_at_most_a_tenth_of_a_case_is_undecidable(name):
    case = C.by_name(name)
    dec = C.case_decidable(case)
    und = sum(1 for v in dec.values() if not v)
    print("pnp_ransac %s: %d of %d hypotheses undecidable (%.1f %%)" % (name, und, len(dec), 100.0 * und / len(dec)))
    assert und <= C.MAX_UNDECIDABLE * len(dec), (name, und, len(dec))


def test_every_reachable_branch_ends_five_decidable_hypotheses():
    seen = collections.Counter()
    for case in C.CASES:
        res, dec = C.case_results(case), C.case_decidable(case)
        seen.update(r.branch for k, r in res.items() if dec[k])
    print("decidable hypotheses per branch:", dict(seen))
    assert set(seen) <= set(C.BRANCHES)
    for b in C.BRANCHES:
        if b in C.UNREACHABLE:
            # named, not silently skipped: no case reaches it (if one does one day, it counts like the others)
            assert seen[b] == 0 or seen[b] >= 5, (b, seen[b], C.UNREACHABLE[b])
            continue
        assert seen[b] >= 5, (b, seen[b])
    assert set(C.UNREACHABLE) == {"dlt0_failed", "refit_failed"}


def test_branches_hand_out_what_the_header_says():
    for case in C.CASES:
        for (p, h), r in C.case_results(case).items():
            if r.branch in ("invalid", "dlt0_failed", "loose_lt6", "refit_failed"):
                assert r.count == -1 and not r.R.any() and not r.T.any()
            else:
                assert r.count >= 0 and abs(np.linalg.det(r.R) - 1) < 1e-9 and np.isfinite(r.T).all()
                assert np.abs(r.R.T @ r.R - np.eye(3)).max() < 1e-9


def _counts(case, p):
    res = C.case_results(case)
    return np.array([res[p, h].count for h in range(case["iters"])])


def test_cases_cover_the_list():
    cases = C.CASES
    assert len(set(NAMES)) == len(NAMES)
    assert all(len(c["cnt"]) <= 8 and c["iters"] <= 300 for c in cases)
    assert {c["cap"] for c in cases} == {1, 10, 32}
    assert {c["iters"] for c in cases} == {1, 63, 64, 65, 130, 300}
    assert {c["seed"] for c in cases} == {0, 7, 2 ** 40 + 3}
    assert {c["reproj_err"] for c in cases} == {5.0, 12.0}
    b = C.by_name("batch8_cnt_edges")
    cap = b["cap"]
    assert sorted(b["cnt"].tolist()) == sorted([1, 2, 6, 7, 10, cap, cap + 3, 0]) and cap == 10
    i, j = b["cnt"].tolist().index(cap), b["cnt"].tolist().index(cap + 3)
    assert C.problem_of(b, i) == C.problem_of(b, j)          # cap + 3 clamps to cap: the same problem, slot for slot
    live = [p for p in range(8) if b["cnt"][p] > 0 and p != j]
    assert len({b["box"][p].tobytes() for p in live}) >= 4 and len({b["K"][p].tobytes() for p in live}) == 2
    assert len({C.problem_of(b, p) for p in live}) == len(live)
    for bx in C.BOXES:
        ext = bx.max(0) - bx.min(0)
        assert 100 - 1e-3 <= np.linalg.norm(ext) <= 290 + 1e-3 and len(set(np.round(ext, 3))) == 3
    assert np.array_equal(C.ape_k().reshape(-1), [572.4114, 0, 325.2611, 0, 573.57043, 242.04899, 0, 0, 1])
    k2 = C.other_k()
    assert k2[0, 0] != C.ape_k()[0, 0] and k2[0, 2] != C.ape_k()[0, 2] and k2[1, 2] != C.ape_k()[1, 2]
    c1 = C.by_name("single_iter_cap1")
    assert c1["cnt"].tolist() == [1, 4, 0] and C.problem_of(c1, 0) == C.problem_of(c1, 1)
    c32 = C.by_name("outliers_cap32")
    assert c32["cnt"].tolist() == [10, 35] and C.problem_of(c32, 1).kp.shape[0] == 32
    # the invalid problems, among valid ones
    inv = C.by_name("invalid_among_valid")
    branch = [C.case_results(inv)[p, 0].branch for p in range(len(inv["cnt"]))]
    assert [x == "invalid" for x in branch] == [False, True, True, True, True, False, False], branch
    assert np.isnan(inv["kp"][1, :4]).sum() == 1 and np.isinf(inv["K"][2]).sum() == 1
    assert len(np.unique(inv["box"][3], axis=0)) == 5 and not inv["box"][4].any()
    assert np.isnan(inv["kp"][6, 6:]).any() and not np.isnan(inv["kp"][6, :6]).any()


def test_late_winner_and_tie_situations_exist():
    lw = C.by_name("late_winner")
    cs = _counts(lw, 0)
    w = int(np.nonzero(cs == cs.max())[0][0])
    assert cs.max() >= 6 and w >= 64 and w % 64 != 0, (w, cs.max())
    assert (cs < 6).mean() > 0.9, "nearly every hypothesis fails"
    dec = C.case_decidable(lw)
    assert all(dec[0, int(h)] for h in np.nonzero(cs == cs.max())[0])
    tied = []
    for case in C.CASES:
        dec = C.case_decidable(case)
        for p in range(len(case["cnt"])):
            if case["cnt"][p] <= 0:
                continue
            cs = _counts(case, p)
            top = np.nonzero(cs == cs.max())[0]
            if cs.max() >= 6 and len(top) >= 2 and len(set(cs[cs >= 6].tolist())) > 1 and all(dec[p, int(h)] for h in top):
                tied.append((case["name"], p, int(cs.max()), len(top)))
    print("tied winners with more than one count >= 6:", tied)
    assert tied
    # loose is a proper superset of tight somewhere: a refined hypothesis whose count is below the loose set's size
    assert any(r.branch == "tight_lt6" for r in C.case_results(C.by_name("noise_half_r12")).values())


def test_comparisons_accept_the_reference_itself():
    """check_slots on the reference's own results rounded to fp32 and check_pick on the host pick of them: the fp32
    rounding of R, T stays far inside TOL_PX."""
    worst = 0.0
    for case in C.CASES:
        ws = C.pack_slots(case, C.case_results(case))
        st = C.check_slots(ws, case)
        worst = max(worst, st["worst_px"])
        ok, R, T, ni, _ = C.host_pick(ws, case["cnt"])
        C.check_pick(ws, ok, R, T, ni, case["cnt"])
        assert st["compared"] >= (1 - C.MAX_UNDECIDABLE) * st["total"]
        dead = [p for p in range(len(case["cnt"])) if case["cnt"][p] <= 0]
        assert np.isnan(ws[dead]).all() and not ok[dead].any()
    assert worst <= 1e-4, worst


def test_comparisons_see_single_slot_errors():
    case = C.by_name("batch8_cnt_edges")
    good = C.pack_slots(case, C.case_results(case))
    ok, R, T, ni, win = C.host_pick(good, case["cnt"])
    for p, h, f, delta in ((4, 64, 11, 0.05), (2, 3, 5, 2e-4), (1, 0, 0, None), (7, 9, 12, 1e-3)):
        ws = good.copy()
        if delta is None:
            ws[p, h, 0:1].view(np.int32)[0] += 1
        else:
            ws[p, h, f] += np.float32(delta)
        with pytest.raises(AssertionError):
            C.check_slots(ws, case)
    for arr, idx in ((ok, 4), (ni, 2), (R, (3, 1, 1)), (T, (0, 2))):
        bad = [ok.copy(), R.copy(), T.copy(), ni.copy()]
        k = [i for i, a in enumerate((ok, R, T, ni)) if a is arr][0]
        bad[k][idx] = bad[k][idx] + (1 if bad[k].dtype == np.int32 else np.float32(1e-3))
        with pytest.raises(AssertionError):
            C.check_pick(good, bad[0], bad[1], bad[2], bad[3], case["cnt"])
    # a pose reported for a problem without one
    ok2, R2 = ok.copy(), R.copy()
    R2[7, 0, 0] = 1.0
    with pytest.raises(AssertionError):
        C.check_pick(good, ok2, R2, T, ni, case["cnt"])


def _fails(check):
    try:
        check()
    except AssertionError as e:
        return str(e)[:300]
    return None


@pytest.mark.parametrize("name", list(C.MUTATIONS))
def test_every_mutation_is_caught(name):
    m = C.MUTATIONS[name]
    caught = []
    for cn in m["cases"]:
        case = C.by_name(cn)
        if m["where"] == "pick":
            ws = C.pack_slots(case, C.case_results(case))
            ok, R, T, ni, _ = C.host_pick(ws, case["cnt"], mutate=name)
            why = _fails(lambda: C.check_pick(ws, ok, R, T, ni, case["cnt"]))
        else:
            ws = C.pack_slots(case, C.case_results(case, mutate=name))
            why = _fails(lambda: C.check_slots(ws, case))
        if why:
            caught.append((cn, why))
    print("mutation %s:" % name, caught if caught else "not seen")
    if m.get("unobservable"):
        assert not caught, (name, "is observable after all: drop its `unobservable` note", caught)
        return
    assert caught, name


def test_mutation_list_is_the_issue_s():
    assert set(C.MUTATIONS) == {"skip_second_refinement", "stale_count", "loose_factor_2", "refit_ignored", "gn_steps_3",
                                "hash_swapped", "z_check_dropped", "strict_to_nonstrict", "cap_stride", "tie_highest_h"}
    assert [k for k, m in C.MUTATIONS.items() if m.get("unobservable")] == ["strict_to_nonstrict"]


def _angle_mm(Ra, Ta, Rb, Tb):
    ang = np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))
    return ang, float(np.linalg.norm(np.reshape(Ta, 3) - np.reshape(Tb, 3)))


@pytest.mark.parametrize("name,p", [("batch8_cnt_edges", 0), ("batch8_cnt_edges", 2), ("batch8_cnt_edges", 4),
                                    ("invalid_among_valid", 5), ("outliers_cap32", 1)])
def test_winner_agrees_with_the_shipped_host_solver(name, p):
    from kd6d.libs import pnp
    case = C.by_name(name)
    pb = C.problem_of(case, p)
    res = C.case_results(case)
    cs = _counts(case, p)
    r = res[p, int(np.argmax(cs))]
    n = pb.kp.shape[0]
    ok, R, T, _ = pnp.solve_pnp_ransac(np.tile(pb.box.astype(np.float64), (n, 1)), pb.kp.reshape(-1, 2).astype(np.float64),
                                       pb.K.astype(np.float64), reproj_err=case["reproj_err"])
    assert ok and r.count >= 6
    ang, mm = _angle_mm(r.R, r.T, R.astype(np.float64), T)
    print("%s p%d: reference winner vs solve_pnp_ransac %.4f deg, %.3f mm" % (name, p, ang, mm))
    assert ang <= 1.0 and mm <= 10.0, (ang, mm)


def test_gate_cases_choose_the_classes_they_claim():
    g3, g5 = C.by_name("gate_rows3"), C.by_name("gate_rows5")
    assert (g3["n_cls"], g3["n_class_rows"], g5["n_cls"], g5["n_class_rows"]) == (3, 3, 3, 5)
    assert len(g3["cnt"]) == len(g5["cnt"]) == 4
    assert g3["chosen"] == [0, 1, 2, 0] and g5["chosen"] == [0, 1, 2, 0]
    thr = np.float32(0.5)
    assert (g3["prob"][0] > thr).sum() == 2 and not (g3["prob"][1] > thr).any()
    assert g3["prob"][2, 0] == thr and g3["prob"][2, 2] > thr              # exactly at the threshold: not above it
    assert (g5["prob"][3] == thr).all()
    assert not (g5["prob"][2] > thr).any() and int(np.argmax(g5["prob"][2])) == 2
    for g in (g3, g5):
        assert (g["t_row"][:, 0] != 0).sum() >= 3                           # the first cell's row is not row 0
        for p in range(4):
            others = [c for c in range(g["n_class_rows"]) if c != g["chosen"][p]]
            assert not g["kp3d"][p, others].any() and (g["kp3d"][p, g["chosen"][p]].any() or g["cnt"][p] == 0)
    assert C.gate_expected(g3) == [10, 10, 6, 0]
    assert C.gate_expected(g5) == [0, 6, 7, 10]
