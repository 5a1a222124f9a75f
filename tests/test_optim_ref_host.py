"""CPU: the references of tests/optim_ref.py on their own -- what tests/test_optim_gpu.py measures csrc/optim.hip with.
The accumulator emulation against csrc/kd6d_det.h built for the host (tests/det_host.cpp), the slab sum against exact
and float64 sums, the AdamW formula against torch.optim.AdamW in float64, and every bound against an independent fp32
evaluation that must sit inside it."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as R
from test_det_accumulator import det  # noqa: F401  (fixture: kd6d_det.h compiled with g++)

f32 = np.float32


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _same(a, b):
    """bitwise equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (_bits(a) == _bits(b))))


WORD_SETS = [("grad", R.DET_GRAD, R.planar_words(c)) for c in R.PLANAR_COUNTS] + \
            [(kind, E, R.acc_read_words(n, E)) for kind, E in (("act", R.DET_ACT), ("grad", R.DET_GRAD))
             for n in R.ACC_READ_N]


def test_part_groups_and_region_blocks():
    want = {1: 1, 16: 1, 17: 2, 32: 2, 33: 4, 64: 4, 65: 8, 128: 8, 129: 16, 256: 16, 257: 32, 512: 32, 600: 32, 5000: 32}
    for parts, pg in want.items():
        assert R.part_groups(parts) == pg
    assert R.region_blocks(1, 0) == 1 and R.region_blocks(1024, 0) == 1 and R.region_blocks(1025, 0) == 2
    assert R.region_blocks(512, 17) == 1 and R.region_blocks(513, 17) == 2 and R.region_blocks(33, 600) == 2
    desc, blk = R.region_table([(0, 1025, 0, 0), (2000, 100, 600, 64), (3000, 5, 3, 128)])
    assert desc == [0, 1025, 0, 0, 0, 2000, 100, 2, 600, 64, 3000, 5, 6, 3, 128] and blk == 7
    for parts in R.SLAB_PARTS:
        E = 1024 // R.part_groups(parts)
        assert R.slab_counts(parts) == [1, E - 1, E, E + 1, 3 * E + 7]


def test_word_sets_hold_every_kind():
    lo, hi, kind = R.planar_words(2500)
    assert set(kind.tolist()) == {0, 1, 2, 3, 4, 5}
    assert np.all((lo[kind == 2] != 0) & (hi[kind == 2] == 0)) and np.all((lo[kind == 3] == 0) & (hi[kind == 3] != 0))
    assert np.all((lo[kind == 4] == 0) & (hi[kind == 4] == 0))
    assert sorted(hi[kind == 5].tolist()) == sorted(R.SPECIAL_HI)
    assert np.abs(lo[kind == 0]).max() > 2 ** 59 and (np.sign(lo[kind == 0]) != np.sign(hi[kind == 0])).any()
    v = R.det_value_grad(lo, hi)
    nan_hi = (np.abs(hi) >= 2 ** 46)
    assert np.array_equal(np.isnan(v), nan_hi) and nan_hi.sum() == 3
    # kind 1 cancels: the value is far smaller than either term
    k1 = kind == 1
    assert np.all(np.abs(v[k1].astype(np.float64)) * 2.0 ** 52 <= np.abs(lo[k1]).astype(np.float64) * 2.0 ** -10)


@pytest.mark.parametrize("idx", range(len(WORD_SETS)))
def test_det_value_emulation_is_the_header_function(det, idx):  # noqa: F811
    """optim_ref.det_value_* == det_value<E> of csrc/kd6d_det.h, bit for bit, on the word sets of the GPU tests; and it
    sits inside the exact-rational bound."""
    kind, E, (lo, hi, _) = WORD_SETS[idx]
    fn = getattr(det, "det_value_" + kind)
    want = np.asarray([fn(ctypes.c_longlong(int(l)), ctypes.c_longlong(int(h))) for l, h in zip(lo, hi)], f32)
    got = (R.det_value_grad if kind == "grad" else R.det_value_act)(lo, hi)
    assert _same(got, want)
    finite = np.abs(hi) < 2 ** 46
    assert np.array_equal(np.isnan(got), ~finite)
    err, bnd = R.det_error_units(np.where(finite, got, 0), lo, hi, E)
    assert np.all(err <= bnd)
    assert np.allclose(bnd[finite], np.asarray(R.det_bound_units(lo, hi))[finite], rtol=1e-12)
    assert [int(x) for x in R.det_exact_units(lo[:3], hi[:3])] == [int(h) * 2 ** 47 + int(l) for l, h in zip(lo[:3], hi[:3])]


@pytest.mark.parametrize("parts", R.SLAB_PARTS)
def test_slab_sum_is_exact_on_integers_and_inside_its_bound(parts):
    count = R.slab_counts(parts)[3] if parts > 16 else 67
    a = R.slab_data(parts, count, "int", parts)
    assert np.abs(a).max() <= 8 and np.array_equal(a, np.round(a))
    assert np.array_equal(R.slab_sum(a).astype(np.int64), a.astype(np.int64).sum(0))
    a = R.slab_data(parts, count, "rand", parts)
    mags = np.abs(a[a != 0])
    assert mags.max() / mags.min() > 1e5                       # magnitudes spread over several decades
    g0 = R.grads_data(count, "rand", parts + 1)
    assert np.all(g0 != 0)
    ref = g0.astype(np.float64) + a.astype(np.float64).sum(0)
    bound = R.slab_bound(g0, a)
    for fn in (R.slab_sum, R.slab_sum_in_part_order):
        got = (g0 + fn(a)).astype(f32)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)
    # a dropped part is outside the bound somewhere, and the integer comparison sees it everywhere it is non-zero
    b = a.copy()
    b[parts - 1] = 0
    assert np.any(np.abs((g0 + R.slab_sum(b)).astype(f32).astype(np.float64) - ref) > bound)


def test_the_bitwise_slab_comparison_tells_the_two_associations_apart():
    """Four running sums per group vs one: the same bits up to three parts per group, different bits beyond."""
    for parts in (1, 2, 3, 17, 33):
        a = R.slab_data(parts, 300, "rand", parts)
        if -(-parts // R.part_groups(parts)) <= 3:
            assert _same(R.slab_sum(a), R.slab_sum_in_part_order(a))
    for parts in (4, 5, 16, 32, 64, 65, 257, 600):
        a = R.slab_data(parts, 300, "rand", parts)
        assert not _same(R.slab_sum(a), R.slab_sum_in_part_order(a))


def _torch_adamw(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm):
    P = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.AdamW([P], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    P.grad = torch.tensor(g, dtype=torch.float64)
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([P], max_norm)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.tensor(m, dtype=torch.float64),
                        exp_avg_sq=torch.tensor(v, dtype=torch.float64))
    opt.step()
    st = opt.state[P]
    return P.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _state(n, seed, gscale):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(f32)
    g = (rng.standard_normal(n) * gscale).astype(f32)
    m = (rng.standard_normal(n) * 0.1).astype(f32)
    v = (rng.standard_normal(n) ** 2 * 0.01).astype(f32)
    return p, g, m, v


@pytest.mark.parametrize("gscale,max_norm", [(10.0, 1.0), (1e-4, 1.0), (1.0, 0.0)])
def test_adamw_step_is_torch_adamw_in_float64(gscale, max_norm):
    p, g, m, v = _state(257, 3, gscale)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4, step=7)
    ref = R.adamw_step(p, g, m, v, max_norm=max_norm, clip=max_norm > 0, round_hyper=False, **hp)
    assert (ref["coef"] < 1.0) == (gscale == 10.0)
    tp, tm, tv = _torch_adamw(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 7, max_norm)
    for got, want in ((ref["p"], tp), (ref["m"], tm), (ref["v"], tv)):
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))


def _adamw_fp32(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, clip):
    """The same formula in numpy float32, operation by operation (an independent evaluation for the bounds)."""
    bc1, bc2s = (f32(x) for x in R.bias_corrections(b1, b2, step))
    lr, b1, b2, eps, wd, max_norm = (f32(x) for x in (lr, b1, b2, eps, wd, max_norm))
    one = f32(1)
    coef = one
    g2 = None
    if clip:
        parts = np.zeros(R.SUMSQ_PARTS, f32)
        sq = (g * g).astype(f32)
        nb = R.sumsq_blocks(len(g))
        for b in range(nb):                  # a 10-level tree per workgroup: 1 + 10 + 7 roundings <= sumsq_roundings(n)
            t = np.zeros(1024, f32)
            t[:len(sq[b::nb])] = sq[b::nb]
            while t.size > 1:
                t = (t[:t.size // 2] + t[t.size // 2:]).astype(f32)
            parts[b] = t[0]
        g2 = R.sum_partials(parts)
        if max_norm > 0:
            coef = min(one, f32(max_norm / f32(np.sqrt(g2) + f32(1e-6))))
    gs = (g * coef).astype(f32)
    pn = (p * f32(one - f32(lr * wd))).astype(f32)
    mn = ((b1 * m).astype(f32) + (f32(one - b1) * gs).astype(f32)).astype(f32)
    vn = ((b2 * v).astype(f32) + ((f32(one - b2) * gs).astype(f32) * gs).astype(f32)).astype(f32)
    den = ((np.sqrt(vn).astype(f32) / bc2s).astype(f32) + eps).astype(f32)
    pn = (pn - ((f32(lr / bc1) * mn).astype(f32) / den).astype(f32)).astype(f32)
    return pn, mn, vn, g2


@pytest.mark.parametrize("n,gscale,max_norm,clip", [(1, 10.0, 1.0, True), (255, 10.0, 1.0, True), (257, 1e-4, 1.0, True),
                                                    (257, 1.0, 0.0, True), (1031, 1.0, 0.0, False)])
def test_adamw_bounds_hold_for_an_fp32_evaluation_and_catch_swapped_betas(n, gscale, max_norm, clip):
    p, g, m, v = _state(n, n, gscale)
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4, step=3)
    ref = R.adamw_step(p, g, m, v, max_norm=max_norm, clip=clip, **hp)
    bnd = R.adamw_bounds(ref, n, clip and max_norm > 0)
    gp, gm, gv, g2 = _adamw_fp32(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 3, max_norm, clip)
    for k, got in (("p", gp), ("m", gm), ("v", gv)):
        assert np.all(np.abs(got.astype(np.float64) - ref[k]) <= bnd[k]), k
    if clip:
        assert abs(float(g2) - ref["gnorm_sq"]) <= R.sumsq_rel_bound(n) * ref["gnorm_sq"]
    # the bounds are tight enough to see a real mistake: betas swapped in the moment updates
    sp, sm, sv, _ = _adamw_fp32(p, g, m, v, 1e-3, 0.999, 0.9, 1e-8, 1e-4, 3, max_norm, clip)
    assert np.any(np.abs(sm.astype(np.float64) - ref["m"]) > bnd["m"])
    assert np.any(np.abs(sv.astype(np.float64) - ref["v"]) > bnd["v"])
    # and below rtol 1e-5 of the magnitudes they are made of
    r = R.adamw_roundings(n, clip and max_norm > 0)
    assert max(r.values()) * R.U * R.MARGIN < 1e-5


def test_decay_only_bound():
    p = _state(300, 5, 1.0)[0]
    z = np.zeros_like(p)
    ref = R.adamw_step(p, z, z, z, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1)
    assert np.array_equal(ref["m"], z) and np.array_equal(ref["v"], z) and np.all(np.isfinite(ref["p"]))
    want = p.astype(np.float64) * (1.0 - float(f32(1e-3)) * float(f32(1e-4)))
    assert np.allclose(ref["p"], want, rtol=1e-15)
    got = (p * f32(f32(1) - f32(f32(1e-3) * f32(1e-4)))).astype(f32)
    assert np.all(np.abs(got.astype(np.float64) - ref["p"]) <= R.decay_only_bound(p, 1e-3, 1e-4))


def test_sumsq_launch_shape_and_roundings():
    assert [R.sumsq_blocks(n) for n in (1, 1024, 1025, 131072, 131073, 10 ** 7)] == [1, 1, 2, 128, 128, 128]
    assert R.sumsq_roundings(1) == 22 and R.sumsq_roundings(1024) == 23 and R.sumsq_roundings(131072) == 23
    assert R.sumsq_roundings(131073) == 23 and R.sumsq_roundings(131076) == 24 and R.sumsq_roundings(2 * 131072 + 4099 + 3) == 25
    p = np.arange(128, dtype=f32)
    assert float(R.sum_partials(p)) == 127 * 64
    # a sequential fp32 sum of squares of 1025 normals (1024 roundings per term at worst) is far inside 1024 u, and a
    # tree of the depth the bound counts is inside the bound
    x = np.random.default_rng(0).standard_normal(4096).astype(f32)
    ref = float(np.sum(x.astype(np.float64) ** 2))
    sq = (x * x).astype(f32)
    while sq.size > 1:
        sq = (sq[:sq.size // 2] + sq[sq.size // 2:]).astype(f32)       # 12 levels + the square: 13 roundings
    assert abs(float(sq[0]) - ref) <= R.MARGIN * 13 * R.U * ref


def test_bf16_bits_is_torch_round_to_nearest_even():
    pat = np.asarray(R.CAST_PATTERNS, np.uint32)
    rng = np.random.default_rng(1)
    x = np.concatenate([pat.view(f32), rng.standard_normal(5000).astype(f32),
                        rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32).view(f32)])
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_bits(x)
    ok = ~np.isnan(x)
    assert np.array_equal(got[ok], want[ok])
    nan_out = (got[~ok] & 0x7f80) == 0x7f80
    assert np.all(nan_out & ((got[~ok] & 0x7f) != 0))
    # the crafted patterns do what their comments say
    f = dict(zip(R.CAST_PATTERNS, R.bf16_bits(pat.view(f32)).tolist()))
    assert f[0x3f808000] == 0x3f80 and f[0x3f818000] == 0x3f82 and f[0x3f808001] == 0x3f81 and f[0x3f807fff] == 0x3f80
    assert f[0x7f7fffff] == 0x7f80 and f[0xff7fffff] == 0xff80 and f[0x7f7f7fff] == 0x7f7f
    assert f[0x00000000] == 0 and f[0x80000000] == 0x8000 and f[0x00008000] == 0 and f[0x00018000] == 2
    # truncation differs from rounding on these
    assert np.any((pat >> 16).astype(np.uint16)[~np.isnan(pat.view(f32))] != got[:len(pat)][~np.isnan(pat.view(f32))])
