"""GPU: the gradient tail of the step (csrc/optim.hip), every entry point on its own through the C ABI, against the plain
references of tests/optim_ref.py: kd6d_grad_acc_resolve (region table, planar fixed-point accumulators, partial-image
slabs on both sides of every split class and workgroup tail), ParamStore.resolve_grads (the engine's region table),
kd6d_sumsq, kd6d_clip_adamw, kd6d_cast_f32_to_bf16 and kd6d_acc_read.  Bounds and their derivations:
profiles/optim_kernel_tolerances.md; tests/test_optim_ref_host.py checks the references alone.

The tests own every byte the kernels may touch: accumulator planes sit between guard planes, slabs between NaN gaps,
outputs in front of guard elements, and all of them must come back bit for bit."""
import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 5            # gradient elements between and around the regions (odd: the regions start unaligned)
GAP = 3              # NaN floats between and around the slabs
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4)


def _ops():
    from kd6d import ops
    return ops


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, nan_equal=True):
    """bitwise equal; with nan_equal any NaN matches any NaN (a NaN's payload is not part of any contract here)"""
    a, b = np.asarray(a), np.asarray(b)
    eq = _bits(a) == _bits(b)
    if nan_equal and a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return bool(eq.all())


def _report(name, err, bound):
    """largest error as a fraction of its bound, printed before the assertion (pytest -s shows it)"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
    print("optim-tolerance %-34s max error / bound = %.4f" % (name, frac))
    return frac


# ---- 1. kd6d_grad_acc_resolve ---------------------------------------------------------------------------------------
class Scenario:
    """Host image of one kd6d_grad_acc_resolve launch.  specs: [(count, parts)] in launch order.
    grads: GUARD elements around every region.  Accumulators: lo plane and hi plane of `stride` > n words, a guard plane
    in front of and behind them (a lo/hi addressing slip, in either direction, lands in words the test owns and
    checks); every word outside the planar regions holds a non-zero sentinel.  Slabs: views into one NaN-filled fp32
    buffer, GAP NaNs between them."""

    def __init__(self, specs, kind, seed):
        self.specs, self.kind = list(specs), kind
        rng = np.random.default_rng(seed)
        self.first, pos = [], GUARD
        for count, parts in self.specs:
            self.first.append(pos)
            pos += count + GUARD
        self.n = pos
        self.stride = self.n + 11
        self.g0 = R.grads_data(self.n, kind, seed + 1)
        self.acc = rng.integers(1, 1 << 62, 4 * self.stride, dtype=np.int64)          # [guard | lo | hi | guard]
        self.in_planar = np.zeros(self.n, bool)
        self.words, self.slab_off, self.data, self.tsum = {}, {}, {}, {}
        off = GAP
        for r, (count, parts) in enumerate(self.specs):
            a = self.first[r]
            if parts == 0:
                lo, hi, wk = R.planar_words(count)
                self.words[r] = (lo, hi, wk)
                self.acc[self.stride + a:self.stride + a + count] = lo
                self.acc[2 * self.stride + a:2 * self.stride + a + count] = hi
                self.in_planar[a:a + count] = True
                zero = np.flatnonzero(wk == 4)
                self.g0[a + zero[::2]] = f32(-0.0)          # untouched words must leave even a -0.0 as it is
            else:
                self.slab_off[r] = off
                off += parts * count + GAP
        self.slab = np.full(off, np.nan, f32)
        for r, (count, parts) in enumerate(self.specs):
            if parts:
                d = R.slab_data(parts, count, kind, seed + 100 + r)
                self.data[r] = d
                self.slab[self.slab_off[r]:self.slab_off[r] + parts * count] = d.ravel()
                self.tsum[r] = R.slab_sum(d)
        self.in_region = np.zeros(self.n, bool)
        for r, (count, parts) in enumerate(self.specs):
            self.in_region[self.first[r]:self.first[r] + count] = True

    def zero_start(self):
        """grads = 0 inside the regions (the += then adds no rounding), -0.0 where the words are both zero; guards kept"""
        g = np.where(self.in_region, f32(0), self.g0).astype(f32)
        for r, (lo, hi, wk) in self.words.items():
            g[self.first[r] + np.flatnonzero(wk == 4)] = f32(-0.0)
        return g

    def expected(self, start):
        """fp32 emulation of the launch: start + det_value of the words (skipped where both are zero) / + slab_sum"""
        exp = start.copy()
        for r, (count, parts) in enumerate(self.specs):
            s = slice(self.first[r], self.first[r] + count)
            if parts == 0:
                lo, hi, _ = self.words[r]
                exp[s] = np.where((lo | hi) != 0, (start[s] + R.det_value_grad(lo, hi)).astype(f32), start[s])
            else:
                exp[s] = (start[s] + self.tsum[r]).astype(f32)
        return exp

    def acc_expected(self):
        a = self.acc.copy()
        a[self.stride:self.stride + self.n][self.in_planar] = 0
        a[2 * self.stride:2 * self.stride + self.n][self.in_planar] = 0
        return a

    def launch(self, dev, start):
        """-> (grads, accumulator image, slab buffer) after one launch, as numpy arrays"""
        ops = _ops()
        grads, acc, slab = _dev(start, dev), _dev(self.acc, dev), _dev(self.slab, dev)
        regions = [(self.first[r], count, parts, slab.data_ptr() + 4 * self.slab_off[r] if parts else 0)
                   for r, (count, parts) in enumerate(self.specs)]
        desc, blocks = R.region_table(regions, pg_of=ops.lib.kd6d_grad_acc_resolve_part_groups)
        desc = torch.tensor(desc, dtype=torch.int64, device=dev)
        planes = acc[self.stride:3 * self.stride]                      # what the entry point is handed: lo then hi plane
        ops.check(ops.lib.kd6d_grad_acc_resolve(ops._ptr(desc), len(regions), blocks, ops._ptr(planes), self.stride,
                                                ops._ptr(grads), ops._stream()), "kd6d_grad_acc_resolve")
        torch.cuda.synchronize()
        return grads.cpu().numpy(), acc.cpu().numpy(), slab.cpu().numpy()


def _all_specs():
    """every slab region of the issue (18 split counts x 5 element counts), a planar region after every 18th"""
    slabs = [(count, parts) for parts in R.SLAB_PARTS for count in R.slab_counts(parts)]
    specs = []
    for i, sp in enumerate(slabs):
        specs.append(sp)
        if i % 18 == 17:
            specs.append((R.PLANAR_COUNTS[i // 18], 0))
    assert len(specs) == 95 and sum(1 for _, p in specs if p == 0) == 5
    return specs


@pytest.fixture(scope="module")
def resolved(gpu_device):
    """The one big launch, per kind of data: from random non-zero grads (A), the same again (A2), from zero grads (B)."""
    out = {}
    for kind, seed in (("int", 11), ("rand", 23)):
        scn = Scenario(_all_specs(), kind, seed)
        out[kind] = dict(scn=scn, A=scn.launch(gpu_device, scn.g0), A2=scn.launch(gpu_device, scn.g0),
                         B=scn.launch(gpu_device, scn.zero_start()))
    return out


def test_resolve_part_groups_rule(gpu_device):
    lib = _ops().lib
    for parts in list(range(-3, 700)) + [1 << 20]:
        want = 1 if parts <= 16 else 2 if parts <= 32 else 4 if parts <= 64 else 8 if parts <= 128 else \
            16 if parts <= 256 else 32
        assert lib.kd6d_grad_acc_resolve_part_groups(parts) == want == R.part_groups(parts), parts


def test_resolve_planar_values(resolved):
    """The value added is det_value<KD6D_ACC_GRAD> of the two words, bit for bit, and within the three roundings of the
    exact rational value; |hi| >= 2^46 reads as NaN, 2^46 - 1 is finite; both words zero leaves the element alone."""
    scn, (gB, _, _), (gA, _, _) = resolved["rand"]["scn"], resolved["rand"]["B"], resolved["rand"]["A"]
    expB, expA = scn.expected(scn.zero_start()), scn.expected(scn.g0)
    assert len(scn.words) == 5
    for r, (lo, hi, wk) in scn.words.items():
        s = slice(scn.first[r], scn.first[r] + len(lo))
        got = gB[s]
        nan = np.abs(hi) >= (1 << 46)
        assert np.array_equal(np.isnan(got), nan)
        if len(lo) >= 16:
            assert nan.sum() == 3 and np.isfinite(got[np.abs(hi) == (1 << 46) - 1]).all()
        err, bnd = R.det_error_units(np.where(nan, 0, got), lo, hi, R.DET_GRAD)
        _report("resolve planar n=%d (exact)" % len(lo), err, bnd)
        assert np.all(err <= bnd)
        assert _same(got, expB[s])                                      # bitwise: the fp32 emulation of the formula
        assert _same(gA[s], expA[s])                                    # from non-zero grads: one more fp32 addition
        zero = wk == 4
        assert _same(got[zero], np.full(zero.sum(), -0.0, f32), nan_equal=False)
        assert _same(gA[s][zero], scn.g0[s][zero], nan_equal=False)
        assert not zero.any() or (np.signbit(gA[s][zero]).any() and not np.signbit(gA[s][zero]).all())


@pytest.mark.parametrize("kind", ["int", "rand"])
def test_resolve_clears_its_words_and_touches_nothing_else(resolved, kind):
    scn = resolved[kind]["scn"]
    for run, start in (("A", scn.g0), ("A2", scn.g0), ("B", scn.zero_start())):
        g, acc, slab = resolved[kind][run]
        assert np.array_equal(acc, scn.acc_expected())        # resolved words 0, every other word (guard planes too) kept
        assert _same(slab, scn.slab)                          # slabs are read, never cleared
        assert _same(g[~scn.in_region], start[~scn.in_region], nan_equal=False)
        assert (~scn.in_region).sum() == GUARD * (len(scn.specs) + 1)


def test_resolve_slab_integer_data_is_exact(resolved):
    """Integers in [-8, 8]: every association is exact, so the result IS the int64 sum -- no tolerance.  A dropped,
    doubled or mis-indexed part or element, or a NaN read from a gap, cannot hide."""
    scn, (g, _, _) = resolved["int"]["scn"], resolved["int"]["A"]
    for r, d in scn.data.items():
        s = slice(scn.first[r], scn.first[r] + d.shape[1])
        want = scn.g0[s].astype(np.int64) + d.astype(np.int64).sum(0)
        assert np.abs(want).max() < 1 << 24
        assert np.array_equal(g[s].astype(np.float64), want.astype(np.float64)), (scn.specs[r],)
    assert len(scn.data) == 90


def test_resolve_slab_random_data_within_the_order_free_bound(resolved):
    scn, (g, _, _) = resolved["rand"]["scn"], resolved["rand"]["A"]
    worst = 0.0
    for r, d in scn.data.items():
        s = slice(scn.first[r], scn.first[r] + d.shape[1])
        ref = scn.g0[s].astype(np.float64) + d.astype(np.float64).sum(0)
        err, bnd = np.abs(g[s].astype(np.float64) - ref), R.slab_bound(scn.g0[s], d)
        worst = max(worst, float(np.max(err / bnd)))
        assert np.all(err <= bnd), (scn.specs[r], float(np.max(err / bnd)))
    print("optim-tolerance %-34s max error / bound = %.4f" % ("resolve slab (fp64 sum)", worst))


def test_resolve_slab_association_is_the_one_the_header_states(resolved):
    """Bitwise against optim_ref.slab_sum, the fp32 emulation written from include/kd6d.h: PG groups of four running
    sums each, (t0 + t1) + (t2 + t3), groups in g order, then one addition to grads."""
    for kind in ("rand", "int"):
        scn = resolved[kind]["scn"]
        for run, start in (("A", scn.g0), ("B", scn.zero_start())):
            g, exp = resolved[kind][run][0], scn.expected(start)
            for r, d in scn.data.items():
                s = slice(scn.first[r], scn.first[r] + d.shape[1])
                assert _same(g[s], exp[s]), (kind, run, scn.specs[r])


@pytest.mark.parametrize("kind", ["int", "rand"])
def test_resolve_is_bitwise_reproducible(resolved, kind):
    assert _same(resolved[kind]["A"][0], resolved[kind]["A2"][0])
    assert _same(resolved[kind]["A"][0], resolved[kind]["scn"].expected(resolved[kind]["scn"].g0))


@pytest.mark.parametrize("spec", [(1025, 0), (1, 0), (1025, 5), (1, 16), (513, 17), (257, 33), (3 * 32 + 7, 600),
                                  (33, 257), (3 * 64 + 7, 129)])
def test_resolve_single_region_launch(gpu_device, spec):
    """n_regions == 1: the region search has nothing to search, the first workgroup is 0"""
    for kind in ("int", "rand"):
        scn = Scenario([spec], kind, 5 + spec[0] + spec[1])
        for start in (scn.g0, scn.zero_start()):
            g, acc, slab = scn.launch(gpu_device, start)
            assert _same(g, scn.expected(start))
            assert np.array_equal(acc, scn.acc_expected()) and _same(slab, scn.slab)


# ---- 2. ParamStore.resolve_grads ------------------------------------------------------------------------------------
def test_param_store_resolve_grads(gpu_device):
    """The engine's region table: contiguous det entries merge, padding and unmarked entries stay out, [lo, hi) selects
    entries by their base, det words are cleared (a second call adds nothing), slabs are not (it adds them again), a new
    split count rebuilds the plan."""
    from kd6d.engine import ParamStore
    dev = gpu_device
    st = ParamStore()
    e1 = st.add("a", "vec", (16,))                      # a multiple of 8: e2 follows directly, one region
    e2 = st.add("b", "vec", (20,))                      # padded to 24: e3 does not merge
    e3 = st.add("c", "vec", (13,))                      # padded to 16
    e4 = st.add("w", "vec", (1030,))                    # slab, 17 parts: 2 groups, 512 elements per workgroup, ragged
    e5 = st.add("u", "vec", (9,))                       # never marked
    e6 = st.add("d", "vec", (1100,))                    # det, two workgroups
    e7 = st.add("f", "vec", (5,), trainable=False)      # frozen: no gradient at all
    st.finalize()
    st.to(dev)
    st.ensure_grads()
    bases = [st.base(e) for e in (e1, e2, e3, e4, e5, e6)]
    assert bases == [0, 16, 40, 56, 1088, 1104] and st.n_train == 2208 and st.base(e7) >= st.n_train
    n, stride = st.n_train, st.acc_stride
    rng = np.random.default_rng(3)
    words = {e.name: R.acc_words(e.numel, 900 + e.numel) for e in (e1, e2, e3, e6)}
    acc0 = rng.integers(1, 1 << 62, 2 * stride, dtype=np.int64)          # sentinels: padding, e4, e5
    for e in (e1, e2, e3, e6):
        lo, hi, _ = words[e.name]
        acc0[st.base(e):st.base(e) + e.numel] = lo
        acc0[stride + st.base(e):stride + st.base(e) + e.numel] = hi
        assert st.acc(e).data_ptr() == st.gacc.data_ptr() + 8 * st.base(e)
    d17, d33 = R.slab_data(17, e4.numel, "rand", 17), R.slab_data(33, e4.numel, "rand", 33)
    st.slab(e4, 17).copy_(_dev(d17, dev))
    g0 = R.grads_data(n, "rand", 4)
    st.gacc.copy_(_dev(acc0, dev))
    st.grads.copy_(_dev(g0, dev))

    def span(e):
        return slice(st.base(e), st.base(e) + e.numel)

    def det_add(g, e):
        lo, hi, _ = words[e.name]
        g[span(e)] = np.where((lo | hi) != 0, (g[span(e)] + R.det_value_grad(lo, hi)).astype(f32), g[span(e)])

    def state():
        torch.cuda.synchronize()
        return st.grads.cpu().numpy(), st.gacc.cpu().numpy()

    def cleared(acc, entries):
        for e in entries:
            acc[span(e)] = 0
            acc[stride + st.base(e):stride + st.base(e) + e.numel] = 0
        return acc

    # first half: the split falls INSIDE e4, whose base lies below it -- e1..e4 resolve, e6 does not
    mid = st.base(e4) + 100
    st.resolve_grads(0, mid)
    exp = g0.copy()
    for e in (e1, e2, e3):
        det_add(exp, e)
    exp[span(e4)] = (exp[span(e4)] + R.slab_sum(d17)).astype(f32)
    g, acc = state()
    assert _same(g, exp)                                  # e5, e6 and every padding element bit for bit
    assert np.array_equal(acc, cleared(acc0.copy(), (e1, e2, e3)))
    # the complement
    st.resolve_grads(mid, None)
    det_add(exp, e6)
    g, acc = state()
    assert _same(g, exp)
    acc_done = cleared(acc0.copy(), (e1, e2, e3, e6))
    assert np.array_equal(acc, acc_done)
    # the full table: e1 + e2 merged, e3 alone behind the padding, the slab, e6; e5 and e7 absent
    st.resolve_grads()
    desc, n_regions, blocks = st._resolve_plans[(0, n)]
    want_desc, want_blocks = R.region_table([(0, 36, 0, 0), (40, 13, 0, 0), (56, 1030, 17, e4.slab.data_ptr()),
                                             (1104, 1100, 0, 0)])
    assert n_regions == 4 and blocks == want_blocks == 7 and desc.cpu().tolist() == want_desc
    # ... and that call added nothing for the det entries (their words were cleared) and the slab once more
    exp[span(e4)] = (exp[span(e4)] + R.slab_sum(d17)).astype(f32)
    g, acc = state()
    assert _same(g, exp) and np.array_equal(acc, acc_done)
    # another split count: a new slab, a new plan, the 33-part association (4 groups, 256 elements per workgroup)
    st.slab(e4, 33).copy_(_dev(d33, dev))
    assert e4.parts == 33 and not st._resolve_plans
    st.grads.copy_(_dev(g0, dev))
    st.resolve_grads()
    exp = g0.copy()
    exp[span(e4)] = (exp[span(e4)] + R.slab_sum(d33)).astype(f32)
    g, acc = state()
    assert _same(g, exp) and np.array_equal(acc, acc_done)
    assert st._resolve_plans[(0, n)][2] == 1 + 1 + 5 + 2


# ---- 3. kd6d_sumsq --------------------------------------------------------------------------------------------------
SUMSQ_N = [1, 3, 4, 5, 1023, 1024, 1025, 131072, 131073] + [2 * 131072 + 4099 + r for r in range(4)]


@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq(gpu_device, n):
    """x in {-1, 0, 1}: the partials add up to the count of non-zeros exactly.  Normal x: within sumsq_roundings(n)
    roundings of the float64 sum, relative.  Unused slots are written 0, nothing behind slot 127 is written, nothing
    behind x[n - 1] is read (NaNs sit there)."""
    ops = _ops()
    rng = np.random.default_rng(n)
    nb = R.sumsq_blocks(n)
    for kind in ("tern", "rand"):
        x = rng.integers(-1, 2, n).astype(f32) if kind == "tern" else rng.standard_normal(n).astype(f32)
        x[-1] = f32(1.0) if kind == "tern" else x[-1]                       # the last element counts
        buf = torch.full((n + 8,), float("nan"), device=gpu_device)
        buf[:n] = _dev(x, gpu_device)
        guards = rng.standard_normal(8).astype(f32)
        parts = torch.full((R.SUMSQ_PARTS + 8,), float("nan"), device=gpu_device)
        parts[R.SUMSQ_PARTS:] = _dev(guards, gpu_device)
        ops.check(ops.lib.kd6d_sumsq(ops._ptr(buf), n, ops._ptr(parts), ops._stream()), "kd6d_sumsq")
        torch.cuda.synchronize()
        p = parts.cpu().numpy()
        assert _same(p[R.SUMSQ_PARTS:], guards, nan_equal=False)
        assert np.all(_bits(p[nb:R.SUMSQ_PARTS]) == 0)
        assert np.all(np.isfinite(p[:nb])) and np.all(p[:nb] >= 0)
        total = float(R.sum_partials(p[:R.SUMSQ_PARTS]))
        if kind == "tern":
            assert total == float(np.count_nonzero(x))
        else:
            ref = float(np.sum(x.astype(np.float64) ** 2))
            _report("sumsq n=%d D=%d" % (n, R.sumsq_roundings(n)), abs(total - ref), R.sumsq_rel_bound(n) * ref)
            assert abs(total - ref) <= R.sumsq_rel_bound(n) * ref


# ---- 3. kd6d_clip_adamw ---------------------------------------------------------------------------------------------
def _adamw_launch(dev, p, g, m, v, n, step, partials, max_norm, want_gnorm, shadow, hyper, lr=None):
    """one kd6d_clip_adamw launch on fresh device copies -> dict of numpy results"""
    ops = _ops()
    lib, P, S = ops.lib, ops._ptr, ops._stream
    tp, tg, tm, tv = (_dev(a, dev) for a in (p, g, m, v))
    parts = gn = sh = hy = None
    if partials:
        parts = torch.full((R.SUMSQ_PARTS,), float("nan"), device=dev)
        ops.check(lib.kd6d_sumsq(P(tg), n, P(parts), S()), "kd6d_sumsq")
    if want_gnorm:
        gn = torch.full((1,), float("nan"), device=dev)
    if shadow:
        sh = torch.full((n + 8,), 1.0, dtype=torch.bfloat16, device=dev).view(torch.int16).fill_(0x1234)
    lr_arg, step_arg = HP["lr"] if lr is None else lr, step
    if hyper:            # the device-resident schedule wins over contradicting host scalars
        hy = torch.zeros(4, device=dev)
        ops.check(lib.kd6d_set_hyper(P(hy), lr_arg, HP["beta1"], HP["beta2"], step, S()), "kd6d_set_hyper")
        lr_arg, step_arg = 123.0, 0
    ops.check(lib.kd6d_clip_adamw(P(tp), P(tg), P(tm), P(tv), n, P(parts), P(gn), max_norm, lr_arg, HP["beta1"],
                                  HP["beta2"], HP["eps"], HP["wd"], step_arg, P(hy), P(sh), S()), "kd6d_clip_adamw")
    torch.cuda.synchronize()
    out = dict(p=tp.cpu().numpy(), m=tm.cpu().numpy(), v=tv.cpu().numpy(), g=tg.cpu().numpy())
    if want_gnorm:
        out["gnorm_sq"] = float(gn)
    if shadow:
        out["shadow"] = sh.cpu().numpy().view(np.uint16)
    return out


def _adamw_state(n, seed, gscale):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(f32)
    g = (rng.standard_normal(n) * gscale).astype(f32)
    m = (rng.standard_normal(n) * 0.1).astype(f32)
    v = (rng.standard_normal(n) ** 2 * 0.01).astype(f32)
    return p, g, m, v


def _check_adamw(tag, out, p, g, m, v, n, step, partials, max_norm, shadow):
    clip = bool(partials) and max_norm > 0
    ref = R.adamw_step(p, g, m, v, step=step, max_norm=max_norm, clip=clip, **HP)
    bnd = R.adamw_bounds(ref, n, clip)
    assert _same(out["g"], g, nan_equal=False)                          # the gradient is read, never written
    for k in ("p", "m", "v"):
        err = np.abs(out[k].astype(np.float64) - ref[k])
        _report("adamw %s %s n=%d" % (k, tag, n), err, bnd[k])
        assert np.all(np.isfinite(out[k])) and np.all(err <= bnd[k]), (tag, k)
    if partials:                        # *gnorm_sq_out is written whenever the partials are given, clipping or not
        assert abs(out["gnorm_sq"] - ref["gnorm_sq"]) <= R.sumsq_rel_bound(n) * ref["gnorm_sq"]
    if shadow:
        want = torch.from_numpy(out["p"]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(out["shadow"][:n], want) and np.all(out["shadow"][n:] == 0x1234)
    return ref


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 1024 + 1031])
def test_clip_adamw_single_step(gpu_device, n):
    """One step from random p, m, v >= 0, g against the float64 formula: p, exp_avg and exp_avg_sq each within the
    roundings of its own expression; every combination of the optional arguments."""
    dev = gpu_device
    big, small = 10.0, 1e-4 / max(1.0, np.sqrt(n / 1e4))        # |g| ~ 10 sqrt(n) >> 1 and << 1: clipping, not clipping
    #        tag              gscale partials max_norm gnorm shadow hyper step
    combos = [("clipping", big, True, 1.0, True, True, False, 3),
              ("not-clipping", small, True, 1.0, True, False, False, 1),
              ("max_norm=0", big, True, 0.0, True, True, False, 50),
              ("no-partials", big, False, 1.0, False, False, False, 2),
              ("no-partials-gnorm-ptr", 1.0, False, 0.0, True, True, False, 7)]
    for tag, gscale, partials, max_norm, want_gnorm, shadow, hyper, step in combos:
        p, g, m, v = _adamw_state(n, n % 1000 + step, gscale)
        out = _adamw_launch(dev, p, g, m, v, n, step, partials, max_norm, want_gnorm, shadow, hyper)
        ref = _check_adamw(tag, out, p, g, m, v, n, step, partials, max_norm, shadow)
        if tag == "clipping":
            assert ref["coef"] < 1.0
        if tag == "not-clipping":
            assert ref["coef"] == 1.0
        if not partials and want_gnorm:
            assert np.isnan(out["gnorm_sq"])                            # no norm is formed, the pointer is left alone
        if tag in ("clipping", "max_norm=0"):
            # the device-resident schedule, handed contradicting host lr / step: the same bits as the host-scalar form
            hy = _adamw_launch(dev, p, g, m, v, n, step, partials, max_norm, want_gnorm, shadow, True)
            for k in ("p", "m", "v", "shadow"):
                assert _same(hy[k], out[k], nan_equal=False), (tag, k)
            assert hy["gnorm_sq"] == out["gnorm_sq"]


@pytest.mark.parametrize("n", [1, 257])
def test_clip_adamw_zero_state_and_zero_gradients(gpu_device, n):
    p, _, m, v = _adamw_state(n, 9, 1.0)
    z = np.zeros(n, f32)
    # g = m = v = 0: the weight decay alone, no 0 / 0
    for partials in (False, True):
        out = _adamw_launch(gpu_device, p, z, z, z, n, 1, partials, 1.0, partials, True, False)
        assert _same(out["m"], z, nan_equal=False) and _same(out["v"], z, nan_equal=False)
        err = np.abs(out["p"].astype(np.float64) - R.adamw_step(p, z, z, z, step=1, **HP)["p"])
        assert np.all(np.isfinite(out["p"])) and np.all(err <= R.decay_only_bound(p, HP["lr"], HP["wd"]))
        if partials:
            assert out["gnorm_sq"] == 0.0
    # all-zero gradients with clipping on: the norm is 0, the coefficient stays 1, everything finite
    out = _adamw_launch(gpu_device, p, z, m, v, n, 4, True, 1.0, True, True, False)
    _check_adamw("zero-grad", out, p, z, m, v, n, 4, True, 1.0, True)
    assert out["gnorm_sq"] == 0.0


# ---- 3. kd6d_cast_f32_to_bf16 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 2048 * 1024 + 3])
def test_cast_f32_to_bf16(gpu_device, n):
    """Round to nearest even, bit for bit torch's CPU conversion: ties with an even and an odd upper half, their
    neighbours, overflow to inf, +-0, subnormals, +-inf; NaN stays NaN; nothing behind y[n - 1] is written."""
    ops = _ops()
    rng = np.random.default_rng(n)
    pat = np.asarray(R.CAST_PATTERNS, np.uint32).view(f32)
    x = rng.standard_normal(n).astype(f32)
    if n >= 2 * len(pat):
        x[:len(pat)] = pat
        x[-len(pat):] = pat[::-1]                       # the tie with an even upper half is the LAST element
        mid = slice(n // 2, n // 2 + 1000) if n > 4000 else slice(len(pat), len(pat) + 50)
        x[mid] = rng.integers(0, 1 << 32, mid.stop - mid.start, dtype=np.uint64).astype(np.uint32).view(f32)
    else:
        x[:] = pat[1:1 + n]                             # n == 1: a tie that must go UP (truncation would not)
    y = torch.full((n + 8,), 0x1234, dtype=torch.int16, device=gpu_device)
    tx = _dev(x, gpu_device)
    ops.check(ops.lib.kd6d_cast_f32_to_bf16(ops._ptr(tx), ops._ptr(y), n, ops._stream()), "kd6d_cast_f32_to_bf16")
    torch.cuda.synchronize()
    got = y.cpu().numpy().view(np.uint16)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    ok = ~np.isnan(x)
    assert np.array_equal(got[:n][ok], want[ok]) and np.array_equal(want[ok], R.bf16_bits(x)[ok])
    assert np.all(((got[:n][~ok] & 0x7f80) == 0x7f80) & ((got[:n][~ok] & 0x7f) != 0))
    assert np.all(got[n:] == 0x1234)
    assert _same(tx.cpu().numpy(), x)


# ---- 3. kd6d_acc_read -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E", [("act", R.DET_ACT), ("grad", R.DET_GRAD)])
@pytest.mark.parametrize("n", R.ACC_READ_N)
def test_acc_read(gpu_device, kind, E, n):
    """interleaved {lo, hi}: = / += of det_value<E>, bit for bit; clear zeroes exactly the n accumulators, no clear
    leaves them bit-identical; guards behind words and values stay."""
    ops = _ops()
    lo, hi, _ = R.acc_read_words(n, E)
    rng = np.random.default_rng(n + E)
    words = rng.integers(1, 1 << 62, 2 * n + 6, dtype=np.int64)
    words[0:2 * n:2], words[1:2 * n:2] = lo, hi
    out0 = R.grads_data(n + 4, "rand", n)
    val = R.det_value(lo, hi, E)
    err, bnd = R.det_error_units(np.where(np.isnan(val), 0, val), lo, hi, E)
    assert np.all(err <= bnd)
    for accumulate in (0, 1):
        for clear in (0, 1):
            w, out = _dev(words, gpu_device), _dev(out0, gpu_device)
            ops.check(ops.lib.kd6d_acc_read(ops._ptr(w), n, E, ops._ptr(out), accumulate, clear, ops._stream()),
                      "kd6d_acc_read")
            torch.cuda.synchronize()
            got, w = out.cpu().numpy(), w.cpu().numpy()
            want = (out0[:n] + val).astype(f32) if accumulate else val
            assert _same(got[:n], want), (accumulate, clear)
            assert _same(got[n:], out0[n:], nan_equal=False)
            want_w = words.copy()
            if clear:
                want_w[:2 * n] = 0
            assert np.array_equal(w, want_w), (accumulate, clear)
