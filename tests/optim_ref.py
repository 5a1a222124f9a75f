"""Plain references for the gradient tail of the step (csrc/optim.hip): kd6d_grad_acc_resolve, kd6d_acc_read,
kd6d_sumsq, kd6d_clip_adamw, kd6d_cast_f32_to_bf16.  numpy and Python integers only, no GPU: tests/test_optim_gpu.py
compares the kernels with these, tests/test_optim_ref_host.py checks these alone (against csrc/kd6d_det.h built for the
host, torch.optim.AdamW in float64 and their own bounds).  Every bound the GPU tests assert is a function here; the
derivations are in profiles/optim_kernel_tolerances.md."""
import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32 (round to nearest)
MARGIN = 1.01                  # second-order terms of a product of (1 + delta) factors
DET_ACT, DET_GRAD = 32, 52     # KD6D_ACC_ACT / KD6D_ACC_GRAD
SUMSQ_PARTS = 128              # KD6D_SUMSQ_PARTS
WG_ELEMS = 1024                # elements a workgroup of kd6d_grad_acc_resolve / kd6d_sumsq covers per pass
f32 = np.float32


# ---- region table of kd6d_grad_acc_resolve (include/kd6d.h, "reproducible reductions") ----------------------------
def part_groups(parts):
    """PG of the header: 1 for parts <= 16, doubling at 32, 64, 128, 256, capped at 32."""
    pg = 1
    while pg < 32 and parts > 16 * pg:
        pg *= 2
    return pg


def region_blocks(count, parts, pg=None):
    """Workgroups of one region: ceil(count / 1024) for parts == 0, ceil(count / (1024 / PG)) otherwise."""
    per = WG_ELEMS if parts == 0 else WG_ELEMS // (part_groups(parts) if pg is None else pg)
    return (count + per - 1) // per


def region_table(regions, pg_of=part_groups):
    """regions: [(first, count, parts, slab address)] -> (flat int64 quintuples, total workgroups)."""
    desc, blk = [], 0
    for first, count, parts, addr in regions:
        desc += [first, count, blk, parts, addr]
        blk += region_blocks(count, parts, pg_of(parts) if parts else 1)
    return desc, blk


# ---- fixed-point accumulators (csrc/kd6d_det.h) --------------------------------------------------------------------
def det_value(lo, hi, E):
    """fp32 emulation of det_value<E>: float32(hi) * 2^(47 - E) + float32(lo) * 2^-E added in fp32, NaN for
    |hi| >= 2^46.  lo, hi: int64 arrays."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    v = np.ldexp(hi.astype(f32), 47 - E).astype(f32) + np.ldexp(lo.astype(f32), -E).astype(f32)
    v = v.astype(f32)
    return np.where((hi >= (1 << 46)) | (hi <= -(1 << 46)), f32(np.nan), v).astype(f32)


def det_value_grad(lo, hi):
    return det_value(lo, hi, DET_GRAD)


def det_value_act(lo, hi):
    return det_value(lo, hi, DET_ACT)


def det_exact_units(lo, hi):
    """Exact value of the accumulators in units of 2^-E, as Python integers: hi * 2^47 + lo."""
    return [int(h) * (1 << 47) + int(l) for l, h in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist())]


def det_bound_units(lo, hi):
    """Bound on |det_value - exact| in units of 2^-E: the three roundings of the formula (each word to fp32, then the
    sum), 2^-24 * (|hi * 2^47| + |lo| + |hi * 2^47 + lo|).  Floats (the bound itself needs no exactness)."""
    return [U * (abs(int(h)) * float(1 << 47) + abs(int(l)) + abs(int(h) * (1 << 47) + int(l)))
            for l, h in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist())]


def det_error_units(got, lo, hi, E):
    """|got - exact| in units of 2^-E for finite fp32 `got` (exact: every fp32 is an integer multiple of 2^-149 and
    Python integers carry it), and the bound, both as float arrays.  Entries whose hi word reads as NaN are skipped
    (error 0, bound 0): the caller checks those with isnan."""
    from fractions import Fraction
    err, bnd = [], []
    for g, l, h in zip(np.asarray(got, np.float64).tolist(), np.asarray(lo).tolist(), np.asarray(hi).tolist()):
        if abs(h) >= (1 << 46):
            err.append(0.0); bnd.append(0.0)
            continue
        if not np.isfinite(g):
            err.append(float("inf")); bnd.append(0.0)
            continue
        exact = h * (1 << 47) + l
        err.append(float(abs(Fraction(g) * (1 << E) - exact)))
        bnd.append(U * (abs(h) * float(1 << 47) + abs(l) + abs(exact)))
    return np.asarray(err), np.asarray(bnd)


SPECIAL_HI = [1 << 46, -(1 << 46), 1 << 47, (1 << 46) - 1, -((1 << 46) - 1)]      # NaN, NaN, NaN, finite, finite


def acc_words(n, seed):
    """n accumulator states {lo, hi} (int64 arrays) that are NOT images of single addends:
      kind 0  lo uniform in +-2^61, hi uniform in +-2^40, signs independent (the two terms partly cancel)
      kind 1  hi = k, lo = -k * 2^47 + r with |k| < 2^13, |r| < 2^30: the terms cancel to a small remainder
      kind 2  lo != 0, hi = 0          kind 3  lo = 0, hi != 0          kind 4  both zero
    kinds cycle with the index from a seeded start; the first and the last element are kind 0 (a dropped tail element
    shows); for n >= 16 five seeded positions carry hi = +-2^46, 2^47 (NaN) and +-(2^46 - 1) (finite)."""
    rng = np.random.default_rng(seed)
    kind = (np.arange(n) + int(rng.integers(0, 5))) % 5
    kind[0] = kind[-1] = 0
    lo = rng.integers(-(1 << 61), 1 << 61, n, dtype=np.int64)
    hi = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    lo[lo == 0] = 1
    hi[hi == 0] = -1
    k = rng.integers(-(1 << 13) + 1, 1 << 13, n, dtype=np.int64)
    k[k == 0] = 7
    r = rng.integers(-(1 << 30), 1 << 30, n, dtype=np.int64)
    lo = np.where(kind == 1, -k * (1 << 47) + r, lo)
    hi = np.where(kind == 1, k, hi)
    hi = np.where(kind == 2, 0, hi)
    lo = np.where(kind == 3, 0, lo)
    lo = np.where(kind == 4, 0, lo)
    hi = np.where(kind == 4, 0, hi)
    if n >= 16:
        pos = 1 + rng.permutation(n - 2)[:len(SPECIAL_HI)]
        for p, h in zip(pos, SPECIAL_HI):
            hi[p] = h
            kind[p] = 5
    return lo.astype(np.int64), hi.astype(np.int64), kind


# the word sets and shapes the GPU tests use (tests/test_optim_ref_host.py checks the emulation on exactly these)
PLANAR_COUNTS = [1, 1023, 1024, 1025, 2500]
SLAB_PARTS = [1, 2, 3, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 600]
ACC_READ_N = [1, 1025]


def planar_words(count):
    return acc_words(count, 7000 + count)


def acc_read_words(n, E):
    return acc_words(n, 100 * E + n)


def slab_counts(parts):
    """1, E - 1, E, E + 1, 3 E + 7 with E = 1024 / PG elements per workgroup."""
    E = WG_ELEMS // part_groups(parts)
    return [1, E - 1, E, E + 1, 3 * E + 7]


# ---- partial-image slabs -------------------------------------------------------------------------------------------
def slab_sum(slab, pg=None):
    """fp32 emulation of the slab sum of kd6d_grad_acc_resolve in the association include/kd6d.h states: PG groups;
    group g owns parts g, g + PG, g + 2 PG, ... and keeps FOUR running sums t_0..t_3 that start at 0, t_k adding parts
    g + k PG, g + (k + 4) PG, g + (k + 8) PG, ... in that order; the group's sum is (t_0 + t_1) + (t_2 + t_3); the
    group sums are added in g order.  slab: fp32 (parts, count) -> fp32 (count,)."""
    slab = np.asarray(slab, f32)
    parts, count = slab.shape
    pg = part_groups(parts) if pg is None else pg
    total = None
    for g in range(pg):
        t = [np.zeros(count, f32) for _ in range(4)]
        for s in range(g, parts, 4 * pg):
            for k in range(4):
                if s + k * pg < parts:
                    t[k] = (t[k] + slab[s + k * pg]).astype(f32)
        sg = ((t[0] + t[1]).astype(f32) + (t[2] + t[3]).astype(f32)).astype(f32)
        total = sg if total is None else (total + sg).astype(f32)
    return total


def slab_sum_in_part_order(slab, pg=None):
    """What the header said before: group g adds its parts g, g + PG, ... one after the other, the groups in g order.
    NOT what the kernel does; kept so that the host test can show that the bitwise comparison tells the two apart."""
    slab = np.asarray(slab, f32)
    parts, count = slab.shape
    pg = part_groups(parts) if pg is None else pg
    total = None
    for g in range(pg):
        sg = np.zeros(count, f32)
        for s in range(g, parts, pg):
            sg = (sg + slab[s]).astype(f32)
        total = sg if total is None else (total + sg).astype(f32)
    return total


def slab_bound(g0, slab):
    """Per-element bound on |fp32 result - fp64 sum| of grads + sum of parts, for ANY order of adding the parts + 1
    fp32 terms: every term passes through at most `parts` additions, each rounding by at most 2^-24 relative, so
    |error| <= parts * 2^-24 * (|g0| + sum |a_p|); 1 % for the second-order terms."""
    slab = np.asarray(slab, np.float64)
    return MARGIN * slab.shape[0] * U * (np.abs(np.asarray(g0, np.float64)) + np.abs(slab).sum(0))


def slab_data(parts, count, kind, seed):
    """kind 'int': integers in [-8, 8] (every partial sum of <= 601 terms stays below 2^24: any association is exact);
    kind 'rand': normals times 10^u, u uniform in [-3, 3]."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-8, 9, (parts, count)).astype(f32)
    return (rng.standard_normal((parts, count)) * 10.0 ** rng.uniform(-3, 3, (parts, count))).astype(f32)


def grads_data(n, kind, seed):
    """Non-zero starting gradients (the resolve is +=): small non-zero integers or spread normals."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        return (rng.integers(1, 9, n) * rng.choice([-1, 1], n)).astype(f32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
    g[g == 0] = f32(1.0)
    return g


# ---- kd6d_sumsq ----------------------------------------------------------------------------------------------------
def sumsq_blocks(n):
    """Workgroups kd6d_sumsq launches: one per 1024 elements, at most KD6D_SUMSQ_PARTS."""
    return max(1, min(SUMSQ_PARTS, (n + WG_ELEMS - 1) // WG_ELEMS))


def sum_partials(p):
    """fp32 sum of the 128 partials as a binary tree (7 roundings per term)."""
    p = np.asarray(p, f32).copy()
    assert p.shape == (SUMSQ_PARTS,)
    while p.size > 1:
        p = (p[:p.size // 2] + p[p.size // 2:]).astype(f32)
    return p[0]


def sumsq_roundings(n):
    """Longest chain of fp32 roundings between one x_i^2 and the fp32 total of the 128 partials, from the launch
    shape (at most 128 workgroups x 256 threads x float4 per pass):
      1      the square
      3      the three additions inside a float4
      iters  one addition to the thread's running sum per grid-stride pass, iters = ceil((n // 4) / (nb * 256))
      1      the scalar tail (n % 4 elements, one per thread of workgroup 0)
      6      the butterfly over the 64 lanes of a wave
      4      the four wave sums of a workgroup, added in turn
      7      the 128 partials (a pair, then a 64-lane butterfly in the kernel; a binary tree in sum_partials)
    A fused multiply-add only removes roundings."""
    nb = sumsq_blocks(n)
    iters = -(-(n // 4) // (nb * 256))
    return 1 + 3 + iters + 1 + 6 + 4 + 7


def sumsq_rel_bound(n):
    """All terms are non-negative, so D roundings give a RELATIVE error of at most (1 + 2^-24)^D - 1."""
    return MARGIN * sumsq_roundings(n) * U


# ---- kd6d_clip_adamw -----------------------------------------------------------------------------------------------
def bias_corrections(beta1, beta2, step):
    """(1 - beta1^t, sqrt(1 - beta2^t)) in double from the UNROUNDED betas, rounded to fp32 once: what the entry point
    and kd6d_set_hyper hand to the kernel."""
    return float(f32(1.0 - beta1 ** step)), float(f32(np.sqrt(1.0 - beta2 ** step)))


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, max_norm=0.0, clip=False, round_hyper=True):
    """float64 evaluation of the header's formula (torch.optim.AdamW semantics, step counted from 1), one step.
    clip: the gradient is first scaled by min(1, max_norm / (sqrt(sum g^2) + 1e-6)) when max_norm > 0 (clip_grad_norm_).
    round_hyper: the hyper-parameters are rounded to fp32 first, as the kernel receives them (and the 1e-6 of the clip
    is the fp32 constant); False gives plain double arithmetic for the comparison with torch.
    -> dict(p, m, v, gnorm_sq, coef, and the magnitudes the bounds are made of)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if round_hyper:
        bc1, bc2s = bias_corrections(beta1, beta2, step)
        lr, beta1, beta2, eps, wd, max_norm = (float(f32(x)) for x in (lr, beta1, beta2, eps, wd, max_norm))
        tiny = float(f32(1e-6))
    else:
        bc1, bc2s = 1.0 - beta1 ** step, float(np.sqrt(1.0 - beta2 ** step))
        tiny = 1e-6
    gnorm_sq = float(np.sum(g * g))
    coef = 1.0
    if clip and max_norm > 0:
        coef = min(1.0, max_norm / (np.sqrt(gnorm_sq) + tiny))
    gs = g * coef
    decay = 1.0 - lr * wd
    m_new = beta1 * m + (1.0 - beta1) * gs
    v_new = beta2 * v + (1.0 - beta2) * gs * gs
    denom = np.sqrt(v_new) / bc2s + eps
    step_size = lr / bc1
    p_new = p * decay - step_size * m_new / denom
    return dict(p=p_new, m=m_new, v=v_new, gnorm_sq=gnorm_sq, coef=coef,
                m_mag=np.abs(beta1 * m) + np.abs((1.0 - beta1) * gs), v_mag=np.abs(v_new),
                p_mag=np.abs(p * decay) + step_size / denom * (np.abs(beta1 * m) + np.abs((1.0 - beta1) * gs)))


def adamw_roundings(n, clip):
    """fp32 roundings behind each output of one kd6d_clip_adamw element (sqrtf and the division are correctly rounded in
    this build: no fast-math).  Rg, the scaled gradient g * coef: 0 without clipping; with it, the D(n) roundings of the
    squared norm are halved by the square root, then sqrt, + 1e-6, the division and the product: D / 2 + 4.
      m = beta1 m + (1 - beta1) g':        1 - beta1, two products, the sum, and g':                    Rm = Rg + 4
      v = beta2 v + (1 - beta2) g' g':     1 - beta2, three products, the sum, and g' twice:            Rv = 2 Rg + 5
      denom = sqrt(v) / bc2 + eps:         v's roundings halved (all terms >= 0: relative), sqrt, /, +: Rd = Rv / 2 + 3
      p = p (1 - lr wd) - (lr / bc1) m / denom:   lr wd, 1 -, the product | lr / bc1, the product with m, the
                                           division, m and denom | the difference:         Rp = 3 + (3 + Rm + Rd) + 1"""
    rg = (sumsq_roundings(n) / 2.0 + 4.0) if clip else 0.0
    rm = rg + 4.0
    rv = 2.0 * rg + 5.0
    rd = rv / 2.0 + 3.0
    rp = 3.0 + (3.0 + rm + rd) + 1.0
    return dict(g=rg, m=rm, v=rv, p=rp)


def adamw_bounds(ref, n, clip):
    """Per-element absolute bounds on |fp32 kernel - float64 formula| for p, exp_avg and exp_avg_sq: roundings of the
    expression x 2^-24 x the sum of the magnitudes of its terms (ref: the dict adamw_step returned)."""
    r = adamw_roundings(n, clip)
    return dict(p=MARGIN * r["p"] * U * ref["p_mag"], m=MARGIN * r["m"] * U * ref["m_mag"],
                v=MARGIN * r["v"] * U * ref["v_mag"])


def decay_only_bound(p, lr, wd):
    """g = m = v = 0: the update term is exactly 0 and p (1 - lr wd) has three roundings (lr wd, 1 -, the product)."""
    return MARGIN * 3 * U * np.abs(np.asarray(p, np.float64) * (1.0 - float(f32(lr)) * float(f32(wd))))


# ---- kd6d_cast_f32_to_bf16 -----------------------------------------------------------------------------------------
def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of fp32 x by integer arithmetic; NaN -> a quiet NaN."""
    b = np.asarray(x, f32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, f32))
    return np.where(nan, np.uint16(0x7fc0), r).astype(np.uint16)


CAST_PATTERNS = [
    0x3f808000, 0x3f818000,              # ties: even upper half stays, odd upper half goes up
    0xbf808000, 0xbf818000,
    0x3f808001, 0x3f807fff,              # just above / just below a tie
    0x3f818001, 0x3f817fff,
    0x7f7fffff, 0xff7fffff,              # largest finite fp32 -> +-inf
    0x7f7f8000, 0x7f7f7fff,              # tie at the top of the range -> inf; just below it stays finite
    0x00000000, 0x80000000,              # +-0
    0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00018000, 0x0000ffff,      # fp32 subnormals
    0x00800000, 0x7f800000, 0xff800000,  # smallest normal, +-inf
    0x7fc00000, 0xffc00001, 0x7f800001, 0x7fffffff, 0x7f80ffff,      # NaNs (quiet, signalling, payload in the low half)
]
