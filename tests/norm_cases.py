"""The cases of the exact tests of csrc/norm_ops.hip: one row per path of the normalisation, pooling and resampling
kernels, the inputs, the CPU references and the comparisons.  Shared by tests/test_norm_cases_host.py (CPU: the tables
cover what csrc/norm_plan.h accepts, the exact rows are exact in fp32, the references agree with torch autograd, the
comparisons reject broken results) and tests/test_norm_kernels_gpu.py (one GPU test per row).  No GPU and no libkd6d here.

Exact inputs.  x: integers of [-4, 4]; dz / dy: integers of [-3, 3]; mean: integers of [-1, 1]; invstd of {1/2, 1/4};
gamma of {-1/2, 1/2, 1, 2} (a negative gamma flips the sign of the pre-activation); beta: an integer + 1/16, so the
pre-activation (a multiple of 1/8 plus 1/16) is never 0.  Then xhat is a multiple of 1/4, every fp32 partial sum a
thread or a workgroup forms is exact in any order, and for ACT_NONE / ACT_RELU the kernels' results are determined:

  words     accumulators {lo, hi} (kd6d_det.h): hi * 2^47 + lo == S * 2^E in Python integers / Fractions, E = 32 for
            colstats and the GroupNorm statistics, E = 52 for every sum of a backward
  dgamma    fp32, bit-equal (S * 32 fits the 24 bits of the hi word's conversion: test_norm_cases_host.py)
  dx        with a power-of-two row count 1/rows is exact and so is every intermediate of the backward: bit-equal to the
            fp64 result rounded once to the stored dtype (mode "exact").  On other row counts the sums are still
            compared to the word and dx under the tolerance of tests/test_kernels_gpu.py (mode "sums").

LeakyReLU multiplies by 0.1f, which rounds: those rows (mode "tol") compare sums, dgamma / dbeta and dx with fp64 under
the tolerances test_batchnorm_train_fwd_bwd uses.  Everything behind an rsqrtf (forward y, GroupNorm y / dx / dgamma)
stays on those tolerances as well; the GroupNorm dbeta and the first group sum (sum of dz * gamma over the rows whose
pre-activation is positive) are exact to the word as long as no pre-activation is near 0: beta is chosen so that
|pre| > 1e-2 everywhere (gn_case; asserted in fp64 by the host test)."""
import collections
import functools
from fractions import Fraction

import torch

from conv_variant_cases import check_stat_words, words_of  # noqa: F401  (words_of: the STATS_READY rows, host tests)

ACT_NONE, ACT_LEAKY, ACT_RELU = 0, 1, 2          # KD6D_ACT_* (include/kd6d.h)
ACT_NAME = {ACT_NONE: "none", ACT_LEAKY: "leaky", ACT_RELU: "relu"}
UNIT_ACT, UNIT_GRAD = 32, 52                     # KD6D_DET_ACT / KD6D_DET_GRAD (csrc/kd6d_det.h)
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
EG = {"bf16": 8, "f32": 4}                       # elements of a 16-byte granule
COMBOS = [("bf16", False), ("bf16", True), ("f32", False)]      # (activation dtype, x kept in fp32)
EPS = 1e-5
GUARD_ROWS = 8            # NaN rows behind every destination (the kernels write whole rows of granules, never tiles)
NAN = float("nan")


def x_dtype(dtype, xf32):
    return torch.float32 if xf32 else TORCH_DTYPE[dtype]


# ---- comparisons ------------------------------------------------------------------------------------------------------
def total_words(acc_int64, replicas=1):
    """[lo, hi] word pairs of `replicas` rows of accumulators (an int64 view of the workspace, on the host), the rows added
    as integers -- never through kd6d_acc_read, which rounds to fp32."""
    return acc_int64.reshape(replicas, -1, 2).sum(0).tolist()


def planar_words(acc_int64, offset, n, stride):
    """[lo, hi] of n PLANAR accumulators: lo of element i at [offset + i], hi at [offset + i + stride]."""
    return torch.stack([acc_int64[offset:offset + n], acc_int64[offset + stride:offset + stride + n]], 1).tolist()


def words_value(words, unit):
    """fp64 value of word pairs (the tolerance rows)."""
    return torch.tensor([float(Fraction((hi << 47) + lo, 1 << unit)) for lo, hi in words], dtype=torch.float64)


def check_sums_close(words, want, unit, what=""):
    """The LeakyReLU rows: accumulators against fp64 sums at the dgamma / dbeta tolerance of test_batchnorm_train_fwd_bwd."""
    ref = torch.as_tensor([float(v) for v in want], dtype=torch.float64)
    scale = max(1.0, float(ref.abs().max()))
    torch.testing.assert_close(words_value(words, unit), ref, rtol=1e-3, atol=1e-3 * scale, msg=lambda m: "%s: %s" % (what, m))


def check_equal(got, ref, dtype, what=""):
    """Bit-equal to the fp64 reference rounded once to the stored dtype.  got: the stored tensor as fp32 on the host."""
    want = ref.to(dtype).float()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ from the exact result; first at %s: got %r, want %r" % (
            what, len(bad), want.numel(), i, float(got[i]), float(want[i])))


def landed(got, rows, what=""):
    """The destination rows of a guarded buffer (fp32 on the host), once the guard rows behind them are seen untouched and
    no destination element is left unwritten (NaN)."""
    assert torch.isnan(got[rows:]).all(), "%s: wrote behind the last destination row" % what
    holes = torch.isnan(got[:rows]).nonzero()
    assert len(holes) == 0, "%s: %d destination elements never written, first %s" % (what, len(holes), holes[0].tolist())
    return got[:rows]


# ---- BatchNorm --------------------------------------------------------------------------------------------------------
# mode: "exact" words and dx to the bit | "sums" words to the bit, dx under tolerance | "tol" LeakyReLU, all under tolerance
# fill: what dgamma / dbeta hold before the backward (the kernels +=): "zero", "ints" or "none" (null pointers)
BnRow = collections.namedtuple("BnRow", "name dtype xf32 C rows act replicas mode fill note")

# k: C = eg << k, the nine channel classes channels_ok accepts (C / eg divides 256)
BN_CLASSES = [
    (0, "cgs 1: flush `pre`, all four DPP rotations (fp32 C = 4)"),
    (1, "cgs 2: flush `pre`, three rotations"),
    (2, "cgs 4: flush `pre`, two rotations"),
    (3, "cgs 8: flush `pre`, one rotation"),
    (4, "cgs 16: slots, 16 partials per channel"),
    (5, "cgs 32: slots, 8 partials"),
    (6, "cgs 64: slots, 4 partials"),
    (7, "cgs 128: slots, 2 partials (bf16 C = 1024: the last table class of bn_fwd_scale_shift)"),
    (8, "cgs 256: slots, nparts 1 (bf16 C = 2048 > kBnTabC: the non-table branch of bn_fwd_scale_shift)"),
]
# every class, in each dtype combination, runs these
BN_PER_CLASS = [
    # rows, act, mode, fill, note
    (64, ACT_NONE, "exact", "ints", "KD6D_ACT_NONE; dgamma / dbeta pre-filled"),
    (64, ACT_RELU, "exact", "zero", "KD6D_ACT_RELU"),
    (64, ACT_LEAKY, "tol", "zero", "KD6D_ACT_LEAKY"),
    (77, ACT_RELU, "sums", "none", "tail rows, 1 / rows inexact; dgamma = dbeta = NULL"),
]
BN_EXTRA = [
    # dtype, xf32, C, rows, act, replicas, mode, fill, note
    ("bf16", False, 64, 4096, ACT_RELU, 1, "exact", "zero", "16 reduce workgroups, 64 one-launch workgroups, one replica row"),
    ("bf16", False, 64, 4096, ACT_RELU, 3, "exact", "ints", "replica_totals: one batch of 8 with 5 rows masked"),
    ("bf16", False, 64, 4096, ACT_RELU, 8, "exact", "zero", "replica_totals: one full batch"),
    ("bf16", False, 64, 4096, ACT_RELU, 9, "exact", "zero", "replica_totals: a second batch of one row"),
    ("bf16", False, 64, 4096, ACT_RELU, 64, "exact", "zero", "replica_totals: eight batches; more rows than reduce workgroups"),
    ("f32", False, 16, 64, ACT_NONE, 64, "exact", "zero", "replicas larger than every grid of the row (one workgroup)"),
]
# one tensor above every cap: bn_apply_fwd / bn_bwd_apply (grid_for, 2048 workgroups x 4 granules a thread) and
# bn_bwd_reduce_grid (512 x 8 granules); the host test asks the planner
BN_LONG = BnRow("long-bf16-C64-r262221-relu-R8", "bf16", False, 64, 262144 + 77, ACT_RELU, 8, "sums", "zero",
                "second trip of bn_apply_fwd, bn_bwd_reduce and bn_bwd_apply; too long for the one-launch form")


def _bn_name(dtype, xf32, C, rows, act, replicas):
    return "%s%s-C%d-r%d-%s-R%d" % (dtype, "-xf32" if xf32 else "", C, rows, ACT_NAME[act], replicas)


def _bn_rows():
    out = []
    for dtype, xf32 in COMBOS:
        for k, cnote in BN_CLASSES:
            for rows, act, mode, fill, note in BN_PER_CLASS:
                C = EG[dtype] << k
                out.append(BnRow(_bn_name(dtype, xf32, C, rows, act, 1), dtype, xf32, C, rows, act, 1, mode, fill,
                                 "%s; %s" % (cnote, note)))
    for dtype, xf32, C, rows, act, R, mode, fill, note in BN_EXTRA:
        out.append(BnRow(_bn_name(dtype, xf32, C, rows, act, R), dtype, xf32, C, rows, act, R, mode, fill, note))
    return out


BN_ROWS = _bn_rows()

ColRow = collections.namedtuple("ColRow", "name dtype C rows sumsq note")
COLSTATS_ROWS = [ColRow("%s-C%d-r%d%s" % (d, C, r, "" if q else "-nosumsq"), d, C, r, q, note) for d, C, r, q, note in [
    ("bf16", 24, 77, True, "cgs 3: 85 partials per channel, LDS accumulators, thread 255 idle"),
    ("bf16", 40, 77, True, "cgs 5: 51 partials, LDS accumulators"),
    ("bf16", 240, 77, True, "cgs 30: 8 partials in slots, threads 240.. idle"),
    ("f32", 12, 77, True, "cgs 3, fp32"),
    ("f32", 20, 77, True, "cgs 5, fp32"),
    ("bf16", 64, 1, True, "rows = 1: one thread row has work"),
    ("f32", 4, 1, True, "rows = 1, cgs 1"),
    ("bf16", 64, 77, False, "sumsq = NULL"),
    ("f32", 20, 77, False, "sumsq = NULL on the LDS-accumulator path"),
    ("bf16", 2048, 1500, True, "long: rows > 128 * 8 * (256 / cgs), second trip of the colstats_grid cap"),
]]


@functools.lru_cache(maxsize=2)
def bn_inputs(rows, C):
    """x, dz: int8 (rows, C); mean, invstd, gamma, beta: fp64 (C).  Do not modify the result."""
    g = torch.Generator().manual_seed(7919 * rows + C)
    r = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
    return dict(x=r(-4, 4, rows, C).to(torch.int8), dz=r(-3, 3, rows, C).to(torch.int8), mean=r(-1, 1, C).double(), invstd=0.5 ** r(1, 2, C).double(),
                gamma=torch.tensor([-0.5, 0.5, 1.0, 2.0], dtype=torch.float64)[r(0, 3, C)], beta=r(-2, 2, C).double() + 1.0 / 16)


def prefill(C, fill):
    """What dgamma, dbeta hold before the backward: fp32 (C) each, or None."""
    if fill == "none":
        return None, None
    if fill == "zero":
        return torch.zeros(C), torch.zeros(C)
    g = torch.Generator().manual_seed(C)
    return tuple(torch.randint(-5, 6, (C,), generator=g).float() for _ in range(2))


def act_grad(dz, pre, act):
    """dz * act'(pre), fp64"""
    if act == ACT_NONE:
        return dz
    return torch.where(pre > 0, dz, dz * 0.1 if act == ACT_LEAKY else torch.zeros_like(dz))


def act_fwd(t, act):
    if act == ACT_NONE:
        return t
    return torch.where(t > 0, t, t * 0.1 if act == ACT_LEAKY else torch.zeros_like(t))


def column_sums(x):
    """{sum[C], sumsq[C]} of an integer (rows, C) tensor: Python integers."""
    x = x.to(torch.int64)
    return x.sum(0).tolist(), (x * x).sum(0).tolist()


def bn_forward_ref(x, gamma, beta, act, eps=EPS, momentum=0.1):
    """Train-mode BatchNorm + activation from the definition, fp64: y, batch mean, invstd, the running statistics after
    one update of (0, 1)."""
    x = x.double()
    rows = x.shape[0]
    mean = x.sum(0) / rows
    var = ((x - mean) ** 2).sum(0) / rows
    invstd = 1.0 / torch.sqrt(var + eps)
    y = act_fwd((x - mean) * invstd * gamma + beta, act)
    unbias = rows / (rows - 1.0) if rows > 1 else 1.0
    return dict(y=y, mean=mean, invstd=invstd, running_mean=momentum * mean, running_var=(1 - momentum) + momentum * var * unbias)


def bn_backward_ref(x, dz, mean, invstd, gamma, beta, act, exact=None, chunk=1 << 15):
    """BatchNorm backward for GIVEN mean / invstd, from the definition, in row chunks (the long rows).  exact (default: the
    activation is not LeakyReLU; needs the exact inputs above): the two sums are formed in int64 -- integer arithmetic on
    d and 4 * xhat, no autograd -- and returned as Python integers and Fractions of quarter integers; else in fp64.
    sums = sum d [C] + sum d xhat [C]; dx fp64; steps: every intermediate of the kernels' arithmetic (fp64, of the last
    chunk) for the exactness proof of the host test; abs_sums: sum |d|, sum |4 d xhat| per channel."""
    rows, C = x.shape
    exact = act != ACT_LEAKY if exact is None else exact

    def parts(lo):
        xhat = (x[lo:lo + chunk].double() - mean) * invstd
        pre = xhat * gamma + beta
        return xhat, pre, act_grad(dz[lo:lo + chunk].double(), pre, act)

    s1 = torch.zeros(C, dtype=torch.int64 if exact else torch.float64)
    s2 = torch.zeros_like(s1)
    a1, a2 = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for lo in range(0, rows, chunk):
        xhat, pre, d = parts(lo)
        a1 += d.abs().sum(0)
        a2 += (4 * d * xhat).abs().sum(0)
        if exact:
            xh4 = (4 * xhat).round()
            assert torch.equal(xh4, 4 * xhat) and torch.equal(d, d.round()), "not the exact inputs"
            s1 += d.to(torch.int64).sum(0)
            s2 += (d.to(torch.int64) * xh4.to(torch.int64)).sum(0)
        else:
            s1 += d.sum(0)
            s2 += (d * xhat).sum(0)
    sums = s1.tolist() + ([Fraction(v, 4) for v in s2.tolist()] if exact else s2.tolist())
    s1, s2 = s1.double(), s2.double() / (4 if exact else 1)
    k1, k2, sc = s1 / rows, s2 / rows, gamma * invstd
    dx, min_pre = torch.empty(rows, C, dtype=torch.float64), float("inf")
    for lo in range(0, rows, chunk):
        xhat, pre, d = parts(lo)
        t1 = d - k1
        t2 = xhat * k2
        t3 = t1 - t2
        dx[lo:lo + chunk] = sc * t3
        min_pre = min(min_pre, float(pre.abs().min()))
    steps = dict(xhat=xhat, pre=pre, d=d, d_xhat=d * xhat, s1=s1, s2=s2, k1=k1, k2=k2, t1=t1, t2=t2, t3=t3, sc=sc,
                 sh=beta - mean * sc, dx=dx[lo:lo + chunk])
    return dict(sums=sums, s1=s1, s2=s2, dx=dx, min_pre=min_pre, steps=steps, abs_sums=(a1, a2))


# ---- max-pool, pooled BatchNorm -----------------------------------------------------------------------------------------
def first_max(a):
    """2x2 / 2 max-pool of (B, H, W, C), H and W floored to even: an explicit loop over the four taps in row-major window
    order with a strict `>`, so `arg` (0..3) is the FIRST maximum.  No torch tie rule involved."""
    Ho, Wo = a.shape[1] // 2, a.shape[2] // 2
    best, arg = None, None
    for k in range(4):
        tap = a[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2]
        if k == 0:
            best, arg = tap.clone(), torch.zeros(tap.shape, dtype=torch.int64)
        else:
            m = tap > best
            best = torch.where(m, tap, best)
            arg = torch.where(m, torch.full_like(arg, k), arg)
    return best, arg


def last_max(a):
    """The wrong rule (`>=`): what the host test feeds the comparison to see it rejected."""
    best, arg = first_max(a.flip(1, 2))                  # flipping both axes reverses the window order
    return best.flip(1, 2), (3 - arg).flip(1, 2)


def route(arg, dy):
    """Max-pool backward: (B, H, W, C) with dy at the tap `arg` of every window, 0 elsewhere (H, W even)."""
    B, Ho, Wo, C = dy.shape
    out = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=dy.dtype)
    for k in range(4):
        out[:, (k >> 1)::2, (k & 1)::2] = torch.where(arg == k, dy, torch.zeros_like(dy))
    return out


def sumpool_ref(x):
    """(B, H, W, C) -> the sums of the 2x2 blocks."""
    return x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]


def upsample_ref(coarse):
    """nearest x2 of (B, Hc, Wc, C) by index: out[y, x] = coarse[y // 2, x // 2]"""
    B, Hc, Wc, C = coarse.shape
    iy, ix = torch.arange(2 * Hc) // 2, torch.arange(2 * Wc) // 2
    return coarse[:, iy][:, :, ix]


PoolBnRow = collections.namedtuple("PoolBnRow", "name dtype xf32 B H W C act mode note")
POOL_BN_SHAPES = [
    # B, H, W, act, mode, note
    (1, 2, 2, ACT_RELU, "exact", "one window per channel granule, 4 rows: 1 / rows exact"),
    (3, 4, 2, ACT_NONE, "sums", "Wo = 1, three images"),
    (2, 6, 10, ACT_RELU, "sums", "30 windows per granule: several workgroups at the wide classes"),
]
POOL_BN_CLASSES = [(0, "smallest class"), (4, "cgs 16"), (8, "largest class, cgs 256")]
POOL_BN_LONG = PoolBnRow("long-bf16-4x192x192-C128-relu", "bf16", False, 4, 192, 192, 128, ACT_RELU, "sums",
                         "589824 windows: above grid_for's 2048 x 256 (forward, apply) and bn_pool_bwd_reduce_grid's 512 x 512")


def _pool_bn_rows():
    out = []
    for dtype, xf32 in COMBOS:
        for k, cnote in POOL_BN_CLASSES:
            C = EG[dtype] << k
            shapes = POOL_BN_SHAPES + ([(2, 6, 10, ACT_LEAKY, "tol", "KD6D_ACT_LEAKY")] if k == 4 else [])
            for B, H, W, act, mode, note in shapes:
                out.append(PoolBnRow("%s%s-%dx%dx%d-C%d-%s" % (dtype, "-xf32" if xf32 else "", B, H, W, C, ACT_NAME[act]),
                                     dtype, xf32, B, H, W, C, act, mode, "%s; %s" % (cnote, note)))
    return out


POOL_BN_ROWS = _pool_bn_rows()


def pool_bn_acts(x, mean, invstd, gamma, beta, act, dtype):
    """The activations whose maximum the pooled kernels look for: act(fma(x, sc, sh)) in fp32 as bn_act forms it (every
    operation is exact on these inputs except LeakyReLU's one multiplication by 0.1f, done here in fp32 as well), rounded
    to the stored dtype.  x: integers (B, H, W, C)."""
    sc = (gamma * invstd).float()
    sh = (beta - mean * gamma * invstd).float()
    t = x.float() * sc + sh
    if act == ACT_LEAKY:
        t = torch.where(t > 0, t, t * torch.tensor(0.1, dtype=torch.float32))
    elif act == ACT_RELU:
        t = t.clamp_min(0)
    return t.to(dtype).float()


def pool_bn_argmax(*args):
    """(maxima, argmax) the pooled kernels re-derive: the first maximum of pool_bn_acts."""
    return first_max(pool_bn_acts(*args))


def pool_bn_backward_ref(row, inp, argmax=None):
    """Pooled BatchNorm backward = max-pool backward (first maximum of the rounded activations) + bn_backward_ref."""
    B, H, W, C = row.B, row.H, row.W, row.C
    x = inp["x"].reshape(B, H, W, C)
    _, arg = (argmax or pool_bn_argmax)(x, inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], row.act, TORCH_DTYPE[row.dtype])
    dz = route(arg, inp["dy"].reshape(B, H // 2, W // 2, C)).reshape(B * H * W, C)
    return bn_backward_ref(inp["x"], dz, inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], row.act)


@functools.lru_cache(maxsize=2)
def pool_bn_inputs(B, H, W, C):
    inp = dict(bn_inputs(B * H * W, C))
    g = torch.Generator().manual_seed(31 * B * H * W + C)
    inp["dy"] = torch.randint(-3, 4, (B * (H // 2) * (W // 2), C), generator=g).to(torch.int8)
    del inp["dz"]
    return inp


# ---- GroupNorm --------------------------------------------------------------------------------------------------------
GnRow = collections.namedtuple("GnRow", "name dtype xf32 C G levels batch backward note")
_L4 = (36, 9, 4, 1)
GN_ROWS = [GnRow("%s%s-C%d-G%d-%s-B%d" % (d, "-xf32" if xf else "", C, G, "x".join(map(str, lv)), B), d, xf, C, G, lv, B, bwd, note)
           for d, xf, C, G, lv, B, bwd, note in [
    ("f32", False, 64, 32, _L4, 3, True, "cpg 2: the (cpg & 3) != 0 branches of gn_stats, gn_bwd_block_sums and the k1 / k2 reload; cgs 16 fold"),
    ("f32", False, 128, 64, _L4, 2, True, "cpg 2 with G = 64: all of s_st[64 * 4]; cgs 32 fold"),
    ("bf16", False, 128, 32, _L4, 3, True, "cpg 4: a granule straddles two groups; cgs 16 fold"),
    ("bf16", True, 128, 32, _L4, 3, True, "the same with x kept in fp32 (load_x<float, 8>)"),
    ("bf16", False, 256, 64, _L4, 2, True, "cpg 4 straddle with G = 64; cgs 32 fold"),
    ("bf16", False, 64, 16, _L4, 3, True, "cgs 8: no fold"),
    ("bf16", False, 512, 32, (127, 128, 129), 2, True, "cgs 64, the widest backward: one-pass chunks of 32 rows, ragged last chunks"),
    ("bf16", False, 8, 2, _L4, 3, True, "smallest: cgs 1, one granule a row"),
    ("f32", False, 4, 1, _L4, 2, True, "smallest fp32, G = 1"),
    ("bf16", True, 64, 1, _L4, 2, True, "G = 1: a single group of 64 channels"),
    ("bf16", False, 128, 32, (64, 16, 4, 1, 9), 2, True, "nseg = KD6D_MAX_SEG = 5, a 1x1 level in the middle of the table"),
    ("bf16", False, 128, 32, (1,), 3, True, "a level of hw = 1 alone"),
    ("bf16", False, 128, 32, (127, 128, 129), 2, True, "127 / 128 / 129 rows around gn_chunk_rows() = 128"),
    ("f32", False, 64, 32, (127, 128, 129), 1, True, "the same with cpg 2 and batch = 1"),
    ("bf16", False, 1024, 32, (9, 1), 2, False, "forward only: above the backward's 512 channels, cgs 128"),
    ("bf16", False, 2048, 64, (9, 1), 2, False, "forward only: the widest tensor, cgs 256, G = 64"),
    ("f32", False, 1024, 32, (9, 1), 1, False, "forward only: fp32 cgs 256"),
]]


def gn_ref(x, dz, gamma, beta, levels, batch, G, eps=EPS, boundary_shift=0):
    """GroupNorm + ReLU forward and backward from the definition, fp64, over packed rows (level-major, then image).
    x, dz: (rows, C).  stats / gsum: [(level, image, group)] lists of {sum x, sum x^2} (Python integers for integer x) and
    of {sum dz' gamma, sum dz' gamma xhat}, dz' = dz where the pre-activation is positive.  boundary_shift: the wrong
    grouping (every group starts that many channels late, cyclically) for the host test's mutation."""
    C = x.shape[1]
    cpg = C // G
    if boundary_shift:
        perm = (torch.arange(C) + boundary_shift) % C
        inv = torch.argsort(perm)
        r = gn_ref(x[:, perm], dz[:, perm], gamma[perm], beta[perm], levels, batch, G, eps)
        return dict(r, y=r["y"][:, inv], dx=r["dx"][:, inv], dgamma=r["dgamma"][inv], dbeta=r["dbeta"][inv])
    integer = not x.is_floating_point()
    xd, dzd = x.double(), dz.double()
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    dgamma, dbeta = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    stats, gsum, margin, r0 = [], [], float("inf"), 0
    ga, be = gamma.reshape(G, cpg), beta.reshape(G, cpg)
    for hw in levels:
        n = hw * cpg
        blk = xd[r0:r0 + batch * hw].reshape(batch, hw, G, cpg)
        dblk = dzd[r0:r0 + batch * hw].reshape(batch, hw, G, cpg)
        if integer:
            bi = x[r0:r0 + batch * hw].reshape(batch, hw, G, cpg).to(torch.int64)
            s1, s2 = bi.sum((1, 3)), (bi * bi).sum((1, 3))
            stats += [v for pair in zip(s1.reshape(-1).tolist(), s2.reshape(-1).tolist()) for v in pair]
            s1, s2 = s1.double(), s2.double()
        else:
            s1, s2 = blk.sum((1, 3)), (blk * blk).sum((1, 3))
            stats += [v for pair in zip(s1.reshape(-1).tolist(), s2.reshape(-1).tolist()) for v in pair]
        mu = s1 / n
        rs = 1.0 / torch.sqrt((s2 / n - mu * mu).clamp_min(0) + eps)
        mu, rs = mu[:, None, :, None], rs[:, None, :, None]
        xh = (blk - mu) * rs
        pre = xh * ga + be
        margin = min(margin, float(pre.abs().min()))
        d = torch.where(pre > 0, dblk, torch.zeros_like(dblk))
        gd = d * ga
        a, b = gd.sum((1, 3)), (gd * xh).sum((1, 3))
        gsum += [v for pair in zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()) for v in pair]
        y[r0:r0 + batch * hw] = pre.clamp_min(0).reshape(batch * hw, C)
        dx[r0:r0 + batch * hw] = (rs * (gd - a[:, None, :, None] / n - xh * b[:, None, :, None] / n)).reshape(batch * hw, C)
        dgamma += (d * xh).sum((0, 1)).reshape(C)
        dbeta += d.sum((0, 1)).reshape(C)
        r0 += batch * hw
    return dict(y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, stats=stats, gsum=gsum, margin=margin)


@functools.lru_cache(maxsize=None)
def gn_case(row):
    """Inputs (x, dz: int64 (rows, C); gamma, beta: fp64) and the reference of a GroupNorm row.  beta = integer + 1/16, then
    moved up by eighths on the channels where some |pre-activation| <= 0.02, until none is left.  Do not modify the result."""
    rows = row.batch * sum(row.levels)
    g = torch.Generator().manual_seed(104729 * row.C + 31 * row.G + rows)
    x = torch.randint(-4, 5, (rows, row.C), generator=g)
    dz = torch.randint(-3, 4, (rows, row.C), generator=g)
    gamma = torch.tensor([-0.5, 0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (row.C,), generator=g)]
    beta = torch.randint(-1, 2, (row.C,), generator=g).double() + 1.0 / 16
    for _ in range(64):
        near = (gn_pre(x, gamma, beta, row.levels, row.batch, row.G).abs() <= 0.02).any(0)
        if not near.any():
            break
        beta = torch.where(near, beta + 0.125, beta)
    return dict(x=x, dz=dz, gamma=gamma, beta=beta, ref=gn_ref(x, dz, gamma, beta, row.levels, row.batch, row.G))


def gn_pre(x, gamma, beta, levels, batch, G, eps=EPS):
    """The pre-activations xhat * gamma + beta of gn_ref, (rows, C) fp64."""
    C = x.shape[1]
    cpg = C // G
    out, r0 = torch.empty(x.shape, dtype=torch.float64), 0
    for hw in levels:
        blk = x[r0:r0 + batch * hw].double().reshape(batch, hw, G, cpg)
        mu = blk.mean((1, 3), keepdim=True)
        var = (blk * blk).mean((1, 3), keepdim=True) - mu * mu
        xh = (blk - mu) / torch.sqrt(var.clamp_min(0) + eps)
        out[r0:r0 + batch * hw] = (xh * gamma.reshape(G, cpg) + beta.reshape(G, cpg)).reshape(batch * hw, C)
        r0 += batch * hw
    return out


# ---- pool / upsample / eltwise / image ----------------------------------------------------------------------------------
PoolRow = collections.namedtuple("PoolRow", "name dtype B H W C note")
POOL_ROWS = [PoolRow("%s-%dx%dx%d-C%d" % (d, B, H, W, C), d, B, H, W, C, note) for d, B, H, W, C, note in [
    ("bf16", 1, 2, 2, 8, "2x2 minimal, C = eg: one pooled granule"),
    ("f32", 1, 2, 2, 4, "2x2 minimal, C = eg, fp32"),
    ("bf16", 2, 20, 12, 64, "multi-workgroup: 3840 fine granules (15 workgroups), 960 pooled (4)"),
    ("f32", 3, 10, 14, 32, "multi-workgroup, fp32, three images: 3360 fine granules"),
    ("bf16", 2, 6, 10, 24, "cgs 3: no power of two"),
    ("f32", 2, 6, 10, 12, "cgs 3, fp32"),
    ("bf16", 4, 192, 192, 128, "long: 589824 pooled granules > 2048 x 256, second trip of every grid_for kernel"),
]]
POOL_ODD = PoolRow("bf16-2x7x5-C16-odd", "bf16", 2, 7, 5, 16, "odd H and W: maxpool2_fwd floors, the last row and column are never read")
ImgRow = collections.namedtuple("ImgRow", "name dtype B Cimg H W Cpad note")
IMAGE_ROWS = [ImgRow("%s-%dx%dx%dx%d-pad%d" % (d, B, ci, H, W, cp), d, B, ci, H, W, cp, note) for d, B, ci, H, W, cp, note in [
    ("bf16", 2, 3, 37, 29, 8, "the step's case (one 16-byte store per pixel) on 9 workgroups"),
    ("bf16", 2, 3, 37, 29, 16, "bf16 outside Cpad = 8: the scalar loop"),
    ("f32", 2, 3, 37, 29, 8, "fp32, Cpad 8"),
    ("f32", 2, 3, 37, 29, 16, "fp32, Cpad 16"),
    ("bf16", 2, 8, 37, 29, 8, "Cimg == Cpad: nothing padded, vector path"),
    ("f32", 2, 16, 37, 29, 16, "Cimg == Cpad, scalar loop"),
]]


@functools.lru_cache(maxsize=2)
def pool_inputs(B, H, W, C):
    """int16 tensors: x (B, H, W, C) of [-4, 4] (most windows tied), dy / coarse (B, H/2, W/2, C) of [-3, 3], the
    destinations' contents before an accumulate = 1 call.  Do not modify the result."""
    g = torch.Generator().manual_seed(B * 1000003 + H * 1009 + W * 13 + C)
    r = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int16)
    Ho, Wo = H // 2, W // 2
    return dict(x=r(-4, 4, B, H, W, C), dy=r(-3, 3, B, Ho, Wo, C), coarse=r(-3, 3, B, Ho, Wo, C), other=r(-3, 3, B, H, W, C),
                dx0=r(-5, 5, B, 2 * Ho, 2 * Wo, C), dc0=r(-5, 5, B, Ho, Wo, C))


def image_ref(img, cpad):
    """NCHW (B, Cimg, H, W) -> (B * H * W, Cpad), zero padded channels."""
    B, ci, H, W = img.shape
    out = torch.zeros(B, H, W, cpad, dtype=img.dtype)
    out[..., :ci] = img.permute(0, 2, 3, 1)
    return out.reshape(B * H * W, cpad)
