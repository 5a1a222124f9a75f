"""One row per compiled convolution kernel variant (csrc/conv_plan.h, KD6D_CONV_*_TILES) and direction: the shape and
the kd6d_set_option values that make the planner choose exactly that variant, the inputs of the two passes each row
runs, the CPU references and the comparisons.  Shared by tests/test_conv_variant_cases_host.py (CPU: the table is
complete, every row plans what it declares, the integer pass is exact, the comparisons reject broken results) and
tests/test_conv_variants_gpu.py (one GPU test per row).  No GPU and no libkd6d here.

ROWS is written by hand: the declared variant of a row is what a reviewer expects the planner to choose, and the host
test fails when the planner disagrees.  Adding a tile to a KD6D_CONV_*_TILES list needs a row here.

Two passes per row:
  integer  activations, weights and gradients are integers of {-3..3}: exact in bf16 and fp32, every product and every
           partial sum of n terms is an integer of magnitude <= 9 n < 2^24, so the fp32 result is exact in ANY summation
           order, split or tile shape.  Compared with torch.equal against the convolution in fp64 (rounded once to bf16
           where the kernel stores bf16).  No tolerance.
  random   Gaussian inputs rounded to the dtype, built and compared as test_conv_fwd_plain / test_conv_dgrad /
           test_conv_wgrad of tests/test_kernels_gpu.py do: catches what integers cannot (a lost low mantissa bit, a
           wrong rounding on the store).

Every forward row also runs the fused per-channel statistics on NARROW integers (activations and weights of {-1, 0, 1}, an
integer shift): with |y| <= 255 the sum of squares over the 256 rows of the tallest tile stays below 2^24, every fp32
partial a workgroup forms is exact, and the accumulators (fixed point, unit 2^-32, two int64 words) are compared to the
word with the integer sums of the fp64 reference.  STAT_ROWS holds the rows of the group statistics and of the fused
instantiations (NORM, XF, the fused-normalisation halo tiles), compared the same way."""
import collections
import functools
from fractions import Fraction

import torch
import torch.nn.functional as F

import conv_plan_lib as P
from util_pack import round_to

Row = collections.namedtuple("Row", "id list variant kind dtype options case budgets note extra why", defaults=({}, ()))

# the lists whose variants serve forward and data gradient / forward only / the weight gradient
DIRECTIONS = {"igemm": ("fwd", "dgrad"), "glds": ("fwd", "dgrad"), "smallc": ("fwd", "dgrad"), "halo": ("fwd", "dgrad"),
              "splitk": ("fwd",), "wgrad": ("wgrad",), "wgrad_tr": ("wgrad",), "wgrad_small": ("wgrad",)}
DTYPES = {"igemm": ("bf16", "f32"), "glds": ("bf16",), "smallc": ("bf16",), "halo": ("bf16",), "splitk": ("bf16",),
          "wgrad": ("f32",), "wgrad_tr": ("bf16",), "wgrad_small": ("bf16",)}
# taken on trust from tests/test_kernels_gpu.py::test_conv_halo_two_per_cu_variants (conv.halo = 11 ... 15), which runs
# forward, data gradient and fused statistics of exactly these five single-patch-buffer twins (plain forward and data
# gradient only: their per-channel and group statistics have exact rows of their own in STAT_ROWS)
HALO_TWINS = ((128, 128, 2, 2, 33, 0), (128, 128, 4, 2, 33, 0), (128, 64, 4, 2, 33, 0), (64, 64, 4, 2, 33, 0),
              (128, 32, 4, 1, 33, 0))

ROWS = []


def _make_row(lst, variant, kind, dtype, options, case, budgets=(0,), note=""):
    variant = tuple(variant) + (0,) * (6 - len(variant))
    opt = ",".join("%s=%d" % (k.split(".")[1], v) for k, v in sorted(options.items())) or "default"
    B, cin, cout, k, stride, levels = case
    rid = "%s-%s-%s-%s-%s-b%dc%dn%dk%ds%d_%s" % (lst, "x".join(str(v) for v in variant), kind, dtype, opt, B, cin, cout, k, stride,
                                                "_".join("%dx%d" % l for l in levels))
    if budgets != (0,):
        rid += "-cu" + "_".join(str(b) for b in budgets)
    return Row(rid, lst, variant, kind, dtype, dict(options), (B, cin, cout, k, stride, [tuple(l) for l in levels]), tuple(budgets), note)


def _row(*args, **kw):
    r = _make_row(*args, **kw)
    assert all(q.id != r.id for q in ROWS), r.id
    ROWS.append(r)


# ---- register-staged kernel: 7 tiles x forward / data gradient x bf16 / fp32 -----------------------------------------
# fp32 always runs it; bf16 once the other families are switched off.  The tile follows N and the tile count (N = cout
# forward, N = cin for the data gradient), so each direction has its own shapes.
PLAIN = {"conv.halo": 0, "conv.smallc": 0, "conv.tile": 0}
IGEMM_FWD = [
    ((256, 16, 4, 1), (1, 16, 12, 1, 1, [(363, 361)])),                 # 512 tiles of 256 pixels, the last 29 rows short
    ((64, 16, 4, 1), (2, 24, 12, 3, 1, [(9, 7), (4, 3)])),              # two levels, N tail, k-steps straddle taps
    ((256, 32, 4, 1), (1, 8, 24, 3, 1, [(363, 361)])),
    ((64, 32, 4, 1), (2, 8, 24, 3, 2, [(19, 17)])),                     # stride 2
    ((128, 64, 2, 2), (1, 8, 40, 3, 1, [(222, 221)])),                  # N <= 64: 384 pixel tiles
    ((128, 64, 2, 2), (1, 64, 136, 1, 1, [(129, 127)])),                # N > 64: 128 x 3 tiles, 1x1, one full k-step
    ((64, 64, 2, 2), (2, 128, 72, 3, 1, [(9, 7), (4, 3)])),
    ((128, 128, 2, 2), (1, 8, 200, 3, 2, [(313, 311)])),                # 192 x 2 tiles, stride 2, K = 72
]
IGEMM_DGRAD = [
    ((256, 16, 4, 1), (1, 8, 16, 1, 1, [(363, 361)])),
    ((64, 16, 4, 1), (2, 8, 24, 3, 1, [(9, 7), (4, 3)])),
    ((256, 32, 4, 1), (1, 24, 8, 1, 1, [(363, 361)])),
    ((64, 32, 4, 1), (2, 24, 8, 3, 2, [(19, 17)])),
    ((128, 64, 2, 2), (1, 40, 8, 3, 1, [(222, 221)])),
    ((128, 64, 2, 2), (1, 136, 64, 1, 1, [(129, 127)])),
    ((64, 64, 2, 2), (2, 72, 128, 3, 1, [(9, 7), (4, 3)])),
    ((128, 128, 2, 2), (1, 200, 8, 1, 2, [(157, 157)])),                # 1x1, stride 2
]
for _dtype, _opts in (("bf16", PLAIN), ("f32", {})):
    for _v, _c in IGEMM_FWD:
        _row("igemm", _v, "fwd", _dtype, _opts, _c)
    for _v, _c in IGEMM_DGRAD:
        _row("igemm", _v, "dgrad", _dtype, _opts, _c)

# ---- LDS-DMA kernel: conv.tile = 1 ... 4 -------------------------------------------------------------------------------
GLDS_TILE = {1: (128, 128, 2, 2, 3), 2: (128, 64, 2, 2, 3), 3: (64, 64, 2, 2, 4), 4: (64, 64, 2, 2, 6)}
GLDS_BOTH = [(1, 192, 200, 3, 2, [(17, 15)]), (2, 128, 136, 1, 1, [(13, 11)])]
GLDS_FWD = [(2, 24, 72, 3, 1, [(9, 7), (4, 3)]),           # k-steps straddle taps, two levels
            (2, 8, 40, 1, 1, [(5, 5)])]                    # a single k-step under a ring of 3, 4 and 6 stages
GLDS_DGRAD = [(2, 72, 24, 3, 1, [(9, 7), (4, 3)])]         # the data gradient with a channel tail (N = cin = 72)
for _t, _v in GLDS_TILE.items():
    _o = {"conv.halo": 0, "conv.smallc": 0, "conv.tile": _t}
    for _c in GLDS_BOTH:
        _row("glds", _v, "fwd", "bf16", _o, _c)
        _row("glds", _v, "dgrad", "bf16", _o, _c)
    for _c in GLDS_FWD:
        _row("glds", _v, "fwd", "bf16", _o, _c)
    for _c in GLDS_DGRAD:
        _row("glds", _v, "dgrad", "bf16", _o, _c)

# ---- split-K (forward only, needs a workspace): conv.splitk = 100 * tile + splits asked for ---------------------------
SPLITK_CASES = [(2, 256, 128, 3, 1, [(8, 8)]), (1, 512, 200, 3, 2, [(16, 16)]), (2, 1024, 64, 1, 1, [(6, 6), (3, 3)])]
SPLITK_FORCE = {104: (128, 64, 2, 2, 3), 105: (128, 64, 2, 2, 3), 116: (128, 64, 2, 2, 3), 207: (64, 64, 2, 2, 3)}
for _f, _v in SPLITK_FORCE.items():
    for _c in SPLITK_CASES:
        _row("splitk", _v, "fwd", "bf16", {"conv.halo": 0, "conv.splitk": _f}, _c)

# ---- halo-patch kernel: conv.halo = 1 ... 9 on maps up to 64 wide (HMAX 65) and 65 ... 80 wide (HMAX 81) --------------
HALO_PICK = {1: (256, 128, 4, 2), 2: (128, 128, 2, 2), 3: (128, 128, 4, 2), 4: (128, 64, 4, 2), 5: (128, 32, 4, 1),
             6: (192, 128, 4, 2), 9: (64, 64, 4, 2)}
HALO_LEVELS = {65: ([(5, 40), (3, 20)], [(3, 33)], [(3, 64)]),          # a pyramid and the two edges of HMAX 65
               81: ([(4, 72), (2, 36)], [(3, 65)], [(3, 80)])}          # ... of HMAX 81
# 192 x 128 and the 4-wave 128 x 128 tile have no HMAX 81 form: the planner's documented fallback is 128 x 128 on 8 waves
HALO_FALLBACK_81 = (2, 6)
for _hmax, _lv in HALO_LEVELS.items():
    for _pick, _tile in HALO_PICK.items():
        _note = ""
        if _hmax == 81 and _pick in HALO_FALLBACK_81:
            _tile, _note = (128, 128, 4, 2), "fallback: conv.halo=%d has no HMAX 81 form" % _pick
        for _levels in _lv:
            # the 128 x 32 tile serves N <= 32: a narrow forward result with an N tail, the data gradient into 16 channels
            _f, _d = ((2, 128, 24, 3, 1, _levels), (2, 16, 128, 3, 1, _levels)) if _pick == 5 else \
                ((2, 192, 136, 3, 1, _levels), (2, 136, 192, 3, 1, _levels))
            _row("halo", _tile + (_hmax, 1), "fwd", "bf16", {"conv.halo": _pick}, _f, note=_note)
            _row("halo", _tile + (_hmax, 1), "dgrad", "bf16", {"conv.halo": _pick}, _d, note=_note)

# ---- resident-patch kernel: conv.smallc = 1; CG = source channels / 8, NB = 1, 2, 4, 8 by result channels -------------
SMALLC_LEVELS = [(9, 7), (5, 3)]
for _ci, _c in enumerate((8, 16, 32)):
    for _ni, (_n, _nb) in enumerate(((12, 1), (24, 2), (40, 4), (72, 8))):
        _row("smallc", (_c // 8, _nb), "fwd", "bf16", {"conv.smallc": 1}, (2, _c, _n, 3, 1, SMALLC_LEVELS))
        _cin = _n if _n != 12 else 8                                   # dgrad: cin % 8 == 0
        _row("smallc", (_c // 8, _nb), "dgrad", "bf16", {"conv.smallc": 1}, (2, _cin, _c, 3, 1, SMALLC_LEVELS))
_row("smallc", (1, 1), "dgrad", "bf16", {"conv.smallc": 1}, (2, 16, 8, 3, 1, SMALLC_LEVELS))      # a full channel tile

# ---- narrow weight gradient: wgrad.small = 1, no bias; CG = cin / 8, NB = ceil(cout / 16), KS = k ---------------------
WGRAD_BUDGETS = (0, 1, 16)
for _k in (1, 3):
    for _ci, _c in enumerate((8, 16, 32)):
        for _ni, (_n, _nb) in enumerate((((8, 16), 1), ((24, 32), 2), ((56, 64), 4))):
            _row("wgrad_small", (_c // 8, _nb, _k), "wgrad", "bf16", {"wgrad.small": 1},
                 (3, _c, _n[(_ci + _ni + _k) % 2], _k, 1, [(9, 7)]), budgets=WGRAD_BUDGETS)
# R = 9, five tiles per image, the last 4 rows short; at cu_budget 1 two persistent workgroups loop over several tiles
_row("wgrad_small", (1, 4, 3), "wgrad", "bf16", {"wgrad.small": 1}, (1, 8, 64, 3, 1, [(40, 13)]), budgets=WGRAD_BUDGETS)
# R halved to 1, 139264 bytes of LDS: one workgroup per CU
_row("wgrad_small", (4, 4, 3), "wgrad", "bf16", {"wgrad.small": 1}, (2, 32, 64, 3, 1, [(5, 200)]), budgets=WGRAD_BUDGETS)
# the widest map the rule accepts
_row("wgrad_small", (4, 4, 1), "wgrad", "bf16", {"wgrad.small": 1}, (2, 32, 64, 1, 1, [(7, 256)]), budgets=WGRAD_BUDGETS)

# ---- transposing weight gradient (bf16) and the fp32 weight gradient --------------------------------------------------
# what the narrow rule declines although it is forced: buffers over 144 KB even at R = 1; no 3-block variant
_row("wgrad_tr", (64, 1, 4), "wgrad", "bf16", {"wgrad.small": 1}, (2, 32, 64, 3, 1, [(6, 256)]),
     note="fallback: 2 x buf_bytes > 144 KB at R = 1")
_row("wgrad_tr", (64, 1, 4), "wgrad", "bf16", {"wgrad.small": 1}, (3, 16, 40, 3, 1, [(9, 7)]), note="fallback: no 3-block variant")
_row("wgrad_tr", (64, 1, 4), "wgrad", "bf16", {"wgrad.small": 1}, (3, 8, 48, 1, 1, [(9, 7)]), note="fallback: no 3-block variant")
WGRAD_CASES = [(16, (2, 24, 16, 3, 1, [(9, 7), (4, 3)])), (32, (2, 8, 24, 3, 2, [(19, 17)])), (64, (3, 72, 40, 1, 1, [(9, 7)])),
               (128, (2, 24, 136, 3, 1, [(9, 7), (4, 3)]))]
for _bn, _c in WGRAD_CASES:
    _row("wgrad_tr", (_bn,) + ((2, 2) if _bn == 128 else (1, 4)), "wgrad", "bf16", {"wgrad.small": 0}, _c)
    _row("wgrad", {16: (16, 128, 1, 4), 32: (32, 128, 1, 4), 64: (64, 64, 2, 2), 128: (128, 128, 2, 2)}[_bn], "wgrad", "f32", {}, _c)

# ======== the fused statistics and the fused forms of the forward kernels: STAT_ROWS ==================================
# kinds:  fwd_gstats  kd6d_conv2d_fwd with group statistics (extra: groups), {sum, sumsq} per (level, image, group)
#         fwd_norm    kd6d_conv2d_fwd_norm (extra: norm = "group" | "batch", groups): the NORM instantiations
#         fwd_block   kd6d_conv2d_fwd_block(bn = NULL, stats_replicas = R > 1): NORM = true register-staged tiles
#         fwd_xf      kd6d_conv2d_fwd_block(bn given) behind an exact 1x1 block A of 8 channels: XF = true tiles
# Levels the epilogue sums have H * W % 16 == 0 and a first row % 16 == 0 (conv_plan.h stats_level_skipped); the others come
# from the follow-up launch, which takes cout / 4 (cout / 8 for a bf16 tensor) dividing 256 only (conv_plan.h
# stats_followup_ok): the rows with a skipped level have 16, 32 or 64 result channels, the channel tails sit in rows of whole
# levels, and one row records the refusal.  Both kinds of level are compared exactly.
STAT_ROWS = []
STAT_KINDS = ("fwd_gstats", "fwd_norm", "fwd_block", "fwd_xf")
REPLICAS = 3             # replica rows of the fwd_block / fwd_xf rows: workgroup b adds to row b % 3


# what a row is there for (Row.why); the host test computes each on the row and holds the table against its own list
MIXED = ("summed and skipped levels", "M tail, partial fragment")
TAIL, KEYS, LEVELS, SHORT = "channel tail", "several summed keys in a tile", "a tile across a level boundary", "short last tile"


def _stat_row(lst, variant, kind, dtype, options, case, note="", why=(), **extra):
    r = _make_row(lst, variant, kind, dtype, options, case, note=note)
    rid = r.id + "".join("-%s%s" % (k[0], v) for k, v in sorted(extra.items()))
    assert all(q.id != rid for q in STAT_ROWS), rid
    STAT_ROWS.append(r._replace(id=rid, extra=dict(extra), why=(why,) if isinstance(why, str) else tuple(why)))


TINY_PYRAMID = [(8, 8), (4, 4), (2, 2), (1, 1)]      # at a batch of 4: first rows 0, 256, 320, 336; 2x2 and 1x1 are skipped
# ---- group statistics, register-staged kernel: every tile in bf16 and fp32 ------------------------------------------------
IGEMM_GSTATS = [
    # 518 tiles of 256 pixels, the last one 128 rows short; 3 groups of 4 in a 16-channel tile
    ((256, 16, 4, 1), (1, 8, 12, 3, 1, [(368, 360)]), 3, (TAIL, SHORT)),
    # summed and skipped levels in one launch, 170 rows: a partial last fragment
    ((64, 16, 4, 1), (2, 24, 16, 3, 1, TINY_PYRAMID), 4, MIXED),
    ((256, 32, 4, 1), (1, 8, 24, 3, 1, [(368, 360)]), 3, (TAIL, SHORT)),  # 8 channels per group, 3 of 4 groups
    # rows 64 ... 127: the last image of level 0 and two images of level 1 in one tile
    ((64, 32, 4, 1), (3, 8, 24, 3, 1, [(4, 8), (4, 4)]), 6, (LEVELS, KEYS, TAIL)),
    ((128, 64, 2, 2), (12, 8, 40, 3, 1, [(69, 64)]), 10, (KEYS, "N <= 64")),   # 34.5 tiles per image: tiles in two images
    ((128, 64, 2, 2), (1, 64, 136, 1, 1, [(129, 128)]), 17, (TAIL, "N > 64")),   # 130 x 3 tiles, the last with one group of 8
    # tile 4 holds the four 4x4 images, tile 5 only skipped levels and the M tail
    ((64, 64, 2, 2), (4, 16, 64, 3, 1, TINY_PYRAMID), 8, MIXED + (KEYS,)),
    ((64, 64, 2, 2), (3, 16, 40, 3, 1, [(8, 8), (4, 4)]), 5, (TAIL,)),   # 5 of 8 groups of 8 in a 64-channel tile
    ((128, 128, 2, 2), (4, 8, 200, 3, 1, [(88, 70)]), 50, (KEYS, TAIL)),  # 48.125 tiles per image, 18 of 32 groups in the last tile
]
for _dtype, _opts in (("bf16", PLAIN), ("f32", {})):
    for _v, _c, _g, _why in IGEMM_GSTATS:
        _stat_row("igemm", _v, "fwd_gstats", _dtype, _opts, _c, why=_why, groups=_g)

# ---- ... LDS-DMA kernel --------------------------------------------------------------------------------------------------
GLDS_GSTATS = [((4, 24, 64, 3, 1, TINY_PYRAMID), 16, MIXED),             # 4 per group; 16 of 32 groups in a 128-channel tile
               ((3, 64, 136, 1, 1, [(4, 8), (4, 4)]), 17, (LEVELS, TAIL))]   # 8 per group; a tile across the level boundary
for _t, _v in GLDS_TILE.items():
    for _c, _g, _why in GLDS_GSTATS:
        _stat_row("glds", _v, "fwd_gstats", "bf16", {"conv.halo": 0, "conv.smallc": 0, "conv.tile": _t}, _c, why=_why, groups=_g)

# ---- ... halo-patch kernel: every tile of the list, the five twins (conv.halo = 11 ... 15) included -------------------------
# rows 360 (first rows 0, 320, 352) and 616 (0, 576, 608): the 1 x 4 level is skipped, the last fragment partial; without
# it 352 and 608 rows of whole levels
HALO_GSTATS_LEVELS = {65: [(4, 40), (2, 8), (1, 4)], 81: [(4, 72), (2, 8), (1, 4)]}
HALO_TWIN_PICK = {11: (128, 128, 2, 2), 12: (128, 128, 4, 2), 13: (128, 64, 4, 2), 14: (64, 64, 4, 2), 15: (128, 32, 4, 1)}


def _halo_gstats_case(narrow, batch, levels, i):
    """(case, groups) of the i-th tile of a list: even i a pyramid with skipped levels and 64 (32 for the 32-channel tile)
    result channels, odd i its whole levels with a channel tail, 136 (24) channels; groups of 4 and of 8 in turn."""
    if i % 2 == 0:
        cout = 32 if narrow else 64
        return (batch, 64, cout, 3, 1, levels), cout // (8 if i % 4 == 0 and not narrow else 4)
    cout = 24 if narrow else 136
    return (batch, 64, cout, 3, 1, levels[:2]), cout // (8 if i % 4 == 1 and not narrow else 4)


for _hmax, _levels in HALO_GSTATS_LEVELS.items():
    for _i, (_pick, _tile) in enumerate(HALO_PICK.items()):
        if _hmax == 81 and _pick in HALO_FALLBACK_81:
            continue                                                      # (their fallback is pick 3's tile)
        _c, _g = _halo_gstats_case(_pick == 5, 2, _levels, _i)
        _stat_row("halo", _tile + (_hmax, 1), "fwd_gstats", "bf16", {"conv.halo": _pick}, _c, why=TAIL if _i % 2 else MIXED, groups=_g)
for _i, (_pick, _tile) in enumerate(HALO_TWIN_PICK.items()):
    _c, _g = _halo_gstats_case(_pick == 15, 4, TINY_PYRAMID, _i)
    _stat_row("halo", _tile + (33, 0), "fwd_gstats", "bf16", {"conv.halo": _pick}, _c, why=TAIL if _i % 2 else MIXED, groups=_g)

# ---- ... resident-patch kernel: takes no group statistics (smallc_rule); the call goes to the register-staged kernel ------
_stat_row("igemm", (64, 32, 4, 1), "fwd_gstats", "bf16", {"conv.smallc": 1}, (2, 8, 32, 3, 1, TINY_PYRAMID),
          note="fallback: the resident-patch kernel takes no group statistics", why=MIXED, groups=8)
# ---- a skipped level whose follow-up launch does not take the channel count (12 / 4 does not divide 256): refused up front
_stat_row("igemm", (64, 16, 4, 1), "fwd_gstats", "bf16", PLAIN, (2, 24, 12, 3, 1, TINY_PYRAMID),
          note="refused: stats_followup_ok", why=MIXED, groups=3)

# ---- the fused-normalisation halo tiles (KD6D_CONV_HALO_NORM_TILES): GroupNorm and BatchNorm launches ----------------------
# whole levels only; conv.halo = 3 sends these tiny maps to the halo kernel, the NORM tile follows the map width
HALO_NORM = [((33, 0), {"conv.halo": 3}, [(8, 8), (4, 4)], "up to 32 wide"),
             ((65, 1), {"conv.halo": 3}, [(2, 40), (1, 16)], "33 ... 63 wide"),
             ((65, 1), {"conv.halo": 3}, [(1, 64)], "64 wide"),
             ((65, 1), {"conv.halo": 3, "conv.halo_pairing": 0}, [(8, 8), (4, 4)], "up to 32 wide, no twins"),
             ((81, 1), {"conv.halo": 3}, [(2, 72), (1, 16)], "65 ... 79 wide"),
             ((81, 1), {"conv.halo": 3}, [(1, 80)], "80 wide")]
for _hp, _o, _levels, _why in HALO_NORM:
    for _norm, _g in (("group", 32), ("batch", 0)):
        _stat_row("halo_norm", (128, 128, 4, 2) + _hp, "fwd_norm", "bf16", _o, (2, 128, 128, 3, 1, _levels), why=_why, norm=_norm,
                  groups=_g)
# ... and the register-staged kernel's, one launch of each kind per dtype
for _dtype in ("bf16", "f32"):
    for _norm, _g in (("group", 32), ("batch", 0)):
        _stat_row("igemm", (64, 64, 2, 2), "fwd_norm", _dtype, {"conv.halo": 0}, (2, 8, 128, 3, 1, [(8, 8), (4, 4)]),
                  norm=_norm, groups=_g)

# ---- NORM = true and XF = true register-staged tiles: every tile in bf16 and fp32 -----------------------------------------
# BatchNorm on load needs stride 1: the two stride-2 shapes of IGEMM_FWD are replaced
IGEMM_XF = [(v, c) for v, c in IGEMM_FWD if c[4] == 1] + [((64, 32, 4, 1), (2, 8, 24, 3, 1, [(19, 17)])),
                                                        ((128, 128, 2, 2), (1, 8, 200, 1, 1, [(157, 157)]))]
for _dtype in ("bf16", "f32"):
    for _v, _c in IGEMM_FWD:            # (the 128 x 64 tile has two rules: N <= 64, and N > 64 with too few tiles of 128 x 128)
        _stat_row("igemm", _v, "fwd_block", _dtype, {}, _c, why="N <= 64" if _c[2] <= 64 else "N > 64", replicas=REPLICAS)
    for _v, _c in IGEMM_XF:
        _stat_row("igemm", _v, "fwd_xf", _dtype, {}, _c, why="N <= 64" if _c[2] <= 64 else "N > 64", replicas=REPLICAS)

BY_ID = {r.id: r for r in ROWS + STAT_ROWS}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}


def plan_options(row):
    """kd6d_set_option names -> the option fields of the host planner (conv_plan_lib.OPT_NAMES)."""
    return {name.split(".", 1)[1] if name.startswith("conv.") else name.replace(".", "_"): v for name, v in row.options.items()}


def splitk_ws_floats(row):
    """The workspace a split-K row passes: the slabs of the split count ASKED for (what the rule checks) + a guard."""
    layer = geometry(row.case)
    return (row.options["conv.splitk"] % 100) * layer["rows_out"] * row.case[2] + 4096


FWD_FAMILY = ("smallc", "halo", "splitk", "glds", "igemm")               # conv_plan.h Family
WGRAD_FAMILY = ("wgrad_small", "wgrad_tr", "wgrad")                      # ... WgradFamily


def planned(lib, row, ncu, budget=0, stats=0):
    """(list, variant as the list spells it, plan) of the row's call on a device of `ncu` CUs."""
    layer = P.Layer(*row.case)
    dtype = P.BF16 if row.dtype == "bf16" else P.F32
    opts = plan_options(row)
    if row.kind == "wgrad":
        p = P.plan_wgrad(lib, layer, dtype, 0, budget, ncu=ncu, **opts)
        name = WGRAD_FAMILY[p.family]
        v = {"wgrad_small": (p.CG, p.NB, p.KS, 0, 0, 0), "wgrad_tr": (p.BN, p.WN, p.WJ, 0, 0, 0),
             "wgrad": (p.BN, p.BJ, p.WN, p.WJ, 0, 0)}[name]
        return name, v, p
    ws = row.list == "splitk"
    p = P.plan_conv(lib, layer, row.kind, dtype, stats=stats, ws=int(ws), ncu=ncu, ws_bytes=4 * splitk_ws_floats(row) if ws else 0,
                    **opts)
    name = FWD_FAMILY[p.family]
    tile = (p.BP, p.BC, p.WP, p.WC)
    v = {"smallc": (p.CG, p.NB, 0, 0, 0, 0), "halo": tile + (p.HMAX, p.PDB), "splitk": tile + (p.NSTAGE, 0), "glds": tile + (p.NSTAGE, 0),
         "igemm": tile + (0, 0)}[name]
    assert not p.NORM and not p.XF
    return name, v, p


# ---- geometry and sizes ------------------------------------------------------------------------------------------------
def geometry(case):
    B, cin, cout, k, stride, levels = case
    pad = k // 2
    out = [((h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1) for h, w in levels]
    return dict(pad=pad, levels_out=out, rows_in=B * sum(h * w for h, w in levels), rows_out=B * sum(h * w for h, w in out))


def gemm(row):
    """(M, N, K) of the row's GEMM: M destination pixels (the reduction length of a weight gradient), K the reduction length
    of forward / data gradient."""
    B, cin, cout, k, stride, levels = row.case
    g = geometry(row.case)
    if row.kind == "dgrad":
        return g["rows_in"], cin, k * k * cout
    return g["rows_out"], cout, k * k * cin


def reduction_length(row):
    """Terms of the longest sum any element of the row's result is made of (the accumulated dx0 included)."""
    M, N, K = gemm(row)
    return M if row.kind == "wgrad" else K + 1


def reference_flops(row):
    M, N, K = gemm(row)
    return 2 * M * N * K


def largest_tensor_bytes(row):
    B, cin, cout, k, stride, levels = row.case
    g = geometry(row.case)
    extra = splitk_ws_floats(row) if row.list == "splitk" else 0
    return 4 * max(g["rows_in"] * cin, g["rows_out"] * cout, cout * cin * k * k, extra)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float()


@functools.lru_cache(maxsize=16)
def _integer_inputs(case_key):
    B, cin, cout, k, stride, levels = case_key
    g = torch.Generator().manual_seed(20240 + 131 * cin + 17 * cout + k)
    geo = geometry(case_key)
    return dict(xs=[_ints(g, B, cin, h, w) for h, w in levels], w=_ints(g, cout, cin, k, k),
                dys=[_ints(g, B, cout, h, w) for h, w in geo["levels_out"]], dx0=[_ints(g, B, cin, h, w) for h, w in levels])


def _key(case):
    return case[:5] + (tuple(case[5]),)


def integer_inputs(row):
    """xs, w, dys, dx0 (NCHW / OIHW fp32 tensors of integers -3 ... 3); the same for every row of a case."""
    return _integer_inputs(_key(row.case))


def random_inputs(row):
    """The Gaussian inputs of the direction, rounded to the row's dtype, as tests/test_kernels_gpu.py builds them; the
    same for every row of a case, direction and dtype."""
    return _random_inputs(_key(row.case), row.kind, row.dtype)


@functools.lru_cache(maxsize=16)
def _random_inputs(case_key, kind, dtype_name):
    row = Row("", "", (), kind, dtype_name, {}, case_key, (0,), "")
    B, cin, cout, k, stride, levels = row.case
    dtype = TORCH_DTYPE[row.dtype]
    geo = geometry(row.case)
    if row.kind == "fwd":                                    # _check_conv_fwd_plain
        g = torch.Generator().manual_seed(B * 1000 + cin * 7 + cout)
        xs = [round_to(torch.randn(B, cin, h, w, generator=g), dtype) for h, w in levels]
        w = round_to(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5, dtype)
        return dict(xs=xs, w=w)
    if row.kind == "dgrad":                                  # test_conv_dgrad
        g = torch.Generator().manual_seed(11)
        w = round_to(torch.randn(cout, cin, k, k, generator=g) / (cout * k * k) ** 0.5, dtype)
        dys = [round_to(torch.randn(B, cout, h, w_, generator=g), dtype) for h, w_ in geo["levels_out"]]
        dx0 = [round_to(torch.randn(B, cin, h, w_, generator=g), dtype) for h, w_ in levels]
        return dict(w=w, dys=dys, dx0=dx0)
    g = torch.Generator().manual_seed(13)                    # test_conv_wgrad
    xs = [round_to(torch.randn(B, cin, h, w_, generator=g), dtype) for h, w_ in levels]
    dys = [round_to(torch.randn(B, cout, h, w_, generator=g), dtype) for h, w_ in geo["levels_out"]]
    return dict(xs=xs, dys=dys)


def epilogue_inputs(row):
    """Per-channel scale and shift and a residual in the stored dtype for the forward epilogue call (on random_inputs)."""
    B, cin, cout, k, stride, levels = row.case
    g = torch.Generator().manual_seed(7 + cout)
    res = [round_to(torch.randn(B, cout, h, w, generator=g), TORCH_DTYPE[row.dtype]) for h, w in geometry(row.case)["levels_out"]]
    # (per-level factors that are powers of two: exact, so the tolerance of the epilogue call stays what it was)
    seg = torch.tensor((2.0, 0.25, 4.0, 0.5, 8.0)[:len(levels)])
    return dict(res=res, scale=torch.rand(cout, generator=g) + 0.5, shift=torch.randn(cout, generator=g), seg_scale=seg)


# ---- references ----------------------------------------------------------------------------------------------------------
def reference(row, inp, dtype=torch.float32):
    """The row's direction on the CPU in `dtype`: per level for forward (conv) and data gradient (dx, without dx0), one
    (cout, cin, k, k) tensor summed over the levels for the weight gradient."""
    B, cin, cout, k, stride, levels = row.case
    pad = k // 2
    if row.kind == "fwd":
        return [F.conv2d(x.to(dtype), inp["w"].to(dtype), stride=stride, padding=pad) for x in inp["xs"]]
    if row.kind == "dgrad":
        return [torch.nn.grad.conv2d_input((B, cin, h, w), inp["w"].to(dtype), dy.to(dtype), stride=stride, padding=pad)
                for (h, w), dy in zip(levels, inp["dys"])]
    ref = torch.zeros(cout, cin, k, k, dtype=dtype)
    for x, dy in zip(inp["xs"], inp["dys"]):
        ref += torch.nn.grad.conv2d_weight(x.to(dtype), (cout, cin, k, k), dy.to(dtype), stride=stride, padding=pad)
    return ref


@functools.lru_cache(maxsize=16)
def _integer_reference(case_key, kind):
    row = Row("", "", (), kind, "f32", {}, case_key, (0,), "")
    return reference(row, _integer_inputs(case_key), torch.float64)


def integer_reference(row):
    """fp64, exact; shared by the rows of a case and direction.  Do not modify the result."""
    return _integer_reference(_key(row.case), row.kind)


@functools.lru_cache(maxsize=16)
def _random_reference(case_key, kind, dtype_name):
    row = Row("", "", (), kind, dtype_name, {}, case_key, (0,), "")
    return reference(row, _random_inputs(case_key, kind, dtype_name))


def random_reference(row):
    """fp32, as the parity tests of tests/test_kernels_gpu.py compute it; shared.  Do not modify the result."""
    return _random_reference(_key(row.case), row.kind, row.dtype)


def epilogue_reference(conv, epi):
    """scale, shift, the level's factor, leaky ReLU (0.1) and the residual behind the convolutions `conv`, in the order of
    test_conv_fwd_epilogue."""
    return [F.leaky_relu((c * epi["scale"].view(1, -1, 1, 1) + epi["shift"].view(1, -1, 1, 1)) * float(epi["seg_scale"][li]), 0.1) + r
            for li, (c, r) in enumerate(zip(conv, epi["res"]))]


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def tol(dtype, stored):
    """test_kernels_gpu._tol: stored = the result was rounded to `dtype` on the way out."""
    if dtype == torch.float32:
        return dict(rtol=2e-4, atol=2e-4)
    return dict(rtol=1.2e-2, atol=1.2e-2) if stored else dict(rtol=2e-4, atol=2e-4)


def check_integer(got, ref, stored_dtype=torch.float32, what=""):
    """Exact: `got` (fp32 values of what the kernel stored) against the fp64 `ref`, rounded once where the kernel stores bf16."""
    want = ref.float() if stored_dtype == torch.float32 else round_to(ref.float(), stored_dtype)
    assert ref.abs().max() < 2 ** 24
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%s: %d of %d elements differ from the exact result; first at %s: got %r, want %r; last at %s" % (
            what, len(bad), want.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]), bad[-1].tolist()))


def check_random(got, ref, dtype, stored, what=""):
    """Forward and data gradient of the random pass: test_kernels_gpu._tol."""
    torch.testing.assert_close(got, ref, msg=lambda m: "%s: %s" % (what, m), **tol(dtype, stored))


def check_random_wgrad(got, ref, what=""):
    """Weight gradient of the random pass: 2e-4 relative to the largest reference entry (test_conv_wgrad)."""
    torch.testing.assert_close(got, ref, rtol=2e-4, atol=2e-4 * max(float(ref.abs().max()), 1.0), msg=lambda m: "%s: %s" % (what, m))


# ======== fused statistics: plans, inputs, exact references and the word comparison ===================================
def stat_flags(row):
    """plan_conv flags of a STAT_ROWS row's launch."""
    e = row.extra
    return {"fwd_gstats": dict(stats=1, groups=e.get("groups", 0)),
            "fwd_norm": dict(stats=1, groups=e.get("groups", 0), norm=1),
            "fwd_block": dict(stats=1, replicas=e.get("replicas", 0)),
            "fwd_xf": dict(stats=1, replicas=e.get("replicas", 0), xf=1)}[row.kind]


def planned_stat(lib, row, ncu):
    """(list, variant, plan) of a STAT_ROWS row's launch; a halo plan with the fused epilogue is of list halo_norm."""
    p = P.plan_conv(lib, P.Layer(*row.case), "fwd", P.BF16 if row.dtype == "bf16" else P.F32, ncu=ncu, **stat_flags(row),
                    **plan_options(row))
    name = FWD_FAMILY[p.family]
    tile = (p.BP, p.BC, p.WP, p.WC)
    v = {"smallc": (p.CG, p.NB, 0, 0, 0, 0), "halo": tile + (p.HMAX, p.PDB), "glds": tile + (p.NSTAGE, 0), "igemm": tile + (0, 0)}[name]
    if name == "halo" and p.NORM:
        name = "halo_norm"
    assert bool(p.NORM) == (row.kind in ("fwd_norm", "fwd_block")) and bool(p.XF) == (row.kind == "fwd_xf"), row.id
    assert bool(p.fused_epilogue) == bool(p.NORM)
    return name, v, p


def fusable(lib, row):
    """kd6d_conv2d_fwd_norm_fusable of a fwd_norm row, from the host build of the rule."""
    kind = 1 if row.extra["norm"] == "group" else 2
    return P.fusable(lib, P.Layer(*row.case), P.BF16 if row.dtype == "bf16" else P.F32, kind, row.extra["groups"], **plan_options(row))


def level_rows(row):
    """[(first GEMM row, pixels per image, summed by the epilogue)] of the destination levels, as set_stats sees them."""
    out, m = [], 0
    for h, w in geometry(row.case)["levels_out"]:
        out.append((m, h * w, (h * w) % 16 == 0 and m % 16 == 0))
        m += row.case[0] * h * w
    return out


def row_key(row, m):
    """The (level, image) key of GEMM row m: level * batch + image.  THE layout of every group-statistics reference
    here and of the accumulators kd6d_gn_relu_fwd consumes: level-major, image-major, then group, then {sum, sumsq}."""
    key = 0
    for li, (m0, hw, _) in enumerate(level_rows(row)):
        if m >= m0:
            key = li * row.case[0] + (m - m0) // hw
    return key


def row_keys(row):
    """row_key of every GEMM row, as one int64 tensor."""
    B = row.case[0]
    return torch.cat([(li * B + torch.arange(B)).repeat_interleave(hw) for li, (m0, hw, _) in enumerate(level_rows(row))])


@functools.lru_cache(maxsize=16)
def _narrow_inputs(case_key):
    B, cin, cout, k, stride, levels = case_key
    g = torch.Generator().manual_seed(777 + 131 * cin + 17 * cout + k)
    one = lambda *shape: torch.randint(-1, 2, shape, generator=g).float()
    return dict(xs=[one(B, cin, h, w) for h, w in levels], w=one(cout, cin, k, k),
                shift=torch.randint(-2, 3, (cout,), generator=g).float())


def narrow_inputs(row):
    """xs, w of {-1, 0, 1} and an integer shift of {-2 .. 2} per channel: the statistics passes.  With |y| <= 255 every fp32
    partial sum of squares over the at most 256 rows of a tile is an integer below 2^24: exact in any order."""
    return _narrow_inputs(_key(row.case))


@functools.lru_cache(maxsize=16)
def _narrow_reference(case_key):
    B, cin, cout, k, stride, levels = case_key
    inp = _narrow_inputs(case_key)
    return [F.conv2d(x.double(), inp["w"].double(), inp["shift"].double(), stride=stride, padding=k // 2) for x in inp["xs"]]


def narrow_reference(row):
    """conv + shift of narrow_inputs in fp64, per level (B, cout, h, w): integers.  Do not modify the result."""
    return _narrow_reference(_key(row.case))


def packed_rows(ys):
    """(M, cout) as the kernels pack the levels: level-major, image-major, then pixels."""
    return torch.cat([y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]) for y in ys])


def channel_sums(rows):
    """{sum[N], sumsq[N]} of an (M, N) tensor: Python integers for an integer tensor (exact), else fp64."""
    t = rows.to(torch.int64) if torch.equal(rows, rows.round()) else rows.double()
    return t.sum(0).tolist() + (t * t).sum(0).tolist()


def group_sums(rows, row, groups, keys=None):
    """{sum, sumsq} per (key, group) of an (M, N) tensor, in the layout of row_key; `keys`: the key of every GEMM row."""
    B, cout = row.case[0], row.case[2]
    nkeys = B * len(row.case[5])
    if keys is None:
        keys = row_keys(row)
    t = rows.to(torch.int64) if torch.equal(rows, rows.round()) else rows.double()
    t = t.reshape(rows.shape[0], groups, cout // groups)
    s1 = torch.zeros(nkeys, groups, dtype=t.dtype).index_add_(0, keys, t.sum(2))
    s2 = torch.zeros(nkeys, groups, dtype=t.dtype).index_add_(0, keys, (t * t).sum(2))
    return torch.stack([s1, s2], dim=2).reshape(-1).tolist()


def _scaled(s, unit):
    """s * 2^unit without rounding: a Python integer for an integer sum, else a Fraction (half and quarter integers of
    the backward sums; a float converts exactly)."""
    return s << unit if isinstance(s, int) else Fraction(s) * (1 << unit)


def check_stat_words(words, want, what="", unit=32):
    """Exact: accumulators as [lo, hi] int64 word pairs (kd6d_det.h, lo in units of 2^-unit: 32 for the forward
    statistics, 52 for the sums of the reverse sweep) against exact sums (Python integers, Fractions or floats that hold
    the sum exactly): hi * 2^47 + lo == S * 2^unit in Python integers / Fractions.  No rounding anywhere."""
    assert len(words) == len(want), (what, len(words), len(want))
    bad = [i for i, ((lo, hi), s) in enumerate(zip(words, want)) if (hi << 47) + lo != _scaled(s, unit)]
    if bad:
        i = bad[0]
        raise AssertionError("%s: %d of %d statistics differ from the exact sums; first at %d: got %r / 2^%d, want %s" % (
            what, len(bad), len(want), i, (words[i][1] << 47) + words[i][0], unit, want[i]))


def words_of(sums, unit=32):
    """The accumulator words an exact kernel leaves for exact sums (host tests; kd6d_gn_relu_fwd's STATS_READY input)."""
    out = []
    for s in sums:
        q = _scaled(s, unit)
        assert q == int(q), "%r is no multiple of 2^-%d" % (s, unit)
        q, sign = abs(int(q)), -1 if s < 0 else 1
        out.append([sign * (q & ((1 << 47) - 1)), sign * (q >> 47)])
    return out


def check_stat_values(words, want, what=""):
    """Random pass: the accumulators' values against fp64 sums of the stored tensor at the project's statistics tolerance
    (the kernel adds fp32 partial sums, rounded once each, so no word comparison here)."""
    got = torch.tensor([hi * 2.0 ** 15 + lo * 2.0 ** -32 for lo, hi in words], dtype=torch.float64)
    ref = torch.tensor(want, dtype=torch.float64)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4 * max(float(ref.abs().max()), 1.0), msg=lambda m: "%s: %s" % (what, m))
