"""The cases of the grouped weight gradient (csrc/conv_wgrad_group.hip, ops.WgradGroup): one row per launch -- batch,
pyramid levels, the layers of the group and the workgroup budgets it runs under -- with the inputs of the two passes
each row runs, the CPU references and the comparisons.  Shared by tests/test_wgrad_group_cases_host.py (CPU: the real
planner's work list for every row keeps its invariants, the table reaches the loader edges it is there for, the integer
pass is exact and rejects broken results) and tests/test_wgrad_group_gpu.py (one GPU test per row and budget).  No GPU
and no libkd6d here.

The kernel walks PADDED pixel positions in steps of KSTEP = 64: a map row of W pixels is PW = W + 2 positions for a 3x3
layer (PW = W for 1x1), a level has P = B * H * PW of them and starts on a step of its own.  The shapes below are the
smallest at which each relation between 64, PW, H and P exists.

Two passes per row:
  integer  activations and gradients are integers of {-3..3}, dW starts at 5 and dbias at 7: every product and every
           partial sum is an integer of magnitude <= 9 * pixels + 7 < 2^24, so fp32 is exact in ANY summation order,
           split or tile shape.  Compared with torch.equal against conv2d_weight / the column sums in fp64.  No tolerance.
  random   Gaussian inputs rounded to bf16, as test_wgrad_group_matches_torch builds them, under that test's tolerance:
           catches what integers cannot (a lost low mantissa bit)."""
import collections
import functools

import torch

from util_pack import round_to

KSTEP = 64
MAX_SEG = 5
SLAB_STRIDE = 128 * 384 + 128                    # floats of a workgroup's partial tile + its bias partial
V_128x3, V_16x3, V_128x1, V_16x1 = 0, 1, 2, 3      # the tile variants behind the kernel's switch
DW0, DB0 = 5.0, 7.0                              # what dW / dbias hold before the integer pass

Case = collections.namedtuple("Case", "name B levels items n_workgroups")      # items: (cin, cout, ksize, with_bias)

CASES = [
    # all four tile variants in one launch; cout 8 / 16 / 24 / 240 masks; bias absent on a 3x3 and on a 1x1 layer
    Case("variants", 2, [(8, 8), (4, 4), (2, 2), (1, 1)],
         [(128, 128, 3, True), (128, 240, 3, True), (128, 16, 3, True), (128, 128, 1, False), (128, 24, 1, True),
          (128, 8, 1, True), (128, 8, 3, False)], (1, 24, 512)),
    # 3x3 PW = 64, 32, 16, 8, 4: several whole map rows per step, no remainder; five levels; a second 128-tile with 8 live
    # rows; two cin chunks
    Case("pw_divides", 1, [(3, 62), (5, 30), (4, 14), (3, 6), (2, 2)],
         [(128, 136, 3, True), (256, 16, 3, True), (128, 128, 1, False)], (1, 24, 512)),
    Case("pw_divides_1x1", 1, [(2, 64), (3, 32), (5, 16)], [(128, 16, 1, True), (128, 128, 1, True)], (1, 16)),
    # PW = 72, 132, 65 (3x3) and 70, 130, 63 (1x1): no whole map row per step, a wrap every few steps, one-row maps
    Case("pw_long", 2, [(2, 70), (1, 130), (3, 63)], [(128, 128, 3, True), (128, 16, 1, True)], (1, 24, 512)),
    # PW = 3 and PW = 1: 21 / 64 map rows per step; one-row maps, whose ky = 0 / 2 taps are all padding; a batch boundary
    # every few positions
    Case("thin", 3, [(1, 1), (2, 1), (1, 5), (7, 1), (1, 1)],
         [(128, 128, 3, True), (128, 16, 3, False), (128, 128, 1, True), (128, 8, 1, True)], (1, 7)),
    Case("step_edges", 1, [(8, 6), (5, 11), (7, 7), (8, 14), (3, 41)], [(128, 128, 3, True)], (1, 24)),  # P 64 65 63 128 129
    Case("step_edges_1x1", 1, [(8, 8), (5, 13), (7, 9)], [(128, 16, 1, True)], (1, 24)),                 # P 64 65 63
    # three cin chunks x two cout tiles x three ky; works of 2-3 steps
    Case("wide", 2, [(6, 5), (3, 3)], [(384, 256, 3, True), (256, 240, 1, True)], (1, 40)),
    Case("one_step", 1, [(4, 4)], [(128, 128, 3, True), (128, 16, 1, True)], (1, 24)),     # the ring's prologue only
    # 43-47 steps: every branch of the split rule, dozens of splits that start inside a level
    Case("splits", 2, [(32, 32), (16, 16), (8, 8), (4, 4)],
         [(128, 128, 3, True), (128, 16, 3, True), (128, 128, 1, False), (128, 8, 1, True)], (1, 24, 48, 96)),
]
BY_NAME = {c.name: c for c in CASES}
LAUNCHES = [(c.name, n) for c in CASES for n in c.n_workgroups]


# ---- geometry ------------------------------------------------------------------------------------------------------------
def padded_width(w, ksize):
    return w + 2 * (ksize // 2)


def positions(case, ksize):
    """[(H, W, PW, P)] of the case's levels as a layer of `ksize` walks them."""
    return [(h, w, padded_width(w, ksize), case.B * h * padded_width(w, ksize)) for h, w in case.levels]


def steps(case, ksize):
    return sum(-(-p // KSTEP) for _, _, _, p in positions(case, ksize))


def rows(case):
    return case.B * sum(h * w for h, w in case.levels)


def variant_of(ksize, cout):
    return (V_128x3 if cout > 16 else V_16x3) if ksize == 3 else (V_128x1 if cout > 16 else V_16x1)


def tile_shape(variant):
    """(result channels, taps) of a variant's tile; a tile is always 128 input channels wide."""
    return (128 if variant in (V_128x3, V_128x1) else 16), (3 if variant in (V_128x3, V_16x3) else 1)


def split_rule(case, n_workgroups):
    """A copy of the planner's rule, in its tile order: [(item, n0, c0, ky, steps, uncapped splits, splits)].  The
    uncapped value is what the host test needs to tell a split count that the four-steps-per-split cap cut."""
    tiles = []
    for i, (cin, cout, k, _) in enumerate(case.items):
        bn, nt = tile_shape(variant_of(k, cout))
        cost = (8.0 if bn == 128 else 1.0) * nt + 3.0
        for n0 in range(0, cout, bn):
            for c0 in range(0, cin, 128):
                for ky in range(k):
                    tiles.append((i, n0, c0, ky, steps(case, k), cost))
    per_wg = sum(t[5] * t[4] for t in tiles) / float(n_workgroups)
    out = []
    for i, n0, c0, ky, st, cost in tiles:
        ns = int(cost * st / per_wg + 0.5)
        if ns >= 6:
            ns = max((ns + 3) // 8 * 8, 8)
        out.append((i, n0, c0, ky, st, ns, max(min(ns, (st + 3) // 4), 1)))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _seed(case, item):
    return 7919 * (CASES.index(case) + 1) + 101 * item


@functools.lru_cache(maxsize=None)
def _integer_inputs(name):
    case, out = BY_NAME[name], []
    for i, (cin, cout, k, _) in enumerate(case.items):
        g = torch.Generator().manual_seed(_seed(case, i))
        out.append(dict(xs=[torch.randint(-3, 4, (case.B, cin, h, w), generator=g).float() for h, w in case.levels],
                        dys=[torch.randint(-3, 4, (case.B, cout, h, w), generator=g).float() for h, w in case.levels]))
    return out


def integer_inputs(case):
    """Per item: xs, dys (NCHW fp32 tensors of integers -3 ... 3, one per level).  Shared; do not modify."""
    return _integer_inputs(case.name)


@functools.lru_cache(maxsize=None)
def _random_inputs(name):
    case, out = BY_NAME[name], []
    for i, (cin, cout, k, _) in enumerate(case.items):
        g = torch.Generator().manual_seed(_seed(case, i) + 1)
        out.append(dict(xs=[round_to(torch.randn(case.B, cin, h, w, generator=g), torch.bfloat16) for h, w in case.levels],
                        dys=[round_to(torch.randn(case.B, cout, h, w, generator=g), torch.bfloat16) for h, w in case.levels]))
    return out


def random_inputs(case):
    """Per item: Gaussian xs, dys rounded to bf16, as test_wgrad_group_matches_torch builds them.  Shared."""
    return _random_inputs(case.name)


# ---- references ------------------------------------------------------------------------------------------------------------
def reference_item(item, xs, dys):
    """fp64 on the CPU: (dW in the kernel's (cout, ky, kx, cin) layout, column sums of dY), summed over the levels."""
    cin, cout, k, _ = item
    dw = torch.zeros(cout, cin, k, k, dtype=torch.float64)
    db = torch.zeros(cout, dtype=torch.float64)
    for x, dy in zip(xs, dys):
        dw += torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dy.double(), stride=1, padding=k // 2)
        db += dy.double().sum(dim=(0, 2, 3))
    return dw.permute(0, 2, 3, 1).contiguous(), db


@functools.lru_cache(maxsize=None)
def _reference(name, integer):
    case = BY_NAME[name]
    inputs = integer_inputs(case) if integer else random_inputs(case)
    return [reference_item(item, inp["xs"], inp["dys"]) for item, inp in zip(case.items, inputs)]


def integer_reference(case):
    """Per item (dW, dbias) in fp64, exact, without the initial values.  Shared; do not modify."""
    return _reference(case.name, True)


def random_reference(case):
    return _reference(case.name, False)


# ---- comparisons -----------------------------------------------------------------------------------------------------------
def check_integer(got, want, what=""):
    """Exact: `got` (fp32, what the kernel left in dW or dbias) against the fp64 `want` (initial value included)."""
    assert got.dtype == torch.float32 and want.dtype == torch.float64 and got.shape == want.shape, what
    assert want.abs().max() < 2 ** 24 and torch.equal(want, want.round()), what
    want = want.float()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError("%s: %d of %d elements differ from the exact result; first at %s: got %r, want %r; last at %s" % (
            what, len(bad), want.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]), bad[-1].tolist()))


def random_tolerance(ref):
    """test_wgrad_group_matches_torch's: 2e-4 relative, 2e-4 of the largest reference entry absolute."""
    return dict(rtol=2e-4, atol=2e-4 * max(float(ref.abs().max()), 1.0))


def check_random(got, ref, what=""):
    torch.testing.assert_close(got.double(), ref, msg=lambda m: "%s: %s" % (what, m), **random_tolerance(ref))


def random_error(got, ref):
    """The largest error as a fraction of what check_random allows at that element."""
    tol = random_tolerance(ref)
    return float(((got.double() - ref).abs() / (tol["atol"] + tol["rtol"] * ref.abs())).max())
