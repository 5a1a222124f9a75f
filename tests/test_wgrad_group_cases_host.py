"""CPU: the table of tests/wgrad_group_cases.py (the launches of tests/test_wgrad_group_gpu.py) against the REAL planner
of the grouped weight gradient.  kd6d_wgrad_group_plan is pure host code: it is called here through the loaded library
with made-up, never dereferenced pointers, and the plan it returns is decoded with ctypes mirrors of the structures of
csrc/conv_wgrad_group.hip (a layout change there fails test_plan_layout first).  Checked: the work list's invariants
for every launch of the table, that the table reaches the loader and split-rule edges it is there for (computed from
the decoded plans, not from the table's comments), kd6d_wgrad_group_supported at its boundaries, that the integer pass
is exact and rejects the results three broken loaders would give, and the loader's division rule over its whole range.
No device code runs or is read here."""
import collections
import ctypes
import functools

import numpy as np
import pytest
import torch

import wgrad_group_cases as C

i32, f32, ptr = ctypes.c_int32, ctypes.c_float, ctypes.c_void_p


class GLevel(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("H", "W", "PW", "P", "in_row0", "out_row0", "step0")] + [("inv_pw", f32), ("inv_h", f32), ("pad_", i32)]


class GProblem(ctypes.Structure):
    _fields_ = [(n, ptr) for n in ("x", "dy", "dw", "dbias")] + \
               [(n, i32) for n in ("Cin", "Cout", "ks", "J", "nseg", "steps", "x_bytes", "dy_bytes")] + [("lv", GLevel * C.MAX_SEG)]


class GTile(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("problem", "n0", "c0", "ky", "variant", "first_wg", "nsplit", "want_bias")]


class GWork(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("tile", "step_lo", "step_hi", "pad_")]


class GRBlock(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("tile", "chunk")]


class GHeader(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("n_problems", "n_tiles", "n_work", "n_rblocks", "off_problems", "off_tiles", "off_work",
                                   "off_rblocks", "pad0", "pad1", "pad2", "pad3")]


Decoded = collections.namedtuple("Decoded", "nbytes header problems tiles work rblocks info")


def _lib():
    from kd6d import _lib as L
    return L


def _align(v):
    return (v + 63) // 64 * 64


def geom_of(L, B, cin, cout, ksize, levels, stride=1, pad=None):
    g = L.ConvGeom()
    g.nseg, g.batch, g.cin, g.cout, g.ksize, g.stride = len(levels), B, cin, cout, ksize, stride
    g.pad = ksize // 2 if pad is None else pad
    r = 0
    for s, (h, w) in enumerate(levels[:L.MAX_SEG]):
        g.seg[s].in_h, g.seg[s].in_w, g.seg[s].out_h, g.seg[s].out_w = h, w, h, w
        g.seg[s].in_row0 = g.seg[s].out_row0 = r
        r += B * h * w
    return g


def plan(case, n_workgroups):
    """The library's plan of the case's launch, decoded."""
    L = _lib()
    n = len(case.items)
    arr = (L.WgradItem * n)()
    for i, (cin, cout, k, bias) in enumerate(case.items):
        arr[i].geom = geom_of(L, case.B, cin, cout, k, case.levels)
        base = 0x100000 * (i + 1)                                 # never dereferenced by the planner
        arr[i].x, arr[i].dy, arr[i].dw = base, base + 0x40000, base + 0x80000
        arr[i].dbias = base + 0xc0000 if bias else None
    info = (i32 * 4)()
    size = L.lib.kd6d_wgrad_group_plan(arr, n, L.KD6D_BF16, n_workgroups, None, 0, info)
    assert size > 0, L.lib.kd6d_last_error()
    queried = list(info)
    buf = ctypes.create_string_buffer(size + 64)
    buf.raw = b"\xa5" * (size + 64)
    got = L.lib.kd6d_wgrad_group_plan(arr, n, L.KD6D_BF16, n_workgroups, ctypes.cast(buf, ptr), size, info)
    assert got == size and list(info) == queried, "the size query disagrees with the filled plan"
    assert buf.raw[size:] == b"\xa5" * 64, "the planner wrote behind the size it reported"
    h = GHeader.from_buffer_copy(buf, 0)

    def table(kind, off, count):
        assert off % 64 == 0 and off + ctypes.sizeof(kind) * count <= size
        return [kind.from_buffer_copy(buf, off + ctypes.sizeof(kind) * j) for j in range(count)]
    return Decoded(size, h, table(GProblem, h.off_problems, h.n_problems), table(GTile, h.off_tiles, h.n_tiles),
                   table(GWork, h.off_work, h.n_work), table(GRBlock, h.off_rblocks, h.n_rblocks), queried)


@functools.lru_cache(maxsize=None)
def _plan(name, n_workgroups):
    return plan(C.BY_NAME[name], n_workgroups)


def table_plans():
    return [(C.BY_NAME[name], n, _plan(name, n)) for name, n in C.LAUNCHES]


# ---- the layout the mirrors assume -------------------------------------------------------------------------------------
def test_plan_layout():
    assert [ctypes.sizeof(t) for t in (GLevel, GProblem, GTile, GWork, GRBlock, GHeader)] == [40, 264, 32, 16, 8, 48]
    for case, n, p in table_plans():
        h = p.header
        assert h.n_problems == len(case.items) and h.off_problems == _align(ctypes.sizeof(GHeader))
        assert h.off_tiles - h.off_problems == _align(ctypes.sizeof(GProblem) * h.n_problems)
        assert h.off_work - h.off_tiles == _align(ctypes.sizeof(GTile) * h.n_tiles)
        assert h.off_rblocks - h.off_work == _align(ctypes.sizeof(GWork) * h.n_work)
        assert p.nbytes - h.off_rblocks == _align(ctypes.sizeof(GRBlock) * h.n_rblocks)
        assert (h.pad0, h.pad1, h.pad2, h.pad3) == (0, 0, 0, 0)


# ---- (a) invariants of every plan ----------------------------------------------------------------------------------------
def check_plan(case, n_workgroups, p):
    what = "%s at %d workgroups" % (case.name, n_workgroups)
    h = p.header
    for i, ((cin, cout, k, bias), q) in enumerate(zip(case.items, p.problems)):
        base = 0x100000 * (i + 1)
        assert (q.x, q.dy, q.dw, q.dbias) == (base, base + 0x40000, base + 0x80000, base + 0xc0000 if bias else None), what
        assert (q.Cin, q.Cout, q.ks, q.J, q.nseg) == (cin, cout, k, k * k * cin, len(case.levels)), what
        assert q.x_bytes == C.rows(case) * cin * 2 and q.dy_bytes == C.rows(case) * cout * 2, what
        step = row = 0
        for (H, W, PW, P), lv in zip(C.positions(case, k), q.lv):
            assert (lv.H, lv.W, lv.PW, lv.P, lv.in_row0, lv.out_row0, lv.step0) == (H, W, PW, P, row, row, step), what
            assert PW == W + (2 if k == 3 else 0) and P == case.B * H * PW
            assert lv.inv_pw == np.float32(1.0) / np.float32(PW) and lv.inv_h == np.float32(1.0) / np.float32(H), what
            step += -(-P // C.KSTEP)
            row += case.B * H * W
        assert q.steps == step == C.steps(case, k), what
    # tiles: the set {(n0, c0, ky)} of every problem, each once, in the variant its layer dictates; the bias is summed by
    # the c0 = 0, centre-ky tile of every n0 of a problem that has a dbias, and by no other
    want = {}
    for i, (cin, cout, k, bias) in enumerate(case.items):
        v = C.variant_of(k, cout)
        for n0 in range(0, cout, C.tile_shape(v)[0]):
            for c0 in range(0, cin, 128):
                for ky in range(k):
                    want[(i, n0, c0, ky)] = (v, int(bias and c0 == 0 and ky == k // 2))
    got = [(t.problem, t.n0, t.c0, t.ky) for t in p.tiles]
    assert len(got) == len(set(got)) and set(got) == set(want), what
    for t in p.tiles:
        assert (t.variant, t.want_bias) == want[(t.problem, t.n0, t.c0, t.ky)], what
    # works: every id belongs to exactly one tile, a tile's splits partition its steps
    owner = [None] * h.n_work
    for ti, t in enumerate(p.tiles):
        st = p.problems[t.problem].steps
        assert 1 <= t.nsplit <= st and 0 <= t.first_wg and t.first_wg + t.nsplit <= h.n_work, what
        at = 0
        for s in range(t.nsplit):
            w = p.work[t.first_wg + s]
            assert owner[t.first_wg + s] is None and w.tile == ti and w.pad_ == 0, what
            owner[t.first_wg + s] = ti
            assert w.step_lo == at and w.step_hi > w.step_lo, (what, ti, s)
            at = w.step_hi
        assert at == st, what
    assert None not in owner and h.n_work == sum(t.nsplit for t in p.tiles), what
    # reduce blocks: every 1024-float chunk of every tile once, the bias block where the tile sums one
    blocks = {}
    for rb in p.rblocks:
        assert 0 <= rb.tile < h.n_tiles, what
        blocks.setdefault(rb.tile, []).append(rb.chunk)
    for ti, t in enumerate(p.tiles):
        bn, nt = C.tile_shape(t.variant)
        chunks = list(range(-(-bn * nt * 128 // 1024))) + ([-1] if t.want_bias else [])
        assert sorted(blocks.get(ti, [])) == sorted(chunks), (what, ti)
    assert h.n_rblocks == len(p.rblocks) and (p.info[0], p.info[1]) == (h.n_work, h.n_rblocks), what
    slab = h.n_work * C.SLAB_STRIDE
    assert (p.info[2], p.info[3]) == (slab & 0x7fffffff, slab >> 31), what
    # the Python copy of the split rule (which found the table's workgroup counts) agrees with the library
    rule = {(i, n0, c0, ky): ns for i, n0, c0, ky, st, raw, ns in C.split_rule(case, n_workgroups)}
    assert {(t.problem, t.n0, t.c0, t.ky): t.nsplit for t in p.tiles} == rule, what


def test_plan_invariants_of_every_launch():
    for case, n, p in table_plans():
        check_plan(case, n, p)
    case = C.BY_NAME["variants"]
    for n in range(1, 40):
        check_plan(case, n, plan(case, n))


# ---- (b) the table reaches what it is there for ------------------------------------------------------------------------
def test_the_table_reaches_the_edges_it_claims():
    variants, nsplits, capped, lengths, starts = set(), set(), 0, set(), set()
    levels = {1: [], 3: []}
    couts, cins, no_bias, depth = set(), set(), set(), set()
    for case, n, p in table_plans():
        raw = {(i, n0, c0, ky): (r, st) for i, n0, c0, ky, st, r, ns in C.split_rule(case, n)}
        for q in p.problems:
            couts.add(q.Cout); cins.add(q.Cin); depth.add(q.nseg)
            if not q.dbias:
                no_bias.add(q.ks)
            levels[q.ks] += [(lv.H, lv.PW, lv.P) for lv in q.lv[:q.nseg]]
        for t in p.tiles:
            q = p.problems[t.problem]
            variants.add(t.variant)
            nsplits.add(t.nsplit)
            r, st = raw[(t.problem, t.n0, t.c0, t.ky)]
            capped += r > (st + 3) // 4 and t.nsplit == (st + 3) // 4 and t.nsplit > 1
            firsts = [lv.step0 for lv in q.lv[:q.nseg]]
            for w in p.work[t.first_wg:t.first_wg + t.nsplit]:
                lengths.add(w.step_hi - w.step_lo)
                starts.add("first" if w.step_lo in firsts else "inside")
                if any(w.step_lo < f < w.step_hi for f in firsts):
                    starts.add("spans")
    assert variants == {C.V_128x3, C.V_16x3, C.V_128x1, C.V_16x1}
    assert 1 in nsplits and nsplits & {2, 3, 4, 5} and any(v % 8 == 0 for v in nsplits) and capped
    assert {1, 2} <= lengths and starts == {"first", "inside", "spans"}
    for k in (1, 3):
        lv = levels[k]
        assert any(PW == 64 for H, PW, P in lv), k
        assert any(64 % PW == 0 and PW < 64 for H, PW, P in lv), k
        assert any(64 < PW < 128 for H, PW, P in lv), k
        assert any(PW > 128 for H, PW, P in lv), k
        assert any(PW in (1, 3) for H, PW, P in lv), k
        assert any(H == 1 for H, PW, P in lv), k
        assert any(H < 64 // PW for H, PW, P in lv), k
        assert {0, 1, 63} <= {P % 64 for H, PW, P in lv}, k
    assert C.MAX_SEG in depth and C.MAX_SEG == _lib().MAX_SEG
    assert {8, 16, 24, 136, 240, 256} <= couts and {128, 256, 384} <= cins
    assert no_bias == {1, 3}


def test_the_table_stays_small():
    for case in C.CASES:
        for cin, cout, k, _ in case.items:
            assert 9 * C.rows(case) + 7 < 2 ** 23                   # twice over: the reuse launch adds the sums again
            assert 2 * C.rows(case) * cin * cout * k * k <= 2e9, case.name
    assert len(C.LAUNCHES) == len(set(C.LAUNCHES)) <= 32


# ---- (c) kd6d_wgrad_group_supported at its boundaries --------------------------------------------------------------------
def test_supported_boundaries():
    L = _lib()
    BF16, F32 = L.KD6D_BF16, L.KD6D_F32

    def ok(g, dtype=BF16):
        return bool(L.lib.kd6d_wgrad_group_supported(ctypes.byref(g), dtype))
    lv = [(4, 4)]
    assert ok(geom_of(L, 2, 128, 8, 3, lv)) and ok(geom_of(L, 2, 128, 8, 1, lv))
    assert ok(geom_of(L, 2, 128, 128, 3, [(4, 4)] * L.MAX_SEG))
    for cout in (4, 12):
        assert not ok(geom_of(L, 2, 128, cout, 3, lv)), cout
    for cin in (64, 192):
        assert not ok(geom_of(L, 2, cin, 128, 3, lv)), cin
    assert not ok(geom_of(L, 2, 128, 128, 5, lv))
    assert not ok(geom_of(L, 2, 128, 128, 3, lv, pad=0)) and not ok(geom_of(L, 2, 128, 128, 1, lv, pad=1))
    assert not ok(geom_of(L, 2, 128, 128, 3, lv, stride=2))
    for field in ("out_h", "out_w"):
        g = geom_of(L, 2, 128, 128, 3, lv)
        setattr(g.seg[0], field, 3)
        assert not ok(g), field
    g = geom_of(L, 2, 128, 128, 3, lv)
    g.nseg = 0
    assert not ok(g)
    g = geom_of(L, 2, 128, 128, 3, [(4, 4)] * L.MAX_SEG)
    g.nseg = L.MAX_SEG + 1
    assert not ok(g)
    assert not ok(geom_of(L, 2, 128, 128, 3, lv), F32)
    # B * H * (W + 2) < 2^24 positions (the loader's division rule): one-column maps reach it below the byte rule
    assert 3 * 5592405 < 2 ** 24 <= 3 * 5592406
    assert ok(geom_of(L, 1, 128, 128, 3, [(5592405, 1)])) and not ok(geom_of(L, 1, 128, 128, 3, [(5592406, 1)]))
    assert ok(geom_of(L, 5, 128, 128, 1, [(1118481, 1)])) and not ok(geom_of(L, 1, 128, 128, 1, [(5592406, 1)]))
    # 32-bit byte offsets: rows * max(cin, cout) * 2 < 2^31, the level's first row included
    for cin, cout, rows in ((128, 128, 2 ** 23), (128, 256, 2 ** 22), (384, 8, 2796203)):
        assert (rows - 1) * max(cin, cout) * 2 < 2 ** 31 <= rows * max(cin, cout) * 2
        for first, want in ((rows - 17, True), (rows - 16, False)):
            g = geom_of(L, 1, cin, cout, 3, [(4, 4)])
            g.seg[0].in_row0 = g.seg[0].out_row0 = first
            assert ok(g) == want, (cin, cout, first)
    # the planner refuses what the rule refuses, and a null tensor
    case = C.BY_NAME["one_step"]
    arr = (L.WgradItem * 1)()
    arr[0].geom = geom_of(L, 1, 64, 128, 3, case.levels)
    arr[0].x = arr[0].dy = arr[0].dw = 0x1000
    info = (i32 * 4)()
    assert L.lib.kd6d_wgrad_group_plan(arr, 1, BF16, 8, None, 0, info) < 0
    arr[0].geom = geom_of(L, 1, 128, 128, 3, case.levels)
    assert L.lib.kd6d_wgrad_group_plan(arr, 1, BF16, 8, None, 0, info) > 0
    arr[0].dw = None
    assert L.lib.kd6d_wgrad_group_plan(arr, 1, BF16, 8, None, 0, info) < 0
    arr[0].dw = 0x1000
    assert L.lib.kd6d_wgrad_group_plan(arr, 1, BF16, 0, None, 0, info) < 0


# ---- (d) the integer pass is exact and tells broken loaders apart ------------------------------------------------------
def _stacked(item, xs, dys):
    """The images of a batch as one tall map: what a loader without the map-row mask at image boundaries sums."""
    tall = lambda t: t.permute(1, 0, 2, 3).reshape(1, t.shape[1], t.shape[0] * t.shape[2], t.shape[3])
    return C.reference_item(item, [tall(x) for x in xs], [tall(dy) for dy in dys])


def _last_pixel_dropped(item, xs, dys):
    """Every level's last pixel missing from dY: an off-by-one at the level's end."""
    cut = []
    for dy in dys:
        dy = dy.clone()
        dy[-1, :, -1, -1] = 0
        cut.append(dy)
    return C.reference_item(item, xs, cut)


def _columns_wrapped(item, xs, dys):
    """The horizontal taps run on into the neighbouring map row of the image instead of reading padding: a loader without
    the column mask.  Tap (ky, kx) of pixel (y, x) reads pixel (y + ky - 1) * W + x + kx - 1 of the flattened image, if
    it exists."""
    cin, cout, k, _ = item
    dw = torch.zeros(cout, k, k, cin, dtype=torch.float64)
    for x, dy in zip(xs, dys):
        B, _, H, W = x.shape
        flat = torch.cat([x.double().reshape(B, cin, H * W), torch.zeros(B, cin, 1, dtype=torch.float64)], dim=2)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        for ky in range(k):
            for kx in range(k):
                src = (yy + ky - k // 2) * W + xx + kx - k // 2
                src = torch.where((src >= 0) & (src < H * W), src, torch.full_like(src, H * W)).reshape(-1)
                dw[:, ky, kx, :] += torch.einsum("bop,bcp->oc", dy.double().reshape(B, cout, H * W), flat[:, :, src])
    return dw, C.reference_item(item, xs, dys)[1]


def test_integer_pass_is_exact_and_rejects_broken_loaders():
    rejected = {"stacked": 0, "last pixel": 0, "wrapped": 0}
    for case in C.CASES:
        inputs, refs = C.integer_inputs(case), C.integer_reference(case)
        for i, (item, inp, (dw, db)) in enumerate(zip(case.items, inputs, refs)):
            cin, cout, k, bias = item
            what = "%s item %d" % (case.name, i)
            for t in inp["xs"] + inp["dys"]:
                assert t.dtype == torch.float32 and torch.equal(t, t.round()) and t.abs().max() <= 3, what
                assert torch.equal(t, t.to(torch.bfloat16).float()), what
            assert dw.shape == (cout, k, k, cin) and db.shape == (cout,), what
            for ref, init in ((dw, C.DW0), (db, C.DB0)):
                assert ref.dtype == torch.float64 and torch.equal(ref, ref.round()), what
                assert float(ref.abs().max()) * 2 + init < 2 ** 24, what          # the reuse launch adds the sums twice
                C.check_integer((ref + init).float(), ref + init, what)          # the reference itself passes
            # every tap that reaches a pixel of some level at all is non-zero for every result channel, and every input channel
            live = torch.tensor([[any(h > abs(ky - k // 2) and w > abs(kx - k // 2) for h, w in case.levels) for kx in range(k)]
                                 for ky in range(k)])
            assert live[k // 2, k // 2] and torch.equal((dw != 0).any(dim=3), live.expand(cout, k, k)), what
            assert (dw != 0).flatten(0, 2).any(dim=0).all(), what
            # the mutants, wherever they can differ at all:
            #   stacked     needs a vertical tap (3x3) and a second image (B > 1)
            #   last pixel  always
            #   wrapped     needs a horizontal tap (3x3) and a neighbouring map row: every case has a level with H > 1
            mutants = [("last pixel", _last_pixel_dropped(item, inp["xs"], inp["dys"]), True)]
            if k == 3:
                assert any(h > 1 for h, w in case.levels), what
                mutants.append(("wrapped", _columns_wrapped(item, inp["xs"], inp["dys"]), False))
                if case.B > 1:
                    mutants.append(("stacked", _stacked(item, inp["xs"], inp["dys"]), False))
            for name, (mdw, mdb), bias_differs in mutants:
                with pytest.raises(AssertionError, match="differ from the exact result"):
                    C.check_integer((mdw + C.DW0).float(), dw + C.DW0, name)
                if bias_differs:
                    with pytest.raises(AssertionError, match="differ from the exact result"):
                        C.check_integer((mdb + C.DB0).float(), db + C.DB0, name)
                else:
                    assert torch.equal(mdb, db), (what, name)
                rejected[name] += 1
    assert all(v >= 4 for v in rejected.values()), rejected
    # one wrong element in a million is reported with its place
    case = C.BY_NAME["one_step"]
    dw = C.integer_reference(case)[0][0] + C.DW0
    got = dw.float()
    got[127, 2, 2, 127] += 1
    with pytest.raises(AssertionError, match=r"1 of 147456 elements differ.*first at \[127, 2, 2, 127\]"):
        C.check_integer(got, dw, "one element")


def test_random_comparison_rejects_a_lost_pixel():
    case = C.BY_NAME["step_edges"]
    item, inp, (dw, db) = case.items[0], C.random_inputs(case)[0], C.random_reference(case)[0]
    C.check_random(dw.float(), dw, "the reference, rounded to fp32")
    assert C.random_error(dw.float(), dw) < 1e-3
    mdw, mdb = _last_pixel_dropped(item, inp["xs"], inp["dys"])
    with pytest.raises(AssertionError):
        C.check_random(mdw.float(), dw, "last pixel")
    assert C.random_error(mdw.float(), dw) > 1.0


# ---- (e) the loader's division -------------------------------------------------------------------------------------------
def fdiv_model(x, d):
    """fdiv of csrc/conv_wgrad_group.hip in numpy: q = int(float32(x) * float32(1 / d)), then the two corrections."""
    inv = np.float32(1.0) / np.float32(d)
    q = (x.astype(np.float32) * inv).astype(np.int32)
    q = q + ((q + 1) * np.int32(d) <= x)
    return q - (q * np.int32(d) > x)


def test_fdiv_rule_over_the_whole_supported_range():
    """Positions stay below 2^24 (kd6d_wgrad_group_supported) and the loader looks one step and one map row ahead, so
    fdiv sees x < 2^24 + 64 + d.  This models the arithmetic; it does not run the kernel."""
    ds = {1, 2, 3, 65, 130, 4098}
    for case in C.CASES:
        for k in {k for _, _, k, _ in case.items}:
            for H, W, PW, P in C.positions(case, k):
                ds |= {H, PW}
    assert {64, 32, 16, 8, 4, 72, 132, 7} <= ds
    CH = 1 << 22
    for d in sorted(ds):
        end = 2 ** 24 + 64 + d
        for lo in range(0, end, CH):
            x = np.arange(lo, min(lo + CH, end), dtype=np.int32)
            bad = np.nonzero(fdiv_model(x, d) != x // d)[0]
            assert len(bad) == 0, "fdiv(%d, %d) is wrong" % (x[bad[0]], d)
