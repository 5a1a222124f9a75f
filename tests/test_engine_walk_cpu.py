"""CPU: the forward and reverse walk of PoseNet in every mode of its knobs, with the device work replaced by the ledger
of walk_ledger.py.  A real PoseNet walks small CPU tensors; the tests assert what must hold of the launches in any mode
(not a recorded trace: the schedule is meant to change):
  * every ConvBlock / GroupNormReLU / convolution the forward visited gets its backward exactly once;
  * pair_towers 0, 1 and 2 issue the same launches once a pair launch counts for two;
  * accumulating data gradients have a producer, d_head_in is written before it is added to, out3's gradient is added once;
  * the ConvBlock arena layout is one table: disjoint, ordered, of the stated size, the same in forward and backward;
  * WgradSchedule.tail_start on real tapes; the eval walk's cut points.
Modes: pair_towers 0 / 1 / 2, fuse_pool on / off, bn_on_load 0 / 1 / 2, (batch, FUSE_STATS_MAX_ROWS) = (1, 1 << 15) and
(4, 512) at 64x64 input -- the second reaches the separate colstats pass and, at 16384 rows, the 8-replica backward --
and the fused stem launch on / off, for darknet_tiny_h and darknet53."""
import collections

import pytest
import torch

from kd6d import engine, ops as real_ops
from walk_ledger import Ledger, host_only, install, overlap, span

SMALL, LARGE = (1, 1 << 15), (4, 512)
# (arch, pair_towers, fuse_pool, bn_on_load, (batch, cut-off), parts the fused stem launch answers)
MODES = [("darknet_tiny_h", pair, fuse_pool, 0, bc, 0) for fuse_pool, bc in ((True, SMALL), (False, LARGE)) for pair in (0, 1, 2)]
MODES += [("darknet_tiny_h", 1, True, 1, LARGE, 0), ("darknet_tiny_h", 1, True, 2, SMALL, 0),
          ("darknet_tiny_h", 0, True, 2, LARGE, 2), ("darknet_tiny_h", 1, True, 1, SMALL, 2),
          ("darknet_tiny_h", 2, False, 0, SMALL, 2)]
MODES += [("darknet53", pair, True, 0, SMALL, 0) for pair in (0, 1, 2)] + [("darknet53", 1, True, 0, LARGE, 0)]
Walk = collections.namedtuple("Walk", "net led start")
_walks = {}


def walk(mode, train=True):
    """One forward (+ backward) walk of `mode`, done once and shared: the tests only read it."""
    if (mode, train) in _walks:
        return _walks[(mode, train)]
    arch, pair, fuse_pool, bol, (B, cutoff), stem = mode
    led = Ledger()
    led.stem_parts = stem
    with pytest.MonkeyPatch.context() as mp:
        install(mp, led)
        mp.setattr(engine.ConvBlock, "FUSE_STATS_MAX_ROWS", cutoff)
        net = host_only(engine.PoseNet(arch, dtype=torch.bfloat16))
        net.training = train
        net.pair_towers, net.fuse_pool, net.bn_on_load = pair, fuse_pool, bol
        net.cut_hook = lambda: led.events.append(("cut",))
        cls, reg = net.forward(torch.zeros(B, 3, 64, 64))
        start = len(led.events)
        if train:
            net.backward(torch.zeros(net.rows, cls.shape[1], dtype=torch.bfloat16),
                         torch.zeros(net.rows, reg.shape[1], dtype=torch.bfloat16))
    _walks[(mode, train)] = Walk(net, led, start)
    return _walks[(mode, train)]


def _block_recs(tape):
    for rec in tape:
        if isinstance(rec, engine.UnitRec):
            yield rec.conv1
            yield rec.conv2
        elif isinstance(rec, engine.BlockRec):
            yield rec


def _arg(call, pos, kw):
    _, _, a, k = call
    return a[pos] if pos < len(a) else k[kw]


# launch -> positions of (raw, mean, invstd) among its arguments
BN_FWD = {"bn_train_fwd": (0, 10, 11), "bn_train_fwd_res": (0, 11, 12), "bn_pool_train_fwd": (0, 13, 14)}
BN_BWD = {"bn_train_bwd": (0, 3, 4), "bn_pool_train_bwd": (0, 6, 7), "bn_pool_train_bwd_reduce": (0, 5, 6),
          "bn_pool_bwd_wgrad": (2, 4, 5)}


@pytest.mark.parametrize("mode", MODES, ids=str)
def test_every_block_norm_and_convolution_gets_its_backward_once(mode):
    net, led, start = walk(mode)
    recs = list(_block_recs(net.tape))
    assert ("cut",) not in led.events, "cut_hook is the eval walk's"
    assert len(recs) == sum(1 for c in net.convs if c.b is None and c.name.startswith("backbone"))
    by_raw = {rec.raw.data_ptr(): rec.block.name for rec in recs}
    assert len(by_raw) == len(recs)
    # ---- BatchNorm: one backward per block, reading the mean / invstd spans the forward saved
    saved, read = {}, collections.defaultdict(list)
    for call in led.calls:
        idx, name, a, k = call
        if name in BN_FWD:
            r, m, i = BN_FWD[name]
            saved[by_raw[a[r].data_ptr()]] = (span(a[m]), span(a[i]))
        elif name == "conv2d_fwd_norm":
            saved[by_raw[k["raw_out"].data_ptr()]] = (span(k["save_mean"]), span(k["save_invstd"]))
        elif name == "conv2d_fwd_block" and k["bn_in"] is not None:      # the previous block's, applied on load
            saved[by_raw[a[1].data_ptr()]] = (span(k["bn_in"]["save_mean"]), span(k["bn_in"]["save_invstd"]))
        elif name in BN_BWD:
            assert idx >= start
            r, m, i = BN_BWD[name]
            read[by_raw[a[r].data_ptr()]].append((name, span(a[m]), span(a[i])))
    assert set(saved) == set(by_raw.values()), "a block without a normalise launch"
    for blk in by_raw.values():
        names = sorted(n for n, _, _ in read[blk])
        assert names in (["bn_train_bwd"], ["bn_pool_train_bwd"], ["bn_pool_bwd_wgrad", "bn_pool_train_bwd_reduce"]), (blk, names)
        for _, m, i in read[blk]:
            assert (m, i) == saved[blk], "%s: the backward reads other mean / invstd spans than the forward saved" % blk
    fused_stem = [b for b in read if len(read[b]) == 2]
    assert len(fused_stem) == (1 if mode[5] and mode[2] else 0)
    # ---- GroupNorm: one backward per layer (a pair launch counts for two)
    gammas = collections.Counter()
    for _, name, a, k in led.calls:
        if name == "gn_relu_bwd":
            gammas[span(a[6])] += 1
        elif name == "gn_relu_bwd_pair":
            assert len(a[0]) == 2
            for item in a[0]:
                gammas[span(item[3])] += 1
    gns = [gn for tower in (net.cls_tower, net.pose_tower) for _, gn in tower]
    assert gammas == collections.Counter(span(net.store.storage(gn.gamma)) for gn in gns)
    # ---- convolutions: one weight gradient each, one data gradient each but the stem
    owner = {id(g): c.name for c in net.convs for g in c.geoms.values()}
    wgrads, dgrads = collections.Counter(), collections.Counter()
    for idx, name, a, k in led.calls:
        if name == "conv2d_wgrad":
            wgrads[owner[id(k["geom"])]] += 1
        elif name in ("group.add", "bn_pool_bwd_wgrad"):
            wgrads[owner[id(a[0])]] += 1
        elif name == "conv2d_dgrad":
            assert idx >= start
            dgrads[owner[id(a[0])]] += 1
    names = [c.name for c in net.convs]
    assert wgrads == collections.Counter(names)
    assert dgrads == collections.Counter(names[1:]) and net.convs[0].cin == 3
    # ---- the logits of both towers come from their final convolutions
    outs = [_arg(c, 99, "out").data_ptr() for c in led.calls if c[1] == "conv2d_fwd" and c[0] < start]
    for name in ("cls.logits", "pose.logits"):
        assert sum(1 for k, v in net._bufs.items() if k[0] == name and v.data_ptr() in outs) == 1


def _launch_multiset(w):
    """Launches of the walk keyed by name and the buffers they are handed; a pair launch counts as its two halves."""
    net, led, _ = w
    names = {v.data_ptr(): k[0] for k, v in net._bufs.items() if isinstance(k, tuple)}

    def key(t):
        return names.get(t.data_ptr(), tuple(t.shape))
    out = collections.Counter()
    for _, name, a, k in led.calls:
        if name == "gn_relu_bwd_pair":
            for item in a[0]:
                out[("gn_relu_bwd",) + tuple(key(t) for t in item[:3])] += 1
        elif name == "gn_relu_bwd":
            out[("gn_relu_bwd",) + tuple(key(t) for t in a[:3])] += 1
        else:
            vals = list(a) + [k[n] for n in sorted(k)]
            out[(name,) + tuple(key(v) if torch.is_tensor(v) else v for v in vals
                                if torch.is_tensor(v) or isinstance(v, (bool, int)))] += 1
    return out


@pytest.mark.parametrize("triple", [MODES[0:3], MODES[3:6], MODES[11:14]], ids=lambda t: "%s-%s" % (t[0][0], t[0][2]))
def test_pair_towers_changes_only_which_launches_go_out_together(triple):
    assert [m[1] for m in triple] == [0, 1, 2] and len({m[:1] + m[2:] for m in triple}) == 1
    sets = [_launch_multiset(walk(m)) for m in triple]
    assert sets[0] == sets[1] == sets[2]
    pairs = [[e[1] for e in walk(m).led.events if e[0] == "pair"] for m in triple]
    n = len(walk(triple[0]).net.cls_tower)
    assert [sum(p) for p in pairs] == [0, n + n - 1, n], "enabled brackets: none; every forward layer + every data " \
        "gradient but layer 0's; the forward layers alone"
    assert [sum(1 for c in walk(m).led.calls if c[1] == "gn_relu_bwd_pair") for m in triple] == [0, n, n]


@pytest.mark.parametrize("mode", MODES, ids=str)
def test_accumulating_gradients_have_a_producer(mode):
    net, led, start = walk(mode)
    head = [k["accumulate"] for idx, name, a, k in led.calls if name == "conv2d_dgrad"
            and k["dx"].data_ptr() == net.buf("d_head_in", (net.rows, net.out_channel)).data_ptr()]
    assert head == [False, True], "d_head_in: one tower writes it, then the other adds"
    n_acc = 0
    for idx, name, a, k in led.calls:
        if name == "conv2d_dgrad" and k["accumulate"]:
            sp = span(k["dx"])
            assert any(start <= w < idx and overlap(sp, s) for w, s in led.writes), "nothing produced what event %d adds to" % idx
            n_acc += 1
    assert n_acc >= 3           # d_head_in, the FPN's top-down sums, the top feature
    adds = [a[3].data_ptr() for idx, name, a, k in led.calls if name == "eltwise" and a[0] == real_ops.ELT_ADD]
    if mode[0] != "darknet53":
        bufs = {k[0]: v.data_ptr() for k, v in net._bufs.items() if isinstance(k, tuple)}
        assert adds == [bufs["d_p6"], bufs["d_out3"]], "the tiny sweep adds twice: P6's two gradients, then out3's"
        pools = [bufs[name] for name in sorted(bufs) if name.startswith("dpool")]
        got = [a[2].data_ptr() for _, name, a, k in led.calls if name == "maxpool2_bwd"]
        assert got == (pools[::-1] if not mode[2] else []) and len(pools) == (0 if mode[2] else 4)
    else:
        assert len(adds) == 1


@pytest.mark.parametrize("c, stage", [(8, 0), (64, 2)])
@pytest.mark.parametrize("rows", [(1 << 14) - 1, 1 << 14])
def test_convblock_arena_layout_is_one_table(rows, c, stage):
    net = engine.PoseNet("darknet_tiny_h", dtype=torch.bfloat16)
    blk = net.stages[stage][1 if stage else 0]
    assert blk.conv.cout_p == c
    A, R = real_ops.ACC_FLOATS, 8 if rows >= 1 << 14 else 1
    assert blk.bwd_replicas(rows) == R
    v = blk.scratch_views(rows)
    whole = span(net.scratch(blk.name, blk.scratch_floats(rows)))
    fields = [v.ssum, v.ssq, v.mean, v.invstd, v.w1, v.w2, v.barrier]
    assert [f.numel() for f in fields] == [A * c, A * c, c, c, A * R * c, A * R * c, real_ops.BARRIER_WORDS]
    at = whole[0]
    for f in fields:                    # in order, back to back: disjoint and without holes
        assert span(f)[0] == at
        at = span(f)[1]
    assert at == whole[1] and blk.scratch_floats(rows) == (2 * A + 2 + 2 * A * R) * c + real_ops.BARRIER_WORDS
    assert span(v.stats) == (span(v.ssum)[0], span(v.ssq)[1])
    assert list(net._scratch_off) == [(blk.name, blk.scratch_floats(rows))]


@pytest.mark.parametrize("mode", [MODES[0], MODES[3], MODES[7], MODES[11]], ids=str)
def test_tail_start_on_a_real_tape(mode):
    net = walk(mode).net
    tape, sched = net.tape, net.wgrad
    n_units = sum(len(units) for units in net.stages) + (1 if mode[0] == "darknet53" else 0)
    assert sum(1 for rec in tape if rec.is_block) == n_units, "a DarkUnit is one block, markers and pools none"
    assert all(rec.is_block == isinstance(rec, (engine.BlockRec, engine.UnitRec)) for rec in tape)
    assert sched.WGRAD_LIST_TAIL_BLOCKS == 2
    if mode[0] == "darknet53":          # init, down, unit, end of stage 1, down, unit, unit, end of stage 2 ...
        assert [type(rec).__name__ for rec in tape[:5]] == ["BlockRec", "BlockRec", "UnitRec", "Marker", "BlockRec"]
        assert sched.tail_start(tape) == 1 and sched.tail_start(tape[2:]) == 2 and sched.tail_start(tape[3:4]) == -1
    else:                               # block, pool (record or marker), block, pool, ...
        assert [rec.is_block for rec in tape[:4]] == [True, False, True, False]
        assert [rec.stage for rec in tape if not rec.is_block] == [0, 1, 2, 3]
        assert sched.tail_start(tape) == 2 and sched.tail_start(tape[1:]) == 3 and sched.tail_start(tape[:1]) == 0


@pytest.mark.parametrize("mode", [MODES[1], MODES[3], MODES[12]], ids=str)
def test_eval_walk_cuts(mode):
    net, led, _ = walk(mode, train=False)
    cuts = sum(1 for e in led.events if e == ("cut",))
    n_conv = len(net.cls_tower)
    if mode[0] == "darknet53":
        assert cuts == 1 + 28 + 3 + 2 * n_conv == 40
    else:
        assert cuts == len(net.inner) + 2 * n_conv == 10
    assert not net.tape and not any(e[0] == "pair" and e[1] for e in led.events)
