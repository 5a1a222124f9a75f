"""Every kernel of csrc/norm_ops.hip against an exact reference: one test per row of tests/norm_cases.py
(tests/test_norm_cases_host.py proves on the CPU that the rows cover every accepted channel class, every flush class and
every grid cap, that the rows marked exact are exact in fp32, and that the comparisons used here reject wrong results).

Inputs are small integers and binary fractions, so for ACT_NONE / ACT_RELU nothing rounds: the accumulators are read as
int64 words on the host (replica rows added as integers, never through kd6d_acc_read) and must equal S * 2^E; dgamma /
dbeta must be bit-equal; dx must be bit-equal to the fp64 result rounded once to the stored dtype when the row count is a
power of two.  What passes an rsqrtf or LeakyReLU's 0.1f is compared under the tolerances of tests/test_kernels_gpu.py.
Every destination is the head of a NaN-filled buffer: no hole inside, nothing written behind the last row.  Each kernel is
launched once per form and row; nothing here repeats a launch or stresses the in-kernel barriers."""
import pytest
import torch

import norm_cases as N
from test_kernels_gpu import _tol

pytestmark = pytest.mark.gpu

ACC_GUARD = 4             # zeroed accumulators behind every workspace: must stay zero
STAT_TOL = dict(rtol=1e-4, atol=1e-5)      # saved / running statistics, as test_batchnorm_train_fwd_bwd compares them


def _ops():
    from kd6d import ops
    return ops


@pytest.fixture
def pin():
    """pin(name, value): kd6d_set_option for the rest of this test."""
    ops, old = _ops(), []

    def set_(name, value):
        old.append((name, ops.get_option(name)))
        ops.set_option(name, value)
    yield set_
    while old:
        ops.set_option(*old.pop())


def _guarded(rows, cols, dtype, dev, fill=None):
    """(the whole buffer, its leading `rows` rows): NaN everywhere, or `fill` in the leading rows."""
    buf = torch.full((rows + N.GUARD_ROWS, cols), N.NAN, dtype=dtype, device=dev)
    if fill is not None:
        buf[:rows] = fill.to(dtype).to(dev)
    return buf, buf[:rows]


def _landed(buf, rows, what):
    return N.landed(buf.float().cpu(), rows, what)


def _accs(n, dev):
    """n zeroed accumulators and ACC_GUARD more behind them"""
    return _ops().acc_zeros(n + ACC_GUARD, dev)


def _words(acc, n, replicas=1, what=""):
    """[lo, hi] of n accumulators per replica row, the rows added as integers; the guard accumulators must be zero."""
    w = acc.view(torch.int64).cpu()
    assert not w[2 * replicas * n:].any(), "%s: wrote behind the accumulators" % what
    return N.total_words(w[:2 * replicas * n], replicas)


def _finish(ops):
    torch.cuda.synchronize()
    assert ops.lib.kd6d_barrier_timeouts() == 0


def _dev(t, dev, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(dev)


# ---- colstats ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", N.COLSTATS_ROWS, ids=lambda r: r.name)
def test_colstats_exact(gpu_device, row):
    ops, dev = _ops(), gpu_device
    x = N.bn_inputs(row.rows, row.C)["x"]
    s1 = _accs(row.C, dev)
    s2 = _accs(row.C, dev) if row.sumsq else None
    ops.colstats(x.to(N.TORCH_DTYPE[row.dtype]).to(dev), s1, s2)
    _finish(ops)
    want1, want2 = N.column_sums(x)
    N.check_stat_words(_words(s1, row.C, what="sum"), want1, "sum")
    if row.sumsq:
        N.check_stat_words(_words(s2, row.C, what="sumsq"), want2, "sumsq")


def _column_stats(ops, xd, x, C, dev):
    """The batch sums of the forward: kd6d_colstats, compared to the word.  x kept in fp32 at C = 2048 is 512 granules a
    row, more than colstats takes (the engine's come from the convolution epilogue there): the words are built on the host."""
    want1, want2 = N.column_sums(x)
    s1, s2 = _accs(C, dev), _accs(C, dev)
    if C // ops.granule(xd.dtype) > 256:
        for s, want in ((s1, want1), (s2, want2)):
            s.view(torch.int64)[:2 * C].copy_(torch.tensor(N.words_of(want), dtype=torch.int64).reshape(-1).to(dev))
        return s1, s2
    ops.colstats(xd, s1, s2)
    torch.cuda.synchronize()
    N.check_stat_words(_words(s1, C, what="colstats sum"), want1, "colstats sum")
    N.check_stat_words(_words(s2, C, what="colstats sumsq"), want2, "colstats sumsq")
    return s1, s2


# ---- BatchNorm --------------------------------------------------------------------------------------------------------
def _check_backward(row, got, ref, fill, dtype, what):
    C = row.C
    if row.mode == "tol":
        N.check_sums_close(got["words"], ref["sums"], N.UNIT_GRAD, what)
    else:
        N.check_stat_words(got["words"], ref["sums"], what, N.UNIT_GRAD)
    if fill[0] is not None:
        want_g, want_b = fill[0].double() + ref["s2"], fill[1].double() + ref["s1"]
        if row.mode == "tol":
            gs = max(1.0, float(ref["s2"].abs().max()))
            torch.testing.assert_close(got["dgamma"].double(), want_g, rtol=1e-3, atol=1e-3 * gs)
            torch.testing.assert_close(got["dbeta"].double(), want_b, rtol=1e-3, atol=1e-3 * gs)
        else:
            N.check_equal(got["dgamma"], want_g, torch.float32, what + ": dgamma")
            N.check_equal(got["dbeta"], want_b, torch.float32, what + ": dbeta")
    if row.mode == "exact":
        N.check_equal(got["dx"], ref["dx"], dtype, what + ": dx")
    else:
        torch.testing.assert_close(got["dx"].double(), ref["dx"], **_tol(dtype, stored=True))
    assert len(got["words"]) == 2 * C


def _same_bits(a, b, what):
    assert a["words"] == b["words"], what + ": accumulator words"
    assert torch.equal(a["dx"], b["dx"]), what + ": dx"
    if a["dgamma"] is not None:
        assert torch.equal(a["dgamma"], b["dgamma"]) and torch.equal(a["dbeta"], b["dbeta"]), what + ": dgamma / dbeta"


@pytest.mark.parametrize("row", N.BN_ROWS + [N.BN_LONG], ids=lambda r: r.name)
def test_batchnorm_exact(gpu_device, row):
    """colstats -> forward (tolerance: rsqrtf), then the backward on GIVEN exact mean / invstd in its three forms:
    reduce + apply, kd6d_bn_train_bwd without a counter, and with one (the one-launch kernel on every row but the long one)."""
    ops, dev = _ops(), gpu_device
    dtype, xdt = N.TORCH_DTYPE[row.dtype], N.x_dtype(row.dtype, row.xf32)
    rows, C, R = row.rows, row.C, row.replicas
    long_row = row is N.BN_LONG
    inp = N.bn_inputs(rows, C)
    xd, dzd = inp["x"].to(xdt).to(dev), inp["dz"].to(dtype).to(dev)
    gamma, beta = _dev(inp["gamma"], dev), _dev(inp["beta"], dev)
    # forward
    s1, s2 = _column_stats(ops, xd, inp["x"], C, dev)
    ybuf, y = _guarded(rows, C, dtype, dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    smean, sinv = torch.full((C,), N.NAN, device=dev), torch.full((C,), N.NAN, device=dev)
    ops.bn_train_fwd(xd, y, s1, s2, gamma, beta, N.EPS, 0.1, rm, rv, smean, sinv, row.act)
    _finish(ops)
    fwd = N.bn_forward_ref(inp["x"], inp["gamma"], inp["beta"], row.act)
    torch.testing.assert_close(_landed(ybuf, rows, "y").double(), fwd["y"], **_tol(dtype, stored=True))
    for got, key in ((smean, "mean"), (sinv, "invstd"), (rm, "running_mean"), (rv, "running_var")):
        torch.testing.assert_close(got.cpu().double(), fwd[key], **STAT_TOL)
    del fwd, ybuf, y
    # backward
    mean, invstd = _dev(inp["mean"], dev), _dev(inp["invstd"], dev)
    fill = N.prefill(C, row.fill)
    cdt, xf = ops.dt_code(dtype), ops._xf32(xd, dtype)
    p = ops._ptr

    def run(form):
        w1, w2 = _accs(R * C, dev), _accs(R * C, dev)
        dgam, dbet = _dev(fill[0], dev), _dev(fill[1], dev)
        dxbuf, dx = _guarded(rows, C, dtype, dev)
        counter = torch.zeros(ops.BARRIER_WORDS, dtype=torch.int32, device=dev) if form == "counter" else None
        if form == "pair":
            ops.check(ops.lib.kd6d_bn_train_bwd_reduce(cdt, xf, p(xd), p(dzd), rows, C, p(mean), p(invstd), p(gamma), p(beta), row.act,
                                                       p(w1), p(w2), R, ops._stream()), "kd6d_bn_train_bwd_reduce")
            ops.check(ops.lib.kd6d_bn_train_bwd_apply(cdt, xf, p(xd), p(dzd), p(dx), rows, C, p(mean), p(invstd), p(gamma), p(beta),
                                                      row.act, p(w1), p(w2), p(dgam), p(dbet), R, ops._stream()), "kd6d_bn_train_bwd_apply")
        else:
            ops.bn_train_bwd(xd, dzd, dx, mean, invstd, gamma, beta, row.act, w1, w2, dgam, dbet, replicas=R, counter=counter)
        _finish(ops)
        if counter is not None:
            assert (int(counter[0].item()) > 0) == (not long_row), "one-launch backward taken / not taken"
        return dict(words=_words(w1, C, R, form + ": sum_dy") + _words(w2, C, R, form + ": sum_dy_xhat"),
                    dx=_landed(dxbuf, rows, form + ": dx"), dgamma=None if dgam is None else dgam.cpu(),
                    dbeta=None if dbet is None else dbet.cpu())

    ref = N.bn_backward_ref(inp["x"], inp["dz"], inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], row.act)
    first = None
    for form in ("pair", "counter") if long_row else ("pair", "nocounter", "counter"):
        got = run(form)
        _check_backward(row, got, ref, fill, dtype, "%s, %s" % (row.name, form))
        if row.mode == "exact" and first is not None:
            _same_bits(first, got, "%s against pair" % form)
        first = first or got


# ---- pooled BatchNorm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", N.POOL_BN_ROWS + [N.POOL_BN_LONG], ids=lambda r: r.name)
def test_pooled_batchnorm_exact(gpu_device, row):
    """kd6d_bn_pool_train_fwd (tolerance), then kd6d_bn_pool_train_bwd without and with a counter and
    kd6d_bn_pool_train_bwd_reduce alone on given exact mean / invstd.  Integer x ties most windows: dx checks the
    first-maximum rule at every one of them."""
    ops, dev = _ops(), gpu_device
    dtype, xdt = N.TORCH_DTYPE[row.dtype], N.x_dtype(row.dtype, row.xf32)
    B, H, W, C = row.B, row.H, row.W, row.C
    rows, prows = B * H * W, B * (H // 2) * (W // 2)
    long_row = row is N.POOL_BN_LONG
    R = 8 if long_row else 1
    inp = N.pool_bn_inputs(B, H, W, C)
    xd, dyd = inp["x"].to(xdt).to(dev), inp["dy"].to(dtype).to(dev)
    gamma, beta = _dev(inp["gamma"], dev), _dev(inp["beta"], dev)
    s1, s2 = _column_stats(ops, xd, inp["x"], C, dev)
    ybuf, y = _guarded(prows, C, dtype, dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    smean, sinv = torch.full((C,), N.NAN, device=dev), torch.full((C,), N.NAN, device=dev)
    ops.bn_pool_train_fwd(xd, y, B, H, W, s1, s2, gamma, beta, N.EPS, 0.1, rm, rv, smean, sinv, row.act)
    _finish(ops)
    fwd = N.bn_forward_ref(inp["x"], inp["gamma"], inp["beta"], row.act)
    want_y = N.first_max(fwd["y"].reshape(B, H, W, C))[0].reshape(prows, C)
    torch.testing.assert_close(_landed(ybuf, prows, "pooled y").double(), want_y, **_tol(dtype, stored=True))
    for got, key in ((smean, "mean"), (sinv, "invstd"), (rm, "running_mean"), (rv, "running_var")):
        torch.testing.assert_close(got.cpu().double(), fwd[key], **STAT_TOL)
    del fwd, want_y, ybuf, y
    mean, invstd = _dev(inp["mean"], dev), _dev(inp["invstd"], dev)
    fill = N.prefill(C, "ints")

    def run(form):
        w1, w2 = _accs(R * C, dev), _accs(R * C, dev)
        words = lambda: _words(w1, C, R, form + ": sum_dy") + _words(w2, C, R, form + ": sum_dy_xhat")
        if form == "reduce":
            ops.bn_pool_train_bwd_reduce(xd, dyd, B, H, W, mean, invstd, gamma, beta, row.act, w1, w2, replicas=R)
            _finish(ops)
            return dict(words=words())
        dgam, dbet = _dev(fill[0], dev), _dev(fill[1], dev)
        dxbuf, dx = _guarded(rows, C, dtype, dev)
        counter = torch.zeros(ops.BARRIER_WORDS, dtype=torch.int32, device=dev) if form == "counter" else None
        ops.bn_pool_train_bwd(xd, dyd, dx, B, H, W, mean, invstd, gamma, beta, row.act, w1, w2, dgam, dbet, replicas=R, counter=counter)
        _finish(ops)
        if counter is not None:
            assert (int(counter[0].item()) > 0) == (not long_row), "one-launch backward taken / not taken"
        return dict(words=words(), dx=_landed(dxbuf, rows, form + ": dx"), dgamma=dgam.cpu(), dbeta=dbet.cpu())

    ref = N.pool_bn_backward_ref(row, inp)
    pair = run("pair")
    _check_backward(row, pair, ref, fill, dtype, row.name + ", pair")
    assert run("reduce")["words"] == pair["words"], "kd6d_bn_pool_train_bwd_reduce leaves other words than the pair"
    one = run("counter")
    _check_backward(row, one, ref, fill, dtype, row.name + ", counter")
    if row.mode == "exact":
        _same_bits(pair, one, "counter against pair")


# ---- GroupNorm --------------------------------------------------------------------------------------------------------
def _stat_buffer(n_acc, dev, zero):
    """n_acc accumulators as fp32 -- NaN patterns unless zeroed -- and NaN guard floats behind them"""
    t = torch.full((n_acc * 4 + 16,), N.NAN, device=dev)
    if zero:
        t[:n_acc * 4] = 0
    return t


def _stat_words(t, n_acc, what):
    assert torch.isnan(t[n_acc * 4:]).all(), "%s: wrote behind the accumulators" % what
    return t[:n_acc * 4].view(torch.int64).cpu().reshape(-1, 2).tolist()


@pytest.mark.parametrize("row", N.GN_ROWS, ids=lambda r: r.name)
def test_groupnorm_exact(gpu_device, row, pin):
    ops, dev = _ops(), gpu_device
    dtype, xdt = N.TORCH_DTYPE[row.dtype], N.x_dtype(row.dtype, row.xf32)
    case = N.gn_case(row)
    ref, C, G, B, hw = case["ref"], row.C, row.G, row.batch, list(row.levels)
    rows, nkeys = B * sum(hw), len(hw) * B
    nstat = nkeys * G * 2
    xd, dzd = case["x"].to(xdt).to(dev), case["dz"].to(dtype).to(dev)
    gamma, beta = _dev(case["gamma"], dev), _dev(case["beta"], dev)
    tol = _tol(dtype, stored=True)

    # forward: flags 0 (clears the statistics itself), WS_ZEROED on a cleared workspace, STATS_READY on the host's words
    def fwd(flags, stats):
        ybuf, y = _guarded(rows, C, dtype, dev)
        ops.gn_relu_fwd(xd, y, hw, B, G, gamma, beta, N.EPS, stats, flags=flags)
        _finish(ops)
        return _landed(ybuf, rows, "y, flags %d" % flags), _stat_words(stats, nstat, "statistics, flags %d" % flags)

    y0, w0 = fwd(0, _stat_buffer(nstat, dev, zero=False))
    N.check_stat_words(w0, ref["stats"], "group statistics")
    torch.testing.assert_close(y0.double(), ref["y"], **tol)
    y1, w1 = fwd(ops.GN_WS_ZEROED, _stat_buffer(nstat, dev, zero=True))
    assert w1 == w0 and torch.equal(y1, y0), "KD6D_GN_WS_ZEROED"
    ready = _stat_buffer(nstat, dev, zero=True)
    host_words = N.words_of(ref["stats"])
    ready[:nstat * 4].view(torch.int64).copy_(torch.tensor(host_words, dtype=torch.int64).reshape(-1).to(dev))
    y2, w2 = fwd(ops.GN_STATS_READY, ready)
    assert w2 == host_words and torch.equal(y2, y0), "KD6D_GN_STATS_READY"
    if not row.backward:
        return
    stats = ready
    nws = ops.gn_bwd_workspace_floats(len(hw), B, G)
    gs = max(1.0, float(ref["dgamma"].abs().max()))

    def workspace(zero):
        t = torch.full((nws + 16,), N.NAN, device=dev)
        if zero:
            t[:nws] = 0
        return t

    def check(dxbuf, gsum, acc, off, stride, what, grads=True):
        dx = _landed(dxbuf, rows, what + ": dx")
        torch.testing.assert_close(dx.double(), ref["dx"], rtol=tol["rtol"], atol=3 * tol["atol"])
        assert torch.isnan(gsum[nws:]).all(), what + ": wrote behind the workspace"
        gw = gsum[:nstat * 4].view(torch.int64).cpu().reshape(-1, 2).tolist()
        N.check_stat_words(gw[0::2], ref["gsum"][0::2], what + ": group sums of dz * gamma", N.UNIT_GRAD)
        N.check_sums_close(gw[1::2], ref["gsum"][1::2], N.UNIT_GRAD, what + ": group sums of dz * gamma * xhat")
        if grads:
            a = acc.cpu()
            N.check_stat_words(N.planar_words(a, off + C, C, stride), [int(v) for v in ref["dbeta"].tolist()], what + ": dbeta", N.UNIT_GRAD)
            dgam = N.words_value(N.planar_words(a, off, C, stride), N.UNIT_GRAD)
            torch.testing.assert_close(dgam, ref["dgamma"], rtol=1e-3, atol=1e-3 * gs)
        return dx

    def single(onepass, flags, grads=True):
        pin("gn.onepass", onepass)
        gsum = workspace(bool(flags & ops.GN_WS_ZEROED))
        acc = ops.planar_acc(2 * C, dev)
        dxbuf, dx = _guarded(rows, C, dtype, dev)
        ops.gn_relu_bwd(xd, dzd, dx, hw, B, G, gamma, beta, stats, gsum, acc[:C] if grads else None, acc[C:2 * C] if grads else None,
                        2 * C if grads else 0, eps=N.EPS, flags=flags)
        _finish(ops)
        what = "gn.onepass %d, flags %d%s" % (onepass, flags, "" if grads else ", no parameter gradients")
        if not grads:
            assert not acc.any()
        return check(dxbuf, gsum, acc, 0, 2 * C, what, grads)

    one = single(1, 0)
    single(0, 0)
    assert torch.equal(single(1, ops.GN_WS_ZEROED), one), "KD6D_GN_WS_ZEROED, one pass"
    single(0, ops.GN_WS_ZEROED)
    assert torch.equal(single(1, 0, grads=False), one), "dgamma = dbeta = NULL"
    # the pair entry point: two identical items in one launch, one accumulator image for both
    pin("gn.onepass", 1)
    acc = ops.planar_acc(4 * C, dev)
    items, outs = [], []
    for k in range(2):
        gsum = workspace(False)
        dxbuf, dx = _guarded(rows, C, dtype, dev)
        items.append((xd, dzd, dx, gamma, beta, stats, gsum, acc[2 * k * C:(2 * k + 1) * C], acc[(2 * k + 1) * C:(2 * k + 2) * C]))
        outs.append((dxbuf, gsum))
    ops.gn_relu_bwd_pair(items, hw, B, G, 4 * C, eps=N.EPS)
    _finish(ops)
    for k, (dxbuf, gsum) in enumerate(outs):
        assert torch.equal(check(dxbuf, gsum, acc, 2 * k * C, 4 * C, "pair item %d" % k), one), "pair item %d against the single launch" % k


# ---- pool / upsample / eltwise / image --------------------------------------------------------------------------------
def _pool_run(ops, dev, dtype, fn, rows, C, what, fill=None):
    buf, out = _guarded(rows, C, dtype, dev, fill=fill)
    fn(out)
    torch.cuda.synchronize()
    return _landed(buf, rows, what)


@pytest.mark.parametrize("row", N.POOL_ROWS, ids=lambda r: r.name)
def test_pool_upsample_eltwise_exact(gpu_device, row):
    ops, dev = _ops(), gpu_device
    dtype = N.TORCH_DTYPE[row.dtype]
    B, H, W, C = row.B, row.H, row.W, row.C
    rows, prows = B * H * W, B * (H // 2) * (W // 2)
    inp = N.pool_inputs(B, H, W, C)
    put = lambda t: t.reshape(-1, C).to(dtype).to(dev)
    flat = lambda t: t.reshape(-1, C).float()
    x, dy, coarse, other = put(inp["x"]), put(inp["dy"]), put(inp["coarse"]), put(inp["other"])
    run = lambda fn, n, what, fill=None: _pool_run(ops, dev, dtype, fn, n, C, what, None if fill is None else fill.reshape(-1, C))
    best, arg = N.first_max(inp["x"])
    routed = N.route(arg, inp["dy"])
    assert torch.equal(run(lambda o: ops.maxpool2_fwd(x, o, B, H, W), prows, "maxpool2_fwd"), flat(best))
    assert torch.equal(run(lambda o: ops.maxpool2_bwd(x, dy, o, B, H, W), rows, "maxpool2_bwd"), flat(routed))
    assert torch.equal(run(lambda o: ops.maxpool2_bwd(x, dy, o, B, H, W, accumulate=True), rows, "maxpool2_bwd, accumulate", inp["dx0"]),
                       flat(inp["dx0"] + routed))
    assert torch.equal(run(lambda o: ops.upsample2_add(x, coarse, o, B, H, W), rows, "upsample2_add"),
                       flat(inp["x"] + N.upsample_ref(inp["coarse"])))
    assert torch.equal(run(lambda o: ops.sumpool2(x, o, B, H, W), prows, "sumpool2"), flat(N.sumpool_ref(inp["x"])))
    assert torch.equal(run(lambda o: ops.sumpool2(x, o, B, H, W, accumulate=True), prows, "sumpool2, accumulate", inp["dc0"]),
                       flat(inp["dc0"] + N.sumpool_ref(inp["x"])))
    assert torch.equal(run(lambda o: ops.eltwise(ops.ELT_RELU, x, None, o), rows, "ELT_RELU"), flat(inp["x"].clamp_min(0)))
    assert torch.equal(run(lambda o: ops.eltwise(ops.ELT_RELU_BWD, x, other, o), rows, "ELT_RELU_BWD"),
                       flat(torch.where(inp["x"] > 0, inp["other"], torch.zeros_like(inp["other"]))))
    assert torch.equal(run(lambda o: ops.eltwise(ops.ELT_ADD, x, other, o), rows, "ELT_ADD"), flat(inp["x"] + inp["other"]))


def test_maxpool_forward_floors_odd_sizes(gpu_device):
    ops, dev, row = _ops(), gpu_device, N.POOL_ODD
    dtype = N.TORCH_DTYPE[row.dtype]
    B, H, W, C = row.B, row.H, row.W, row.C
    x = N.pool_inputs(B, H, W, C)["x"]
    prows = B * (H // 2) * (W // 2)
    xd = x.reshape(-1, C).to(dtype).to(dev)
    got = _pool_run(ops, dev, dtype, lambda o: ops.maxpool2_fwd(xd, o, B, H, W), prows, C, "maxpool2_fwd, odd H and W")
    assert torch.equal(got, N.first_max(x)[0].reshape(prows, C).float())


@pytest.mark.parametrize("row", N.IMAGE_ROWS, ids=lambda r: r.name)
def test_image_to_nhwc_exact(gpu_device, row):
    ops, dev = _ops(), gpu_device
    dtype = N.TORCH_DTYPE[row.dtype]
    g = torch.Generator().manual_seed(row.Cimg * 100 + row.Cpad)
    img = torch.randint(-4, 5, (row.B, row.Cimg, row.H, row.W), generator=g).float()
    n = row.B * row.H * row.W
    imgd = img.to(dev)
    got = _pool_run(ops, dev, dtype, lambda o: ops.image_to_nhwc(imgd, dtype, cpad=row.Cpad, out=o), n, row.Cpad, "image_to_nhwc")
    assert torch.equal(got, N.image_ref(img, row.Cpad))
