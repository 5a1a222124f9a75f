"""GPU: kd6d_bn_pool_bwd_wgrad -- the apply pass of the pooled BatchNorm backward and the weight gradient of the convolution
in front of it as one launch (csrc/stem_bwd.hip) -- against the library's own separate path on identical inputs:
ops.bn_pool_train_bwd (reduce + apply, the gradient of the convolution output stored as bf16) followed by the weight
gradient of that stored tensor.

The fused launch forms the same bf16 gradient values in registers, so both weight gradients are fp32 sums of the SAME
products in another association.  Each is held against the sum formed in float64 on the CPU from the separate path's
stored gradient, within the fp32 summation bound n * 2^-24 * sum|terms| (n = terms of the sum), computed here per
element: no free constant.  dgamma / dbeta come from the same exact totals and must agree bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ACT_LEAKY = 1
# (B, H, W, Cout, cu_budget)
CASES = [
    (1, 4, 4, 8, 0),            # every pixel has out-of-image taps
    (2, 8, 8, 8, 0),
    (3, 20, 12, 16, 0),         # width no multiple of the vector width, tiles straddle nothing but the pad columns
    (1, 6, 128, 8, 0),          # 4-row tiles on a 6-row image: the last tile's lower half lies below the image
    (2, 64, 64, 8, 0),          # several workgroups per image
    (4, 128, 128, 8, 4),        # 128 tiles on 22 workgroups: every workgroup walks several tiles
]


def _ops():
    from kd6d import ops
    return ops


def _accs(n, dev):
    return torch.zeros(n * 4, device=dev)


def _inputs(B, H, W, C):
    """x: 3 real + 5 zero channels; raw with constant 2x2-aligned patches (exact ties) and a region whose four
    pre-activations are all negative; dz with all-zero pooled rows."""
    g = torch.Generator().manual_seed(B * 100003 + H * 1009 + W * 31 + C)
    x = torch.zeros(B, H, W, 8)
    x[..., :3] = torch.randn(B, H, W, 3, generator=g)
    raw = torch.randn(B, H, W, C, generator=g) * 2 + 0.5
    raw[:, 0:2, 0:2, :] = 1.25                          # a whole window equal: the first maximum wins
    raw[:, 2:4, 0:2, :] = raw[:, 2:3, 0:1, :]           # equal per channel
    raw[:, H // 2:, W // 2:, :] = -6.0 - torch.rand(B, H - H // 2, W - W // 2, C, generator=g)      # all four negative
    if H >= 8:
        raw[:, H - 2:, W - 2:, :] = -7.0                # ... and tied
    dz = torch.randn(B, H // 2, W // 2, C, generator=g)
    dz[:, ::3] = 0.0                                    # all-zero rows of the pooled gradient
    return (x.reshape(-1, 8).to(torch.bfloat16), raw.reshape(-1, C).contiguous(), dz.reshape(-1, C).to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _run(B, H, W, C, budget):
    """Both paths once per case; everything the tests read, on the CPU."""
    ops = _ops()
    dev = torch.device("cuda:0")
    x, raw, dz = (t.to(dev) for t in _inputs(B, H, W, C))
    rows = B * H * W
    g = torch.Generator().manual_seed(7 + C)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = (torch.randn(C, generator=g) * 0.1).to(dev)
    s1, s2 = _accs(C, dev), _accs(C, dev)
    ops.colstats(raw, s1, s2)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    z = torch.empty(rows // 4, C, dtype=torch.bfloat16, device=dev)
    ops.bn_pool_train_fwd(raw, z, B, H, W, s1, s2, gamma, beta, 1e-5, 0.1, torch.zeros(C, device=dev),
                          torch.ones(C, device=dev), mean, invstd, ACT_LEAKY)
    geom = ops.Geom(B, 8, C, 3, 1, 1, [(H, W)])
    R = 1 if rows < 1000 else 8

    # the separate path: reduce + apply (no barrier counter: never the one-launch form), then the weight gradient
    w1, w2 = _accs(R * C, dev), _accs(R * C, dev)
    u_dg, u_db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    draw = torch.empty(rows, C, dtype=torch.bfloat16, device=dev)
    ops.bn_pool_train_bwd(raw, dz, draw, B, H, W, mean, invstd, gamma, beta, ACT_LEAKY, w1, w2, u_dg, u_db, replicas=R)
    u_dw, _ = ops.conv2d_wgrad_f32(geom, x, draw)

    def fused():
        parts = ops.bn_pool_bwd_wgrad_parts(geom, torch.bfloat16, budget)
        assert parts >= 1, "the fused launch must take this geometry"
        w1, w2 = _accs(R * C, dev), _accs(R * C, dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        slab = torch.full((parts, C * 72), float("nan"), device=dev)      # every element of every part is written
        ops.bn_pool_train_bwd_reduce(raw, dz, B, H, W, mean, invstd, gamma, beta, ACT_LEAKY, w1, w2, replicas=R)
        ops.bn_pool_bwd_wgrad(geom, x, raw, dz, mean, invstd, gamma, beta, ACT_LEAKY, w1, w2, dg, db, slab, replicas=R,
                              cu_budget=budget)
        dw = slab[0].clone()
        for k in range(1, parts):              # in part order, in fp32
            dw += slab[k]
        torch.cuda.synchronize()
        return parts, slab.cpu(), dw.cpu(), dg.cpu(), db.cpu()

    f1, f2 = fused(), fused()
    # float64 sums of the separate path's stored gradient, and sum|terms|, per element
    d = draw.cpu().double().reshape(B, H, W, C)
    xp = torch.zeros(B, H + 2, W + 2, 8, dtype=torch.float64)
    xp[:, 1:-1, 1:-1] = x.cpu().double().reshape(B, H, W, 8)
    ref = torch.zeros(C, 3, 3, 8, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, ky:ky + H, kx:kx + W]
            ref[:, ky, kx] = torch.einsum("bhwn,bhwc->nc", d, patch)
            mag[:, ky, kx] = torch.einsum("bhwn,bhwc->nc", d.abs(), patch.abs())
    bound = rows * 2.0 ** -24 * mag
    return dict(f1=f1, f2=f2, u_dw=u_dw.cpu(), u_dg=u_dg.cpu(), u_db=u_db.cpu(), ref=ref.reshape(-1), bound=bound.reshape(-1))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_%dx%d_c%d_cu%d" % c)
def test_param_gradients_bitwise_equal_to_the_separate_path(gpu_device, case):
    r = _run(*case)
    for f in (r["f1"], r["f2"]):
        assert torch.equal(f[3], r["u_dg"]) and torch.equal(f[4], r["u_db"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_%dx%d_c%d_cu%d" % c)
def test_two_executions_bitwise_equal(gpu_device, case):
    r = _run(*case)
    assert r["f1"][0] == r["f2"][0]
    assert not torch.isnan(r["f1"][1]).any(), "a part of the slab was left unwritten"
    assert torch.equal(r["f1"][1], r["f2"][1]) and torch.equal(r["f1"][2], r["f2"][2])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_%dx%d_c%d_cu%d" % c)
def test_weight_gradient_within_fp32_summation_bound(gpu_device, case):
    r = _run(*case)
    for name, dw in (("separate", r["u_dw"]), ("fused", r["f1"][2])):
        err = (dw.double() - r["ref"]).abs()
        worst = int(torch.argmax(err / r["bound"].clamp_min(1e-300)))
        print("%s: max |err| %.3e; closest to its bound: err %.3e of %.3e" % (name, float(err.max()), float(err[worst]),
                                                                             float(r["bound"][worst])))
        assert bool((err <= r["bound"]).all()), (name, worst, float(err[worst]), float(r["bound"][worst]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "b%d_%dx%d_c%d_cu%d" % c)
def test_zero_padded_input_channels_get_exactly_zero(gpu_device, case):
    r = _run(*case)
    C = case[3]
    assert bool((r["f1"][1].reshape(-1, C, 9, 8)[..., 3:] == 0).all())
    assert bool((r["f1"][2].reshape(C, 9, 8)[..., 3:] == 0).all())
    assert float(r["f1"][2].reshape(C, 9, 8)[..., :3].abs().max()) > 0


def test_workgroups_loop_when_tiles_exceed_the_grid(gpu_device):
    """The last case runs on fewer workgroups than tiles (the pixel split of a budget of 4 CUs), the same geometry on the
    whole device does not: both are the same sum up to the association."""
    ops = _ops()
    B, H, W, C, budget = CASES[-1]
    geom = ops.Geom(B, 8, C, 3, 1, 1, [(H, W)])
    few, all_ = ops.bn_pool_bwd_wgrad_parts(geom, torch.bfloat16, budget), ops.bn_pool_bwd_wgrad_parts(geom, torch.bfloat16, 0)
    tiles = B * H // 4                       # 4-row tiles at this width (conv_plan.h, stem_bwd_rule)
    assert few < tiles and all_ == tiles
    full = _run(B, H, W, C, 0)
    r = _run(B, H, W, C, budget)
    assert bool(((full["f1"][2].double() - r["ref"]).abs() <= r["bound"]).all())


# Where a workgroup's tiles are exactly one pixel split of the transposing weight-gradient kernel, in whole 32-pixel steps
# (tests/test_stem_plan_host.py states the condition), the fused launch accumulates the same products in the same order:
# the slab is the separate path's slab bit for bit.  Two small geometries and the stem of the benchmark step.
ALIGNED = [(8, 2, 32, 8), (4, 4, 32, 16), (16, 256, 256, 8)]


@pytest.mark.parametrize("case", ALIGNED, ids=lambda c: "b%d_%dx%d_c%d" % c)
def test_slab_bitwise_equal_to_the_separate_path_where_the_splits_coincide(gpu_device, case):
    ops = _ops()
    dev = gpu_device
    B, H, W, C = case
    x, raw, _ = (t.to(dev) for t in _inputs(B, H, W, C))
    rows = B * H * W
    dz = torch.randn(rows // 4, C, generator=torch.Generator().manual_seed(rows + C))
    dz[::3] = 0.0                               # (pooled pixels, not pooled rows: the 2-row image has one pooled row)
    dz = dz.to(torch.bfloat16).to(dev)
    gamma = torch.linspace(0.5, 1.5, C, device=dev)
    beta = torch.linspace(-0.1, 0.1, C, device=dev)
    s1, s2 = _accs(C, dev), _accs(C, dev)
    ops.colstats(raw, s1, s2)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    z = torch.empty(rows // 4, C, dtype=torch.bfloat16, device=dev)
    ops.bn_pool_train_fwd(raw, z, B, H, W, s1, s2, gamma, beta, 1e-5, 0.1, torch.zeros(C, device=dev),
                          torch.ones(C, device=dev), mean, invstd, ACT_LEAKY)
    geom = ops.Geom(B, 8, C, 3, 1, 1, [(H, W)])
    parts = ops.bn_pool_bwd_wgrad_parts(geom, torch.bfloat16)
    assert parts == ops.conv2d_wgrad_parts(geom, torch.bfloat16) and parts > 1
    R = 8
    w1, w2 = _accs(R * C, dev), _accs(R * C, dev)
    draw = torch.empty(rows, C, dtype=torch.bfloat16, device=dev)
    ops.bn_pool_train_bwd(raw, dz, draw, B, H, W, mean, invstd, gamma, beta, ACT_LEAKY, w1, w2, None, None, replicas=R)
    u_slab = torch.full((parts, C * 72), float("nan"), device=dev)
    ops.conv2d_wgrad(geom, x, draw, u_slab)
    w1, w2 = _accs(R * C, dev), _accs(R * C, dev)
    f_slab = torch.full((parts, C * 72), float("nan"), device=dev)
    ops.bn_pool_train_bwd_reduce(raw, dz, B, H, W, mean, invstd, gamma, beta, ACT_LEAKY, w1, w2, replicas=R)
    ops.bn_pool_bwd_wgrad(geom, x, raw, dz, mean, invstd, gamma, beta, ACT_LEAKY, w1, w2, None, None, f_slab, replicas=R)
    torch.cuda.synchronize()
    assert not torch.isnan(u_slab).any() and float(u_slab.abs().max()) > 0
    assert torch.equal(f_slab, u_slab)
