"""Cases, fp64 reference and tolerances of the kernel distances (csrc/kernel_loss.hip; --gtype gaussian | laplacian |
energy under --kd_kernel_losses).

The reference is the three-term expression of geomloss 0.2.4 kernel_samples.py (tensorized path) in fp64 torch, under
autograd:

    L = 1/2 sum_ij a_i a_j k(x_i,x_j) + 1/2 sum_ij b_i b_j k(y_i,y_j) - sum_ij a_i b_j k(x_i,y_j)
    gaussian k = exp(-r2 / (2 blur^2));  laplacian k = exp(-sqrt(clamp_min(r2 / blur^2, 1e-8)));
    energy k = -sqrt(clamp_min(r2, 1e-8)),   r2 from direct differences, the weights used as given.

`closed_form` restates value and gradients without autograd (what the kernels evaluate); in fp64 it must agree with the
reference to 1e-12, in fp32 its deviation from fp64 is the yardstick of the GPU tolerances (loss_cases.FACTOR / FLOOR
rule, profiles/kernel_loss_tolerances.md).

Inputs are drawn in fp32 and upcast, so both sides see the same numbers: points uniform in [0.3, 0.6]^D, weights in
[0.05, 0.95].  Every builder plants exact duplicates (two student points, a student point on a teacher point, two
teacher points: k at the clamp, no gradient), a zero weight, and a NEAR pair -- a student point 5e-4 beside a teacher
point in every coordinate.  The near pair keeps the largest gradient of a case an ordinary number: with blur = 0.001
and a handful of points 0.1 apart, every other pair's laplacian kernel is an fp32 denormal (exp(-100)) and the
"largest magnitude of the reference" would be one.  Every builder asserts that no pair has its clamped variable (r2 for
energy, r2 / blur^2 for laplacian) strictly between 0 and 1e-7, which keeps fp32 and fp64 on the same side of the 1e-8
clamp; the seeds below are ones for which that holds (`python tests/kernel_loss_cases.py --seeds` searches them).
"""
import functools

import torch

F64 = torch.float64
KINDS = ("gaussian", "laplacian", "energy")
OUTPUTS = ("loss", "grad_alpha", "grad_x")
BLURS = (0.05, 0.001)
CLAMP = 1e-8
NEAR = 5e-4
CANARY = 7.25

# (N, M) of the small kernel: one lane, a float4 tail, the second row of a lane (64 | 65), a full set
SMALL_SIZES = ((1, 1), (3, 5), (16, 17), (63, 64), (64, 65), (65, 17), (128, 128))
N_PROBLEMS = 6
# the dense kernel's tiles (csrc/kernel_loss.hip: kTile columns per LDS tile, kRows rows per workgroup)
TILE, ROWS = 128, 64
DENSE_DIMS = (2, 4, 8, 16)
DENSE_SIZES = ((1, 1), (TILE - 1, TILE + 1), (2 * TILE + 3, 5), (300, 280), (ROWS + 1, 3))
DENSE_BLUR = 0.05
CROSS_SIZE = (100, 90)                  # D = 2: the dense kernel against the small one
# (B, N, M, D) of the SamplesLoss test: the shapes of test_losses_gpu.py::test_samples_loss_small_sets_vs_oracle, one dense
SAMPLES_SHAPES = ((8, 10, 9, 2), (8, 10, 10, 2), (3, 7, 12, 2), (1, 40, 33, 2), (2, 300, 280, 16))

# seeds for which the builders' clamp condition holds
SMALL_SEEDS = {(1, 1): 0, (3, 5): 0, (16, 17): 0, (63, 64): 1, (64, 65): 1, (65, 17): 1, (128, 128): 414}
DENSE_SEEDS = {(300, 280, 2): 1}                     # (N, M, D) -> seed; default 0
SAMPLES_SEEDS = {}                      # (B, N, M, D) -> seed; default 0


# --------------------------------------------------------------------------------------------------------------------
# the loss
# --------------------------------------------------------------------------------------------------------------------
def _kernel(u, v, kind, blur):
    """k(u_i, v_j) for u (B,N,D), v (B,M,D) -> (B,N,M), differentiable."""
    d = u[:, :, None, :] - v[:, None, :, :]
    r2 = (d * d).sum(-1)
    if kind == "gaussian":
        return torch.exp(-r2 / (2.0 * blur ** 2))
    if kind == "laplacian":
        return torch.exp(-torch.sqrt(torch.clamp_min(r2 / blur ** 2, CLAMP)))
    if kind == "energy":
        return -torch.sqrt(torch.clamp_min(r2, CLAMP))
    raise ValueError(kind)


def kernel_loss_torch(alpha, x, beta, y, kind, blur):
    """(B,) losses of alpha (B,N), x (B,N,D), beta (B,M), y (B,M,D): the three-term expression, in the inputs' dtype."""
    kxx, kyy, kxy = _kernel(x, x, kind, blur), _kernel(y, y, kind, blur), _kernel(x, y, kind, blur)
    return (0.5 * (alpha[:, :, None] * alpha[:, None, :] * kxx).sum((1, 2))
            + 0.5 * (beta[:, :, None] * beta[:, None, :] * kyy).sum((1, 2))
            - (alpha[:, :, None] * beta[:, None, :] * kxy).sum((1, 2)))


def ot_fn(kind):
    """The loss with the signature of the oracle's OT hook (oracle.kd_step_ref.kd_pose_loss(ot_fn=...))."""
    def fn(al, xs, be, ys, blur, scaling, reach):
        return kernel_loss_torch(al, xs, be, ys, kind, blur)
    return fn


def reference(alpha, x, beta, y, kind, blur):
    """fp64 autograd of the three-term expression -> dict(loss (B,), grad_alpha (B,N), grad_x (B,N,D))."""
    a = alpha.detach().to(F64).requires_grad_(True)
    xx = x.detach().to(F64).requires_grad_(True)
    loss = kernel_loss_torch(a, xx, beta.detach().to(F64), y.detach().to(F64), kind, blur)
    ga, gx = torch.autograd.grad(loss.sum(), (a, xx))
    return dict(loss=loss.detach(), grad_alpha=ga, grad_x=gx)


def _pair_terms(u, v, kind, blur):
    """k, the factor c of grad_1 k(u,v) = c (u - v), and the differences, in u's dtype."""
    d = u[:, :, None, :] - v[:, None, :, :]
    r2 = (d * d).sum(-1)
    if kind == "gaussian":
        k = torch.exp(-r2 / (2.0 * blur ** 2))
        c = -k / blur ** 2
    elif kind == "laplacian":
        s = r2 / blur ** 2
        q = torch.sqrt(torch.clamp_min(s, CLAMP))
        k = torch.exp(-q)
        c = torch.where(s >= CLAMP, -k / (blur ** 2 * q), torch.zeros_like(k))
    else:
        q = torch.sqrt(torch.clamp_min(r2, CLAMP))
        k = -q
        c = torch.where(r2 >= CLAMP, -1.0 / q, torch.zeros_like(q))
    return k, c, d


def closed_form(alpha, x, beta, y, kind, blur, dt=torch.float32):
    """Value and gradients in closed form, every operation in `dt`: row sums over the columns, then over the rows."""
    a, x, b, y = (t.detach().to(dt) for t in (alpha, x, beta, y))
    kxx, cxx, dxx = _pair_terms(x, x, kind, blur)
    kxy, cxy, dxy = _pair_terms(x, y, kind, blur)
    kyy = _pair_terms(y, y, kind, blur)[0]
    sxx, sxy, syy = (kxx * a[:, None, :]).sum(-1), (kxy * b[:, None, :]).sum(-1), (kyy * b[:, None, :]).sum(-1)
    loss = (a * (0.5 * sxx - sxy)).sum(-1) + 0.5 * (b * syy).sum(-1)
    gx = a[..., None] * (((cxx * a[:, None, :])[..., None] * dxx).sum(2) - ((cxy * b[:, None, :])[..., None] * dxy).sum(2))
    return dict(loss=loss, grad_alpha=sxx - sxy, grad_x=gx)


# --------------------------------------------------------------------------------------------------------------------
# builders
# --------------------------------------------------------------------------------------------------------------------
def clamped_variables_ok(x, y, blurs=BLURS):
    """No pair of x (B,N,D) / y (B,M,D) has r2 (energy) or r2 / blur^2 (laplacian) strictly inside (0, 1e-7)."""
    x, y = x.to(F64), y.to(F64)
    for u, v in ((x, x), (x, y), (y, y)):
        if u.shape[1] == 0 or v.shape[1] == 0:
            continue
        d = u[:, :, None, :] - v[:, None, :, :]
        r2 = (d * d).sum(-1)
        for scale in (1.0,) + tuple(1.0 / b ** 2 for b in blurs):
            s = r2 * scale
            if bool(((s > 0) & (s < 1e-7)).any()):
                return False
    return True


def _draw(g, *shape):
    return 0.3 + 0.3 * torch.rand(*shape, generator=g)


def _weights(g, *shape):
    return 0.05 + 0.9 * torch.rand(*shape, generator=g)


def _plant(x, a, y):
    """x (N,K,D), a (N,K), y (M,K,D) of one problem, K independent point sets side by side: duplicates, a zero weight
    and a near pair, as far as the sizes allow."""
    N, M = x.shape[0], y.shape[0]
    if N == 0 or M == 0:
        return
    if N == 1:
        x[0] = y[0] + NEAR                    # the one pair there is: near, so that the case has a gradient
        return
    x[0] = y[0] + NEAR                        # near pair
    x[N - 1] = y[M - 1]                       # a student point on a teacher point
    if N >= 3:
        x[1] = x[N - 1]                       # two student points coincide (and both lie on the teacher point)
    if N >= 4:
        a[2] = 0.0                            # an ordinary value
    if M >= 3:
        y[1] = y[M - 1]                       # two teacher points coincide


def point_sets(B, N, M, D, seed):
    """alpha (B,N), x (B,N,D), beta (B,M), y (B,M,D), fp32."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * N + M + D)
    x, a, y, b = _draw(g, B, N, D), _weights(g, B, N), _draw(g, B, M, D), _weights(g, B, M)
    xv, av, yv = x.permute(1, 0, 2), a.t(), y.permute(1, 0, 2)          # views: the plants land in x, a, y
    _plant(xv, av, yv)
    assert clamped_variables_ok(x, y), "point_sets(%d,%d,%d,%d, seed %d): a pair inside the clamp's margin" % (B, N, M, D, seed)
    return a, x, b, y


def dense_case(N, M, D):
    a, x, b, y = point_sets(1, N, M, D, DENSE_SEEDS.get((N, M, D), 0))
    return a[0].contiguous(), x[0].contiguous(), b[0].contiguous(), y[0].contiguous()


def samples_case(B, N, M, D):
    return point_sets(B, N, M, D, SAMPLES_SEEDS.get((B, N, M, D), 0))


def small_launch(sizes, seed):
    """One launch of the small kernel: problem p has sizes[p] = (N, M) points per keypoint; the segments lie in shuffled
    order with gaps of 1..3 rows; the gaps hold CANARY.  -> dict of fp32 / int32 CPU tensors: the flat arrays xs
    (R,8,2), alpha (R,8), s_start, s_cnt, yt, beta, t_start, t_cnt, and the per-problem views' sources x[p] (N,8,2),
    a[p] (N,8), y[p], b[p]."""
    g = torch.Generator().manual_seed(seed)
    P = len(sizes)
    xs_p, a_p, ys_p, b_p = [], [], [], []
    for p, (N, M) in enumerate(sizes):
        x, a, y, b = _draw(g, N, 8, 2), _weights(g, N, 8), _draw(g, M, 8, 2), _weights(g, M, 8)
        if p < 3 and N <= 128 and M <= 128:          # three planted problems, the others plain
            _plant(x, a, y)
        if N and M:
            assert clamped_variables_ok(x.permute(1, 0, 2), y.permute(1, 0, 2)), "small_launch(%s, seed %d): problem %d" % (sizes, seed, p)
        xs_p.append(x); a_p.append(a); ys_p.append(y); b_p.append(b)

    def lay(parts_pts, parts_w):
        order = torch.randperm(P, generator=g).tolist()
        gaps = torch.randint(1, 4, (P + 1,), generator=g).tolist()
        start, row = [0] * P, 0
        for i, p in enumerate(order):
            row += gaps[i]
            start[p] = row
            row += parts_pts[p].shape[0]
        R = row + gaps[P]
        pts, w = torch.full((R, 8, 2), CANARY), torch.full((R, 8), CANARY)
        seg = torch.zeros(R, dtype=torch.bool)
        for p in range(P):
            n = parts_pts[p].shape[0]
            pts[start[p]:start[p] + n], w[start[p]:start[p] + n] = parts_pts[p], parts_w[p]
            seg[start[p]:start[p] + n] = True
        return pts, w, torch.tensor(start, dtype=torch.int32), torch.tensor([q.shape[0] for q in parts_pts], dtype=torch.int32), seg

    xs, alpha, s_start, s_cnt, s_seg = lay(xs_p, a_p)
    yt, beta, t_start, t_cnt, _ = lay(ys_p, b_p)
    return dict(sizes=tuple(sizes), xs=xs, alpha=alpha, s_start=s_start, s_cnt=s_cnt, s_seg=s_seg, yt=yt, beta=beta,
                t_start=t_start, t_cnt=t_cnt, x=xs_p, a=a_p, y=ys_p, b=b_p)


def launch_valid(N, M, cap=128):
    return 0 if (N <= 0 or M <= 0) else (-1 if (N > cap or M > cap) else 1)


def small_results(L, fn, dt=F64):
    """fn(alpha (8,N), x (8,N,2), beta (8,M), y (8,M,2)) -> dict(loss, grad_alpha, grad_x), per valid problem, assembled
    in the launch's layout: loss_kp (P,8), grad_alpha (R,8), grad_xs (R,8,2) -- zero wherever the kernel does not write."""
    P, R = len(L["sizes"]), L["xs"].shape[0]
    loss_kp, ga, gx = torch.zeros(P, 8, dtype=dt), torch.zeros(R, 8, dtype=dt), torch.zeros(R, 8, 2, dtype=dt)
    written = torch.zeros(R, dtype=torch.bool)
    for p, (N, M) in enumerate(L["sizes"]):
        if launch_valid(N, M) != 1:
            continue
        r = fn(L["a"][p].t(), L["x"][p].permute(1, 0, 2), L["b"][p].t(), L["y"][p].permute(1, 0, 2))
        s0 = int(L["s_start"][p])
        loss_kp[p] = r["loss"]
        ga[s0:s0 + N] = r["grad_alpha"].t()
        gx[s0:s0 + N] = r["grad_x"].permute(1, 0, 2)
        written[s0:s0 + N] = True
    return dict(loss=loss_kp, grad_alpha=ga, grad_x=gx, written=written)


@functools.lru_cache(maxsize=None)
def small_case(N, M):
    """The launch of six (N, M) problems every test of that size shares."""
    return small_launch([(N, M)] * N_PROBLEMS, SMALL_SEEDS[(N, M)])


@functools.lru_cache(maxsize=None)
def small_reference(N, M, kind, blur):
    L = small_case(N, M)
    return small_results(L, lambda a, x, b, y: reference(a, x, b, y, kind, blur))


@functools.lru_cache(maxsize=None)
def dense_reference(N, M, D, kind, blur=DENSE_BLUR):
    a, x, b, y = dense_case(N, M, D)
    r = reference(a[None], x[None], b[None], y[None], kind, blur)
    return dict(loss=r["loss"], grad_alpha=r["grad_alpha"][0], grad_x=r["grad_x"][0])


# --------------------------------------------------------------------------------------------------------------------
# tolerances: fp32-vs-fp64 deviation of the restatement itself (loss_cases.FACTOR / FLOOR rule)
# --------------------------------------------------------------------------------------------------------------------
FACTOR = 8.0
FLOOR = 4.0 * 2.0 ** -23          # 4 fp32 ulps of the output's largest magnitude


def _rel_dev(a32, a64):
    a64 = a64.double()
    m = float(a64.abs().max()) if a64.numel() else 0.0
    return 0.0 if m == 0.0 else float((a32.double() - a64).abs().max()) / m


def measure_deviations():
    """{"kind.output": max over the seeded cases -- every small launch at both blurs, every dense case, the SamplesLoss
    shapes -- of max|fp32 - fp64| / max|fp64| of the closed form}, both sides on the CPU."""
    dev = {}

    def note(kind, r32, r64):
        for o in OUTPUTS:
            k = "%s.%s" % (kind, o)
            dev[k] = max(dev.get(k, 0.0), _rel_dev(r32[o], r64[o]))

    for kind in KINDS:
        for N, M in SMALL_SIZES:
            L = small_case(N, M)
            for blur in BLURS:
                note(kind, small_results(L, lambda a, x, b, y: closed_form(a, x, b, y, kind, blur), torch.float32),
                     small_results(L, lambda a, x, b, y: closed_form(a, x, b, y, kind, blur, F64)))
        for D in DENSE_DIMS:
            for N, M in DENSE_SIZES + (CROSS_SIZE,):
                a, x, b, y = dense_case(N, M, D)
                note(kind, closed_form(a[None], x[None], b[None], y[None], kind, DENSE_BLUR),
                     closed_form(a[None], x[None], b[None], y[None], kind, DENSE_BLUR, F64))
        for shape in SAMPLES_SHAPES:
            a, x, b, y = samples_case(*shape)
            note(kind, closed_form(a, x, b, y, kind, DENSE_BLUR), closed_form(a, x, b, y, kind, DENSE_BLUR, F64))
    return dev


# profiles/kernel_loss_tolerances.md: what measure_deviations() returned when the cases were fixed (the host test
# checks that a fresh measurement does not exceed it)
RECORDED_DEV = {
    "gaussian.loss": 7.201e-05, "gaussian.grad_alpha": 1.434e-06, "gaussian.grad_x": 2.917e-07,
    "laplacian.loss": 1.750e-06, "laplacian.grad_alpha": 9.519e-07, "laplacian.grad_x": 3.985e-07,
    "energy.loss": 5.326e-04, "energy.grad_alpha": 4.891e-06, "energy.grad_x": 1.547e-06,
}


def bound(kind, output):
    """Relative-to-largest-magnitude bound of GPU output `output` of kernel `kind` (profiles/kernel_loss_tolerances.md)."""
    return max(FACTOR * RECORDED_DEV["%s.%s" % (kind, output)], FLOOR)


def assert_within(got, ref, kind, output, what=""):
    """max|got - ref| <= bound(kind, output) * max|ref| (fp64 comparison); prints the figure first."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s %s %s: non-finite output" % (kind, output, what)
    m = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    bd = bound(kind, output)
    print("  %-9s %-10s %-36s max|err| %.3e  max|ref| %.3e  rel %.3e  bound %.3e" % (kind, output, what, err, m, err / max(m, 1e-300), bd))
    assert err <= bd * m, "%s %s %s: max|err| %.3e > %.3e x %.3e" % (kind, output, what, err, bd, m)


def _find_seed(build, limit=20000):
    for seed in range(limit):
        try:
            build(seed)
            return seed
        except AssertionError:
            continue
    raise RuntimeError("no seed below %d" % limit)


if __name__ == "__main__":
    import sys
    if "--seeds" in sys.argv:
        print("SMALL_SEEDS = %r" % {s: _find_seed(lambda seed, s=s: small_launch([s] * N_PROBLEMS, seed)) for s in SMALL_SIZES})
        print("DENSE_SEEDS = %r" % {k: v for k, v in (((N, M, D), _find_seed(lambda seed, N=N, M=M, D=D: point_sets(1, N, M, D, seed)))
                                                      for D in DENSE_DIMS for N, M in DENSE_SIZES + (CROSS_SIZE,)) if v})
        print("SAMPLES_SEEDS = %r" % {k: v for k, v in ((s, _find_seed(lambda seed, s=s: point_sets(*s, seed))) for s in SAMPLES_SHAPES) if v})
        sys.exit(0)
    d = measure_deviations()
    print("| kernel.output | fp32-vs-fp64 deviation of the restatement | x %g | bound used (relative to max magnitude) |" % FACTOR)
    print("|---|---|---|---|")
    for k in sorted(d):
        print("| %s | %.3e | %.3e | %.3e |" % (k, d[k], FACTOR * d[k], max(FACTOR * d[k], FLOOR)))
    print("RECORDED_DEV = {%s}" % ", ".join('"%s": %.3e' % (k, d[k]) for k in sorted(d)))
