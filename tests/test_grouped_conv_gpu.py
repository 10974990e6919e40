"""Grouped convolution (grouped_kernels.hip), per element against float64
``F.conv2d`` / ``F.conv_transpose2d(groups=G)`` on the same bf16 inputs, with
the helpers and bound forms of test_tail_kernels_gpu.py.  Depths D read off
the kernels (CS = KS = max(16, Cg)): convout / dx — one wave runs
ceil(R·R·CS/32) MFMA steps of 32 products into one f32 accumulator, zeros
included: pow2(R·R·CS); dw — a split accumulates its ≤ M rows, the reduce
adds the ≤ 64 splits (one per 1024 rows) in order, then one add onto dW:
pow2(M + splits + 1)."""
import pytest
import torch
import torch.nn.functional as F

from test_tail_kernels_gpu import _C, _check, _gen, _spike, _pow2, _cl, U, E
from test_tail_kernels_gpu import det  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CASES = [  # (N, C, G, H, W, R, stride, pad)
    (1, 16, 4, 5, 5, 3, 1, 1),     # Cg=4, one slab, 8-run spans two groups
    (3, 64, 8, 9, 7, 3, 2, 1),     # Cg=8, four slabs, stride 2, odd H != W
    (2, 32, 2, 8, 8, 3, 1, 1),     # Cg=16, M=128: two tiles per wave
    (3, 64, 2, 9, 7, 3, 1, 1),     # Cg=32, M=189: three tiles, ragged
    (2, 32, 8, 1, 1, 3, 1, 1),     # 1x1 map: only the centre tap is live
    (2, 48, 6, 7, 5, 1, 1, 0),     # 1x1 filter, three slabs
    (4, 16, 4, 32, 32, 3, 1, 1),   # M=4096: wgrad msplit > 1
]
BN_CASES = [CASES[0], CASES[1], CASES[3]]
MOM, EPS = 0.1, 1e-5
ids = lambda c: "x".join(map(str, c))  # noqa: E731


def _geom(case):
    N, C, G, H, W, R, s, p = case
    Ho, Wo = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    return C // G, Ho, Wo, N * Ho * Wo, _pow2(R * R * max(16, C // G))


def _inputs(case):
    N, C, G, H, W, R, s, p = case
    Cg, Ho, Wo, _, _ = _geom(case)
    g = _gen(*case)
    sd = (0, 1, 2, 3) if N >= 3 else (1, 2, 3)
    x = _spike(torch.randn(N, C, H, W, generator=g), *sd).bfloat16()
    w = _spike(torch.randn(C, R, R, Cg, generator=g), 0, 3).bfloat16()
    dz = _spike(torch.randn(N, C, Ho, Wo, generator=g), *sd).bfloat16()
    return x, w, dz


def _oihw(w):
    return w.double().permute(0, 3, 1, 2).contiguous()  # [K,Cg,R,S]


def _dgrad_ref(dz, w4, case):
    N, C, G, H, W, R, s, p = case
    _, Ho, Wo, _, _ = _geom(case)
    op = (H - ((Ho - 1) * s - 2 * p + R), W - ((Wo - 1) * s - 2 * p + R))
    return F.conv_transpose2d(dz, w4, None, s, p, op, G)


def _wgrad_ref(x, dz, case):
    """dw[ko,r,q,c'] = Σ x[n, grp(ko)·Cg + c', ho·s−p+r, wo·s−p+q]·dz[n,ko,ho,wo]"""
    N, C, G, H, W, R, s, p = case
    Cg, Ho, Wo, _, _ = _geom(case)
    xp = F.pad(x, (p, p, p, p))
    K = dz.shape[1]  # == C in the grouped cases; dense stages differ
    dw = torch.zeros(K, R, R, Cg, dtype=torch.float64)
    dzg = dz.reshape(N, G, K // G, Ho, Wo)
    for r in range(R):
        for q in range(R):
            xs = xp[:, :, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s]
            dw[:, r, q] = torch.einsum(
                "ngkhw,ngchw->gkc", dzg,
                xs.reshape(N, G, Cg, Ho, Wo)).reshape(K, Cg)
    return dw


def _wgrad_depth(M):
    return _pow2(M + min(64, -(-M // 1024)) + 1)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gconv_fwd(case):
    N, C, G, H, W, R, s, p = case
    _, _, _, M, D = _geom(case)
    x, w, _ = _inputs(case)
    stats = torch.zeros(2 * C).cuda()
    y = _C().grouped_conv_fwd(_cl(x), w.cuda(), s, p, stats)
    ref = F.conv2d(x.double(), _oihw(w), None, s, p, 1, G)
    A = F.conv2d(x.double().abs(), _oihw(w).abs(), None, s, p, 1, G)
    assert y.dtype == torch.bfloat16
    _check(y, ref, U * ref.abs() + D * E * A, f"gconv_fwd{list(case)}")
    # Σ, Σ² of the unrounded accumulator a = cv·(1+θ), |θ| ≤ u, in f32
    cv = y.double().cpu()
    Dm = _pow2(M + 8)
    S1, A1, S2 = cv.sum((0, 2, 3)), cv.abs().sum((0, 2, 3)), \
        (cv * cv).sum((0, 2, 3))
    _check(stats[:C], S1, (Dm * E + U) * A1, f"gconv_fwd{list(case)}.sum")
    _check(stats[C:], S2, (Dm * E + 2 * U + U * U) * S2,
           f"gconv_fwd{list(case)}.sumsq")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gconv_dgrad(case):
    N, C, G, H, W, R, s, p = case
    D = _geom(case)[4]
    _, w, dz = _inputs(case)
    dx = _C().grouped_conv_dgrad(_cl(dz), w.cuda(), H, W, s, p)
    ref = _dgrad_ref(dz.double(), _oihw(w), case)
    A = _dgrad_ref(dz.double().abs(), _oihw(w).abs(), case)
    assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == (N, C, H, W)
    _check(dx, ref, U * ref.abs() + D * E * A, f"gconv_dgrad{list(case)}")


@pytest.mark.parametrize("prefill", [False, True], ids=["fresh", "prefilled"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gconv_wgrad(case, prefill):
    N, C, G, H, W, R, s, p = case
    Cg, _, _, M, _ = _geom(case)
    x, _, dz = _inputs(case)
    pre = torch.randn(C, R, R, Cg, generator=_gen(*case, 9)) * 3 + 1
    dw_out = pre.cuda() if prefill else None
    before = _C().grouped_wgrad_launches()
    dw = _C().grouped_conv_wgrad(_cl(x), _cl(dz), R, R, s, p, G, dw_out)
    after = _C().grouped_wgrad_launches()
    # the partial (msplit > 1) path runs exactly when M exceeds one m-chunk
    assert (after[1] - before[1], after[0] - before[0]) == \
        ((1, 0) if M > 1024 else (0, 1))
    assert dw.dtype == torch.float32
    if prefill:
        assert dw.data_ptr() == dw_out.data_ptr()
    ref = _wgrad_ref(x.double(), dz.double(), case)
    A = _wgrad_ref(x.double().abs(), dz.double().abs(), case)
    z = pre.double() if prefill else torch.zeros_like(ref)
    _check(dw, ref + z, _wgrad_depth(M) * E * A + E * z.abs(),
           f"gconv_wgrad{list(case)}pre={int(prefill)}")


@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=ids)
def test_gconv_wgrad_repeatable(case):
    N, C, G, H, W, R, s, p = case
    x, _, dz = _inputs(case)
    a = _C().grouped_conv_wgrad(_cl(x), _cl(dz), R, R, s, p, G)
    b = _C().grouped_conv_wgrad(_cl(x), _cl(dz), R, R, s, p, G)
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", BN_CASES, ids=ids)
def test_grouped_conv_bn_fwd_bwd(case, det):  # noqa: F811
    N, C, G, H, W, R, s, p = case
    Cg, Ho, Wo, M, D = _geom(case)
    x, w, dy = _inputs(case)
    g = _gen(*case, 3)
    gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
    rm0, rv0 = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
    cl = _C()
    y, convout, smean, sinvstd = cl.grouped_conv_bn_fwd(
        _cl(x), w.cuda(), gamma.cuda(), beta.cuda(), rm, rv, s, p, MOM, EPS,
        True, 0, None)
    tag = f"gconv_bn{list(case)}det={int(det)}"
    w4 = _oihw(w)
    ref = F.conv2d(x.double(), w4, None, s, p, 1, G)
    A = F.conv2d(x.double().abs(), w4.abs(), None, s, p, 1, G)
    _check(convout, ref, U * ref.abs() + D * E * A, tag + ".convout")
    # statistics against the returned convout: forms of test_dw_conv_bn_fwd
    cv = convout.double().cpu()
    Dm = _pow2(M + 8)
    S1, A1 = cv.sum((0, 2, 3)), cv.abs().sum((0, 2, 3))
    S2 = (cv * cv).sum((0, 2, 3))
    mean = S1 / M
    var = (S2 / M - mean * mean).clamp_min(0)
    ur = 0.0 if det else U
    d_mean = (Dm * E + ur) * A1 / M + 2 * E * mean.abs()
    d_var = ((Dm * E + 2 * ur + ur * ur) * S2 / M + 2 * mean.abs() * d_mean
             + d_mean * d_mean + 4 * E * (S2 / M + mean * mean))
    _check(smean, mean, d_mean, tag + ".smean")
    istd = (var + EPS).rsqrt()
    d_istd = torch.maximum(((var - d_var).clamp_min(0) + EPS).rsqrt() - istd,
                           istd - (var + d_var + EPS).rsqrt()) + 4 * E * istd
    _check(sinvstd, istd, d_istd, tag + ".sinvstd")
    ub = M / (M - 1)
    _check(rm, (1 - MOM) * rm0.double() + MOM * mean,
           MOM * d_mean + 4 * E * (rm0.double().abs() + mean.abs()),
           tag + ".running_mean")
    _check(rv, (1 - MOM) * rv0.double() + MOM * var * ub,
           MOM * ub * d_var + 4 * E * (rv0.double().abs() + var * ub),
           tag + ".running_var")
    bc = lambda t: t.double().cpu()[None, :, None, None]  # noqa: E731
    sm, si, ga, be = bc(smean), bc(sinvstd), bc(gamma), bc(beta)
    y_ref = (cv - sm) * si * ga + be
    y_A = (ga * si).abs() * (cv.abs() + sm.abs()) + be.abs()
    _check(y, y_ref, U * y_ref.abs() + 8 * E * y_A, tag + ".y")
    if not det:  # eval mode once: the affine map of the running statistics
        ye = cl.grouped_conv_bn_fwd(_cl(x), w.cuda(), gamma.cuda(),
                                    beta.cuda(), rm, rv, s, p, MOM, EPS,
                                    False, 0, None)[0]
        rme, ie = bc(rm), (bc(rv) + EPS).rsqrt()
        e_ref = (cv - rme) * ie * ga + be
        _check(ye, e_ref, U * e_ref.abs() + 8 * E * (
            (ga * ie).abs() * (cv.abs() + rme.abs()) + be.abs()), tag + ".eval")

    # ---- backward: reference dconv from the returned convout and stats ----
    dx, dw, sum_dzx, sum_dz, _ = cl.grouped_conv_bn_bwd(
        _cl(dy), y, _cl(x), w.cuda(), convout, gamma.cuda(), beta.cuda(),
        smean, sinvstd, s, p, 0, True, False)
    dz = dy.double()
    xh = (cv - sm) * si
    r_dz, r_dzx = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    b_dz = Dm * E * dz.abs().sum((0, 2, 3))
    b_dzx = Dm * E * (dz * xh).abs().sum((0, 2, 3))
    _check(sum_dz, r_dz, b_dz, tag + ".sum_dz")
    _check(sum_dzx, r_dzx, b_dzx, tag + ".sum_dzx")
    m_dz, m_dzx = bc(r_dz) / M, bc(r_dzx) / M
    dconv = ga * si * (dz - m_dz - xh * m_dzx)
    # cancellation floor of dconv's f32 evaluation (test_dw_conv_bn_bwd)
    F32 = (ga * si).abs() * (
        8 * E * (dz.abs() + m_dz.abs()
                 + si * (cv.abs() + sm.abs()) * m_dzx.abs())
        + (bc(b_dz) + xh.abs() * bc(b_dzx)) / M)
    dx_ref = _dgrad_ref(dconv, w4, case)
    dx_A = _dgrad_ref(dconv.abs(), w4.abs(), case)
    dx_F = _dgrad_ref(F32, w4.abs(), case)
    _check(dx, dx_ref, (2 * U + D * E) * dx_A + U * dx_ref.abs() + dx_F,
           tag + ".dx")
    dw_A = _wgrad_ref(x.double().abs(), dconv.abs(), case)
    _check(dw, _wgrad_ref(x.double(), dconv, case),
           (2 * U + _wgrad_depth(M) * E) * dw_A
           + _wgrad_ref(x.double().abs(), F32, case), tag + ".dw")


def test_grouped_guards():
    cl = _C()

    def fwd(C, Cg, R=3, s=1, p=1, w=None):
        w = torch.zeros(C, R, R, Cg).bfloat16().cuda() if w is None else w
        return cl.grouped_conv_fwd(_cl(torch.zeros(1, C, 6, 6)), w, s, p)

    with pytest.raises(RuntimeError, match="4, 8, 16 or 32"):
        fwd(16, 2)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        fwd(24, 4)
    with pytest.raises(RuntimeError, match="1x1 or 3x3"):
        fwd(16, 4, R=5, p=2)
    with pytest.raises(RuntimeError, match="Kg == Cg"):
        fwd(32, 4, w=torch.zeros(16, 3, 3, 4).bfloat16().cuda())
    with pytest.raises(RuntimeError, match="bf16 \\[K,R,S,Cg\\]"):
        fwd(16, 4, w=torch.zeros(16, 3, 3, 4).cuda())
    with pytest.raises(RuntimeError, match="bf16 \\[K,R,S,Cg\\]"):
        fwd(16, 4, w=torch.zeros(16, 3, 12).bfloat16().cuda())
    x, w = _cl(torch.zeros(1, 16, 6, 6)), torch.zeros(16, 3, 3, 4).bfloat16().cuda()
    f = torch.zeros(16).cuda()
    bad = _cl(torch.zeros(1, 16, 4, 4))
    with pytest.raises(RuntimeError, match="dy shape"):
        cl.grouped_conv_bn_bwd(bad, bad, x, w, bad, f, f, f, f, 1, 1, 0, True,
                               False)


def _stage_check(name, mc, mg, cap):
    """One conv+BN(+residual)(+ReLU) stage of the GPU block against the CPU
    module's own float64 path ON THE GPU STAGE'S OWN INPUTS (x, residual, dy).

    Bounds, first order in u and doubled for the higher orders.  The GPU
    rounds convout to bf16 (|δcv| ≤ u|cv|), which moves the batch mean by
    ≤ u·mean|cv| and the variance by ≤ dvar, hence x̂ by ex and invstd by ei.
    y₀ = γx̂+β(+res) moves by ey; where |y₀| ≤ 2·ey the ReLU mask may differ,
    so g = dy·mask is uncertain by eg = |dy| there.  These carry through Σg,
    Σg·x̂ (es1, es2, plus pow2(M+8)·e of f32 summation) into dconv = γ·invstd·
    (g − Σg/M − x̂·Σgx̂/M), which is also rounded to bf16 and evaluated in f32
    on its TERMS (the 8e floor): ed.  dW and dx are linear in dconv, so ed
    goes through the absolute wgrad / dgrad maps, plus their f32 depth."""
    x, res, dy = (None if t is None else t.detach().double().cpu()
                  for t in cap[:3])
    G, R, s, p = getattr(mc, "groups", 1), mc.kernel_size, mc.stride, mc.padding
    case = (x.shape[0], x.shape[1], G, x.shape[2], x.shape[3], R, s, p)
    xr = x.clone().requires_grad_()
    rr = None if res is None else res.clone().requires_grad_()
    mc.zero_grad()
    out = mc(xr, rr)
    out.backward(dy)
    # the stage's pieces in float64, for the bounds
    w4 = _oihw(mc.weight.detach())
    cv = F.conv2d(x, w4, None, s, p, 1, G)
    M = cv.numel() // cv.shape[1]
    red = lambda t: t.sum((0, 2, 3), keepdim=True)  # noqa: E731
    bc = lambda t: t.detach()[None, :, None, None]  # noqa: E731
    mean, a1, m2 = red(cv) / M, red(cv.abs()) / M, red(cv * cv) / M
    istd = (m2 - mean * mean + mc.eps).rsqrt()
    xh, ga, be = (cv - mean) * istd, bc(mc.bn_weight), bc(mc.bn_bias)
    dvar = 2 * U * (m2 + mean.abs() * a1)
    ex = U * istd * (cv.abs() + a1) + xh.abs() * istd ** 2 * dvar / 2
    ei = istd ** 3 * dvar / 2
    r0 = torch.zeros_like(cv) if res is None else res
    y0 = ga * xh + be + r0
    ey = ga.abs() * ex + 8 * E * (ga.abs() * xh.abs() + be.abs() + r0.abs())
    relu = mc.act == 1
    g = dy * (y0 > 0) if relu else dy
    eg = dy.abs() * (y0.abs() <= 2 * ey) if relu else torch.zeros_like(dy)
    DE = _pow2(M + 8) * E
    s1, s2 = red(g), red(g * xh)
    es1 = red(eg) + DE * red(g.abs())
    es2 = red(eg * xh.abs() + g.abs() * ex) + DE * red((g * xh).abs())
    T = g - s1 / M - xh * s2 / M
    dconv = ga * istd * T
    ed = (ga.abs() * ei * T.abs() + U * dconv.abs() + (ga * istd).abs() * (
        eg + es1 / M + ex * s2.abs() / M + xh.abs() * es2 / M
        + 8 * E * (g.abs() + s1.abs() / M + (xh * s2).abs() / M)))
    D = _pow2(R * R * max(16, x.shape[1] // G))  # conv depth, zeros included
    tag = "resnext_block." + name
    _check(cap[3], out, 4 * ey + 2 * U * out.abs(), tag + ".y")
    _check(mg.bn_bias.grad, mc.bn_bias.grad, 2 * es1.flatten(), tag + ".dbeta")
    _check(mg.bn_weight.grad, mc.bn_weight.grad, 2 * es2.flatten(),
           tag + ".dgamma")
    _check(mg.weight.grad, mc.weight.grad, 2 * (
        _wgrad_ref(x.abs(), ed, case)
        + _pow2(2 * M + 64) * E * _wgrad_ref(x.abs(), dconv.abs(), case)),
        tag + ".dw")
    if rr is not None:
        _check(cap[4], rr.grad, 2 * eg + U * rr.grad.abs(), tag + ".dres")
    dx_b = 2 * (_dgrad_ref(ed, w4.abs(), case)
                + D * E * _dgrad_ref(dconv.abs(), w4.abs(), case))
    return xr.grad, dx_b


def test_resnext_block_autograd(monkeypatch):
    """One grouped bottleneck (width 32, 8 groups of 4) through autograd on
    [2,64,8,8]: every stage's output, parameter and input gradients against
    that stage's CPU module in float64 (_stage_check), res_block not taken.
    (The first form of this test held whole-block gradients to 32·u·max|ref|;
    that scale ignores cancellation and ReLU-mask changes and was missed at
    conv2.weight by 1.825 on an MI355X — a mistake of the bound.)"""
    from horizonml_amd.models import _functional_gpu as FG
    from horizonml_amd.models.resnet import Bottleneck

    def no_res_block(*a, **k):
        raise AssertionError("res_block taken for a grouped bottleneck")
    monkeypatch.setattr(FG, "res_block", no_res_block)
    torch.manual_seed(11)
    # base_width = 8: Cg = 4 (base_width = 4 gives Cg = 2, which is refused)
    cpu = Bottleneck(64, 32, stride=2, groups=8, base_width=8)
    assert tuple(cpu.conv2.weight.shape) == (32, 3, 3, 4)
    with torch.no_grad():
        for prm in cpu.parameters():
            prm.copy_(prm.bfloat16().float())
    gpu = Bottleneck(64, 32, stride=2, groups=8, base_width=8)
    gpu.load_state_dict(cpu.state_dict())
    cpu, gpu = cpu.double(), gpu.cuda()
    names = ("conv1", "conv2", "conv3", "downsample")
    cap = {n: [None] * 6 for n in names}  # x, res, dy, y, dres, dx

    def hook(n):
        def fn(mod, args, kwargs, out):
            c, res = cap[n], kwargs.get("residual")
            c[0], c[1], c[3] = args[0], res, out
            out.register_hook(lambda gr: c.__setitem__(2, gr))
            if res is not None:
                res.register_hook(lambda gr: c.__setitem__(4, gr))
            if not args[0].is_leaf:
                args[0].register_hook(lambda gr: c.__setitem__(5, gr))
        return fn
    for n in names:
        getattr(gpu, n).register_forward_hook(hook(n), with_kwargs=True)
    x = torch.randn(2, 64, 8, 8, generator=_gen(2, 64, 8)).bfloat16()
    gy = torch.randn(2, 128, 4, 4, generator=_gen(2, 128, 4)).bfloat16()
    xg = _cl(x).requires_grad_()
    gpu(xg).backward(_cl(gy))
    dx_ref = dx_b = 0
    for n in names:
        ref, b = _stage_check(n, getattr(cpu, n), getattr(gpu, n), cap[n])
        if cap[n][5] is not None:
            _check(cap[n][5], ref, b + U * ref.abs(), f"resnext_block.{n}.dx")
        else:  # conv1 and downsample both read the block input
            dx_ref, dx_b = dx_ref + ref, dx_b + b + U * ref.abs()
    _check(xg.grad, dx_ref, dx_b + U * dx_ref.abs(), "resnext_block.x.grad")
