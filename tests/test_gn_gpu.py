"""GroupNorm kernels (gn_kernels.hip), per element against float64 on the CPU,
with the helpers and bound forms of test_tail_kernels_gpu.py.  Every reference
is computed from the bf16 ``convout`` the op returns, and ``y`` / backward are
fed the kernel's own ``mean`` / ``rstd``, so each bound is a one-stage bound.
With cnt = HW*Cg elements per (sample, group) and Z row chunks (1 unless the
split form runs), read off the kernels:

* mean: any-order sum of cnt terms, one scale: pow2(cnt)*E*mean|x|; the split
  form's Chan merges add (4 + 4Z)*E*max|x|.
* var: the second pass runs about the kernel's own mean, off by d <= b_mean:
  sum (x - mu - d)^2 = sum (x - mu)^2 + cnt*d^2, so
  b_var = (pow2(cnt) + 4 + 8Z)*E*var + b_mean^2.  No term in mu^2.
* rstd: rsqrt is compiled under -ffast-math and has no bound derivable from
  the source.  RS_REL is the worst relative error of float32 ``torch.rsqrt``
  on the CPU against float64 over 600001 arguments log-spaced in
  [1e-6, 1e6]; 4x that plus 4E (1/cnt, scale, + eps) is allowed on top of
  the argument's error b_var / (2 (var + eps)).
* y = act(a*x + b + res), a = gamma*rstd, b = beta - mean*a: bf16 output of
  an f32 computation over the terms |a x|, |a mean|, |beta|, |res|, D = 6.
* dbeta, dgamma: channel sums over N*HW terms: pow2(N*HW) + 8 (+ 4 for x^).
* dconv = rstd*(g*gamma - (s1 + x^*s2)/cnt): s1, s2 are sums of cnt terms
  (pow2(cnt) + 8 + Z); dconv can cancel to zero, so their bounds and 8E of
  every term enter absolutely.  dres is bitwise dy*mask.

TINY covers flushed subnormals, as in test_se_gpu.py.
"""
import pytest
import torch
import torch.nn.functional as F

from test_tail_kernels_gpu import (_C, _check, _gen, _spike, _pow2, _cl, U, E,
                                   det)  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [  # (N, C, G, H, W)
    (1, 8, 4, 1, 1),       # Cg=2, one pixel, one live lane, variance over 2
    (3, 64, 32, 7, 5),     # Cg=2, 35 rows (odd, below a wave's rows)
    (2, 24, 3, 3, 3),      # Cg=8, C below one slab and not a power of two
    (2, 128, 32, 4, 4),    # Cg=4, two 64-channel slabs
    (2, 512, 32, 2, 2),    # Cg=16, group spans 2 lanes
    (1, 1024, 32, 1, 1),   # Cg=32, HW=1
    (2, 2048, 32, 1, 3),   # Cg=64, widest C, group spans 8 lanes
    (2, 64, 32, 33, 31),   # 1023 rows: beyond the resident budget
]
ACT_RES = [(0, False), (1, False), (1, True), (2, False)]
EPS = 1e-5
TINY = 2.0 ** -126
SPLIT_LOW = 16  # rows: the 35-row and 1023-row cases split, the rest do not

_a = torch.logspace(-6, 6, 600001, dtype=torch.float64)
RS_REL = float(((torch.rsqrt(_a.float()).double() - _a.float().double() ** -0.5)
                .abs() * _a.float().double() ** 0.5).max())


def ids(c):
    return "x".join(str(int(v)) for v in (c if isinstance(c, tuple) else (c,)))


@pytest.fixture(params=[None, SPLIT_LOW], ids=["default", "split16"])
def split(request):
    old = _C().gn_split_hw()
    if request.param:
        _C().set_gn_split_hw(request.param)
    try:
        yield request.param
    finally:
        _C().set_gn_split_hw(old)


def _inputs(case, offset=False):
    N, C, G, H, W = case
    g = _gen(*case, int(offset))
    t = {}
    if offset:
        grp = (torch.arange(C) // (C // G)).double()[None, :, None, None]
        t["x"] = (100 * (1 + grp / G)
                  + 0.25 * torch.randn(N, C, H, W, generator=g)).bfloat16()
    else:
        t["x"] = _spike(torch.randn(N, C, H, W, generator=g), 0, 1, 2, 3) \
            .bfloat16()
    for k in ("dy", "res"):
        t[k] = _spike(torch.randn(N, C, H, W, generator=g), 0, 1, 2, 3) \
            .bfloat16()
    t["gamma"] = 1 + 0.5 * torch.randn(C, generator=g)
    t["beta"] = torch.randn(C, generator=g)
    return t


def _slabs(x, g):
    """Three f32 slabs [3,N,H,W,C] that sum to x (up to f32 rounding)."""
    xl = x.float().permute(0, 2, 3, 1).contiguous()
    s0 = torch.randn(xl.shape, generator=g)
    s1 = torch.randn(xl.shape, generator=g)
    return torch.stack([s0, s1, (xl.double() - s0 - s1).float()])


def _fwd(case, act, res, src="bf16", offset=False):
    t = _inputs(case, offset)
    x = (_cl(t["x"]) if src == "bf16"
         else _slabs(t["x"], _gen(*case, 7)).cuda())
    out = _C().gn_fwd(x, t["gamma"].cuda(), t["beta"].cuda(), case[2], EPS,
                      act, _cl(t["res"]) if res else None,
                      0 if src == "bf16" else 3)
    return t, out


def _bwd(case, act, res, t, fwd, outs=(None, None)):
    y, convout, mean, rstd = fwd
    return _C().gn_bwd(_cl(t["dy"]), y, convout, t["gamma"].cuda(), mean,
                       rstd, case[2], act, res, *outs)


def _per_ch(v, Cg):
    """[N,G] -> [N,C,1,1]"""
    return v.repeat_interleave(Cg, 1)[:, :, None, None]


def _stat_bounds(xg, cnt, Z):
    mu = xg.mean(2)
    b_mean = (_pow2(cnt) * E * xg.abs().mean(2)
              + (4 + 4 * Z) * E * xg.abs().amax(2))
    var = ((xg - mu[..., None]) ** 2).mean(2)
    b_var = (_pow2(cnt) + 4 + 8 * Z) * E * var + b_mean ** 2
    return mu, b_mean, var, b_var


def _check_fwd(case, act, res, src, tag, offset=False):
    N, C, G, H, W = case
    Cg, cnt = C // G, H * W * (C // G)
    Z = _C().gn_split_count(H * W, C, G, False)
    t, (y, convout, mean, rstd) = _fwd(case, act, res, src, offset)
    x = convout.double().cpu()
    assert convout.dtype == y.dtype == torch.bfloat16
    # slabs of magnitude <= 8: three f32 roundings at <= 16, then one to bf16
    _check(convout, t["x"].double(), U * t["x"].double().abs() + 48 * E,
           tag + ".convout")
    mu, b_mean, var, b_var = _stat_bounds(x.reshape(N, G, -1), cnt, Z)
    _check(mean, mu, b_mean + TINY, tag + ".mean")
    r_ref = (var + EPS) ** -0.5
    _check(rstd, r_ref,
           r_ref * (0.5 * b_var / (var + EPS) + 4 * RS_REL + 4 * E),
           tag + ".rstd")
    m_c, r_c = _per_ch(mean.double().cpu(), Cg), _per_ch(rstd.double().cpu(),
                                                         Cg)
    a = t["gamma"].double()[None, :, None, None] * r_c
    beta = t["beta"].double()[None, :, None, None]
    ref = a * (x - m_c) + beta
    A = (a * x).abs() + (a * m_c).abs() + beta.abs()
    if res:
        ref, A = ref + t["res"].double(), A + t["res"].double().abs()
    if act:
        ref = ref.clamp(0, 6) if act == 2 else ref.clamp_min(0)
    _check(y, ref, U * ref.abs() + 6 * E * A + TINY, tag + ".y")
    return var, b_var, x


@pytest.mark.parametrize("src", ["bf16", "f32x3"])
@pytest.mark.parametrize("act,res", ACT_RES, ids=ids)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gn_fwd(case, act, res, src, split):
    _check_fwd(case, act, res, src, f"gn{list(case)}a{act}r{int(res)}{src}")


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=ids)
def test_gn_fwd_offset_data(case, split):
    """Means of 100..200 over a spread of 0.25: a one-pass E[x^2] - mu^2
    loses the variance, and must fail the bound the kernel meets."""
    var, b_var, x = _check_fwd(case, 0, False, "bf16",
                               f"gn_offset{list(case)}", offset=True)
    xf = x.float().reshape(case[0], case[2], -1)
    two = ((xf - xf.mean(2, keepdim=True)) ** 2).mean(2).double()
    one = ((xf * xf).mean(2) - xf.mean(2) ** 2).double()
    assert bool(((two - var).abs() <= b_var).all())
    assert bool(((one - var).abs() > b_var).any())


@pytest.mark.parametrize("act,res", ACT_RES, ids=ids)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gn_bwd(case, act, res, split):
    N, C, G, H, W = case
    Cg, HW = C // G, H * W
    cnt = HW * Cg
    tag = f"gn_bwd{list(case)}a{act}r{int(res)}"
    t, fwd = _fwd(case, act, res)
    dconv, dres, dgamma, dbeta = _bwd(case, act, res, t, fwd)
    y, convout, mean, rstd = (v.double().cpu() for v in fwd)
    g = t["dy"].double()
    if act:
        g = g * ((y > 0) & (y < 6) if act == 2 else y > 0)
    if res:
        assert torch.equal(dres.float().cpu(), g.float()), tag + ".dres"
    else:
        assert dres is None
    m_c, r_c = _per_ch(mean, Cg), _per_ch(rstd, Cg)
    xh = (convout - m_c) * r_c
    Dc = _pow2(N * HW) + 8
    _check(dbeta, g.sum((0, 2, 3)), Dc * E * g.abs().sum((0, 2, 3)) + TINY,
           tag + ".dbeta")
    _check(dgamma, (g * xh).sum((0, 2, 3)),
           (Dc + 4) * E * (g * xh).abs().sum((0, 2, 3)) + TINY,
           tag + ".dgamma")
    gg = g * t["gamma"].double()[None, :, None, None]
    Ds = _pow2(cnt) + 8 + _C().gn_split_count(HW, C, G, True)

    def grp(v):  # per-group sum over the sample -> [N,C,1,1]
        return _per_ch(v.reshape(N, G, -1).sum(2), Cg)
    s1, s2 = grp(gg), grp(gg * xh)
    b_s1, b_s2 = Ds * E * grp(gg.abs()), (Ds + 4) * E * grp((gg * xh).abs())
    ref = r_c * (gg - (s1 + xh * s2) / cnt)
    bound = U * ref.abs() + TINY + r_c * (
        (b_s1 + xh.abs() * b_s2) / cnt
        + 8 * E * (gg.abs() + (s1.abs() + (xh * s2).abs()) / cnt))
    assert dconv.dtype == torch.bfloat16
    _check(dconv, ref, bound, tag + ".dconv")


def test_gn_bwd_adds_onto_destinations(split):
    case = CASES[1]
    t, fwd = _fwd(case, 1, True)
    fresh = _bwd(case, 1, True, t, fwd)
    pre = [torch.randn(case[1], generator=_gen(*case, 9 + i)) * 3 + 1
           for i in range(2)]
    outs = [p.cuda() for p in pre]
    got = _bwd(case, 1, True, t, fwd, outs)
    for name, o, f, p, d in zip(("dgamma", "dbeta"), outs, fresh[2:], pre,
                                got[2:]):
        assert d.data_ptr() == o.data_ptr()
        ref = f.double().cpu() + p.double()
        _check(o, ref, E * ref.abs(), "gn_direct." + name)


@pytest.mark.parametrize("shape", [(64, 32, 7, 5), (512, 32, 2, 2),
                                   (64, 32, 33, 31)], ids=ids)
def test_gn_batch_independent(shape, split):
    """A sample's bits do not depend on what else is in the batch."""
    case = (5, *shape)
    t, fwd = _fwd(case, 1, True)
    dconv = _bwd(case, 1, True, t, fwd)[0]
    gamma, beta = t["gamma"].cuda(), t["beta"].cuda()
    for n in range(5):
        one = {k: t[k][n:n + 1] for k in ("x", "dy", "res")}
        f1 = _C().gn_fwd(_cl(one["x"]), gamma, beta, case[2], EPS, 1,
                         _cl(one["res"]), 0)
        for name, a, b in zip(("y", "convout", "mean", "rstd"), fwd, f1):
            assert torch.equal(a[n:n + 1], b), f"{name}[{n}]"
        d1 = _C().gn_bwd(_cl(one["dy"]), f1[0], f1[1], gamma, f1[2], f1[3],
                         case[2], 1, True, None, None)[0]
        assert torch.equal(dconv[n:n + 1], d1), f"dconv[{n}]"


def test_gn_repeatable(det, split):
    case = CASES[7]
    runs = []
    for _ in range(2):
        t, fwd = _fwd(case, 1, True, "f32x3")
        runs.append(list(fwd) + list(_bwd(case, 1, True, t, fwd)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


CONVS = [  # (N, C, K, k, stride, pad, H)
    (2, 64, 64, 3, 1, 1, 8),     # non-split
    (2, 512, 512, 3, 1, 1, 2),   # split-K forward and dgrad, clipped taps
    (2, 3, 64, 7, 2, 3, 16),     # the stem
    (2, 64, 128, 1, 2, 0, 8),    # 1x1 stride 2
]


@pytest.mark.parametrize("cfg", CONVS, ids=ids)
def test_conv_gn_act_is_the_composition(cfg):
    N, C, K, k, stride, pad, H = cfg
    g = _gen(*cfg)
    x = _cl(torch.randn(N, C, H, H, generator=g))
    w = (torch.randn(K, k, k, C, generator=g) * (k * k * C) ** -0.5) \
        .bfloat16().cuda()
    gamma = (1 + 0.5 * torch.randn(K, generator=g)).cuda()
    beta = torch.randn(K, generator=g).cuda()
    y, convout, mean, rstd = _C().conv_gn_act_fwd(x, w, gamma, beta, 32,
                                                  stride, pad, EPS, 1, None)
    ref = F.conv2d(x.double().cpu(), w.double().cpu().permute(0, 3, 1, 2),
                   stride=stride, padding=pad)
    relerr = float((convout.double().cpu() - ref).norm() / ref.norm())
    print(f"REL conv {relerr:.5f}")
    assert relerr < 3e-2
    alone = _C().gn_fwd(convout, gamma, beta, 32, EPS, 1, None, 0)
    for name, a, b in zip(("y", "convout", "mean", "rstd"),
                          (y, convout, mean, rstd), alone):
        assert torch.equal(a, b), name
    dy = _cl(torch.randn(y.shape, generator=g))
    need_dx = C % 8 == 0
    dx, dw, dgamma, dbeta, _ = _C().conv_gn_act_bwd(
        dy, y, x, w, convout, gamma, mean, rstd, 32, stride, pad, 1, need_dx,
        False, None, None, None)
    dconv, _, dg, db = _C().gn_bwd(dy, y, convout, gamma, mean, rstd, 32, 1,
                                   False, None, None)
    assert torch.equal(dgamma, dg) and torch.equal(dbeta, db)
    assert torch.equal(dw, _C().wgrad_only(x, dconv, K, k, k, stride, pad,
                                           False, None))
    if need_dx:
        assert torch.equal(dx, _C().conv_dgrad_only(dconv, w, H, H, stride,
                                                    pad, None, None))


def test_gn_guards_and_launch_counts():
    before = _C().gn_launches()
    for C, G in ((48, 16), (128, 1), (12, 3), (64, 5)):
        x = _cl(torch.zeros(1, C, 2, 2))
        with pytest.raises(RuntimeError):
            _C().gn_fwd(x, torch.ones(C).cuda(), torch.zeros(C).cuda(), G,
                        EPS, 0, None, 0)
    assert _C().gn_launches() == before
    old = _C().gn_split_hw()
    try:
        for rows, want in ((None, (1, 2)), (SPLIT_LOW, (2, 3))):
            if rows:
                _C().set_gn_split_hw(rows)
            t, fwd = _fwd(CASES[1], 1, True)
            _bwd(CASES[1], 1, True, t, fwd)
            after = _C().gn_launches()
            assert (after[0] - before[0], after[1] - before[1]) == want
            before = after
    finally:
        _C().set_gn_split_hw(old)


def test_gn_model_overfits_under_flat_engine(tmp_path):
    from horizonml_amd.engine.flat import FlatParamManager, HorizonAdam
    from horizonml_amd.models import resnet18_gn
    from horizonml_amd.models._functional_gpu import cross_entropy
    from horizonml_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = resnet18_gn(num_classes=10).to(dev).train()
    mgr = FlatParamManager(model, dev)
    opt = HorizonAdam(mgr, lr=1e-3)
    x = _cl(torch.randn(4, 3, 32, 32, generator=_gen(4, 3)))
    yb = (torch.arange(4) % 10).to(dev)

    def step():
        loss = cross_entropy(model(x), yb)
        loss.backward()
        opt.step()
        return loss

    losses = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            losses.append(float(step()))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = step()
    for _ in range(17):
        graph.replay()
        losses.append(float(static_loss))
    print("LOSSES", " ".join(f"{v:.4f}" for v in losses))
    assert all(v == v and abs(v) < float("inf") for v in losses), losses
    assert losses[-1] < losses[0], losses
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    path = save_checkpoint(str(tmp_path / "gn.pt"), model)
    fresh = resnet18_gn(num_classes=10)
    load_checkpoint(path, fresh, restore_rng=False)
    sd = model.state_dict()
    assert list(fresh.state_dict()) == list(sd)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k].cpu()), k
