"""Squeeze-and-Excitation kernels (se_kernels.hip), per element against
float64 on the CPU, with the helpers and bound forms of
test_tail_kernels_gpu.py.  Forward stages are fed the kernel's own previous
stage (s, h, g come back from se_fwd), so each bound is a one-stage bound.
Depths D read off the kernels:

* s: a thread adds its pixels, the lanes / waves / splits fold in order, one
  scale by fl(1/HW): pow2(HW + splits).
* h, ds: pow2(C); the FC2 argument, dh: pow2(Cr).  An MFMA step rounds once
  per 32 k; h adds the wave combine and the bias.  (dh reduces over C in C/32
  steps, and C/32 <= Cr for every reduction <= 32.)
* dW1, dW2, db1, db2: pow2(N); added onto a destination, one more rounding
  at the size of the result.
* y, du, dres: bf16 output of an f32 computation (D = 4); dres is bitwise dz.
  A saturated gate (g down to 1e-38 under the sentinels) puts u*g into the
  f32 / bf16 subnormal range, where the build flushes to zero and the relative
  forms do not hold: g, y and du carry the absolute term 2^-126 (TINY).
  The same gate makes da2 = dg*g*(1-g) subnormal: da2 and its split remainder
  may flush (2*TINY, carried like b_da2), and so may each of the N products of
  a weight-gradient element (N*TINY).

The sigmoid is compiled under -ffast-math, so its exp and divide have no
bound derivable from the source (the cross-entropy tests take theirs from the
kernel's output, which does not fit here).  SIG_REL is the worst relative
error of float32 ``torch.sigmoid`` on the CPU against float64 over a grid of
arguments; 4x that is allowed on top of the argument's error dz, which enters
as g*(exp(dz) - 1) and grows with |z| as the fast exp's own error does.

se_bwd returns no intermediate (dg, dh, ds), so the backward carries each
stage's bound into the next through the stage's absolute map: b_dg -> b_da2
-> (dW2, db2, b_dh) -> (dW1, db1, b_ds) -> du.
"""
import pytest
import torch

from test_tail_kernels_gpu import _C, _check, _gen, _spike, _pow2, _cl, U, E

pytestmark = pytest.mark.gpu

CASES = [  # (N, C, reduction, H, W)
    (1, 16, 4, 1, 1),      # one image, one pixel, Cr=4: tiles mostly padding
    (3, 64, 16, 7, 5),     # Cr=4, odd H != W, 35 pixels
    (17, 32, 2, 3, 3),     # N crosses the 16-image row tile by one; Cr=16
    (2, 256, 16, 9, 9),    # 32 lanes per pixel: two pixels per wave load
    (2, 48, 4, 33, 31),    # C % 32 != 0; 1023 pixels
    (4, 2048, 16, 2, 2),   # widest C, Cr=128: all waves, all column tiles
    (70, 64, 16, 1, 1),    # beyond the issue's list: N past the backward's
                           # 64-row tile and 32-row batch step
]
RAGGED = CASES[4]
ids = lambda c: "x".join(map(str, c))  # noqa: E731

_z = torch.linspace(-30, 30, 600001)
_s64 = torch.sigmoid(_z.double())
SIG_REL = float(((torch.sigmoid(_z).double() - _s64).abs() / _s64).max())
TINY = 2.0 ** -126


def _inputs(case, with_res):
    N, C, r, H, W = case
    Cr = C // r
    g = _gen(*case, int(with_res))
    t = {}
    for k in ("u", "dy", "res"):
        t[k] = _spike(torch.randn(N, C, H, W, generator=g), 0, 1, 2, 3) \
            .bfloat16()
    t["w1"] = _spike(torch.randn(Cr, C, generator=g) * C ** -0.5, 0, 1) \
        .bfloat16()
    t["w2"] = _spike(torch.randn(C, Cr, generator=g) * Cr ** -0.5, 0, 1) \
        .bfloat16()
    t["b1"], t["b2"] = torch.randn(Cr, generator=g), torch.randn(C, generator=g)
    if not with_res:
        t["res"] = None
    return t


def _run(case, with_res, outs=(None, None, None, None), act=None):
    t = _inputs(case, with_res)
    act = int(with_res if act is None else act)
    dev = [t["w1"].cuda(), t["b1"].cuda(), t["w2"].cuda(), t["b2"].cuda()]
    u = _cl(t["u"])
    fwd = _C().se_fwd(u, *dev, None if t["res"] is None else _cl(t["res"]),
                      act)
    bwd = _C().se_bwd(_cl(t["dy"]), fwd[0], u, dev[0], dev[2], *fwd[1:], act,
                      with_res, *outs)
    return t, fwd, bwd


def _check_all(case, with_res, tag, act=None):
    act = with_res if act is None else act
    N, C, r, H, W = case
    Cr, HW = C // r, H * W
    Ds = _pow2(HW + _C().se_split_count(N, HW))
    t, (y, s, h, g), (du, dres, dw1, db1, dw2, db2) = _run(case, with_res,
                                                           act=act)
    d = {k: (None if v is None else v.double()) for k, v in t.items()}
    u, w1, w2 = d["u"], d["w1"], d["w2"]
    s_, h_, g_ = s.double().cpu(), h.double().cpu(), g.double().cpu()
    # ---- forward
    _check(s, u.mean((2, 3)), Ds * E * u.abs().mean((2, 3)), tag + ".s")
    _check(h, (s_ @ w1.T + d["b1"]).clamp_min(0),
           _pow2(C) * E * (s_.abs() @ w1.abs().T + d["b1"].abs()), tag + ".h")
    g_ref = torch.sigmoid(h_ @ w2.T + d["b2"])
    dz_arg = _pow2(Cr) * E * (h_ @ w2.abs().T + d["b2"].abs())
    _check(g, g_ref, g_ref * (torch.expm1(dz_arg) + 4 * SIG_REL + E) + TINY,
           tag + ".g")
    gb = g_[:, :, None, None]
    y_ref, y_A = u * gb, u.abs() * gb
    if with_res:
        y_ref, y_A = y_ref + d["res"], y_A + d["res"].abs()
    if act:
        y_ref = y_ref.clamp_min(0)
    assert y.dtype == torch.bfloat16
    _check(y, y_ref, U * y_ref.abs() + 4 * E * y_A + TINY, tag + ".y")
    # ---- backward
    dz = d["dy"] * (y.double().cpu() > 0) if act else d["dy"]
    if with_res:
        assert torch.equal(dres.float().cpu(), dz.float()), tag + ".dres"
    else:
        assert dres is None
    dg = (dz * u).sum((2, 3))
    b_dg = Ds * E * (dz * u).abs().sum((2, 3))
    da2 = dg * g_ * (1 - g_)
    b_da2 = b_dg * g_ * (1 - g_) + 4 * E * da2.abs() + 2 * TINY
    DN, NT = _pow2(N) * E, N * TINY
    _check(db2, da2.sum(0), b_da2.sum(0) + DN * da2.abs().sum(0) + NT,
           tag + ".db2")
    _check(dw2, da2.T @ h_, b_da2.T @ h_ + DN * (da2.abs().T @ h_) + NT,
           tag + ".dw2")
    live = (h_ > 0).double()
    dh = (da2 @ w2) * live
    b_dh = (b_da2 @ w2.abs() + _pow2(Cr) * E * (da2.abs() @ w2.abs())) * live
    _check(db1, dh.sum(0), b_dh.sum(0) + DN * dh.abs().sum(0) + NT,
           tag + ".db1")
    _check(dw1, dh.T @ s_, b_dh.T @ s_.abs() + DN * (dh.abs().T @ s_.abs())
           + NT, tag + ".dw1")
    ds = dh @ w1
    b_ds = b_dh @ w1.abs() + _pow2(C) * E * (dh.abs() @ w1.abs())
    du_ref = dz * gb + ds[:, :, None, None] / HW
    du_A = dz.abs() * gb + ds.abs()[:, :, None, None] / HW
    assert du.dtype == torch.bfloat16
    _check(du, du_ref, U * du_ref.abs() + 4 * E * du_A
           + b_ds[:, :, None, None] / HW + TINY, tag + ".du")


@pytest.mark.parametrize("with_res", [True, False], ids=["res_relu", "plain"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_se_stages(case, with_res):
    before = _C().se_launches()
    _check_all(case, with_res, f"se{list(case)}res={int(with_res)}")
    after = _C().se_launches()
    assert (after[0] - before[0], after[1] - before[1]) == (3, 4)


@pytest.mark.parametrize("with_res,act", [(True, False), (False, True)],
                         ids=["res_noact", "relu_nores"])
def test_se_stages_mixed_flags(with_res, act):
    """The two scale / apply instantiations the models do not launch."""
    _check_all(CASES[1], with_res, f"se{list(CASES[1])}res={with_res}"
               f"act={act}", act)


def test_se_stages_forced_splits(monkeypatch):
    monkeypatch.setenv("HZ_SE_SPLITS", "3")
    assert _C().se_split_count(RAGGED[0], RAGGED[3] * RAGGED[4]) == 3
    _check_all(RAGGED, True, f"se{list(RAGGED)}splits=3")


def test_se_bwd_adds_onto_destinations():
    case = (3, 64, 16, 7, 5)
    _, _, fresh = _run(case, True)
    g = _gen(*case, 9)
    pre = [torch.randn(f.shape, generator=g) * 3 + 1 for f in fresh[2:]]
    outs = [p.cuda() for p in pre]
    _, _, got = _run(case, True, outs)
    for name, o, f, p, d in zip(("dw1", "db1", "dw2", "db2"), outs, fresh[2:],
                                pre, got[2:]):
        assert d.data_ptr() == o.data_ptr()
        ref = f.double().cpu() + p.double()
        _check(o, ref, E * ref.abs(), "se_direct." + name)


def test_se_weights_at_8_byte_offsets():
    """Weights as the flat engine slices them after a Cr % 8 == 4 bias: 8 mod
    16 bytes.  Same bits as from aligned copies."""
    case = (3, 64, 16, 7, 5)
    t, fwd, bwd = _run(case, True)
    w = []
    for k in ("w1", "w2"):
        buf = torch.empty(4 + t[k].numel(), dtype=torch.bfloat16).cuda()
        w.append(buf[4:].view(t[k].shape).copy_(t[k]))
        assert w[-1].data_ptr() % 16 == 8
    u = _cl(t["u"])
    f2 = _C().se_fwd(u, w[0], t["b1"].cuda(), w[1], t["b2"].cuda(),
                     _cl(t["res"]), 1)
    b2 = _C().se_bwd(_cl(t["dy"]), f2[0], u, w[0], w[1], *f2[1:], 1, True,
                     None, None, None, None)
    for x, y in zip(list(fwd) + list(bwd), list(f2) + list(b2)):
        assert torch.equal(x, y)


def test_se_repeatable():
    a, b = _run(RAGGED, True), _run(RAGGED, True)
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("direct", [False, True], ids=["eager", "direct"])
def test_se_module_autograd(direct):
    """The module through autograd is the binding, slot for slot."""
    from horizonml_amd.models.layers import SqueezeExcite
    case = (3, 64, 16, 7, 5)
    t = _inputs(case, True)
    torch.manual_seed(3)
    mod = SqueezeExcite(64, 16).cuda()
    fcs = (mod.fc1, mod.fc2)
    for fc in fcs:
        fc.refresh_shadow()
        if direct:  # what FlatParamManager sets up: zeroed .grad to add onto
            fc._managed = True
            fc.weight.grad = torch.zeros_like(fc.weight)
            fc.bias.grad = torch.zeros_like(fc.bias)
    u, res = _cl(t["u"]).requires_grad_(), _cl(t["res"]).requires_grad_()
    dy = _cl(t["dy"])
    y = mod(u, res)
    y.backward(dy)
    args = [mod.fc1.weight_bf16, mod.fc1.bias.detach(), mod.fc2.weight_bf16,
            mod.fc2.bias.detach()]
    fwd = _C().se_fwd(u.detach(), *args, res.detach(), 1)
    ref = _C().se_bwd(dy, fwd[0], u.detach(), args[0], args[2], *fwd[1:], 1,
                      True, None, None, None, None)
    assert torch.equal(y, fwd[0])
    got = [u.grad, res.grad, mod.fc1.weight.grad, mod.fc1.bias.grad,
           mod.fc2.weight.grad, mod.fc2.bias.grad]
    for name, a, b in zip(("du", "dres", "dw1", "db1", "dw2", "db2"), got, ref):
        assert torch.equal(a, b), name


def test_se_model_overfits_under_flat_engine():
    from horizonml_amd.engine.flat import FlatParamManager, HorizonAdam
    from horizonml_amd.models._functional_gpu import cross_entropy
    from horizonml_amd.models.resnet import Bottleneck, ResNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = ResNet(Bottleneck, [1, 1, 1, 1], num_classes=10, stem="cifar",
                   se_reduction=16).to(dev).train()
    mgr = FlatParamManager(model, dev)
    opt = HorizonAdam(mgr, lr=1e-3)
    x = _cl(torch.randn(16, 3, 16, 16, generator=_gen(16, 3)))
    yb = (torch.arange(16) % 10).to(dev)

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
