"""Folded-BatchNorm inference kernels (infer_kernels.hip) against float64.

Per-element bound of the one-launch ops, derived, not tuned:
    |y − ref| ≤ U·|ref| + (Kd_live + 8)·E·(|scale|·A + |bias| + |res|)
with A = conv(|x|, |w|): one bf16 rounding of the result, f32 accumulation
over the live reduction plus the three epilogue roundings; the activations
are 1-Lipschitz and add nothing.  Inputs are bf16-representable, so the
float64 reference sees exactly what the kernel sees.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -8    # bf16 unit roundoff
E = 2.0 ** -24   # f32 unit roundoff


def _C():
    from horizonml_amd import ops
    return ops.extension()


def _spike(t, *dims):
    """First and last slice of each listed dim get large bf16-exact
    magnitudes (5…6 and 6…7), signs kept."""
    for d in dims:
        for pos, base in ((0, 5.0), (t.shape[d] - 1, 6.0)):
            sl = t.select(d, pos)
            mag = base + (torch.arange(sl.numel()) % 5).reshape(sl.shape) \
                .to(t.dtype) * 0.25
            sl.copy_(torch.where(sl >= 0, mag, -mag))
    return t


def _cl(t):
    return t.to(torch.bfloat16).cuda().contiguous(
        memory_format=torch.channels_last)


def _live(H, R, s, p):
    """Filter taps of one axis that meet a real input row somewhere."""
    Ho = (H + 2 * p - R) // s + 1
    return sum(any(0 <= ho * s - p + r < H for ho in range(Ho))
               for r in range(R))


@functools.lru_cache(maxsize=None)
def _case(case, depthwise):
    """Inputs and the float64 pieces of the reference, once per case."""
    N, Cn, H, W = case[:4]
    K, R, s, p = (Cn,) + case[4:] if depthwise else case[4:]
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = _spike(torch.randn(N, Cn, H, W, generator=g), 1, 2, 3).bfloat16()
    if depthwise:
        w = _spike(torch.randn(R, R, Cn, generator=g), 2).bfloat16()
        w64 = w.double().permute(2, 0, 1).unsqueeze(1)     # [C,1,R,S]
    else:
        w = _spike(torch.randn(K, R, R, Cn, generator=g), 0, 3).bfloat16()
        w64 = w.double().permute(0, 3, 1, 2)               # OIHW
    groups = Cn if depthwise else 1
    conv = F.conv2d(x.double(), w64, None, s, p, groups=groups)
    A = F.conv2d(x.double().abs(), w64.abs(), None, s, p, groups=groups)
    scale = 0.5 + torch.rand(K, generator=g)
    bias = torch.randn(K, generator=g)
    res = _spike(torch.randn(conv.shape, generator=g), 1, 2, 3).bfloat16()
    kd_live = _live(H, R, s, p) * _live(W, R, s, p) * (1 if depthwise
                                                       else Cn)
    return x, w, scale, bias, res, conv, A, kd_live


def _run_op(case, depthwise, act, with_res, slot):
    x, w, scale, bias, res, conv, A, kd_live = _case(case, depthwise)
    s, p = case[-2:]
    C = _C()
    fn = C.dw_conv_affine_act_fwd if depthwise else C.conv_affine_act_fwd
    before = C.infer_launches()
    y = fn(_cl(x), w.cuda(), scale.cuda(), bias.cuda(), s, p, act,
           _cl(res) if with_res else None)
    torch.cuda.synchronize()
    after = C.infer_launches()
    assert [a - b for a, b in zip(after, before)] == \
        [int(i == slot) for i in range(3)]

    sc = scale.double().view(1, -1, 1, 1)
    bi = bias.double().view(1, -1, 1, 1)
    r64 = res.double() if with_res else torch.zeros_like(conv)
    ref = conv * sc + bi + r64
    if act:
        ref = ref.clamp(0.0, 6.0 if act == 2 else None)
    bound = U * ref.abs() + (kd_live + 8) * E * (sc.abs() * A + bi.abs()
                                                  + r64.abs())
    err = (y.double().cpu() - ref).abs()
    print(f"RATIO {case} act={act} res={with_res} "
          f"{float((err / bound.clamp_min(1e-300)).max()):.4f}")
    assert y.shape == ref.shape
    assert bool((err <= bound).all()), \
        f"{int((err > bound).sum())}/{err.numel()} elements out of bound"


DENSE_CASES = [                      # (N, C, H, W, K, R, stride, pad)
    (2, 3, 9, 7, 16, 3, 1, 1),       # scalar gather, H != W, K below a tile
    (1, 3, 20, 20, 64, 7, 2, 3),     # 7x7 stride-2 stem
    (2, 32, 5, 5, 40, 1, 1, 0),      # 1x1, ragged M = 50, ragged K
    (3, 64, 7, 5, 128, 1, 2, 0),     # strided 1x1 downsample
    (2, 64, 8, 8, 64, 3, 1, 1),      # exactly full tiles
    (2, 136, 4, 4, 22, 3, 2, 1),     # Kd = 1224: uneven quarters; K % 4 != 0
    (2, 256, 2, 2, 256, 3, 1, 1),    # 4 of 9 taps live
    (4, 512, 1, 1, 512, 3, 1, 1),    # 1 of 9 taps live; empty wave quarters
]
DW_CASES = [                         # (N, C, H, W, R, stride, pad)
    (2, 8, 5, 5, 3, 1, 1), (2, 96, 9, 7, 3, 2, 1), (1, 72, 6, 6, 5, 1, 2),
    (1, 64, 1, 1, 3, 1, 1), (2, 20, 7, 5, 3, 2, 1),
]
EPILOGUES = [(0, False), (1, False), (1, True), (2, False), (0, True)]
_ids = dict(ids=lambda c: "x".join(map(str, c)))


@pytest.mark.parametrize("wsplit", [0, 1], ids=["tile", "wsplit"])
@pytest.mark.parametrize("act,with_res", EPILOGUES)
@pytest.mark.parametrize("case", DENSE_CASES, **_ids)
def test_conv_affine_act(case, act, with_res, wsplit):
    C = _C()
    mode = C.infer_wsplit()
    C.set_infer_wsplit(wsplit)
    try:
        _run_op(case, False, act, with_res, wsplit)
    finally:
        C.set_infer_wsplit(mode)


@pytest.mark.parametrize("act,with_res", EPILOGUES)
@pytest.mark.parametrize("case", DW_CASES, **_ids)
def test_dw_conv_affine_act(case, act, with_res):
    _run_op(case, True, act, with_res, 2)


def test_guards_raise_before_any_launch():
    C = _C()
    x, w, sc, bi = (_cl(torch.randn(2, 8, 6, 6)),
                    torch.randn(16, 3, 3, 8).bfloat16().cuda(),
                    torch.ones(16).cuda(), torch.zeros(16).cuda())
    dw7 = torch.randn(7, 7, 8).bfloat16().cuda()
    dw3 = torch.randn(3, 3, 8).bfloat16().cuda()
    one8 = torch.ones(8).cuda()
    bad = [
        lambda: C.dw_conv_affine_act_fwd(x, dw7, one8, one8, 1, 3, 0),
        lambda: C.dw_conv_affine_act_fwd(x, dw3, sc, sc, 1, 1, 0),
        lambda: C.dw_conv_affine_act_fwd(x.float(), dw3, one8, one8, 1, 1, 0),
        lambda: C.conv_affine_act_fwd(x.float(), w, sc, bi, 1, 1, 1),
        lambda: C.conv_affine_act_fwd(x.contiguous(), w, sc, bi, 1, 1, 1),
        lambda: C.conv_affine_act_fwd(x, w.float(), sc, bi, 1, 1, 1),
        lambda: C.conv_affine_act_fwd(x, w, sc[:8].contiguous(), bi, 1, 1, 1),
        lambda: C.conv_affine_act_fwd(x, w, sc, bi.double(), 1, 1, 1),
        lambda: C.conv_affine_act_fwd(x, w, sc, bi, 1, 1, 3),
        lambda: C.conv_affine_act_fwd(x, w, sc, bi, 1, 1, 1, x),
    ]
    before = C.infer_launches()
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError, match="R\\*S <= 25"):
        bad[0]()
    assert C.infer_launches() == before


# ------------------------------------------------------------- models ------
def _model(name):
    from horizonml_amd import models
    torch.manual_seed(11)
    model = getattr(models, name)(num_classes=10)
    g = torch.Generator().manual_seed(12)
    for m in model.modules():
        if hasattr(m, "running_var"):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.running_mean.shape,
                                                 generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape,
                                               generator=g) + 0.5)
                m.bn_weight.copy_(torch.rand(m.bn_weight.shape,
                                             generator=g) * 0.5 + 0.75)
                m.bn_bias.copy_(torch.randn(m.bn_bias.shape,
                                            generator=g) * 0.2)
    x = torch.randn(2, 3, 32, 32, generator=g).bfloat16()
    return model.eval(), x


def _n_foldable(model):
    from horizonml_amd.models import ConvBNAct, DepthwiseConvBNAct
    return sum(isinstance(m, (ConvBNAct, DepthwiseConvBNAct))
               for m in model.modules())


@pytest.mark.parametrize("name", ["resnet18", "resnet50", "mobilenet_v2"])
def test_model_route_and_agreement(name):
    from horizonml_amd.models import fold_for_inference
    C = _C()
    model, x = _model(name)
    # float64 CPU model on the bf16 weights the kernels read
    ref_model = copy.deepcopy(model).double()
    for m in ref_model.modules():
        if hasattr(m, "weight_bf16"):
            with torch.no_grad():
                m.weight.copy_(m.weight.float().bfloat16().double())
    with torch.no_grad():
        ref = ref_model(x.double())
        model = model.cuda()
        xg = _cl(x)
        unfolded = model(xg).double().cpu()
        fold_for_inference(model)
        before = sum(C.infer_launches())
        folded = model(xg).double().cpu()
        assert sum(C.infer_launches()) - before == _n_foldable(model)
    e_unf = float((unfolded - ref).abs().max())
    e_fold = float((folded - ref).abs().max())
    print(f"LOGIT_ERR {name} unfolded={e_unf:.6f} folded={e_fold:.6f} "
          f"max|ref|={float(ref.abs().max()):.4f}")
    assert e_fold <= 2.0 * e_unf
    # a training-mode forward drops the fold for good
    model.train()
    model(xg)
    model.eval()
    before = sum(C.infer_launches())
    with torch.no_grad():
        model(xg)
    torch.cuda.synchronize()
    assert sum(C.infer_launches()) == before


def test_folded_forward_captures():
    from horizonml_amd.models import fold_for_inference
    model, x = _model("resnet18")
    model = fold_for_inference(model.cuda())
    xg = _cl(x)
    with torch.no_grad():
        eager = model(xg).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(xg)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = model(xg)
    for _ in range(2):
        static.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static, eager)
