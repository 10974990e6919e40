"""KRSC-direct dgrad: the dgrad implicit GEMM reads the KRSC weight itself
(transposed LDS read) instead of a permuted RSCK image.

The two layouts feed the MFMAs the same operands in the same K order, so the
main check is BITWISE equality of dx between them, per shape, with and
without the fused accumulate.  Float64 ``conv2d_input`` from the bf16-rounded
operands is the independent reference, under the dx bound of
``test_ops_gpu.py::test_conv_bn_relu_bwd``.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DX_REL_BOUND = 5e-2  # test_conv_bn_relu_bwd's bound on rel(dx)


def _C():
    from horizonml_amd import ops
    return ops.extension()


def rel(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    d = (a - b).norm()
    return (d / b.norm().clamp_min(1e-12)).item()


# (Nb, C, H, W, K, R, stride, pad)
SHAPES = [
    (2, 64, 8, 8, 64, 3, 1, 1),     # split-K on (Kd = 576, 2 tiles)
    (2, 64, 8, 8, 128, 3, 2, 1),    # stride 2, split
    (1, 8, 5, 7, 8, 3, 1, 1),       # C, K << tile; M = 35; K-steps straddle (r,s)
    (2, 24, 6, 6, 40, 3, 1, 1),     # K % 32 != 0; C no multiple of 16
    (2, 72, 4, 4, 16, 1, 1, 0),     # 1x1; second, ragged n-tile
    (3, 16, 9, 9, 32, 1, 2, 0),     # 1x1 stride 2; odd spatial size
    (1, 12, 4, 4, 20, 3, 1, 1),     # C % 8 and K % 8 != 0: scalar gathers
    (2, 128, 4, 4, 512, 3, 1, 1),   # layer4 class: Kd = 4608, 32-way split
    # the mixed gathers: the A side vectorises on K % 8, the B side on C % 8
    (1, 16, 4, 4, 20, 3, 1, 1),     # scalar A gather, vec8 B rows
    (1, 12, 4, 4, 24, 3, 1, 1),     # vec8 A gather, scalar B rows
]

# One shape per throughput tile pick_tile_dgrad selects (dgrad: M = Nb*H*W,
# N = C), at the M of test_conv_throughput_tiles_fwd_bwd (16 x 56^2, 16 x 72^2)
# plus the fill-split 128x128 shape of test_conv_bwd_fill_split_shape.
TILE_SHAPES = [
    (16, 64, 56, 56, 64, 3, 1, 1),    # M = 50176, N = 64  -> 128x64
    (16, 128, 56, 56, 64, 3, 1, 1),   # M = 50176, N = 128 -> 128x128
    (16, 64, 72, 72, 64, 3, 1, 1),    # M = 82944, N = 64  -> 256x64
    (32, 128, 28, 28, 128, 3, 1, 1),  # M = 25088 -> 128x128, fill-split K
]


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """Seeded O(1) bf16 operands of one shape, on the GPU: (dz, w, acc)."""
    Nb, C, H, W, K, R, stride, pad = shape
    Ho = (H + 2 * pad - R) // stride + 1
    Wo = (W + 2 * pad - R) // stride + 1
    g = torch.Generator().manual_seed(
        sum(v * (i + 1) for i, v in enumerate(shape)))
    dz = torch.randn(Nb, K, Ho, Wo, generator=g)
    w = torch.randn(K, R, R, C, generator=g)
    acc = torch.randn(Nb, C, H, W, generator=g)
    cl = torch.channels_last
    return (dz.cuda().to(memory_format=cl).to(torch.bfloat16),
            w.cuda().to(torch.bfloat16).contiguous(),
            acc.cuda().to(memory_format=cl).to(torch.bfloat16))


def _dx(shape, layout, accum):
    Nb, C, H, W, K, R, stride, pad = shape
    dz, w, acc = _operands(shape)
    w_rsck = w.permute(1, 2, 3, 0).contiguous() if layout == "rsck" else None
    out = _C().conv_dgrad_only(dz, w, H, W, stride, pad, w_rsck,
                               acc.clone() if accum else None)
    torch.cuda.synchronize()
    return out


def _assert_layouts_bitwise(shape):
    for accum in (False, True):
        direct = _dx(shape, "krsc", accum)
        legacy = _dx(shape, "rsck", accum)
        assert direct.shape == legacy.shape
        ndiff = int((direct != legacy).sum())
        assert torch.equal(direct, legacy), (
            f"{shape} accum={accum}: {ndiff} of {direct.numel()} differ")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_krsc_equals_rsck_bitwise(shape):
    _assert_layouts_bitwise(shape)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_krsc_against_float64(shape):
    Nb, C, H, W, K, R, stride, pad = shape
    dz, w, _ = _operands(shape)
    ref = torch.nn.grad.conv2d_input(
        (Nb, C, H, W), w.cpu().double().permute(0, 3, 1, 2).contiguous(),
        dz.cpu().double().contiguous(), stride=stride, padding=pad)
    got = _dx(shape, "krsc", False)
    r = rel(got, ref)
    print(f"{shape}: rel(dx, float64) = {r:.3e}")
    assert tuple(got.shape) == (Nb, C, H, W)
    assert r < DX_REL_BOUND, f"{shape} rel={r}"


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=str)
def test_krsc_throughput_tiles_bitwise(shape):
    _assert_layouts_bitwise(shape)


def test_conv_bn_act_bwd_slot_semantics():
    """None, the KRSC weight itself and the RSCK image in the w_rsck slot
    give the same dx, dw, dgamma, dbeta (fixed-order reductions on)."""
    C_ = _C()
    Nb, C, H, W, K, R, stride, pad = 4, 32, 8, 8, 48, 3, 1, 1
    g = torch.Generator().manual_seed(5)
    cl = torch.channels_last
    x = (torch.randn(Nb, C, H, W, generator=g).cuda()
         .to(memory_format=cl).to(torch.bfloat16))
    w = torch.randn(K, R, R, C, generator=g).mul(0.1).cuda().to(
        torch.bfloat16).contiguous()
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).cuda()
    beta = (0.1 * torch.randn(K, generator=g)).cuda()
    dy = (torch.randn(Nb, K, H, W, generator=g).cuda()
          .to(memory_format=cl).to(torch.bfloat16))
    was = C_.deterministic_enabled()
    C_.set_deterministic(True)
    try:
        y, convout, smean, sinvstd = C_.conv_bn_act_fwd(
            x, w, gamma, beta, torch.zeros(K).cuda(), torch.ones(K).cuda(),
            stride, pad, 0.1, 1e-5, True, 1, None, None)
        outs = []
        for slot in (None, w, w.permute(1, 2, 3, 0).contiguous()):
            dx, dw, dgamma, dbeta, _ = C_.conv_bn_act_bwd(
                dy, y, x, w, slot, convout, gamma, beta, smean, sinvstd,
                stride, pad, 1, True, False, None, None, None, None, None, 0,
                False, None, None)
            torch.cuda.synchronize()
            outs.append((dx, dw, dgamma, dbeta))
    finally:
        C_.set_deterministic(was)
    assert float(outs[0][0].float().abs().max()) > 0.0
    for other in outs[1:]:
        for name, a, b in zip(("dx", "dw", "dgamma", "dbeta"), outs[0],
                              other):
            assert torch.equal(a, b), name


def _three_flat_steps(krsc):
    from horizonml_amd.engine.flat import FlatParamManager, HorizonAdam
    from horizonml_amd.models import build_model
    from horizonml_amd.models._functional_gpu import cross_entropy
    from horizonml_amd.models.layers import ConvBNAct
    C_ = _C()
    C_.set_dgrad_krsc(krsc)
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)
    model = build_model("resnet18", num_classes=10).to(dev).train()
    mgr = FlatParamManager(model, dev)
    opt = HorizonAdam(mgr, lr=1e-3)
    x = (torch.randn(8, 3, 32, 32, device=dev)
         .to(memory_format=torch.channels_last).to(torch.bfloat16))
    y = torch.randint(0, 10, (8,), device=dev)
    for _ in range(3):
        cross_entropy(model(x), y).backward()
        opt.step()
    torch.cuda.synchronize()
    has_image = [hasattr(m, "_w_rsck") for m in model.modules()
                 if isinstance(m, ConvBNAct)]
    return mgr.master.clone(), mgr.rsck.numel(), has_image


def test_flat_engine_same_weights_without_rsck_image():
    """Three optimizer steps of ResNet18 (batch 8, fixed-order reductions)
    end in bitwise the same master weights with and without the RSCK image;
    direct mode keeps no image at all."""
    C_ = _C()
    was_det, was_krsc = C_.deterministic_enabled(), C_.dgrad_krsc_enabled()
    C_.set_deterministic(True)
    try:
        master_d, rsck_d, img_d = _three_flat_steps(True)
        master_l, rsck_l, img_l = _three_flat_steps(False)
    finally:
        C_.set_deterministic(was_det)
        C_.set_dgrad_krsc(was_krsc)
        C_.set_wgrad_defer(False)
    assert rsck_d == 0 and not any(img_d)
    assert rsck_l > 11e6 and all(img_l)
    assert torch.equal(master_d, master_l)
