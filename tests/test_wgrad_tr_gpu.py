"""Row-major wgrad staging: the weight-gradient m-loop stages its operand
tiles as [32 m][k3] / [32 m][ko] LDS images and fetches the MFMA fragments
with transposed reads, instead of scattering both tiles transposed with
2-byte stores.

Both bodies feed the MFMAs the same operands in the same m order, so the
main check is BITWISE equality of dW between them (``set_wgrad_tr``), per
shape, in immediate and in deferred (batched) mode, into a zero gradient and
accumulating into a non-zero one.  Float64 ``conv2d_weight`` from the
bf16-rounded operands is the independent reference, under the plain f32
accumulation bound.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    from horizonml_amd import ops
    return ops.extension()


# (Nb, C, H, W, K, R, stride, pad), named for what each can break
M16 = (16, 32, 1, 1, 64, 1, 1, 0)       # one partial K-step, 16 zero rows
M32 = (1, 32, 8, 4, 64, 3, 1, 1)        # exactly one full step (prologue only)
M64 = (2, 32, 8, 4, 64, 3, 1, 1)        # two steps: buffer swap
M96 = (3, 32, 8, 4, 64, 3, 1, 1)        # three steps: last-prefetch guard
M175 = (7, 16, 5, 5, 136, 3, 1, 1)      # ragged M; Kd=144, K=136 partial tiles
STEM = (4, 3, 16, 16, 64, 7, 2, 3)      # scalar gather (C=3), Kd=147
M1024 = (16, 64, 8, 8, 64, 3, 1, 1)     # msplit>1 slabs + reduce / wgrad_msplit
TK3_64 = (8, 32, 28, 28, 64, 3, 1, 1)   # M=6272, Kd=288: the 128x64 class
TK3_128 = (8, 32, 28, 28, 128, 3, 1, 1)  # ... and 128x128 (deferred mode)
S2 = (16, 64, 8, 8, 128, 3, 2, 1)       # stride 2, TKO=128
DOWN = (16, 64, 8, 8, 128, 1, 2, 0)     # downsample form, Kd=64: one k3 tile

SHAPES = [M16, M32, M64, M96, M175, STEM, M1024, TK3_64, TK3_128, S2, DOWN]
REF_SHAPES = [M175, M1024, STEM]


def _out_hw(shape):
    Nb, C, H, W, K, R, stride, pad = shape
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """Seeded O(1) bf16 operands of one shape, on the GPU: (x, dz)."""
    Nb, C, H, W, K, R, stride, pad = shape
    Ho, Wo = _out_hw(shape)
    g = torch.Generator().manual_seed(
        sum(v * (i + 1) for i, v in enumerate(shape)))
    x = torch.randn(Nb, C, H, W, generator=g)
    dz = torch.randn(Nb, K, Ho, Wo, generator=g)
    cl = torch.channels_last
    return (x.cuda().to(memory_format=cl).to(torch.bfloat16),
            dz.cuda().to(memory_format=cl).to(torch.bfloat16))


def _dw_twice(shape, tr, defer):
    """dW of one backward into zeros, and of a second one accumulated on top
    of it, with the row-major body on or off."""
    C_ = _C()
    Nb, C, H, W, K, R, stride, pad = shape
    x, dz = _operands(shape)
    was = C_.wgrad_tr_enabled()
    C_.set_wgrad_tr(tr)
    try:
        outs = []
        dw = torch.zeros(K, R, R, C, device="cuda")
        for _ in range(2):
            got = C_.wgrad_only(x, dz, K, R, R, stride, pad, defer, dw)
            if defer:
                C_.flush_wgrad()
            torch.cuda.synchronize()
            assert got.data_ptr() == dw.data_ptr()
            outs.append(dw.clone())
    finally:
        C_.set_wgrad_tr(was)
    return outs


@functools.lru_cache(maxsize=None)
def _legacy(shape, defer):
    return _dw_twice(shape, False, defer)


@pytest.mark.parametrize("defer", [False, True], ids=["immediate", "deferred"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_tr_equals_scatter_bitwise(shape, defer):
    new = _dw_twice(shape, True, defer)
    old = _legacy(shape, defer)
    assert float(old[0].abs().max()) > 0.0
    for what, a, b in zip(("fresh", "accumulated"), new, old):
        ndiff = int((a != b).sum())
        assert torch.equal(a, b), (
            f"{shape} defer={defer} {what}: {ndiff} of {a.numel()} differ")


@pytest.mark.parametrize("shape", REF_SHAPES, ids=str)
def test_tr_against_float64(shape):
    """Per element |dW - ref| <= n * 2^-24 * S: the plain f32 accumulation
    bound over the n = M summed products, S their absolute sum."""
    Nb, C, H, W, K, R, stride, pad = shape
    Ho, Wo = _out_hw(shape)
    x, dz = _operands(shape)
    xd = x.cpu().double().contiguous()
    dzd = dz.cpu().double().contiguous()
    wsize = (K, C, R, R)
    ref = torch.nn.grad.conv2d_weight(xd, wsize, dzd, stride=stride,
                                      padding=pad)
    S = torch.nn.grad.conv2d_weight(xd.abs(), wsize, dzd.abs(),
                                    stride=stride, padding=pad)
    n = Nb * Ho * Wo
    bound = (n * 2.0 ** -24 * S).permute(0, 2, 3, 1)  # KCRS -> KRSC
    ref = ref.permute(0, 2, 3, 1)
    for defer in (False, True):
        got = _dw_twice(shape, True, defer)[0].cpu().double()
        assert tuple(got.shape) == (K, R, R, C)
        err = (got - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{shape} defer={defer}: max |dW-ref|/bound = {worst:.3e}")
        assert bool((err <= bound).all()), f"{shape} defer={defer} {worst}"
