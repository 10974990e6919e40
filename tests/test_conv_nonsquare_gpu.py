"""Non-square inputs (H != W) through the MFMA conv + BN path, default and
deterministic mode.

Every other conv test uses H == W, so an H/W or Ho/Wo swap in an address
computation (the m -> (n, ho, wo) gather, dgrad's m -> (n, hi, wi)) would go
unseen.  Such a swap is an O(1) error, so the norm-based assertions and
tolerances of ``test_conv_shape_fuzz`` are sufficient here.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    from horizonml_amd import ops
    return ops.extension()


@pytest.fixture(params=[False, True], ids=["default", "det"])
def det(request):
    if request.param:
        _C().set_deterministic(True)
    try:
        yield request.param
    finally:
        _C().set_deterministic(False)


def rel(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def to_gpu_cl(x):
    return x.cuda().to(memory_format=torch.channels_last).to(torch.bfloat16)


def _make_pair(in_ch, out_ch, k, stride, seed=0):
    from horizonml_amd.models.layers import ConvBNAct
    torch.manual_seed(seed)
    cpu = ConvBNAct(in_ch, out_ch, k, stride=stride)
    gpu = ConvBNAct(in_ch, out_ch, k, stride=stride)
    gpu.load_state_dict(cpu.state_dict())
    return cpu, gpu.cuda()


@pytest.mark.parametrize("cfg", [
    # (cin, cout, k, stride, H, W, bs)
    (16, 24, 3, 1, 6, 10, 3),
    (8, 16, 3, 2, 9, 5, 4),
    (3, 16, 7, 2, 12, 20, 2),    # scalar-gather stem
    (32, 32, 1, 2, 7, 4, 5),
    (64, 64, 3, 1, 4, 2, 16),    # small M: owner-BN range
], ids=lambda c: "-".join(map(str, c)))
def test_conv_nonsquare_fwd_bwd(cfg, det):
    cin, cout, k, s, H, W, bs = cfg
    cpu, gpu = _make_pair(cin, cout, k, s)
    x = torch.randn(bs, cin, H, W)
    xc = x.clone().requires_grad_(True)
    xg = to_gpu_cl(x).requires_grad_(True)
    yc = cpu(xc)
    yg = gpu(xg)
    assert yg.shape == yc.shape
    assert rel(yg, yc) < 6e-2, f"y rel={rel(yg, yc)}"
    r = rel(gpu.running_mean, cpu.running_mean)
    assert r < 3e-2, f"running_mean rel={r}"
    yc.square().mean().backward()
    yg.float().square().mean().backward()
    assert xg.grad.shape == xc.grad.shape
    assert rel(xg.grad, xc.grad) < 6e-2, f"dx rel={rel(xg.grad, xc.grad)}"
    assert rel(gpu.weight.grad, cpu.weight.grad) < 6e-2
    assert rel(gpu.bn_bias.grad, cpu.bn_bias.grad) < 6e-2
