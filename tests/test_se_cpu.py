"""SE models and the SqueezeExcite module on the CPU path."""
import pytest
import torch

from horizonml_amd.models import (SqueezeExcite, build_model, resnet50,
                                  resnext50_32x4d, se_resnet50)
from horizonml_amd.parallel.flat_reducer import grad_units

_BN = ("bn_weight", "bn_bias", "running_mean", "running_var",
       "num_batches_tracked")


def _block_keys(prefix, convs):
    """state_dict entries of one bottleneck: {conv: weight shape}."""
    out = {}
    for conv, shape in convs.items():
        out[f"{prefix}.{conv}.weight"] = shape
        for k in _BN:
            out[f"{prefix}.{conv}.{k}"] = () if k == _BN[4] else (shape[0],)
    return out


@pytest.mark.parametrize("name", ["se_resnet50", "se_resnext50",
                                  "se_resnext50_32x4d"])
def test_build_model_names(name):
    m = build_model(name, num_classes=10)
    assert sum(isinstance(x, SqueezeExcite) for x in m.modules()) == 16


def test_se_resnet50_layout():
    m = se_resnet50(10)
    for li, (n, cr) in enumerate(((3, 16), (4, 32), (6, 64), (3, 128)), 1):
        blocks = list(getattr(m, f"layer{li}"))
        assert len(blocks) == n
        for b in blocks:
            assert tuple(b.se.fc1.weight.shape) == (cr, 16 * cr)
            assert tuple(b.se.fc2.weight.shape) == (16 * cr, cr)
            assert b.conv3.act == 0 and not b._fusable()
    units = grad_units(m)
    assert [id(p) for _, ps in units for p in ps] == \
        [id(p) for p in m.parameters()]


@pytest.mark.parametrize("make,grouped", [(resnet50, False),
                                          (resnext50_32x4d, True)])
def test_defaults_did_not_move(make, grouped):
    sd = make(10).state_dict()
    assert not any(".se." in k for k in sd)
    in_ch = 64
    for li, ch in enumerate((64, 128, 256, 512), 1):
        w = ch * 2 if grouped else ch
        want = _block_keys(f"layer{li}.0", {
            "conv1": (w, 1, 1, in_ch),
            "conv2": (w, 3, 3, w // 32 if grouped else w),
            "conv3": (ch * 4, 1, 1, w),
            "downsample": (ch * 4, 1, 1, in_ch)})
        got = {k: tuple(v.shape) for k, v in sd.items()
               if k.startswith(f"layer{li}.0.")}
        assert got == want and list(got) == list(want)
        in_ch = ch * 4


def test_squeeze_excite_cpu_forward():
    torch.manual_seed(1)
    mod = SqueezeExcite(32, 4).double()
    u, res = torch.randn(3, 32, 5, 4).double(), torch.randn(3, 32, 5, 4).double()
    s = u.sum((2, 3)) / 20
    h = (s @ mod.fc1.weight.T + mod.fc1.bias).clamp_min(0)
    g = 1 / (1 + torch.exp(-(h @ mod.fc2.weight.T + mod.fc2.bias)))
    ref = (u * g[:, :, None, None] + res).clamp_min(0)
    torch.testing.assert_close(mod(u, res), ref, rtol=1e-12, atol=1e-12)
    plain = SqueezeExcite(32, 4, act=False).double()
    plain.load_state_dict(mod.state_dict())
    torch.testing.assert_close(plain(u), u * g[:, :, None, None],
                               rtol=1e-12, atol=1e-12)


def test_tp_full_refuses_se():
    from horizonml_amd.models.resnet import Bottleneck, ResNet
    from horizonml_amd.parallel import tp_models
    m = ResNet(Bottleneck, [1, 1, 1, 1], stem="cifar", se_reduction=16)
    with pytest.raises(ValueError, match="SqueezeExcite"):
        tp_models._shard_convs(m, 2, 0, None)
