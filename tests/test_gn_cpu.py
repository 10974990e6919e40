"""ConvGNAct and the GroupNorm ResNets on the CPU path."""
import pytest
import torch
import torch.nn as nn

from horizonml_amd.models import (ConvGNAct, build_model, resnet18,
                                  resnet18_gn, resnet50)
from horizonml_amd.models.resnet import BasicBlock, Bottleneck, ResNet

BN_KEYS = ["weight", "bn_weight", "bn_bias", "running_mean", "running_var",
           "num_batches_tracked"]
# (convs per block, blocks per layer, layers whose first block downsamples)
LAYOUT = {"resnet18": (2, [2, 2, 2, 2], [2, 3, 4]),
          "resnet50": (3, [3, 4, 6, 3], [1, 2, 3, 4])}


def _bn_keys(name):
    """The state_dict keys of the default models as they were before the
    norm option existed."""
    nconv, blocks, ds = LAYOUT[name]
    convs = ["stem.conv"]
    for li, nb in enumerate(blocks, 1):
        for b in range(nb):
            convs += [f"layer{li}.{b}.conv{i + 1}" for i in range(nconv)]
            if b == 0 and li in ds:
                convs.append(f"layer{li}.{b}.downsample")
    return ([f"{c}.{k}" for c in convs for k in BN_KEYS]
            + ["tail.fc.weight", "tail.fc.bias"])


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_default_state_dict_keys_unchanged(name):
    assert list(build_model(name).state_dict()) == _bn_keys(name)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_conv_gn_act_matches_torch(res):
    torch.manual_seed(0)
    mod = ConvGNAct(6, 16, 3, stride=2, groups=4).double()
    with torch.no_grad():
        mod.gn_weight.normal_(1, 0.5)
        mod.gn_bias.normal_()
    conv = nn.Conv2d(6, 16, 3, stride=2, padding=1, bias=False).double()
    gn = nn.GroupNorm(4, 16, eps=mod.eps).double()
    with torch.no_grad():
        conv.weight.copy_(mod.weight.permute(0, 3, 1, 2))
        gn.weight.copy_(mod.gn_weight)
        gn.bias.copy_(mod.gn_bias)
    x = torch.randn(3, 6, 9, 7, dtype=torch.double, requires_grad=True)
    x2 = x.detach().clone().requires_grad_()
    r = torch.randn(3, 16, 5, 4, dtype=torch.double) if res else None
    y = mod(x, r)
    ref = gn(conv(x2))
    ref = torch.relu(ref + r if res else ref)
    torch.testing.assert_close(y, ref, rtol=1e-12, atol=1e-12)
    dy = torch.randn_like(ref)
    y.backward(dy)
    ref.backward(dy)
    for a, b in ((x.grad, x2.grad), (mod.gn_weight.grad, gn.weight.grad),
                 (mod.gn_bias.grad, gn.bias.grad),
                 (mod.weight.grad.permute(0, 3, 1, 2), conv.weight.grad)):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10)


def test_gn_models_have_no_running_statistics():
    m = build_model("resnet50_gn")
    assert not [n for n, _ in m.named_buffers() if "running_" in n]
    assert sum(isinstance(x, ConvGNAct) for x in m.modules()) == 53
    m18 = resnet18_gn(num_classes=10)
    assert all(not blk._fusable() for blk in m18.modules()
               if isinstance(blk, BasicBlock))
    assert m18(torch.randn(2, 3, 32, 32)).shape == (2, 10)
    assert (len(list(m18.parameters()))
            == len(list(resnet18(num_classes=10).parameters())))
    assert len(list(resnet50().parameters())) == len(list(m.parameters()))


def test_gn_refusals():
    with pytest.raises(ValueError, match="groups"):
        ConvGNAct(8, 24, groups=16)
    with pytest.raises(ValueError, match="gn"):
        ResNet(Bottleneck, [1, 1, 1, 1], norm="gn", groups=32,
               width_per_group=4)
    with pytest.raises(ValueError, match="gn"):
        ResNet(Bottleneck, [1, 1, 1, 1], norm="gn", se_reduction=16)
    with pytest.raises(ValueError, match="norm"):
        ResNet(BasicBlock, [1, 1, 1, 1], norm="ln")
    from horizonml_amd.parallel.tp_models import _shard_convs
    with pytest.raises(ValueError, match="ConvGNAct"):
        _shard_convs(resnet18_gn(), 2, 0, None)
