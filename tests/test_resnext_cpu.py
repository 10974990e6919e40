"""ResNeXt on the CPU path: model structure, parameter count, and the grouped
block against torch's own grouped conv + BatchNorm."""
import pytest
import torch
import torch.nn as nn

from horizonml_amd.models import (GroupedConvBNAct, build_model, resnet50,
                                  resnext50_32x4d)


def test_resnext50_groups_and_widths():
    model = build_model("resnext50_32x4d", 10)
    for li, cg in zip(range(1, 5), (4, 8, 16, 32)):
        for blk in getattr(model, f"layer{li}"):
            assert isinstance(blk.conv2, GroupedConvBNAct)
            assert blk.conv2.groups == 32
            assert tuple(blk.conv2.weight.shape) == (32 * cg, 3, 3, cg)


def test_resnext50_parameter_count():
    # torchvision's published count for resnext50_32x4d, 1000 classes
    n = sum(p.numel() for p in resnext50_32x4d(1000).parameters())
    assert n == 25_028_904


@pytest.mark.parametrize("cin,groups,k,stride", [(16, 4, 3, 1), (32, 2, 3, 2),
                                                 (24, 6, 1, 1)])
def test_grouped_block_matches_torch(cin, groups, k, stride):
    torch.manual_seed(cin + groups)
    blk = GroupedConvBNAct(cin, cin, k, stride=stride, groups=groups,
                           act="relu").double()
    conv = nn.Conv2d(cin, cin, k, stride, k // 2, groups=groups,
                     bias=False).double()
    bn = nn.BatchNorm2d(cin).double()
    with torch.no_grad():
        blk.bn_weight.uniform_(0.5, 1.5)
        blk.bn_bias.normal_()
        conv.weight.copy_(blk.weight.permute(0, 3, 1, 2))
        bn.weight.copy_(blk.bn_weight)
        bn.bias.copy_(blk.bn_bias)
    x = torch.randn(3, cin, 7, 5, dtype=torch.float64)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = blk(xa), torch.relu(bn(conv(xb)))
    torch.testing.assert_close(ya, yb, rtol=1e-10, atol=1e-10)
    g = torch.randn_like(ya)
    ya.backward(g)
    yb.backward(g)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(blk.weight.grad.permute(0, 3, 1, 2),
                               conv.weight.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(blk.bn_weight.grad, bn.weight.grad,
                               rtol=1e-9, atol=1e-9)


def test_resnet50_state_dict_unchanged():
    sd = resnet50(10).state_dict()
    assert len(sd) == 320
    assert tuple(sd["layer2.0.conv2.weight"].shape) == (128, 3, 3, 128)
    assert tuple(sd["layer2.0.downsample.weight"].shape) == (512, 1, 1, 256)
    assert sum(v.numel() for k, v in sd.items()
               if not k.endswith("num_batches_tracked")) == 23_581_642
