"""Folded-BatchNorm inference on the CPU reference path, in float64: a folded
module computes what its eval-mode BatchNorm computed, the fold stays out of
``state_dict`` and ``unfold_inference`` takes it away again."""
import pytest
import torch

from horizonml_amd.models import (BasicBlock, ConvBNAct, DepthwiseConvBNAct,
                                  fold_for_inference, unfold_inference)


def _perturb(model, g):
    """Running statistics and γ/β away from their defaults, so the fold is
    not the identity."""
    for m in model.modules():
        if hasattr(m, "running_var"):
            with torch.no_grad():
                m.running_mean.copy_(torch.randn(m.running_mean.shape,
                                                 generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.running_var.shape,
                                               generator=g) + 0.5)
                m.bn_weight.copy_(torch.rand(m.bn_weight.shape,
                                             generator=g) + 0.5)
                m.bn_bias.copy_(torch.randn(m.bn_bias.shape, generator=g))
    return model


CASES = {
    "conv_relu": (lambda: ConvBNAct(5, 7, 3, stride=2, act=True), 5, True),
    "conv_relu6": (lambda: ConvBNAct(4, 6, 1, act="relu6"), 4, False),
    "depthwise": (lambda: DepthwiseConvBNAct(6, 3, stride=1), 6, True),
    "basic_block": (lambda: BasicBlock(4, 8, stride=2), 4, False),
}


@pytest.mark.parametrize("name", CASES)
@torch.no_grad()
def test_fold_matches_eval_forward(name):
    make, in_ch, with_res = CASES[name]
    g = torch.Generator().manual_seed(3)
    model = _perturb(make().double(), g).eval()
    x = torch.randn(2, in_ch, 9, 7, generator=g, dtype=torch.float64)
    res = (torch.randn(model(x).shape, generator=g, dtype=torch.float64)
           if with_res else None)
    args = (x, res) if res is not None else (x,)
    ref = model(*args)
    keys = list(model.state_dict().keys())

    fold_for_inference(model)
    assert all(m._folded for m in model.modules()
               if isinstance(m, (ConvBNAct, DepthwiseConvBNAct)))
    assert list(model.state_dict().keys()) == keys
    got = model(*args)
    tol = 1e-12 * float(ref.abs().max())
    assert float((got - ref).abs().max()) <= tol
    # the fold is really in use: moving the running mean changes nothing now
    first = next(m for m in model.modules() if hasattr(m, "running_mean"))
    saved = first.running_mean.clone()
    first.running_mean.add_(1.0)
    assert torch.equal(model(*args), got)
    first.running_mean.copy_(saved)

    unfold_inference(model)
    assert not any(getattr(m, "_folded", False) for m in model.modules())
    assert not any("fold_" in n for n, _ in model.named_buffers())
    assert torch.equal(model(*args), ref)


def test_training_forward_drops_fold():
    g = torch.Generator().manual_seed(5)
    m = _perturb(ConvBNAct(3, 4, 3).double(), g).eval()
    x = torch.randn(2, 3, 6, 6, generator=g, dtype=torch.float64)
    fold_for_inference(m)
    m.train()
    m(x)  # moves the running statistics: the fold is stale and must go
    assert not m._folded and not hasattr(m, "fold_scale")
    m.eval()
    y = m(x)
    unfold_inference(m)
    assert torch.equal(m(x), y)
