from .resnet import (ResNet, BasicBlock, Bottleneck, resnet18, resnet34,  # noqa: F401
                     resnet50, resnext50_32x4d, se_resnet50,
                     se_resnext50_32x4d, resnet18_gn, resnet50_gn,
                     build_model)
from .mobilenet import mobilenet_v2  # noqa: F401
from .partition import partition_model, partition_units, split_counts  # noqa: F401
from .layers import (ConvBNAct, DepthwiseConvBNAct, GroupedConvBNAct,  # noqa: F401
                     ConvGNAct, Linear, GlobalAvgPool, MaxPool2d3x3s2, SqueezeExcite,
                     refresh_all_shadows)
from .infer import fold_for_inference, unfold_inference  # noqa: F401
