from .cifar import (SyntheticCIFAR10, CIFAR10Local, build_dataset,  # noqa: F401
                    get_dataloader)
from .augment import (DeviceAugment, augment_params,  # noqa: F401
                      augment_reference)
