from .build import HipAdam, HipLARS, HipSGD, make_lr_scheduler, make_optimizer  # noqa: F401
from .lr_scheduler import WarmupMultiStepLR, cosine_momentum, dino_teacher_temp  # noqa: F401
