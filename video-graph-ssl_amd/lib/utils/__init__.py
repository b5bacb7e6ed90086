"""lib.utils of the reference, as far as the downstream trainer imports it (tools/train_ds.py:20).  The reference imports
``creat_criterion`` from here but never defines it; MODEL.METRIC_LOSS_TYPE = 'CrossEntropyLoss' (lib/config/defaults.py:15)
is its only statement of the loss, so that is what this builds."""
import torch

from ...engine import ops


class CrossEntropyLoss(object):
    """Mean softmax cross-entropy of (b, C) fp32 device logits against int64 labels -> (1,) device tensor, by the row pass
    of gca_classifier_fwd (no backward: ActionTrainer runs head and loss fused, engine.layers.f_classifier)."""
    reduction = 'mean'

    def __call__(self, output, target):
        return ops.cross_entropy_fwd(output, target)[2]


def creat_criterion(cfg):
    kind = getattr(cfg.MODEL, 'METRIC_LOSS_TYPE', 'CrossEntropyLoss')
    if kind != 'CrossEntropyLoss':
        raise NotImplementedError('MODEL.METRIC_LOSS_TYPE %r: only CrossEntropyLoss is built' % (kind,))
    return CrossEntropyLoss()
