"""VideoModelWrapper: a 3D / RGB backbone with a class head, for action-recognition fine-tuning and linear probing
(reference: lib/modeling/model_wrappers.py).

Constructor signature, attributes, state-dict keys and their order, the head's init and train() follow the reference:

  dropout == 0   base_model.fc = Linear(feature_dim, num_class), new_fc = None      keys base_model.fc.{weight,bias}   (:102-104)
  dropout  > 0   base_model.fc = Dropout(p), new_fc = Linear(feature_dim, num_class) keys new_fc.{weight,bias}, last    (:105-107)
  init           normal_(weight, 0, 0.001), bias = 0                                                                 (:109-115)
  train()        with partial_bn every BatchNorm3d of base_model except the first goes to eval mode and its weight /
                 bias stop requiring gradients (:131-147)

S3D with dropout == 0 applies the Linear to the (B, 1024, T', 1, 1) map in the reference and crashes there; here it raises at
construction.  The 2D backbones, optical flow and the after-softmax output are not built (ValueError).  The head itself is
engine.layers.f_classifier: logits alone, or logits + mean cross-entropy + top-k ranks in one fused call."""
import torch.nn as nn

from . import backbone
from ..ops import get_agg
from ...engine import layers as L


class VideoModelWrapper(nn.Module):
    def __init__(self, num_class, clip_length, modality, backbone_name='resnet101', backbone_type='2D', new_length=None,
                 agg_fun='avg', before_softmax=True, dropout=0.8, crop_num=1, partial_bn=True, fc_sche=False,
                 reason_flag=False, module_name_list=None, pretrained=False, pretrain_path=None):
        super().__init__()
        if backbone_type != '3D':
            raise ValueError('Only the 3D backbones are built (got %r)' % (backbone_type,))
        if modality != 'RGB':
            raise ValueError('Only RGB clips are built (got %r)' % (modality,))
        if not before_softmax:
            raise ValueError('before_softmax=False is not built: the head returns logits')
        if int(num_class) < 1:
            raise ValueError('num_class must be positive (got %r)' % (num_class,))
        self.modality, self.backbone_name, self.backbone_type = modality, backbone_name, backbone_type
        self.clip_length, self.reshape, self.before_softmax = clip_length, True, before_softmax
        self.dropout, self.crop_num, self.reason_flag = dropout, crop_num, reason_flag
        self.module_name_list, self.agg_fun = module_name_list, agg_fun
        self.pretrained, self.fc_sche, self.pretrain_path = pretrained, fc_sche, pretrain_path
        self.num_class = int(num_class)
        self.new_length = 1 if new_length is None else new_length
        self._prepare_base_model(backbone_name)
        self.feature_dim = self._prepare_video_model(self.num_class)
        self.aggregation = get_agg(agg_fun=agg_fun, model_type=backbone_type)
        self._enable_pbn = partial_bn

    def _prepare_base_model(self, backbone_name):
        ctor = getattr(backbone.backbone_3d, backbone_name, None)
        if ctor is None:
            raise ValueError('unknown 3D backbone %r' % (backbone_name,))
        self.base_model = ctor()
        if self.pretrained and self.pretrain_path not in (None, 'none'):
            import torch
            self.base_model.load_state_dict(torch.load(self.pretrain_path))
        self.base_model.last_layer_name = 'fc'

    def _prepare_video_model(self, num_class):
        name = self.base_model.last_layer_name
        last = getattr(self.base_model, name)
        feature_dim = last[0].in_channels if self.backbone_name == 'S3D' else last.in_features
        if self.dropout == 0:
            if self.backbone_name == 'S3D':
                raise ValueError('S3D needs MODEL.DROPOUT > 0: with dropout 0 the reference puts the Linear head on the '
                                 '(B, 1024, T, 1, 1) map and fails (model_wrappers.py:102-104, s3d_1.py:30-33)')
            setattr(self.base_model, name, L.HipClassifier(feature_dim, num_class))
            self.new_fc = None
        else:
            setattr(self.base_model, name, nn.Dropout(p=self.dropout))
            self.new_fc = L.HipClassifier(feature_dim, num_class)
        return feature_dim

    @property
    def classifier(self):
        """The class head wherever it lives: base_model.fc (dropout 0) or new_fc."""
        return getattr(self.base_model, self.base_model.last_layer_name) if self.new_fc is None else self.new_fc

    @property
    def classifier_prefix(self):
        """State-dict / parameter-name prefix of the head ('base_model.fc.' or 'new_fc.')."""
        return 'base_model.%s.' % self.base_model.last_layer_name if self.new_fc is None else 'new_fc.'

    def train(self, mode=True):
        """Override the default train() to freeze the BN parameters (:131-147)."""
        super().train(mode)
        count = 0
        if self._enable_pbn:
            for m in self.base_model.modules():
                if isinstance(m, L.HipBatchNorm3d):
                    count += 1
                    if count >= 2:
                        m.eval()
                        m.weight.requires_grad = False
                        m.bias.requires_grad = False
        return self

    def features(self, tape, xv):
        """(B, 3, T, H, W) -> pooled features (B, feature_dim), after the dropout when there is one."""
        out = self.base_model.fwd(tape, xv)
        if out.t.dim() != 2 or out.t.shape[1] != self.feature_dim:
            raise RuntimeError('backbone returned %r, expected (B, %d)' % (tuple(out.t.shape), self.feature_dim))
        return out

    def fwd(self, tape, xv):
        """(B, 3, T, H, W) NCDHW fp32 -> logits Var (B, num_class)   (reference forward :74-91, 3D branch)."""
        return L.f_classifier(tape, self.classifier, self.features(tape, xv))

    def fwd_loss(self, tape, xv, target):
        """-> (loss Var (1,), logits (B, num_class), row_lse (B,), rank_ge (B,)): forward + nn.CrossEntropyLoss +
        the counts accuracy() needs, the head fused with the loss (engine.layers.f_classifier).  `target`: int64 labels on
        the device, already range-checked by the caller."""
        return L.f_classifier(tape, self.classifier, self.features(tape, xv), target)
