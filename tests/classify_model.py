"""The action-recognition oracle of the tests: an oracle encoder (oracle/encoders.py) with the reference's class head
(lib/modeling/model_wrappers.py:99-117) as a plain nn.Linear.  Same module tree and state-dict keys as the product's
VideoModelWrapper, so state dicts pass between the two.  tests/test_classify_ref.py pins it to the reference through
tests/golden/classify.npz; tests/test_gpu_classify.py uses it in fp64 as the ground truth on the device."""
import torch
import torch.nn as nn

from oracle import encoders as oenc

SEED, NUM_CLASS, BACKBONE, T = 77, 7, 'R2P1D10T', 8


class OracleVideoModel(nn.Module):
    def __init__(self, num_class=NUM_CLASS, backbone=BACKBONE, dropout=0.0, partial_bn=False):
        super().__init__()
        self.base_model = oenc.BACKBONES[backbone]()
        feat = self.base_model.fc.in_features
        if dropout == 0:
            self.base_model.fc = nn.Linear(feat, num_class)
            self.new_fc = None
        else:
            self.base_model.fc = nn.Dropout(p=dropout)
            self.new_fc = nn.Linear(feat, num_class)
        head = self.base_model.fc if self.new_fc is None else self.new_fc
        nn.init.normal_(head.weight, 0, 0.001)
        nn.init.constant_(head.bias, 0)
        self._enable_pbn = partial_bn

    @property
    def head(self):
        return self.base_model.fc if self.new_fc is None else self.new_fc

    def train(self, mode=True):
        super().train(mode)
        if self._enable_pbn:
            for m in [m for m in self.base_model.modules() if isinstance(m, nn.BatchNorm3d)][1:]:
                m.eval()
        return self

    def forward(self, x, mask=None):
        """mask: an explicit dropout keep-mask (already scaled by 1 / (1 - p)) in place of the Dropout module's own draw."""
        if mask is not None:
            drop, self.base_model.fc = self.base_model.fc, nn.Identity()
            try:
                out = self.base_model(x) * mask
            finally:
                self.base_model.fc = drop
        else:
            out = self.base_model(x)
        return out if self.new_fc is None else self.new_fc(out)


def register():
    oenc.BACKBONES.setdefault(BACKBONE, lambda: oenc.R2Plus1D(10, widen_factor=0.125))


def golden_model(golden, dtype=torch.float64):
    """The model of tests/golden/classify.npz: backbone weights from the oracle builder under SEED (make_golden_classify.py
    asserts they are the reference's), class head from the fixture."""
    register()
    torch.manual_seed(SEED)
    m = OracleVideoModel()
    with torch.no_grad():
        m.base_model.fc.weight.copy_(golden.t('fc.weight'))
        m.base_model.fc.bias.copy_(golden.t('fc.bias'))
    return m.to(dtype)
