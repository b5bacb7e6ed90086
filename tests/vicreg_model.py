"""The VICReg oracle of the tests: the oracle's encoder (oracle.wrappers.VisualModelWrapper) + the plain-torch expander of
tests/barlow_model.py (VICReg's expander is the Barlow Twins projector: two Linear-BN-ReLU layers and a bare last Linear; keys
``model.encoder.*``, ``model.projection.l{1,2}.{0,1}.*``, ``model.projection.l3.weight``), and the published loss as torch
ops (tests/vicreg_ref.py: torch_chain).  The two views go through the model in two passes -- BatchNorm statistics per view, as
the product's wrapper documents -- and the running statistics therefore update twice per step."""
import torch
import torch.nn as nn

from oracle import wrappers as owrap
from barlow_model import Projector, Wrapper
from vicreg_ref import torch_chain


class VICReg(nn.Module):
    def __init__(self, encoder, hid_dim):
        super().__init__()
        self.encoder = encoder
        self.projection = Projector(encoder.feature_dim, hid_dim, hid_dim)

    def forward(self, x):
        return self.projection(self.encoder(x))


def oracle_vicreg(backbone, clip_length, feat_dim, state=None, double=True):
    model = Wrapper(VICReg(owrap.VisualModelWrapper(clip_length, backbone), feat_dim))
    if state is not None:
        model.load_state_dict(state)
    return (model.double() if double else model).train()


def model_loss(model, x, sim=25.0, std=25.0, cov=1.0, eps=1e-4):
    """x (b, 6, T, H, W) -> (loss, inv, varl, covl, z1, z2) through `model` (train mode), view 1 first."""
    x1, x2 = torch.chunk(x, 2, dim=1)
    z1 = model.model(x1)
    z2 = model.model(x2)
    return torch_chain(z1, z2, sim, std, cov, eps) + (z1, z2)
